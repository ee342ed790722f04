"""CPU checks of tests/dense_ref.py: every float64 statement the GPU parity tests
of tests/test_hip_dense_rows.py compare a kernel with is tied here to an
independent one (torch float64 matmul / autograd, the oracle's interpolation),
and every data recipe is shown to be able to fail: an f32 evaluation of the
reference itself lies within the bar, the bar is far below what one dropped
8-term k-group changes, and the exact sums are exact in f32 but mostly NOT
representable in the activation type."""
import numpy as np
import pytest
import torch

import oracle as O
import dense_ref as D
import pointwise_ref as R

F64 = torch.float64
# (rows, K, N): one shape per K of each kernel form; rows kept small, the recipes
# are row-wise i.i.d.
RECIPE_SHAPES = [(17, 32, 1), (50, 64, 40), (50, 96, 70), (100, 128, 102),
                 (100, 128, 300), (33, 256, 130), (77, 384, 200), (100, 512, 512)]


def test_dense_statements_under_autograd_f64():
  """dense_rows_act and dense_wgrad are the two gradients of dense_rows."""
  rng = np.random.RandomState(0)
  for rows, K, N in ((1, 1, 1), (7, 5, 3), (40, 33, 17)):
    x = torch.tensor(rng.randn(rows, K), dtype=F64, requires_grad=True)
    W = torch.tensor(rng.randn(K, N), dtype=F64, requires_grad=True)
    b = torch.tensor(rng.randn(N), dtype=F64)
    dy = rng.randn(rows, N)
    y = x @ W + b
    y.backward(torch.tensor(dy))
    xn, Wn = x.detach().numpy(), W.detach().numpy()
    np.testing.assert_allclose(D.dense_rows(xn, Wn, b.numpy()), y.detach().numpy(),
                               rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(D.dense_rows(xn, Wn, b.numpy(), 'sigmoid'),
                               torch.sigmoid(y).detach().numpy(), rtol=1e-13)
    # dh = dz W^T: the operand of cg_dense_rows_act is packed from W transposed
    np.testing.assert_allclose(D.dense_rows(dy, Wn.T), x.grad.numpy(), rtol=1e-12,
                               atol=1e-13)
    np.testing.assert_allclose(D.dense_wgrad(xn, dy), W.grad.numpy(), rtol=1e-12,
                               atol=1e-13)
  # the rounded statement, on integers (float64 sums exact in any order)
  xi = rng.randint(-40, 41, (9, 64)).astype(np.float64)
  wi = rng.randint(-40, 41, (64, 11)).astype(np.float64)
  want = (torch.tensor(xi) @ torch.tensor(wi)).numpy()
  for f16 in (False, True):
    np.testing.assert_array_equal(D.dense_rows_act(xi, wi, f16),
                                  R.round_act(want, f16))
  # saturation and non-finite arguments of the sigmoid
  s = D.sigmoid([-np.inf, -1000.0, -30.0, 0.0, 30.0, 1000.0, np.inf, np.nan])
  assert s[0] == 0 and s[1] == 0 and 0 < s[2] < 1e-12 and s[3] == 0.5
  assert 1 - 1e-12 < s[4] <= 1 and s[5] == 1 and s[6] == 1 and np.isnan(s[7])


def test_interp_composition_matches_the_oracle():
  rng = np.random.RandomState(1)
  n, B, L, K, N = 3, 2, 5, 12, 7
  x, W, b = rng.randn(n * B * L, K), 0.3 * rng.randn(K, N), 0.1 * rng.randn(N)
  real, alpha = rng.rand(B * L, N), rng.rand(n * B)
  alpha[:3] = [0.0, 1.0, 0.5]
  for f16 in (False, True):
    got = D.dense_rows_interp(x, W, b, 'sigmoid', real, alpha, n, B, L, f16)
    fake = torch.sigmoid(torch.tensor(x) @ torch.tensor(W) + torch.tensor(b))
    fake = fake.reshape(n, B, L, N)
    rt = torch.tensor(real).reshape(B, L, N)
    for k in range(n):
      want = O.interpolation(rt, fake[k], torch.tensor(alpha[k * B:(k + 1) * B]))
      np.testing.assert_allclose(got[k]['xhat'], want.numpy(), rtol=1e-13)
      np.testing.assert_allclose(got[k]['fake'], fake[k].numpy(), rtol=1e-13)
      # rounded once, from the unrounded values
      np.testing.assert_array_equal(got[k]['xhat_r'], R.round_act(want.numpy(), f16))
      np.testing.assert_array_equal(got[k]['real_r'],
                                    R.round_act(real, f16).reshape(B, L, N))
    # alpha 0 / 1: x^ is fake / real
    np.testing.assert_array_equal(got[0]['xhat'][0], got[0]['fake'][0])
    np.testing.assert_allclose(got[0]['xhat'][1], rt[1].numpy(), rtol=1e-15)
    none = D.dense_rows_interp(x, W, b, None, real, None, n, B, L, f16)
    assert none[0]['xhat'] is None and none[0]['xhat_r'] is None


def test_flush_argument():
  for f16 in (False, True):
    tiny = R.act_limits(f16)[0]
    mn = D.min_normal(f16)
    x = np.array([[tiny, -tiny, mn, mn / 2]])
    W = np.full((4, 1), 2.0**10)
    assert D.dense_rows(x, W)[0, 0] == (mn + mn / 2) * 2.0**10
    assert D.dense_rows(x, W, None, None, True, f16)[0, 0] == mn * 2.0**10
    f = D.flush(np.array([-tiny, tiny, -mn]), f16)
    assert np.signbit(f[0]) and f[0] == 0 and not np.signbit(f[1]) and f[2] == -mn


@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'f16'])
@pytest.mark.parametrize('rows,K,N', RECIPE_SHAPES)
def test_real_recipe_meets_and_needs_its_bar(rows, K, N, f16):
  """(a) A numpy f32 matmul of the recipe's operands lies within acc_bound of the
  float64 result: a correct f32 contraction passes.  (b) The bar cannot hide a
  dropped k-group: for EVERY 8-term k-group, on at least half of the outputs the
  bar is at most 1/20 of what dropping that group changes (the median over the
  outputs of bar / |group's contribution| <= 1/20)."""
  x, W32, Wq, bias = D.real_recipe(7, rows, K, N, f16)
  assert np.abs(D.dense_rows(x, Wq, bias)).max() <= D.T_MAX * 1.01
  want = D.dense_rows(x, Wq, bias)
  bar = D.acc_bound(x, Wq, bias)
  got = (x.astype(np.float32) @ Wq.astype(np.float32) +
         bias.astype(np.float32)).astype(np.float64)
  assert (np.abs(got - want) <= bar).all()
  sig = D.group_signal(x, Wq)
  with np.errstate(divide='ignore'):
    ratio = np.median((bar[None] / sig).reshape(sig.shape[0], -1), axis=1)
  assert ratio.max() <= 1 / 20, ratio.max()
  # the sigmoid: through the largest slope of the reference itself
  s = D.sigmoid(want)
  s32 = (1 / (1 + np.exp(-got.astype(np.float32)))).astype(np.float64)
  assert (np.abs(s32 - s) <= D.sigmoid_bar(bar, s)).all()
  # the planted values are in place and nothing non-finite is
  tiny = R.act_limits(f16)[0]
  assert (x[:, 2] == tiny).all() and np.signbit(x[:, 1]).all() and (x[:, 1] == 0).all()
  assert np.isfinite(x).all() and np.isfinite(Wq).all()
  np.testing.assert_array_equal(R.round_act(x, f16), x)


@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'f16'])
def test_special_recipe(f16):
  rows, K, N = 45, 128, 40
  x, W32, Wq, bias, rr = D.special_recipe(9, rows, K, N, f16)
  with np.errstate(invalid='ignore'):
    t = D.dense_rows(x, Wq, bias)
    s = D.dense_rows(x, Wq, bias, 'sigmoid')
  odd = set(rr.values())
  assert len(odd) == 5
  plain = np.array([r not in odd for r in range(rows)])
  assert np.isfinite(t[plain]).all() and np.abs(t[plain]).max() <= D.T_MAX * 1.01
  # inf x 0 (the zero column) is NaN, elsewhere +-inf by the sign of W[7, n]
  assert np.isnan(t[rr['inf'], D.ZC])
  other = np.arange(N) != D.ZC
  assert (t[rr['inf'], other] == np.inf * np.sign(Wq[7, other])).all()
  assert np.isnan(t[rr['nan']]).all()
  big = R.act_limits(f16)[1]
  assert t[rr['big'], D.ZC] == x[rr['big']] @ Wq[:, D.ZC] + bias[D.ZC]
  assert np.isfinite(t[rr['big']]).all()
  assert np.abs(np.float32(big) * Wq[8].astype(np.float32)).max() < np.inf
  # planted saturations: within the epilogue's atol of 0 or 1
  for key, mag in (('sat30', 30.0), ('sat100', 100.0)):
    assert (np.abs(np.abs(t[rr[key], other]) - mag) < 1).all()
    sat = s[rr[key], other]
    assert (np.minimum(sat, 1 - sat) < D.SIG_ATOL).all()


@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'f16'])
@pytest.mark.parametrize('rows,K,N', [(9, 128, 102), (33, 256, 130), (77, 384, 200),
                                      (100, 512, 512), (40, 128, 8)])
def test_exact_recipe_is_exact_in_f32_and_needs_rounding(rows, K, N, f16):
  x, W, ties, over = D.exact_recipe(11, rows, K, N, f16)
  ux, uw = D.exact_units(f16)
  # operands are values of the activation type
  np.testing.assert_array_equal(R.round_act(x, f16), x)
  np.testing.assert_array_equal(R.round_act(W, f16), W)
  # every partial sum of every subset is an integer below 2^24 product units
  units = (np.abs(x) @ np.abs(W)) / (ux * uw)
  assert units.max() < 2.0**24
  exact = D.dense_rows(x, W)
  np.testing.assert_array_equal(
      (x.astype(np.float32) @ W.astype(np.float32)).astype(np.float64), exact)
  # the sums are well past what the type keeps: most of them must be rounded
  share = (R.round_act(exact, f16) != exact).mean()
  assert share >= 0.25, share
  assert np.median(np.abs(exact)) / (ux * uw) > (2.0**11 if f16 else 2.0**8)
  # the four ties: a 9- / 12-bit odd integer of units, rounded to even
  T = 2**11 if f16 else 2**8
  want = [T, T + 4, T + 4, T + 8]
  for j, (r, c) in enumerate(ties):
    assert abs(exact[r, c]) == (T + 2 * j + 1) * ux * uw
    assert abs(D.dense_rows_act(x, W, f16)[r, c]) == want[j] * ux * uw
  # beyond fp16's range, both signs
  (r4, c4), (r5, c5) = over
  assert exact[r4, c4] > 1.5 * 65504 and exact[r5, c5] < -1.5 * 65504
  got = D.dense_rows_act(x, W, f16)
  if f16:
    assert got[r4, c4] == np.inf and got[r5, c5] == -np.inf
  else:
    assert np.isfinite(got).all()


@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'f16'])
@pytest.mark.parametrize('rows,cx,cg', [(1, 1, 1), (31, 102, 102), (70, 32, 256),
                                        (1000, 130, 40)])
def test_wgrad_recipe_meets_its_bar(rows, cx, cg, f16):
  x, g = D.wgrad_recipe(13, rows, cx, cg, f16)
  want, bar = D.dense_wgrad(x, g), D.wgrad_bound(x, g)
  got = (x.astype(np.float32).T @ g.astype(np.float32)).astype(np.float64)
  assert (np.abs(got - want) <= bar).all()
  # the same bound, term by term
  if rows <= 70:
    terms = x[:, :, None] * g[:, None, :]
    np.testing.assert_allclose(bar, 2 * R.sum_bound(terms, axis=0), rtol=1e-12)
  if rows >= 1000:
    # the sum over rows outgrows its worst-case bound: a dropped 32-row stage (what
    # the kernel walks) still moves at least half of the weights by 20 bars here;
    # an 8-row group no longer does, and at 4097 rows neither -- the GPU test
    # therefore runs every shape on exact integers as well
    worst = 0.0
    for r0 in range(0, rows - 31, 32):
      sig = np.abs(x[r0:r0 + 32].T @ g[r0:r0 + 32])
      with np.errstate(divide='ignore'):
        worst = max(worst, np.median(bar / sig))
    assert worst <= 1 / 20, worst


def test_wgrad_workspace_sizing_statement():
  # one tile, few rows: 8 ranges; many rows: 512 ranges of whole 32-row stages
  assert D.wgrad_ws_elems(1, 1, 1) == 8
  assert D.wgrad_ws_elems(4097, 102, 102) == 136 * 102 * 102  # 129 stages -> 136
  assert D.wgrad_ws_elems(262144, 102, 102) == 512 * 102 * 102
  assert D.wgrad_ws_elems(70, 32, 256) == 8 * 32 * 256
  # 16 tiles: 1024 / 16 = 64 ranges
  assert D.wgrad_ws_elems(2**21, 512, 512) == 64 * 512 * 512
