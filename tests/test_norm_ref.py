"""CPU tests of the float64 statements of tests/norm_ref.py: each equals float64
autograd of the oracle's layers (O.layer_norm, O.leaky_relu, a biased-variance
batch norm written in torch, the adjoint of O.phase_shuffle) at rtol = 1e-12; the
two-pass LayerNorm bars are no looser than swconv_ref.layernorm_bounds; and on the
random-real recipes every derived bar (plus the store's ulp, where an activation
is stored) is below the tolerance the old test of tests/test_hip_kernels.py allowed
for the same quantity -- so the parity tests of tests/test_hip_norm.py can never
be weaker than the tests they stand beside."""
import numpy as np
import pytest
import torch

import oracle as O

import norm_ref as N
import pointwise_ref as R
import swconv_ref as S
import wgrad_ref as W

F64 = torch.float64
ALPHA = R.f32(O.LEAKY_ALPHA)
EPS = R.f32(O.LN_EPS)
RTOL = 1e-12


def t64(a, grad=False):
  return torch.tensor(np.asarray(a, np.float64), dtype=F64, requires_grad=grad)


def close(got, want, scale=None):
  """rtol = 1e-12 against the largest magnitude of the array (sums cancel)."""
  want = np.asarray(want, np.float64)
  atol = RTOL * (np.abs(want).max() if scale is None else scale)
  np.testing.assert_allclose(got, want, rtol=RTOL, atol=atol)


def shuffle_batch(x, shifts, seg):
  return torch.cat([O.phase_shuffle(x[b:b + 1], int(shifts[b // seg]))
                    for b in range(x.shape[0])], 0)


# ---------------------------------------------------------------------------
# the statements against autograd
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('f16', [False, True])
@pytest.mark.parametrize('rows,C', [(7, 5), (33, 102), (4, 500)])
def test_ln_is_autograd_of_the_oracle(rows, C, f16):
  y, gamma, beta, dh = N.ln_recipe(1, rows, C, f16, big=False)
  yt, gt, bt = t64(y, True), t64(gamma, True), t64(beta, True)
  ln = O.layer_norm(yt, gt, bt, EPS)
  h_ref = O.leaky_relu(ln, ALPHA)
  f = N.ln_fwd(y, gamma, beta, EPS, ALPHA, f16)
  close(f['h'], h_ref.detach().numpy())
  mean = y.mean(axis=1)
  close(f['mean'], mean)
  close(f['rstd'], 1.0 / np.sqrt(((y - mean[:, None])**2).mean(axis=1) + EPS))
  # backward: the mask from a rounded h with zeros of both signs planted
  h = R.round_act(f['h'], f16)
  N.plant_mask_zeros(h, dh)
  mask = np.where(h > 0, 1.0, ALPHA)
  (ln * t64(dh * mask)).sum().backward()
  b = N.ln_bwd(dh, h, y, f['mean'], f['rstd'], gamma, ALPHA)
  close(b['dy'], yt.grad.numpy())
  close(b['dgamma'], gt.grad.numpy(), np.abs(dh).sum(axis=0).max())
  close(b['dbeta'], bt.grad.numpy(), np.abs(dh).sum(axis=0).max())
  dbias, _ = N.dbias(b['dy'])
  close(dbias, yt.grad.numpy().sum(axis=0), np.abs(b['dy']).sum(axis=0).max())


def test_ln_bwd_uses_the_statistics_it_is_given():
  """An rstd that is not 1 / sqrt(var + eps) of the data and a mean that is not the
  data's: the statement is the autograd of the same formula with mean and rstd held
  as constants in xhat and as the outer factor."""
  rows, C = 9, 30
  y, gamma, _, dh = N.ln_recipe(2, rows, C, False, big=False)
  rng = np.random.RandomState(3)
  mean, rstd = rng.randn(rows) * 0.5, rng.uniform(0.3, 2.0, rows)
  h = R.round_act(rng.randn(rows, C), False)
  N.plant_mask_zeros(h, dh)
  b = N.ln_bwd(dh, h, y, mean, rstd, gamma, ALPHA)
  do = t64(dh * np.where(h > 0, 1.0, ALPHA))
  xh = (t64(y) - t64(mean)[:, None]) * t64(rstd)[:, None]
  dyh = do * t64(gamma)
  dy = t64(rstd)[:, None] * (dyh - dyh.mean(1, keepdim=True) -
                             xh * (dyh * xh).mean(1, keepdim=True))
  close(b['dy'], dy.numpy())
  close(b['dgamma'], (do * xh).sum(0).numpy(), float((do * xh).abs().sum(0).max()))
  close(b['dbeta'], do.sum(0).numpy(), float(do.abs().sum(0).max()))
  assert not np.allclose(b['dy'], N.ln_bwd(dh, h, y, y.mean(1), rstd, gamma, ALPHA)['dy'])


def test_mask_at_zero_and_nan():
  h = np.array([0.0, -0.0, np.nan, 1e-30, -1.0])
  np.testing.assert_array_equal(N.mask_factor(h, 0.25), [0.25, 0.25, 0.25, 1.0, 0.25])


def torch_bn(y, gamma, beta, eps):
  mean = y.mean(dim=0)
  var = ((y - mean)**2).mean(dim=0)
  return (y - mean) * torch.rsqrt(var + eps) * gamma + beta, mean, var


@pytest.mark.parametrize('f16', [False, True])
@pytest.mark.parametrize('rows,C,act', [(257, 5, 1), (40, 30, 0), (600, 12, 1)])
def test_bn_is_autograd_of_a_biased_variance_batch_norm(rows, C, act, f16):
  y, gamma, beta, dout = N.bn_recipe(4, rows, C, f16)
  alpha = ALPHA if act else 1.0
  yt, gt, bt = t64(y, True), t64(gamma, True), t64(beta, True)
  t, mean, var = torch_bn(yt, gt, bt, EPS)
  h_ref = torch.maximum(t, alpha * t)
  mm, mv = np.full(C, 0.25), np.full(C, 2.0)
  mom = R.f32(0.99)
  s = N.bn_stats(y, mom, mm, mv)
  close(s['mean'], mean.detach().numpy())
  close(s['var'], var.detach().numpy())
  close(s['mm'], 0.25 * mom + (1 - mom) * mean.detach().numpy())
  close(s['mv'], 2.0 * mom + (1 - mom) * var.detach().numpy())
  hr, _ = N.bn_apply(y, s['mean'], s['var'], gamma, beta, EPS, alpha)
  close(hr, h_ref.detach().numpy())
  h = R.round_act(hr, f16)
  N.plant_mask_zeros(h, dout)
  mask = np.where(h > 0, 1.0, alpha) if act else np.ones_like(h)
  (t * t64(dout * mask)).sum().backward()
  b = N.bn_bwd(dout, h if act else None, y, s['mean'], s['var'], gamma, EPS, alpha, act)
  scale = np.abs(dout).sum(axis=0).max() / np.sqrt(EPS)
  close(b['dgamma'], gt.grad.numpy(), scale)
  close(b['dbeta'], bt.grad.numpy(), scale)
  close(b['dy'], yt.grad.numpy(), np.abs(b['dy']).max() + np.abs(dout).max() / np.sqrt(EPS))
  # handed the sums, the statement evaluates dy with them
  b2 = N.bn_bwd(dout, h if act else None, y, s['mean'], s['var'], gamma, EPS, alpha, act,
                dgamma=b['dgamma'], dbeta=b['dbeta'])
  np.testing.assert_array_equal(b2['dy'], b['dy'])
  assert (b2['e_dy'] <= b['e_dy']).all()


@pytest.mark.parametrize('f16', [False, True])
@pytest.mark.parametrize('nB,w,C,seg', [(7, 2, 8, 2), (9, 8, 33, 1), (11, 64, 6, 2)])
def test_unshuffle_mask_is_the_adjoint_of_the_shuffle(nB, w, C, seg, f16):
  e, h, shifts = N.unshuffle_recipe(5, nB, w, C, seg, f16)
  assert nB % seg or seg == 1
  pre = t64(np.where(h > 0, h, h / ALPHA), True)  # lrelu(pre) has the signs of h
  (shuffle_batch(O.leaky_relu(pre, ALPHA), shifts, seg) * t64(e)).sum().backward()
  delta, exact = N.unshuffle_mask(e, h, shifts, seg, ALPHA)
  np.testing.assert_allclose(delta, pre.grad.numpy(), rtol=RTOL, atol=0)
  # the zeros of h take alpha, whatever their sign
  src = np.zeros_like(e)
  for b in range(nB):
    np.add.at(src[b], W.shuffle_src(np.arange(w), int(shifts[b // seg]), w), e[b])
  np.testing.assert_array_equal(delta[:, :, :2], src[:, :, :2] * ALPHA)
  # exact ties of the activation type are among the sums, and they are `exact`
  a, b = N.tie_values(f16)
  ties = delta[:, :, 2] == a + b
  assert (ties.any() or w == 2) and exact[:, :, 2].all()  # (w = 2: no row has two sources)
  assert (R.round_act(delta[:, :, 2][ties], f16) == 2.0).all()  # half to even
  # no shifts: the mask alone
  d0, _ = N.unshuffle_mask(e, h, None, seg, ALPHA)
  np.testing.assert_array_equal(d0, e * np.where(h > 0, 1.0, ALPHA))


# ---------------------------------------------------------------------------
# the bars
# ---------------------------------------------------------------------------
LN_CAP_SHAPES = [(64, 5), (64, 30), (64, 102), (64, 320), (17, 40), (64, 500)]


@pytest.mark.parametrize('f16', [False, True])
@pytest.mark.parametrize('rows,C', LN_CAP_SHAPES)
def test_ln_two_pass_bars_are_no_looser_than_the_one_pass_bars(rows, C, f16):
  """swconv_ref.layernorm_bounds bars the fused epilogue's E[v^2] - mean^2 form; with
  no error in the pre-activation (err = 0) it is the bar of a one-pass evaluation of
  the same input.  The two-pass bars must not exceed it anywhere."""
  y, gamma, beta, _ = N.ln_recipe(6, rows, C, f16, big=False)
  f = N.ln_fwd(y, gamma, beta, EPS, ALPHA, f16)
  e_h, e_mean, e_rstd = S.layernorm_bounds(y, 0.0, gamma, beta, EPS, ALPHA, f16)
  assert (f['e_mean'] <= e_mean).all()
  assert (f['e_rstd'] <= e_rstd).all()
  assert (f['e_h'] <= e_h).all()


@pytest.mark.parametrize('f16', [False, True])
@pytest.mark.parametrize('rows,C', LN_CAP_SHAPES)
def test_ln_bars_are_below_the_old_tolerances(rows, C, f16):
  """Old test: h rtol = atol = 1e-2; dy 2e-2; dgamma / dbeta 1e-3 (allclose: atol + rtol
  |ref|).  An activation's bar is the derived f32 bar plus the store's ulp."""
  y, gamma, beta, dh = N.ln_recipe(7, rows, C, f16, big=False)
  f = N.ln_fwd(y, gamma, beta, EPS, ALPHA, f16)
  assert (f['e_h'] + R.ulp_act(f['h'], f16) < 1e-2 + 1e-2 * np.abs(f['h'])).all()
  h = R.round_act(f['h'], f16)
  N.plant_mask_zeros(h, dh)
  mean32 = f['mean'].astype(np.float32).astype(np.float64)
  rstd32 = f['rstd'].astype(np.float32).astype(np.float64)
  b = N.ln_bwd(dh, h, y, mean32, rstd32, gamma, ALPHA)
  assert (b['e_dy'] + R.ulp_act(b['dy'], f16) < 2e-2 + 2e-2 * np.abs(b['dy'])).all()
  assert (b['e_dgamma'] < 1e-3 + 1e-3 * np.abs(b['dgamma'])).all()
  assert (b['e_dbeta'] < 1e-3 + 1e-3 * np.abs(b['dbeta'])).all()
  _, e_dbias = N.dbias(R.round_act(b['dy'], f16))
  assert (e_dbias < 1e-4 + 1e-4 * np.abs(N.dbias(R.round_act(b['dy'], f16))[0])).all()


@pytest.mark.parametrize('f16', [False, True])
@pytest.mark.parametrize('rows,C,centre,spread', [(3000, 102, 50.0, 1.0),
                                                  (70000, 64, -200.0, 2.0),
                                                  (517, 320, 50.0, 50.0)])
def test_bn_off_centre_bars_are_below_the_old_tolerances(rows, C, centre, spread, f16):
  """Old test (its three shapes, in its pitch of 32 channels): variance rtol 1e-4 on channels
  with |mean| / std of 50 to 100 before the values are rounded to the activation type.
  (Its rtol 2e-6 on the mean is not capped: the bar of the f32 sum over the P blocks, P U
  |mean|, passes it from a few dozen blocks on.)"""
  y = N.off_centre_recipe(14, rows, C, centre, spread, f16)
  s = N.bn_stats(y, R.f32(0.99), rlanes=N.bn_row_lanes(S.pitch32(C)))
  assert (s['e_var'] < 1e-4 * s['var']).all()
  # the order-free bar of the same sums is looser, never tighter
  s0 = N.bn_stats(y, R.f32(0.99))
  assert (s0['e_var'] >= s['e_var']).all() and (s0['e_mean'] >= s['e_mean']).all()


@pytest.mark.parametrize('f16', [False, True])
@pytest.mark.parametrize('rows,C,act', [(3000, 102, 1), (517, 320, 0), (64, 16, 1)])
def test_bn_bars_are_below_the_old_tolerances(rows, C, act, f16):
  """Old test (its three shapes): mean rtol 1e-4 + atol 1e-5, var rtol 1e-3, the moving pair
  rtol 1e-5 (+ 1e-6 for the mean), h 1e-2, dgamma / dbeta 2e-3 of the largest gradient.  The
  constant column (var = 0) has no relative cap on var: its bar is held against eps."""
  y, gamma, beta, dout = N.bn_recipe(8, rows, C, f16)
  alpha = ALPHA if act else 1.0
  mm, mv = np.full(C, 0.25), np.full(C, 2.0)
  s = N.bn_stats(y, R.f32(0.99), mm, mv, rlanes=N.bn_row_lanes(S.pitch32(C)))
  assert (s['e_mean'] < 1e-5 + 1e-4 * np.abs(s['mean'])).all()
  assert (s['e_var'][:C - 1] < 1e-3 * s['var'][:C - 1]).all()
  assert s['var'][C - 1] == 0 and s['e_var'][C - 1] < 1e-3 * EPS
  assert (s['e_mm'] < 1e-6 + 1e-5 * np.abs(s['mm'])).all()
  assert (s['e_mv'] < 1e-5 * np.abs(s['mv'])).all()
  mean32 = s['mean'].astype(np.float32).astype(np.float64)
  var32 = s['var'].astype(np.float32).astype(np.float64)
  hr, e_h = N.bn_apply(y, mean32, var32, gamma, beta, EPS, alpha)
  assert (e_h + R.ulp_act(hr, f16) < 1e-2 + 1e-2 * np.abs(hr)).all()
  h = R.round_act(hr, f16)
  N.plant_mask_zeros(h, dout)
  b = N.bn_bwd(dout, h if act else None, y, mean32, var32, gamma, EPS, alpha, act)
  for k in ('dgamma', 'dbeta'):
    assert (b['e_' + k] < 2e-3 * np.abs(b[k]).max() + 2e-3 * np.abs(b[k])).all()
  assert (b['e_dy'] + R.ulp_act(b['dy'], f16) < 2e-2 + 2e-2 * np.abs(b['dy'])).all()
