"""CPU checks of tests/wgrad_ref.py: the float64 statements the GPU parity tests
of tests/test_hip_wgrad.py compare cg_wgrad / cg_pack_weights with are tied here
to independent ones (float64 autograd of the oracle's convolutions behind its
PhaseShuffle, hip_utils.numpy_pack), and the data recipes are shown to be able to
fail: f32 evaluations of the reference in several summation orders lie within
the bar, three kinds of mutants of the reference move at least half of the
outputs they touch by 20 bars at every shape the GPU runs on rounded reals, and
the exact recipe's sums are exact in f32."""
import numpy as np
import pytest
import torch

import oracle as O
import hip_utils as H
import pointwise_ref as R
import wgrad_ref as W

F64 = torch.float64
F16 = pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'f16'])


def _shuffle_batch(x, shifts, seg):
  if shifts is None:
    return x
  return torch.cat([O.phase_shuffle(x[b:b + 1], shifts[b // seg])
                    for b in range(x.shape[0])])


@pytest.mark.parametrize('G', [W.geom(5, 8, 8, 3, 4, W.MIXED5, 1),
                               W.geom(3, 16, 24, 2, 5, (31, -31), 2),
                               W.geom(2, 8, 2, 4, 3), W.geom(3, 4, 12, 5, 2, (-3, 3, 0)),
                               W.geom(2, 32, 20, 3, 3, (1, -1))], ids=str)
def test_wgrad_statement_under_autograd_f64(G):
  """dw is the weight gradient of Conv1D(stride 2, 'same') behind PhaseShuffle, and
  -- x and g swapping sides -- of the stride-2 transposed convolution."""
  rng = np.random.RandomState(3)
  stride, Lx, off = W.stride_of(G)
  x, g = rng.randn(G.nB, Lx, G.Cx), rng.randn(G.nB, G.Lu, G.Cg)
  Wt = torch.zeros(G.taps, G.Cx, G.Cg, dtype=F64, requires_grad=True)
  xs = _shuffle_batch(torch.tensor(x), G.shifts, G.seg)
  (O.conv1d_same(xs, Wt, None, 2) * torch.tensor(g)).sum().backward()
  np.testing.assert_allclose(W.wgrad_of(G, x, g), Wt.grad.numpy(), rtol=1e-12, atol=1e-12)
  # the reflect gather itself
  np.testing.assert_array_equal(W.shuffled(x, G.shifts, G.seg), xs.numpy())
  # transposed convolution y = conv_T(h): dW[k][0][co][ci] pairs the long side (dy)
  # with the short side (h)
  Wtt = torch.zeros(G.taps, 1, G.Cx, G.Cg, dtype=F64, requires_grad=True)
  (O.conv1d_transpose_same(torch.tensor(g), Wtt, None, 2) * torch.tensor(x)).sum().backward()
  np.testing.assert_allclose(W.wgrad(x, g, G.taps, stride, off), Wtt.grad.numpy()[:, 0],
                             rtol=1e-12, atol=1e-12)


def test_dense_form_and_dbias():
  rng = np.random.RandomState(4)
  G = W.geom(3, 5, 1, 4, 6)
  x, g = rng.randn(3, 5, 4), rng.randn(3, 5, 6)
  np.testing.assert_allclose(W.wgrad_of(G, x, g)[0], np.einsum('blc,bld->cd', x, g),
                             rtol=1e-13)
  np.testing.assert_allclose(W.dbias(g, 7), g.reshape(15, 6)[:7].sum(0), rtol=1e-15)
  assert (W.dbias(g, 0) == 0).all()


def test_non_finite_values_follow_ieee_and_selection():
  G = W.geom(1, 8, 4, 2, 3)  # Lx 16, off -1: tap 0 of u = 0 reads row -1 (padding)
  x, g = np.ones((1, 16, 2)), np.ones((1, 8, 3))
  g[0, 0, 1] = np.nan      # meets padding under tap 0: selected away there
  dw = W.wgrad_of(G, x, g)
  assert np.isfinite(dw[0]).all() and np.isnan(dw[1:, :, 1]).all()
  assert np.isfinite(dw[:, :, [0, 2]]).all()
  x[0, 5, 0], g[0, 0, 1], g[0, 3, 2] = np.inf, 1.0, 0.0
  dw = W.wgrad_of(G, x, g)  # row 5 = 2 u - 1 + tap: (tap 0, u 3), (tap 2, u 2)
  assert np.isnan(dw[0, 0, 2]) and dw[0, 0, 0] == np.inf and dw[2, 0, 2] == np.inf
  assert np.isfinite(dw[[1, 3]]).all() and np.isfinite(dw[:, 1]).all()
  assert np.isnan(W.dbias(np.array([[[1.0], [np.nan]]]), 2)).all()
  assert W.dbias(np.array([[[1.0], [np.nan]]]), 1)[0] == 1.0
  # unread rows really are unread, reflected rows really come from the mirror
  for s, w in ((3, 16), (-3, 16), (15, 16), (-15, 16), (0, 16)):
    src = W.shuffle_src(np.arange(w), s, w)
    assert src.min() >= 0 and src.max() < w
    assert not set(src.tolist()) & set(W.unread_rows(s, w))
    assert len(set(src.tolist())) + len(W.unread_rows(s, w)) == w
    assert len(W.reflected_rows(s, w)) == abs(s)
    np.testing.assert_array_equal(src, O.phase_shuffle_index(w, s))
  assert W.unread_rows(3, 16) == [0, 1, 2] and W.unread_rows(-3, 16) == [13, 14, 15]
  assert W.unread_rows(15, 16) == [] and W.unread_rows(0, 16) == []


def test_flush():
  f = W.flush(np.array([-2.0**-24, 2.0**-15, -2.0**-14, 1.0]))
  assert np.signbit(f[0]) and f[0] == 0 and f[1] == 0 and f[2] == -2.0**-14 and f[3] == 1


# ---------------------------------------------------------------------------
# f32 evaluations of the reference
# ---------------------------------------------------------------------------
def _tap_operands(G, x, g):
  """Per tap the (rows, cx) / (rows, cg) operand pair in (b, u) order, padding
  rows as exact zeros (what a kernel stages)."""
  stride, Lx, off = W.stride_of(G)
  xs = W.shuffled(x, G.shifts, G.seg)
  u = np.arange(G.Lu)
  for tap in range(G.taps):
    r = stride * u + off + tap
    ok = (r >= 0) & (r < Lx)
    X = np.where(ok[None, :, None], xs[:, np.clip(r, 0, Lx - 1), :], 0.0)
    yield X.reshape(-1, G.Cx).astype(np.float32), g.reshape(-1, G.Cg).astype(np.float32)


def _f32_orders(X, Gm):
  """The same sum in f32: one matmul; 32-row stages added in order; three
  interleaved splits of 64-row tiles, joined last to first."""
  n = X.shape[0]
  yield X.T @ Gm
  acc = np.zeros((X.shape[1], Gm.shape[1]), np.float32)
  for r0 in range(0, n, 32):
    acc = acc + X[r0:r0 + 32].T @ Gm[r0:r0 + 32]
  yield acc
  parts = []
  for z in range(3):
    a = np.zeros_like(acc)
    for t in range(z, -(-n // 64), 3):
      for r in range(t * 64, min(n, t * 64 + 64)):  # row by row
        a = a + np.outer(X[r], Gm[r]).astype(np.float32)
    parts.append(a)
  yield (parts[2] + parts[1]) + parts[0]


REALS = W.real_geoms()


@F16
@pytest.mark.parametrize('G', REALS, ids=str)
def test_real_recipe_meets_and_needs_its_bar(G, f16):
  """(a) f32 evaluations in three orders lie inside acc_bound.  (b) The cap: each
  mutant of the reference -- one 32-row K-step dropped, one tap reading one row
  further, one reflected row taken unshuffled -- moves at least half of the
  outputs it touches by at least 20 bars, for EVERY K-step, tap and reflected
  row (rows whose mirror image is themselves excepted: nothing changes)."""
  x, g = W.real_recipe(G, f16)
  np.testing.assert_array_equal(R.round_act(x, f16), x)
  np.testing.assert_array_equal(R.round_act(g, f16), g)
  assert G.Cx < 8 or (np.signbit(x[:, 0, 1]).all() and (x[:, 0, :2] == 0).all())
  want, bar = W.wgrad_of(G, x, g), W.acc_bound(G, x, g)
  if G.Cx * G.Cg <= 40 * 65:
    for tap, (X, Gm) in enumerate(_tap_operands(G, x, g)):
      for got in _f32_orders(X, Gm):
        assert (np.abs(got.astype(np.float64) - want[tap]) <= bar[tap]).all()
  db, dbar = W.dbias(g, W.rows_of(G)), W.dbias_bound(G, g, W.rows_of(G))
  got = g.reshape(-1, G.Cg).astype(np.float32).sum(axis=0).astype(np.float64)
  assert (np.abs(got - db) <= dbar).all()

  def enough(change, where=None):
    hit = np.abs(change) >= 20 * bar
    return (hit if where is None else hit[where]).mean() >= 0.5

  stride, Lx, off = W.stride_of(G)
  M = W.rows_of(G)
  for r0 in range(0, M, 32):  # one K-step of any tile dropped
    keep = np.zeros(M, bool)
    keep[r0:r0 + 32] = True
    touched = W.wgrad_of(G, np.abs(x) + 1, np.abs(g) + 1, keep) > 0
    assert enough(W.wgrad_of(G, x, g, keep), touched), ('K-step', r0)
  if G.taps > 1:  # one tap reads one row further
    wide = W.wgrad(x, g, G.taps + 1, stride, off, G.shifts, G.seg)
    for tap in range(G.taps):
      assert (np.abs(wide[tap + 1] - want[tap]) >= 20 * bar[tap]).mean() >= 0.5, tap
  if G.shifts:
    for b in range(G.nB):
      s = G.shifts[b // G.seg]
      for t in W.reflected_rows(s, Lx):
        src = int(W.shuffle_src(t, s, Lx))
        if src == t:
          continue
        for tap in range(G.taps):
          u2 = t - off - tap
          if u2 % stride or not 0 <= u2 // stride < G.Lu:
            continue
          change = np.outer(x[b, t] - x[b, src], g[b, u2 // stride])
          assert (np.abs(change) >= 20 * bar[tap]).mean() >= 0.5, (b, t, tap)




@F16
@pytest.mark.parametrize('G', REALS + W.EXACT_ONLY, ids=str)
def test_exact_recipe_is_exact_in_f32_and_uses_every_bit(G, f16):
  x, g = W.exact_recipe(G, f16)
  np.testing.assert_array_equal(R.round_act(x, f16), x)
  np.testing.assert_array_equal(R.round_act(g, f16), g)
  ux, ug = W.exact_unit(f16)
  # every significand bit of x varies; g is 0, +-1 or a negative power of two
  xi = (np.abs(x) / ux).astype(np.int64)
  s = 11 if f16 else 8
  assert (xi >> (s - 1) == 1).all()
  if x.size >= 4096:
    assert all(0.3 < ((xi >> k) & 1).mean() < 0.7 for k in range(s - 1))
  assert set(np.unique(np.abs(g))) <= {0.0, 1.0, 0.5, 0.25, 0.125}
  assert (g == 0).mean() < 0.95 and np.abs(g).min() == 0 and np.abs(g[g != 0]).min() >= ug
  # every partial sum of every subset is an integer below 2^24 product units, the
  # value an adding call starts from (4.0) included
  units = (W.wgrad_of(G, np.abs(x), np.abs(g)) + 4.0) / (ux * ug)
  assert units.max() < 2.0**24
  assert (W.dbias(np.abs(g), W.rows_of(G)) + 4.0).max() / ug < 2.0**24
  want = W.wgrad_of(G, x, g)
  if G.Cx * G.Cg <= 40 * 65 and W.rows_of(G) <= 1200:
    for tap, (X, Gm) in enumerate(_tap_operands(G, x, g)):
      a, b, _ = _f32_orders(X, Gm)
      np.testing.assert_array_equal(a.astype(np.float64), want[tap])
      np.testing.assert_array_equal(b.astype(np.float64), want[tap])
  # an operand bit matters: clearing the lowest significand bit of x changes dw
  low = np.where(xi & 1, x - np.sign(x) * ux, x)
  assert (W.wgrad_of(G, low, g) != want).mean() > 0.5


def test_subnormal_recipe():
  G = W.BIAS_RING
  for which in ('x', 'g'):
    x, g = W.subnormal_recipe(G, which)
    np.testing.assert_array_equal(R.round_act(x, True), x)
    np.testing.assert_array_equal(R.round_act(g, True), g)
    sub = x if which == 'x' else g
    assert 0 < np.abs(sub).min() and np.abs(sub).max() < 2.0**-14
    want = W.wgrad_of(G, x, g)
    assert (W.wgrad_of(G, np.abs(x), np.abs(g)) / 2.0**-16).max() < 2.0**24
    # flushed, everything is an exact zero: far outside the bar of the kept statement
    fl = W.wgrad_of(G, W.flush(x), W.flush(g))
    assert (fl == 0).all()
    assert (np.abs(want) > 20 * W.acc_bound(G, x, g)).mean() > 0.9
    if which == 'g':
      db = W.dbias(g, 128)
      assert (np.abs(db) > 20 * W.dbias_bound(G, g, 128)).mean() > 0.5
      assert (W.dbias(W.flush(g), 128) == 0).all()


# ---------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('taps,C,N,Cx,CK', [(1, 40, 70, 64, 32), (8, 33, 130, 64, 32),
                                            (24, 102, 65, 128, 32), (2, 64, 1, 64, 64)])
def test_pack_plain_layout_is_numpy_pack(taps, C, N, Cx, CK):
  rng = np.random.RandomState(5)
  src = rng.randn(taps, C, N).astype(np.float32)
  d = W.PackDesc(taps, C, N, Cx, CK)
  np.testing.assert_array_equal(W.logical(src, d), src)
  for f16 in (False, True):
    got = W.pack(src, d, f16)
    assert got.size == W.packed_elems(N, taps, Cx, CK)
    ref = H.numpy_pack(R.round_act(src, f16), Cx, CK)  # whole 64-column tiles
    got = got.reshape(-(-N // 128) * 128, -1)
    np.testing.assert_array_equal(got[:ref.shape[0]], ref)
    assert (got[ref.shape[0]:] == 0).all()


def test_pack_orders_strides_and_narrow_chunk():
  rng = np.random.RandomState(6)
  taps, C, N, Cx = 8, 102, 5, 128
  src = rng.randn(taps, C, N).astype(np.float32)
  plain = W.pack(src, W.PackDesc(taps, C, N, Cx), False).reshape(128, 4, 32, 8)
  pm = W.pack(src, W.PackDesc(taps, C, N, Cx, parity_major=1), False).reshape(128, 4, 32, 8)
  order = [0, 2, 4, 6, 1, 3, 5, 7]
  for p, tap in enumerate(order):
    np.testing.assert_array_equal(pm[:, :, 4 * p:4 * p + 4], plain[:, :, 4 * tap:4 * tap + 4])
  nl = W.pack(src, W.PackDesc(taps, C, N, Cx, parity_major=1, narrow_last=1),
              False).reshape(128, 4, 32, 8)
  np.testing.assert_array_equal(nl[:, :3], pm[:, :3])
  for p in range(8):
    np.testing.assert_array_equal(nl[:, 3, (p // 4) * 16 + p % 4], pm[:, 3, 4 * p])
  assert np.count_nonzero(nl[:, 3]) == np.count_nonzero(pm[:, 3]) == 8 * 6 * N
  # a transposed source and a phase walk (tap0, tap_step) over the same numbers
  srcT = np.ascontiguousarray(src.transpose(0, 2, 1))
  dT = W.PackDesc(taps, C, N, Cx, s_tap=C * N, s_c=1, s_n=C)
  np.testing.assert_array_equal(W.pack(srcT, dT, False), plain.ravel())
  ph = W.PackDesc(4, C, N, Cx, tap0=7, tap_step=-2)
  np.testing.assert_array_equal(W.logical(src, ph), src[[7, 5, 3, 1]])
  # admissibility, from the header
  ok = lambda **kw: W.pack_admissible(W.PackDesc(**dict(dict(
      taps=8, C_real=104, N_real=4, Cx=128, parity_major=1, narrow_last=1), **kw)))
  assert ok() and ok(C_real=97) and not ok(C_real=96) and not ok(C_real=105)
  assert not ok(parity_major=0) and not ok(Cx=32, C_real=8) and ok(taps=6)
  assert not ok(taps=2) and not ok(taps=4) and not ok(taps=34) and ok(taps=32)
  assert not ok(CK=64) and not W.pack_admissible(W.PackDesc(2, 9, 4, 8))


def test_gmode_table():
  for cx, cg, mode in W.GROUPING:
    assert W.gmode_of(cx, cg, 4, 128, W.pitch_of(cx), 256, W.pitch_of(cg)) == mode
