"""Float64 parity of the per-timestep Dense entry points of
calciumgan_amd/csrc/dense_rows.hip -- cg_dense_rows (register and LDS-panel
form), cg_dense_rows_interp, cg_dense_rows_act, cg_dense_wgrad -- in both
precision builds, at the smallest shapes that reach each code path (every K,
ragged tails, several panels, row blocks that wrap the capped grids).

Every case compares ONE entry point with the float64 statement of
tests/dense_ref.py (tied to autograd / the oracle in tests/test_dense_ref.py) on
its recipes: random reals (rounding happens), exact sums that are not
representable in the activation type (bit equality, ties, fp16 overflow), and
special values.  Outputs are pre-filled with a sentinel and over-allocated; what
the contract says is not read is NaN.  Bars: bit-equal; dense_ref.acc_bound for
an f32 contraction; the sigmoid's slope times it plus the project's bar of that
epilogue; one activation ulp on top where the result is rounded -- never a
measured number."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from calciumgan_amd import _lib
from calciumgan_amd import geometry as geo

import dense_ref as D
import hip_utils as H
import pointwise_ref as R
import test_hip_pointwise as P

pytestmark = pytest.mark.gpu

EINVAL = _lib.CG_EINVAL
GUARD = 3  # rows allocated past the last one a launch may store


@pytest.fixture(autouse=True)
def _back_to_bf16():
  yield
  _lib.use('bf16')


@pytest.fixture(params=['bf16', 'f16'])
def precision(request):
  """Selects the build; the tests read it as `f16` (bool)."""
  _lib.use(request.param)
  return request.param == 'f16'


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def pack_dense(W):
  """The 1-tap operand (CK 32) of W (K, N) float64 holding f32 values, packed
  by the active build."""
  K, N = W.shape
  src = P.dev32(W)
  return H.pack(src, [(0, 1, 0, N, 1)], K, N, K, 32, 1)


def zero_bits(t):
  """Every element is +0."""
  iv = torch.int16 if t.element_size() == 2 else torch.int32
  return not bool(t.contiguous().view(iv).ne(0).any())


def finite_rows(x):
  return np.isfinite(x).all(axis=1)


def assert_like_ieee(got, want, what=''):
  """Non-finite float64 results: the same NaN pattern, the same infinities."""
  g = P.host(got) if torch.is_tensor(got) else got
  assert np.array_equal(np.isnan(g), np.isnan(want)), what
  inf = np.isinf(want)
  assert np.array_equal(g[inf], want[inf]), what


@functools.lru_cache(maxsize=1)
def real_case(rows, K, N, f16):
  """The real recipe and its float64 results, computed once per shape."""
  x, W32, Wq, bias = D.real_recipe(1000 + rows % 997 + K + N, rows, K, N, f16)
  return dict(x=x, W32=W32, Wq=Wq, bias=bias, t0=D.dense_rows(x, Wq),
              acc0=D.acc_bound(x, Wq))


def run_dense_rows(xd, op, bias, rows, K, N, Cy, epi):
  y = P.sent32(rows + GUARD, Cy)
  bd = P.dev32(bias) if bias is not None else None
  _lib.call('cg_dense_rows', H.p(xd), H.p(op.buf), H.p(bd), H.p(y), rows, K, N, Cy,
            epi, H.stream())
  H.sync()
  return y


def check_dense_rows(rows, K, N, Cy, f16, combos=((3, True), (0, True), (3, False),
                                                  (0, False))):
  c = real_case(rows, K, N, f16)
  xd, op = P.dev_act(c['x'], f16), pack_dense(c['W32'])
  for epi, with_bias in combos:
    bias = c['bias'] if with_bias else None
    y = run_dense_rows(xd, op, bias, rows, K, N, Cy, epi)
    t = c['t0'] + (bias[None, :] if with_bias else 0.0)
    acc = c['acc0'] + ((K + 1) * 2.0**-23 * np.abs(bias)[None, :] if with_bias else 0.0)
    what = 'epi {} bias {}'.format(epi, with_bias)
    if epi == 3:
      s = D.sigmoid(t)
      P.assert_f32(y[:rows, :N], s, D.sigmoid_bar(acc, s), what)
    else:
      P.assert_f32(y[:rows, :N], t, acc, what)
    assert zero_bits(y[:rows, N:]), what      # channel padding: exactly +0
    assert P.is_sentinel(y[rows:]), what      # nothing past the last row
  return c, xd, op


# ---------------------------------------------------------------------------
# cg_dense_rows
# ---------------------------------------------------------------------------
REG = [(1, 32, 1, 4), (17, 64, 40, 40), (50, 96, 70, 72), (1000, 128, 102, 104),
       (1000, 128, 128, 128)]
# a wave of the register form takes a second block beyond 512 x 4 x 16 = 32768
# rows: three blocks here, the last one ragged
REG_WRAP = (2 * 32768 + 17, 32, 6, 8)


@pytest.mark.parametrize('rows,K,N,Cy', REG + [REG_WRAP])
def test_dense_rows_register_form(rows, K, N, Cy, precision):
  check_dense_rows(rows, K, N, Cy, precision)


WIDE = [(33, 256, 130, 136), (77, 384, 200, 200), (1000, 512, 512, 512),
        (100, 128, 300, 304)]
# the wide kernel's stride is (grid / 8 / panels) * 8 * 4 blocks of 32 rows: 8192
# rows at 512 -> 512 (4 panels), 10240 at 512 -> 300 (3 panels), 65536 at K = 128, N
# <= 128 (64 workgroups per XCD)
WIDE_WRAP = [(2 * 8192 + 33, 512, 512, 512), (2 * 10240 + 1, 512, 300, 304)]
ACT_ONLY = [(9, 128, 102, 128), (65536 + 33, 128, 8, 8)]


def check_act_real(c, xd, op, rows, K, N, Cy, f16):
  ya = P.sent_act((rows + GUARD, Cy), f16)
  _lib.call('cg_dense_rows_act', H.p(xd), H.p(op.buf), H.p(ya), rows, K, N, Cy,
            H.stream())
  H.sync()
  P.assert_act(ya[:rows, :N], c['t0'], f16, f32_err=c['acc0'])
  assert zero_bits(ya[:rows, N:])
  assert P.is_sentinel(ya[rows:])


@pytest.mark.parametrize('rows,K,N,Cy', WIDE + WIDE_WRAP)
def test_dense_rows_wide_form_and_act(rows, K, N, Cy, precision):
  """cg_dense_rows (LDS-panel form, both epilogues, with and without bias) and
  cg_dense_rows_act on the same operands."""
  f16 = precision
  combos = ((3, True), (0, False)) if rows > 10000 else ((3, True), (0, True),
                                                         (3, False), (0, False))
  c, xd, op = check_dense_rows(rows, K, N, Cy, f16, combos)
  check_act_real(c, xd, op, rows, K, N, geo.pitch(N), f16)


@pytest.mark.parametrize('rows,K,N,Cy', ACT_ONLY)
def test_dense_rows_act_real(rows, K, N, Cy, precision):
  f16 = precision
  c = real_case(rows, K, N, f16)
  check_act_real(c, P.dev_act(c['x'], f16), pack_dense(c['W32']), rows, K, N, Cy, f16)


@pytest.mark.parametrize('rows,K,N,Cy', [(r, k, n, geo.pitch(n)) for r, k, n, _ in
                                         WIDE + WIDE_WRAP] + ACT_ONLY)
def test_dense_rows_act_exact_sums_round_to_nearest_even(rows, K, N, Cy, precision):
  """Sums that are exact in f32 and (mostly) not representable in the activation
  type: the stored bits are round_act(exact) -- four planted exact ties go to
  the even neighbour, fp16 sums beyond +-65504 to +-inf."""
  f16 = precision
  x, W, ties, over = D.exact_recipe(2000 + rows % 997 + K + N, rows, K, N, f16)
  xd, op = P.dev_act(x, f16), pack_dense(W)
  ya = P.sent_act((rows + GUARD, Cy), f16)
  _lib.call('cg_dense_rows_act', H.p(xd), H.p(op.buf), H.p(ya), rows, K, N, Cy,
            H.stream())
  H.sync()
  want = D.dense_rows_act(x, W, f16)
  P.assert_bits(ya[:rows, :N], want, f16)
  got = P.host(ya[:rows, :N])
  ux, uw = D.exact_units(f16)
  T = 2**11 if f16 else 2**8
  for j, (r, col) in enumerate(ties):
    assert abs(got[r, col]) == [T, T + 4, T + 4, T + 8][j] * ux * uw
  if f16:
    assert got[over[0]] == np.inf and got[over[1]] == -np.inf
  assert zero_bits(ya[:rows, N:])
  assert P.is_sentinel(ya[rows:])
  # the f32 output holds the exact sums
  if K > 128 or N > 128:
    cf = (N + 7) // 8 * 8
    y = run_dense_rows(xd, op, None, rows, K, N, cf, 0)
    np.testing.assert_array_equal(P.host(y[:rows, :N]), D.dense_rows(x, W))


# ---------------------------------------------------------------------------
# cg_dense_rows_interp
# ---------------------------------------------------------------------------
INTERP_REG = [(1, 1, 16, 32, 1), (8, 1, 32, 96, 97), (5, 3, 64, 128, 102)]
# register form: 2048 waves; B L / 16 = 3072 blocks > 2048 -- and the (block,
# update) items of a wave alternate between the two fragment sets
INTERP_REG_WRAP = (2, 3, 16384, 32, 6)
INTERP_WIDE = [(2, 3, 32, 512, 512), (3, 1, 64, 256, 200), (1, 2, 16, 128, 130)]


def real_batch(rng, rows, N, Cr, f16):
  """f32 `real` (rows, Cr) in [0, 1) with NaN in the channels [N, Cr) -- never read
  -- and values whose rounding shows (ties, half the smallest subnormal, beyond
  fp16's range) from the start of row 0."""
  tiny = R.act_limits(f16)[0]
  real = np.full((rows, Cr), np.nan, np.float32)
  v = rng.rand(rows, N).astype(np.float32)
  vals = np.array([0.0, -0.0, tiny / 2, 1 + 2.0**-8, 1 + 3 * 2.0**-8, 1 + 2.0**-11,
                   1 + 3 * 2.0**-11, 1e5, -1e5], np.float32)
  flat = v.reshape(-1)
  k = min(len(vals), flat.size)
  flat[:k] = vals[:k]
  real[:, :N] = v
  return real


@pytest.mark.parametrize('n,B,L,K,N', INTERP_REG + [INTERP_REG_WRAP] + INTERP_WIDE)
def test_dense_rows_interp(n, B, L, K, N, precision):
  """[real | fake_k | x^_k] against the three-step float64 statement: the real
  segment bit-equal to round_act(real); fake within the contraction's (and the
  sigmoid's) bar and one rounding; x^ formed from the UNROUNDED values, within
  |1 - alpha| err_fake + 3 ulp_f32 and one rounding.  alpha planted at 0, 1 and
  1/2; alpha == NULL leaves the third segment alone."""
  f16 = precision
  wide = K > 128 or N > 128
  Cp = geo.pitch(N) if wide else 128
  Cr = N + 4 if N % 4 == 0 else N + 3
  rows = n * B * L
  c = real_case(rows, K, N, f16)
  rng = np.random.RandomState(3000 + rows % 997 + K + N)
  real = real_batch(rng, B * L, N, Cr, f16)
  alpha = rng.rand(n * B).astype(np.float32)
  alpha[:3] = [0.0, 1.0, 0.5][:min(3, n * B)]
  xd, op = P.dev_act(c['x'], f16), pack_dense(c['W32'])
  real_d, alpha_d = P.dev32(real), P.dev32(alpha)
  r64 = real[:, :N].astype(np.float64).reshape(B, L, N)
  combos = ((3, True),) if rows > 10000 else ((3, True), (0, False))
  for epi, with_bias in combos:
    bias = c['bias'] if with_bias else None
    bd = P.dev32(bias) if with_bias else None
    t = c['t0'] + (bias[None, :] if with_bias else 0.0)
    acc = c['acc0'] + ((K + 1) * 2.0**-23 * np.abs(bias)[None, :] if with_bias else 0.0)
    if epi == 3:
      fake = D.sigmoid(t)
      err = D.sigmoid_bar(acc, fake)
    else:
      fake, err = t, acc
    fake, err = fake.reshape(n, B, L, N), err.reshape(n, B, L, N)
    for use_alpha in (True, False):
      x0 = [P.sent_act((3 * B + 1, L, Cp), f16) for _ in range(n)]
      ptrs = (ctypes.c_void_p * n)(*[t_.data_ptr() for t_ in x0])
      _lib.call('cg_dense_rows_interp', H.p(xd), H.p(op.buf), H.p(bd), H.p(real_d),
                H.p(alpha_d) if use_alpha else None, ptrs, n, B, L, K, N, Cr, Cp,
                epi, H.stream())
      H.sync()
      for k in range(n):
        what = 'epi {} alpha {} update {}'.format(epi, use_alpha, k)
        P.assert_bits(x0[k][:B, :, :N], r64, f16)
        P.assert_act(x0[k][B:2 * B, :, :N], fake[k], f16, f32_err=err[k])
        assert zero_bits(x0[k][:2 * B, :, N:]), what
        if use_alpha:
          a = alpha[k * B:(k + 1) * B].astype(np.float64)
          P.assert_act(x0[k][2 * B:3 * B, :, :N], R.interp(r64, fake[k], a), f16,
                       f32_err=D.xhat_err(a, r64, fake[k], err[k]))
          assert zero_bits(x0[k][2 * B:3 * B, :, N:]), what
          assert P.is_sentinel(x0[k][3 * B:]), what
        else:
          assert P.is_sentinel(x0[k][2 * B:]), what


# ---------------------------------------------------------------------------
# cg_dense_wgrad
# ---------------------------------------------------------------------------
def wgrad_forms(xd, gd, rows, Cx, Cg, cx, cg):
  """atomics onto a zeroed dW; the workspace form onto a sentinel dW with a
  NaN-filled workspace, twice -- the same bits.  Returns (atomics, ordered)."""
  need = _lib.load().cg_dense_wgrad_ws_elems(rows, cx, cg)
  assert need == D.wgrad_ws_elems(rows, cx, cg)
  outs = []
  for ordered in (False, True, True):
    # (the guard reaches as far as the padded channels' rows would: Cx x cg)
    dw = P.sent32(Cx * cg + GUARD)
    ws = None
    if ordered:
      ws = torch.full((need,), float('nan'), device=H.DEV)
    else:
      dw[:cx * cg] = 0.0
    _lib.call('cg_dense_wgrad', H.p(xd), H.p(gd), H.p(dw), rows, Cx, Cg, cx, cg,
              H.p(ws), need if ordered else 0, H.stream())
    H.sync()
    assert P.is_sentinel(dw[cx * cg:])
    outs.append(dw[:cx * cg].clone().reshape(cx, cg))
  assert torch.equal(P.bits(outs[1]), P.bits(outs[2]))
  # one float short: refused, dW untouched
  dw = P.sent32(cx * cg)
  ws = torch.full((need,), float('nan'), device=H.DEV)
  assert _lib.load().cg_dense_wgrad(H.p(xd), H.p(gd), H.p(dw), rows, Cx, Cg, cx, cg,
                                    H.p(ws), need - 1, H.stream()) == EINVAL
  H.sync()
  assert P.is_sentinel(dw)
  return outs[0], outs[1]


def nan_padded(v, pitch, f16):
  """(rows, C) values of the activation type -> device (rows, pitch), NaN in the
  channels past C."""
  full = np.full((v.shape[0], pitch), np.nan)
  full[:, :v.shape[1]] = v
  return P.dev_act(full, f16)


@pytest.mark.parametrize('rows,cx,cg', [(1, 1, 1), (31, 102, 102), (70, 32, 256),
                                        (1000, 130, 40), (4097, 102, 102)])
def test_dense_wgrad(rows, cx, cg, precision):
  """dW = x^T g: within the f32 sum's bound on rounded reals and exactly on small
  integers (every partial sum below 2^24: a dropped or doubled row shows whatever
  the bound has grown to).  The channels past C_real hold NaN: C_real bounds what
  is accumulated into dW."""
  f16 = precision
  Cx, Cg = geo.pitch(cx), geo.pitch(cg)
  x, g = D.wgrad_recipe(4000 + rows + cx, rows, cx, cg, f16)
  atom, order = wgrad_forms(nan_padded(x, Cx, f16), nan_padded(g, Cg, f16), rows, Cx,
                            Cg, cx, cg)
  want, bar = D.dense_wgrad(x, g), D.wgrad_bound(x, g)
  P.assert_f32(atom, want, bar, 'atomics')
  P.assert_f32(order, want, bar, 'ordered')
  rng = np.random.RandomState(4100 + rows + cg)
  xi = rng.randint(-3, 4, (rows, cx)).astype(np.float64)
  gi = rng.randint(-3, 4, (rows, cg)).astype(np.float64)
  assert 9 * rows < 2**24
  atom, order = wgrad_forms(nan_padded(xi, Cx, f16), nan_padded(gi, Cg, f16), rows,
                            Cx, Cg, cx, cg)
  np.testing.assert_array_equal(P.host(atom), D.dense_wgrad(xi, gi))
  np.testing.assert_array_equal(P.host(order), D.dense_wgrad(xi, gi))


# ---------------------------------------------------------------------------
# the packed operand
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,N', [(32, 1), (128, 102), (256, 200)])
def test_dense_operand_matches_numpy_layout(K, N, precision):
  """The 1-tap operand under the active build: round_act(W) in the layout of
  hip_utils.numpy_pack, the column padding (up to whole 128-column panels) zero."""
  f16 = precision
  rng = np.random.RandomState(5000 + K)
  W = (0.2 * rng.randn(K, N)).astype(np.float32)
  W[0, 0] = 1 + R.ulp_act(1.0, f16) / 2      # a tie: to the even neighbour, 1
  W[1, 0] = 1 + 3 * R.ulp_act(1.0, f16) / 2  # a tie: up, 1 + 2 ulp
  op = pack_dense(W.astype(np.float64))
  H.sync()
  assert op.buf.dtype == R.act_dtype(f16)
  exp = H.numpy_pack(R.round_act(W, f16)[None].astype(np.float32), K, 32)
  got = op.buf.double().cpu().numpy().reshape(-1, exp.shape[1])
  assert got.shape[0] == (N + 127) // 128 * 128
  np.testing.assert_array_equal(got[:exp.shape[0]], exp)
  assert (got[exp.shape[0]:] == 0).all()


# ---------------------------------------------------------------------------
# refusals: one violated condition per call, outputs untouched
# ---------------------------------------------------------------------------
def test_dense_rows_refusals(precision):
  f16 = precision
  lib = _lib.load()
  rows = 32
  x = P.dev_act(np.zeros((rows, 512)), f16)
  w = torch.zeros(512 * 512, dtype=R.act_dtype(f16), device=H.DEV)
  y = P.sent32(rows, 512)
  ya = P.sent_act((rows, 512), f16)
  st = H.stream()
  # (Cx, N, Cy, epilogue)
  bad = [(48, 8, 8, 0),      # Cx not a multiple of 32
         (160, 8, 8, 0),     # Cx beyond 128 and not 256 / 384 / 512
         (64, 6, 6, 0),      # register form: Cy % 4
         (256, 130, 132, 0),  # LDS-panel form: Cy % 8
         (64, 16, 8, 0),     # Cy < N
         (64, 8, 8, 1),      # an epilogue that is neither NONE nor SIGMOID
         (64, 8, 136, 0)]    # register form: Cy beyond 128
  for Cx, N, Cy, epi in bad:
    assert lib.cg_dense_rows(H.p(x), H.p(w), None, H.p(y), rows, Cx, N, Cy, epi,
                             st) == EINVAL, (Cx, N, Cy, epi)
  assert lib.cg_dense_rows(H.p(x), H.p(w), None, H.p(y), 0, 64, 8, 8, 0, st) == EINVAL
  for Cx, N, Cy in [(64, 8, 8), (160, 8, 8), (256, 130, 132), (256, 16, 8)]:
    assert lib.cg_dense_rows_act(H.p(x), H.p(w), H.p(ya), rows, Cx, N, Cy,
                                 st) == EINVAL, (Cx, N, Cy)
  H.sync()
  assert P.is_sentinel(y) and P.is_sentinel(ya)


def test_dense_rows_interp_refusals(precision):
  f16 = precision
  lib = _lib.load()
  x = P.dev_act(np.zeros((9 * 64, 512)), f16)
  w = torch.zeros(512 * 512, dtype=R.act_dtype(f16), device=H.DEV)
  real = P.dev32(np.zeros((64, 512)))
  alpha = P.dev32(np.zeros(16))
  x0 = P.sent_act((3 * 64 * 512,), f16)
  ptrs = (ctypes.c_void_p * 9)(*[x0.data_ptr()] * 9)
  st = H.stream()
  # (n, B, L, Cx, N, Cr, Cp, epilogue); the first of each form is admissible but
  # for the one condition named
  bad = [(1, 1, 32, 64, 8, 8, 64, 3),     # register form: Cp != 128
         (1, 1, 32, 64, 8, 8, 136, 3),
         (9, 1, 32, 64, 8, 8, 128, 3),    # n > 8
         (1, 1, 24, 64, 8, 8, 128, 3),    # L % 16
         (1, 1, 32, 64, 8, 7, 128, 3),    # Cr < N
         (1, 1, 32, 48, 8, 8, 128, 3),    # Cx % 32
         (1, 1, 32, 64, 8, 8, 128, 1),    # epilogue
         (1, 1, 16, 256, 8, 8, 32, 3),    # LDS-panel form: B L % 32
         (1, 2, 16, 256, 130, 130, 132, 3),  # Cp % 8
         (1, 2, 16, 256, 130, 130, 128, 3),  # Cp < N
         (1, 2, 16, 160, 8, 8, 32, 3),    # Cx not 128 / 256 / 384 / 512
         (9, 2, 16, 256, 8, 8, 32, 3)]    # n > 8
  for a_ in (alpha, None):
    for n, B, L, Cx, N, Cr, Cp, epi in bad:
      assert lib.cg_dense_rows_interp(H.p(x), H.p(w), None, H.p(real), H.p(a_), ptrs,
                                      n, B, L, Cx, N, Cr, Cp, epi, st) == EINVAL, (
                                          n, B, L, Cx, N, Cr, Cp, epi)
  H.sync()
  assert P.is_sentinel(x0)


def test_dense_wgrad_refusals(precision):
  f16 = precision
  lib = _lib.load()
  C = 128 * 17  # 17 x 17 = 289 tiles of dW
  x = P.dev_act(np.zeros((32, C)), f16)
  dw = P.sent32(64 * 64)
  ws = P.sent32(8 * 64 * 64)
  st = H.stream()
  call = lambda rows, Cx, Cg, cx, cg, w, n: lib.cg_dense_wgrad(
      H.p(x), H.p(x), H.p(dw), rows, Cx, Cg, cx, cg, H.p(w), n, st)
  assert lib.cg_dense_wgrad_ws_elems(32, 64, 64) == 8 * 64 * 64
  assert call(32, 64, 64, 64, 64, ws, 8 * 64 * 64 - 1) == EINVAL  # workspace
  assert call(32, 60, 64, 60, 64, None, 0) == EINVAL              # pitch % 8
  assert call(32, 64, 60, 64, 60, None, 0) == EINVAL
  assert call(32, 64, 64, 72, 64, None, 0) == EINVAL              # C_real > pitch
  assert call(32, 64, 64, 64, 0, None, 0) == EINVAL               # C_real < 1
  assert call(0, 64, 64, 64, 64, None, 0) == EINVAL               # no rows
  assert call(1, C, C, C, C, None, 0) == EINVAL                   # > 256 tiles
  assert lib.cg_dense_wgrad_ws_elems(0, 64, 64) < 0
  assert lib.cg_dense_wgrad_ws_elems(32, 0, 64) < 0
  H.sync()
  assert P.is_sentinel(dw) and P.is_sentinel(ws)


# ---------------------------------------------------------------------------
# special values
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('rows,K,N,Cy', [(50, 96, 70, 72), (77, 256, 200, 208)])
def test_special_values(rows, K, N, Cy, precision):
  """A row with inf or NaN gives what float64 IEEE arithmetic gives (inf x 0 is
  NaN, in the zero column of W) and leaves the channel padding +0; every other
  row -- the last, clamped one holds the largest finite value -- stays within its
  bar.  Pre-activations of +-30 and +-100 through the sigmoid: never NaN, within
  the epilogue's atol of 0 or 1, and exactly 0 or 1 wherever f32 arithmetic
  saturates (t >= 30: 1 + e^-t is 1; t <= -100: e^-t is inf).  At t = -30 the f32
  quotient is 9.4e-14, a normal number: the float64 value, not 0."""
  f16 = precision
  x, W32, Wq, bias, rr = D.special_recipe(6000 + K, rows, K, N, f16)
  xd, op = P.dev_act(x, f16), pack_dense(W32)
  fin = finite_rows(x)
  with np.errstate(invalid='ignore'):
    t = D.dense_rows(x, Wq, bias)
  acc = np.where(fin[:, None], D.acc_bound(np.where(fin[:, None], x, 0.0), Wq, bias), 0)
  for epi in (0, 3):
    y = run_dense_rows(xd, op, bias, rows, K, N, Cy, epi)
    want = D.sigmoid(t) if epi == 3 else t
    bar = D.sigmoid_bar(acc, want) if epi == 3 else acc
    got = P.host(y[:rows, :N])
    P.assert_f32(got[fin], want[fin], bar[fin], 'epi {}'.format(epi))
    assert_like_ieee(got[~fin], want[~fin], 'epi {}'.format(epi))
    if epi == 3:
      assert np.isfinite(got[rr['inf']][np.arange(N) != D.ZC]).all()
      for key in ('sat30', 'sat100'):
        v, tv = got[rr[key]], t[rr[key]]
        assert np.isfinite(v).all()
        assert (v[tv >= 29] == 1.0).all() and (v[tv <= -99] == 0.0).all()
        assert (v[np.abs(tv) >= 29] <= 1.0).all() and (v >= 0.0).all()
    assert zero_bits(y[:rows, N:]), epi  # also in the inf and NaN rows
    assert P.is_sentinel(y[rows:])
  if K > 128:
    cp = geo.pitch(N)
    ya = P.sent_act((rows + GUARD, cp), f16)
    _lib.call('cg_dense_rows_act', H.p(xd), H.p(op.buf), H.p(ya), rows, K, N, cp,
              H.stream())
    H.sync()
    t0 = D.dense_rows(x, Wq)
    P.assert_act(ya[:rows, :N][torch.tensor(fin).to(H.DEV)], t0[fin], f16,
                 f32_err=D.acc_bound(x[fin], Wq))
    assert_like_ieee(ya[:rows, :N][torch.tensor(~fin).to(H.DEV)], t0[~fin])
    assert zero_bits(ya[:rows, N:])
    assert P.is_sentinel(ya[rows:])


@pytest.mark.parametrize('rows,K,N', [(20, 64, 8), (40, 128, 136)])
def test_matrix_cores_keep_subnormal_inputs(rows, K, N, precision):
  """Subnormal activations (fp16: 2^-24 .. 2^-15; bf16: 2^-133 .. 2^-127) against W
  = 2^10: every product and every sum is a normal f32 and exact, so the output is
  the float64 statement's, bit for bit -- with dense_ref.FLUSH_SUBNORMAL_INPUTS
  saying what the hardware does with such inputs (a flush would give zeros).
  Loss-scaled fp16 gradients live in this range: DESIGN.md section 3.3."""
  f16 = precision
  lo = -24 if f16 else -133
  span = 10 if f16 else 7
  r, c = np.meshgrid(np.arange(rows), np.arange(K), indexing='ij')
  x = 2.0**(lo + (r + c) % span) * np.where((r + 2 * c) % 3 == 0, -1.0, 1.0)
  assert (np.abs(x) < D.min_normal(f16)).all()
  np.testing.assert_array_equal(R.round_act(x, f16), x)
  W = np.full((K, N), 2.0**10)
  xd, op = P.dev_act(x, f16), pack_dense(W)
  flushed = D.FLUSH_SUBNORMAL_INPUTS[f16]
  want = D.dense_rows(x, W, None, None, flushed, f16)
  kept = D.dense_rows(x, W)
  assert (np.abs(kept[kept != 0]) >= 2.0**-126).all() and (kept != 0).mean() > 0.5
  cf = (N + 7) // 8 * 8
  y = run_dense_rows(xd, op, None, rows, K, N, cf, 0)
  got = P.host(y[:rows, :N])
  print('subnormal inputs, f16 =', f16, ': kept' if np.array_equal(got, kept) else
        ': NOT kept', got[0, :2], kept[0, :2])
  np.testing.assert_array_equal(got, want)
  if K >= 128:
    cp = geo.pitch(N)
    ya = P.sent_act((rows, cp), f16)
    _lib.call('cg_dense_rows_act', H.p(xd), H.p(op.buf), H.p(ya), rows, K, N, cp,
              H.stream())
    H.sync()
    P.assert_bits(ya[:, :N], D.dense_rows_act(x, W, f16, flushed), f16)
