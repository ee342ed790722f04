"""Float64 parity of the pointwise / reduction entry points of
calciumgan_amd/csrc/pointwise.hip at edge shapes, in both precision builds.

Every case compares ONE entry point of the C ABI with the float64 statement of
tests/pointwise_ref.py (tied to autograd / the oracle in
tests/test_pointwise_ref.py).  Inputs are random reals rounded to the type the
kernel reads, with planted +-0, the smallest subnormal, the largest finite
value, exact ties and (fp16) overflowing products.  What the contract says is
not read is NaN (f32 channels past C, the workspace), what it says is stored is
pre-filled with a sentinel.  Every bar is one of: bit-equal; k ulps with k
counted from the operations of the header's formula; sum_bound (n 2^-24 sum
|terms|) for an f32 sum of n terms -- never a measured number.

The BCE head (cg_dense1_bce) is the one entry point here that calls libm: its
bars are f32 spacings counted per operation (pointwise_ref.bce_bars), with a
stated allowance per expf / log1pf call.  The deferred finishing launches
(cg_finish_defer / cg_finish_flush) are compared bit for bit with the
undeferred launches of the same reductions, which have their own parity tests."""
import ctypes

import numpy as np
import pytest
import torch

from calciumgan_amd import _lib
from calciumgan_amd import geometry as geo

import hip_utils as H
import pointwise_ref as R

pytestmark = pytest.mark.gpu

U = R.U32
SENT = -12352.0   # exact in bf16 and fp16; no test value comes near it
SENT32 = 12345.0  # f32 outputs (hip_utils.out_buffers' poison)
ALPHA = 0.3       # Keras LeakyReLU default
A32 = R.f32(ALPHA)


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
def dev32(x):
  return torch.tensor(np.asarray(x, np.float64), dtype=torch.float32).to(H.DEV)


def dev_act(x, f16):
  """x holds values of the activation type already (round_act): exact."""
  return torch.tensor(np.asarray(x, np.float64), dtype=torch.float32).to(
      R.act_dtype(f16)).to(H.DEV)


def sent_act(shape, f16):
  return torch.full(shape, SENT, dtype=R.act_dtype(f16), device=H.DEV)


def sent32(*shape):
  return torch.full(shape, SENT32, dtype=torch.float32, device=H.DEV)


def host(t):
  return t.double().cpu().numpy()


def bits(t):
  return t.cpu().view(torch.int16) if t.element_size() == 2 else t.cpu().view(
      torch.int32)


def assert_bits(got, want64, f16):
  """got (activation tensor) == round_act(want64), sign of zero included."""
  want = torch.tensor(np.asarray(want64, np.float64), dtype=torch.float32).to(
      R.act_dtype(f16))
  g, w = bits(got).numpy(), want.view(torch.int16).numpy().reshape(got.shape)
  bad = np.argwhere(g != w)
  assert bad.size == 0, (bad[:5], host(got)[tuple(bad[0])],
                         want.double().numpy().reshape(got.shape)[tuple(bad[0])])


def assert_act(got, want64, f16, f32_err=0.0):
  """|got - round_act(want)| <= one activation ulp (+ f32_err).  The f32 value
  the kernel rounds differs from the float64 one by f32_err (a few 2^-24, far
  below the activation's ulp unless terms cancel); rounding is monotone, so the
  two rounded values are at most one ulp (+ f32_err) apart -- the
  double-rounding allowance.  Infinities must match exactly, and where the
  float64 result is an exact zero (a product with +-0: IEEE fixes its sign, in
  any precision) the stored zero carries that sign."""
  g = host(got)
  w64 = np.broadcast_to(np.asarray(want64, np.float64), g.shape)
  z = w64 == 0
  assert np.array_equal(np.signbit(g[z]), np.signbit(w64[z])), np.argwhere(
      z & (np.signbit(g) != np.signbit(w64)))[:5]
  r = R.round_act(want64, f16).reshape(g.shape)
  fin = np.isfinite(r)
  assert np.array_equal(g[~fin], r[~fin]), (g[~fin][:5], r[~fin][:5])
  bar = R.ulp_act(r, f16) + f32_err
  ok = np.abs(np.where(fin, g - np.where(fin, r, 0.0), 0.0)) <= bar
  bad = np.argwhere(~ok)
  assert bad.size == 0, (bad[:5], g[tuple(bad[0])], r[tuple(bad[0])])


def assert_f32(got, want, bar, what=''):
  g = host(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
  want = np.broadcast_to(np.asarray(want, np.float64), g.shape)
  bar = np.broadcast_to(np.asarray(bar, np.float64), g.shape)
  ok = np.abs(g - want) <= bar
  bad = np.argwhere(~ok)
  assert bad.size == 0, (what, bad[:5], g[tuple(bad[0])], want[tuple(bad[0])],
                         bar[tuple(bad[0])])


def is_sentinel(t):
  ref = torch.full_like(t, SENT if t.element_size() == 2 else SENT32)
  return torch.equal(bits(t), bits(ref))


def planted(f16):
  tiny, big = R.act_limits(f16)
  return [0.0, -0.0, tiny, -tiny, big, -big]


def act_rows(rng, B, n, f16, scale=1.0, extra=()):
  """(B, n) random reals rounded to the activation type; every row starts with
  the planted values (n >= 8)."""
  x = R.round_act(rng.randn(B, n) * scale, f16)
  vals = (planted(f16) + list(extra))[:n]
  x[:, :len(vals)] = vals
  return x


def three_forms(launch, make_out):
  """A reduction that takes `ws`: atomics onto a zeroed output, ordered onto a
  sentinel output, ordered again -- the two ordered results equal bit for bit.
  Returns (atomics result, ordered result)."""
  outs = []
  for ordered in (False, True, True):
    ws = H.reduce_ws() if ordered else None  # (NaN again before every run)
    o = make_out(ws is None)
    launch(o, ws)
    H.sync()
    outs.append([t.clone() for t in o])
  for a, b in zip(outs[1], outs[2]):
    assert torch.equal(bits(a), bits(b))
  return outs[0], outs[1]


BS = [1, 2, 63, 64, 65, 255, 256, 257, 1000]


def norms_for(rng, B, squared):
  """f32 norms over 1e-3 .. 1e3, one exactly 1 (squared: their squares)."""
  nv = (10.0**rng.uniform(-3, 3, B)).astype(np.float32)
  nv[0 if B < 3 else 2] = 1.0
  if B > 4:
    nv[3], nv[4] = 1e-3, 1e3
  return (nv * nv if squared else nv).astype(np.float32)


# ---------------------------------------------------------------------------
# the WGAN-GP scalar chain: one-block reductions over the batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('squared', [0, 1])
@pytest.mark.parametrize('B', BS)
def test_gp_finalize(B, squared):
  rng = np.random.RandomState(100 + B)
  x = norms_for(rng, B, squared)
  scale = 10.0
  norm = dev32(np.r_[x, SENT32])
  gp, coef = sent32(2), sent32(B + 1)
  _lib.call('cg_gp_finalize', H.p(norm), H.p(gp), H.p(coef), B, scale, squared,
            H.stream())
  H.sync()
  nv, gpr, cr = R.gp_finalize(x, scale, squared)
  # squared: sqrtf, at most 1 ulp; else the norms are not written
  e_nv = R.ulp_f32(nv) if squared else np.zeros(B)
  assert_f32(norm[:B], nv, e_nv, 'norm')
  egp, ecoef = R.gp_bars(nv, scale, 1.0, e_nv)
  assert_f32(gp[:1], gpr, egp, 'gp')
  assert_f32(coef[:B], cr, ecoef, 'coef')
  assert float(coef[0 if B < 3 else 2]) == 0.0  # norm exactly 1
  assert float(norm[B]) == SENT32 and float(coef[B]) == SENT32 and float(
      gp[1]) == SENT32


@pytest.mark.parametrize('B', BS)
def test_critic_loss_and_neg_mean(B):
  rng = np.random.RandomState(200 + B)
  d = (rng.randn(3 * B) * 3).astype(np.float32)
  gpv = np.float32(0.4321)
  d_out, gp = dev32(d), dev32([gpv])
  out = sent32(3)
  _lib.call('cg_critic_loss', H.p(d_out), H.p(gp), 10.0, H.p(out), B, H.stream())
  H.sync()
  assert_f32(out[:2], R.critic_loss(d, float(gpv), 10.0, B),
             R.critic_loss_bars(d, float(gpv), 0.0, 10.0, B), 'critic_loss')
  assert float(out[2]) == SENT32
  nm = sent32(2)
  _lib.call('cg_neg_mean', H.p(d_out), H.p(nm), B, H.stream())
  H.sync()
  # the sum, then one quotient
  want = R.neg_mean(d, B)
  assert_f32(nm[:1], want, R.sum_bound(d[:B]) / B + U * abs(want), 'neg_mean')
  assert float(nm[1]) == SENT32


@pytest.mark.parametrize('B', BS)
def test_gp_critic_loss(B):
  rng = np.random.RandomState(300 + B)
  d = (rng.randn(3 * B) * 3).astype(np.float32)
  d_out = dev32(d)
  for squared, mul in ((1, 2.5), (0, 1.0), (1, -0.75)):
    x = norms_for(rng, B, squared)
    norm = dev32(np.r_[x, SENT32])
    gp, coef, loss = sent32(2), sent32(B + 1), sent32(3)
    _lib.call('cg_gp_critic_loss', H.p(norm), H.p(gp), H.p(coef), H.p(d_out),
              H.p(loss), B, 10.0, squared, mul, H.stream())
    H.sync()
    nv, gpr, cr = R.gp_finalize(x, 10.0, squared, mul)
    e_nv = R.ulp_f32(nv) if squared else np.zeros(B)  # sqrtf: at most 1 ulp
    egp, ecoef = R.gp_bars(nv, 10.0, mul, e_nv)
    assert_f32(norm[:B], nv, e_nv, 'norm')
    assert_f32(gp[:1], gpr, egp, 'gp')
    assert_f32(coef[:B], cr, ecoef, 'coef')
    assert_f32(loss[:2], R.critic_loss(d, gpr, 10.0, B),
               R.critic_loss_bars(d, gpr, egp, 10.0, B), 'loss')
    for t, k in ((norm, B), (gp, 1), (coef, B), (loss, 2)):
      assert float(t[k]) == SENT32


@pytest.mark.parametrize('B,P,n', [(1, 1, 0), (2, 5, 8), (63, 64, 4096),
                                   (64, 1, 4096), (65, 5, 0), (255, 64, 8),
                                   (256, 5, 4096), (257, 1, 8), (1000, 64, 0),
                                   (1000, 5, 4096)])
def test_gp_loss_scale(B, P, n, precision):
  f16 = precision
  rng = np.random.RandomState(400 + B + P)
  d = (rng.randn(3 * B) * 3).astype(np.float32)
  d_out = dev32(d)
  # slot sums whose roots span 1e-3 .. 1e3
  tgt = norms_for(rng, B, 1).astype(np.float64)
  slots = (rng.dirichlet(np.ones(P), B) * tgt[:, None]).astype(np.float32)
  sd = dev32(slots)
  g = act_rows(rng, B, n, f16, 0.05) if n else None
  gd = dev_act(g, f16) if n else None
  mul = 0.5
  # the chain: slots added in slot order -> cg_gp_critic_loss -> cg_scale_rows
  ssum = torch.zeros(B, device=H.DEV)
  for j in range(P):
    ssum = ssum + sd[:, j]
  n3, gp3, c3, l3 = ssum.clone(), sent32(1), sent32(B), sent32(2)
  _lib.call('cg_gp_critic_loss', H.p(n3), H.p(gp3), H.p(c3), H.p(d_out), H.p(l3),
            B, 10.0, 1, mul, H.stream())
  if n:
    a3 = sent_act((B, n), f16)
    _lib.call('cg_scale_rows', H.p(gd), H.p(c3), H.p(a3), B, n, H.stream())
  n4, gp4, c4, l4 = sent32(B + 1), sent32(2), sent32(B + 1), sent32(3)
  a4 = sent_act((B, n), f16) if n else None
  _lib.call('cg_gp_loss_scale', H.p(sd), P, H.p(n4), H.p(gp4), H.p(c4),
            H.p(d_out), H.p(l4), B, 10.0, mul, H.p(gd), H.p(a4), n, H.stream())
  H.sync()
  for x, y in ((n4[:B], n3), (gp4[:1], gp3), (c4[:B], c3), (l4[:2], l3)):
    assert torch.equal(bits(x), bits(y))
  for t, k in ((n4, B), (gp4, 1), (c4, B), (l4, 2)):
    assert float(t[k]) == SENT32
  # float64: norm = sqrt(sum of the slots); the sum within sum_bound, through the
  # root (/ 2 sqrt), and sqrtf's 1 ulp
  S = slots.astype(np.float64).sum(1)
  nv, gpr, cr = R.gp_finalize(S, 10.0, 1, mul)
  e_nv = R.sum_bound(slots, axis=1) / (2 * nv) + R.ulp_f32(nv)
  egp, ecoef = R.gp_bars(nv, 10.0, mul, e_nv)
  assert_f32(n4[:B], nv, e_nv, 'norm')
  assert_f32(gp4[:1], gpr, egp, 'gp')
  assert_f32(c4[:B], cr, ecoef, 'coef')
  assert_f32(l4[:2], R.critic_loss(d, gpr, 10.0, B),
             R.critic_loss_bars(d, gpr, egp, 10.0, B), 'loss')
  if n:
    assert torch.equal(bits(a4), bits(a3))
    # the rows from the coefficients the launch stored: one f32 product
    assert_act(a4, R.scale_rows(g, host(c4[:B])), f16)


def test_gp_loss_scale_refusals():
  """P < 1, g without dst, n not a multiple of 8: refused before any launch."""
  lib = _lib.load()
  B = 4
  sd, d_out = dev32(np.ones((B, 2))), dev32(np.zeros(3 * B))
  norm, gp, coef, loss = sent32(B), sent32(1), sent32(B), sent32(2)
  g = torch.zeros(B, 16, dtype=torch.bfloat16, device=H.DEV)
  dst = sent_act((B, 16), False)
  args = lambda P, gg, dd, n: (H.p(sd), P, H.p(norm), H.p(gp), H.p(coef),
                               H.p(d_out), H.p(loss), B, 10.0, 1.0, gg, dd, n,
                               H.stream())
  assert lib.cg_gp_loss_scale(*args(0, H.p(g), H.p(dst), 16)) != 0
  assert lib.cg_gp_loss_scale(*args(2, H.p(g), None, 16)) != 0
  assert lib.cg_gp_loss_scale(*args(2, H.p(g), H.p(dst), 12)) != 0
  assert lib.cg_gp_loss_scale(*args(2, H.p(g), H.p(dst), 0)) != 0
  H.sync()
  for t in (norm, gp, coef, loss, dst):
    assert is_sentinel(t)


# ---------------------------------------------------------------------------
# cg_rownorm
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('B,n', [(1, 8), (256, 8), (3, 2040), (256, 2048),
                                 (3, 2056), (1, 8 * 256 * 64),
                                 (3, 8 * 256 * 64 + 8), (3, 8 * 256 * 130)])
def test_rownorm(B, n, precision):
  """n = 8*256*64 fills the 64-chunk grid exactly, + 8 and 8*256*130 make it
  wrap.  Row 0 is all zeros (B > 1); the last row's squares sum far beyond
  fp16's range -- the sum is f32 and stays finite."""
  f16 = precision
  rng = np.random.RandomState(500 + B + n % 1000)
  g = R.round_act(rng.randn(B, n) * 10.0**rng.uniform(-2, 0, (B, 1)), f16)
  g[-1] = R.round_act(rng.randn(n) * 300.0, f16)
  tiny = R.act_limits(f16)[0]
  g[-1, :8] = [0.0, -0.0, tiny, -tiny, 320.0, -320.0, 320.0, 320.0]
  if B > 1:
    g[0] = 0.0
  gd = dev_act(g, f16)

  def launch(o, ws):
    _lib.call('cg_rownorm', H.p(gd), H.p(o[0]), B, n, H.p(ws), H.stream())

  # (both forms store: the atomics form zeroes the sums itself)
  atom, order = three_forms(launch, lambda zero: [sent32(B + 1)])
  want = R.rownorm(g)
  assert (g[-1]**2).sum() > 65504 and np.isfinite(want).all()
  # n squares (one rounding each, or none) and their sum: sum_bound, through the
  # root (/ 2 norm); sqrtf and the f32 result: 2 ulps
  sb = R.sum_bound(g * g, axis=1)
  bar = np.where(want > 0, sb / (2 * np.where(want > 0, want, 1.0)), 0.0) + \
      2 * R.ulp_f32(want)
  bar[want == 0] = 0.0
  for o in (atom, order):
    assert_f32(o[0][:B], want, bar, 'norm')
    assert float(o[0][B]) == SENT32


# ---------------------------------------------------------------------------
# cg_scale_rows, cg_lrelu_bwd, cg_lrelu_mix
# ---------------------------------------------------------------------------
# x 5 samples: total8 = 5, 1275, 1280, 1285 -- a ragged last block of 256 for all
# but 2048 (1280 = 5 * 256: the exactly full grid)
PER_SAMPLE = [8, 2040, 2048, 2056]


@pytest.mark.parametrize('n', PER_SAMPLE)
def test_scale_rows(n, precision):
  """Coefficients 0, negative, 1e-6 (fp16: into the subnormals), 4 (fp16: 4 x
  65504 must come out as inf; bf16: 4 x the largest finite value overflows f32
  itself) and 1.5, where 1.5 x (1 + ulp) is an exact tie."""
  f16 = precision
  rng = np.random.RandomState(600 + n)
  B = 5
  one_ulp = 1 + R.ulp_act(1.0, f16)
  g = act_rows(rng, B, n, f16, extra=[one_ulp, -one_ulp])
  coef = np.array([0.0, -1.5, 1e-6, 4.0, 1.5], np.float32)
  gd, cd = dev_act(g, f16), dev32(coef)
  a0 = sent_act((B + 1, n), f16)
  _lib.call('cg_scale_rows', H.p(gd), H.p(cd), H.p(a0), B, n, H.stream())
  H.sync()
  want = R.scale_rows(g, coef)
  assert_act(a0[:B], want, f16)  # one f32 product, then the activation's rounding
  got = host(a0[:B])
  assert np.isinf(got[3, 4]) and got[3, 4] > 0 and np.isinf(got[3, 5]) and \
      got[3, 5] < 0
  assert (got[0] == 0).all()
  # the tie: 1.5 (1 + ulp) = 1.5 + 1.5 ulp -> the even neighbour 1.5 + 2 ulp
  assert got[4, 6] == 1.5 + 2 * R.ulp_act(1.0, f16)
  assert is_sentinel(a0[B])
  lib = _lib.load()
  assert lib.cg_scale_rows(H.p(gd), H.p(cd), H.p(a0[B:]), 1, 12, H.stream()) != 0
  H.sync()
  assert is_sentinel(a0[B])


@pytest.mark.parametrize('n', PER_SAMPLE)
def test_lrelu_bwd(n, precision):
  f16 = precision
  rng = np.random.RandomState(700 + n)
  B = 5
  tiny = R.act_limits(f16)[0]
  # (2 tiny x 1/4 ties to 0, 6 tiny x 1/4 ties to 2 tiny)
  dh = act_rows(rng, B, n, f16, extra=[2 * tiny, 6 * tiny]).reshape(-1)
  h = R.round_act(rng.randn(B * n), f16)
  h[:8] = -1.0          # the planted gradients meet the slope ...
  h[n:n + 8] = 1.0      # ... and the identity
  h[2 * n:2 * n + 2] = [0.0, -0.0]  # lrelu'(+-0) = slope
  dd, hd = dev_act(dh, f16), dev_act(h, f16)
  for slope in (0.25, ALPHA, 1.0):
    out = sent_act((B * n + 8,), f16)
    _lib.call('cg_lrelu_bwd', H.p(dd), H.p(hd), H.p(out), B * n, slope, H.stream())
    H.sync()
    want = R.lrelu_bwd(dh, h, R.f32(slope))
    if slope != ALPHA:
      assert_bits(out[:B * n], want, f16)  # a power of two: exact, rounds once
    else:
      assert_act(out[:B * n], want, f16)   # one f32 product, then the rounding
    assert is_sentinel(out[B * n:])
  out = sent_act((16,), f16)
  assert _lib.load().cg_lrelu_bwd(H.p(dd), H.p(hd), H.p(out), 12, 0.25,
                                  H.stream()) != 0
  H.sync()
  assert is_sentinel(out)


@pytest.mark.parametrize('n', PER_SAMPLE)
def test_lrelu_mix(n, precision):
  f16 = precision
  rng = np.random.RandomState(800 + n)
  B = 5
  tiny, big = R.act_limits(f16)
  act = lambda y: np.maximum(y, A32 * y)
  ha = R.round_act(act(rng.randn(B, n)), f16)
  hb = R.round_act(act(rng.randn(B, n)), f16)
  ha[:, :5] = [0.0, -0.0, tiny, -tiny, big]
  hb[:, 3:8] = [0.0, -0.0, tiny, -tiny, big]
  mix = np.array([0.0, 1.0, 0.5, 0.3, 0.9], np.float32)
  out = sent_act((B + 1, n), f16)
  had, hbd, mixd = dev_act(ha, f16), dev_act(hb, f16), dev32(mix)
  _lib.call('cg_lrelu_mix', H.p(had), H.p(hbd), H.p(mixd), H.p(out), B, n, ALPHA,
            H.stream())
  H.sync()
  pa, pb = R.lrelu_mix_parts(ha, hb, mix, A32)
  # 1 / alpha, h / alpha, 1 - mix, the two products, their sum, alpha y: at most
  # 6 roundings on the magnitudes that meet in the sum (they may cancel)
  assert_act(out[:B], R.lrelu_mix(ha, hb, mix, A32), f16,
             f32_err=6 * U * (np.abs(pa) + np.abs(pb)))
  assert is_sentinel(out[B])
  # slope 1/4, mixing factors in {0, 1/4, 1/2, 3/4, 1}, multiples of 4: every
  # operation is exact in f32 and in the activation type -> bit for bit
  act4 = lambda y: np.maximum(y, 0.25 * y)
  ya = rng.randint(-32, 33, (B, n)).astype(np.float64) * 4
  yb = rng.randint(-32, 33, (B, n)).astype(np.float64) * 4
  mix4 = np.array([0.0, 0.25, 0.5, 1.0, 0.75], np.float32)
  had, hbd, mixd = dev_act(act4(ya), f16), dev_act(act4(yb), f16), dev32(mix4)
  out = sent_act((B + 1, n), f16)
  _lib.call('cg_lrelu_mix', H.p(had), H.p(hbd), H.p(mixd), H.p(out), B, n, 0.25,
            H.stream())
  H.sync()
  assert_bits(out[:B], R.lrelu_mix(act4(ya), act4(yb), mix4, 0.25), f16)
  assert is_sentinel(out[B])


# ---------------------------------------------------------------------------
# cg_step_outputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', [0, 1, 5, 8])
def test_step_outputs(n):
  rng = np.random.RandomState(900 + n)
  loss = np.full((max(n, 1), 2), np.nan, np.float32)
  loss[:, 0] = rng.randn(max(n, 1)) * 5
  gp = (rng.rand(max(n, 1)) * 2).astype(np.float32)
  gen, met = np.float32(rng.randn()), rng.rand(4).astype(np.float32)
  out = sent32(8)
  gend, lossd, gpd, metd = dev32([gen]), dev32(loss), dev32(gp), dev32(met)
  _lib.call('cg_step_outputs', H.p(gend), H.p(lossd), H.p(gpd), H.p(metd), n,
            H.p(out), H.stream())
  H.sync()
  want = R.step_outputs(gen, loss, gp, met, n)
  bar = np.zeros(7)  # copies are exact; the means: the sum, then one quotient
  if n:
    bar[1] = R.sum_bound(loss[:n, 0]) / n + U * abs(want[1])
    bar[2] = R.sum_bound(gp[:n]) / n + U * abs(want[2])
  assert_f32(out[:7], want, bar)
  assert float(out[7]) == SENT32
  out = sent32(8)
  assert _lib.load().cg_step_outputs(H.p(gend), H.p(lossd), H.p(gpd), H.p(metd), -1,
                                     H.p(out), H.stream()) != 0
  H.sync()
  assert is_sentinel(out)


# ---------------------------------------------------------------------------
# casts and packs: every load8f path (16-byte, 8-byte, scalar with zero fill)
# ---------------------------------------------------------------------------
PITCHES = [(102, 102, 128, 104), (102, 103, 128, 128), (6, 6, 8, 8),
           (6, 7, 128, 8), (40, 40, 40, 40), (512, 512, 512, 512)]


def f32_source(rng, rows, C, pitch, f16, plant_at):
  """(rows, pitch) f32 in [0, 1) with NaN in the channels [C, pitch) and planted
  values (ties, overflow, subnormals of the activation type) from flat valid
  position plant_at on."""
  tiny, big = R.act_limits(f16)
  x = np.full((rows, pitch), np.nan, np.float32)
  v = rng.rand(rows, C).astype(np.float32)
  vals = np.array(planted(f16) + [
      1 + 2.0**-8, 1 + 3 * 2.0**-8, 1 + 2.0**-11, 1 + 3 * 2.0**-11,  # ties
      tiny / 2, 1.5 * tiny, 65519.0, 65520.0, 1e5, -1e5], np.float32)
  flat = v.reshape(-1)
  k = min(len(vals), flat.size - plant_at)
  if k > 0:
    flat[plant_at:plant_at + k] = vals[:k]
  x[:, :C] = v
  return x


@pytest.mark.parametrize('mode', ['alpha_real', 'noalpha_real', 'alpha_noreal',
                                  'noalpha_noreal'])
@pytest.mark.parametrize('C,Cr,Cf,Cp', PITCHES)
def test_interp_pack(C, Cr, Cf, Cp, mode, precision):
  f16 = precision
  rng = np.random.RandomState(1000 + C + Cr)
  B, L = 4, 9
  rows = B * L
  real = f32_source(rng, rows, C, Cr, f16, 0)
  fake = f32_source(rng, rows, C, Cf, f16, 3)  # same values, other partners
  # an exact tie of the interpolation: (1 + (1 + 2 ulp)) / 2 = 1 + ulp / 2 ... in
  # the activation type: real = 1, fake = 1 + ulp, alpha = 1/2
  tie = (L * C - 1)  # last valid element of sample 0
  real[tie // C, tie % C] = 1.0
  fake[tie // C, tie % C] = 1 + R.ulp_act(1.0, f16)
  alpha = np.array([0.5, 0.0, 1.0, rng.rand()], np.float32)
  use_alpha, write_real = mode.startswith('alpha'), mode.endswith('_real')
  x0 = sent_act((3 * B, L, Cp), f16)
  real_d, fake_d, alpha_d = dev32(real), dev32(fake), dev32(alpha)
  _lib.call('cg_interp_pack', H.p(real_d), H.p(fake_d),
            H.p(alpha_d) if use_alpha else None, H.p(x0), B, L, C, Cr, Cf, Cp,
            int(write_real), H.stream())
  H.sync()
  r, f = real[:, :C].reshape(B, L, C), fake[:, :C].reshape(B, L, C)
  # real and fake: exact in f32, round once -> bit for bit
  if write_real:
    assert_bits(x0[:B, :, :C], r, f16)
    assert (host(x0[:B, :, C:]) == 0).all()
  else:
    assert is_sentinel(x0[:B])
  assert_bits(x0[B:2 * B, :, :C], f, f16)
  assert (host(x0[B:2 * B, :, C:]) == 0).all()
  if use_alpha:
    # 1 - alpha, two products, one sum (all terms of one sign or one dominant)
    assert_act(x0[2 * B:, :, :C], R.interp(r, f, alpha), f16)
    assert (host(x0[2 * B:, :, C:]) == 0).all()
    assert host(x0[2 * B, L - 1, C - 1]) == 1.0  # the tie went to even
  else:
    assert is_sentinel(x0[2 * B:])


@pytest.mark.parametrize('i', range(len(PITCHES)))
def test_cast_pad(i, precision):
  f16 = precision
  C, Cr, Cf, Cp = PITCHES[i]
  rows = [1, 31, 1000][i % 3]
  rng = np.random.RandomState(1100 + i)
  for Cs in (Cr, Cf):
    src = f32_source(rng, rows, C, Cs, f16, 0)
    dst = sent_act((rows + 1, Cp), f16)
    src_d = dev32(src)
    _lib.call('cg_cast_pad', H.p(src_d), H.p(dst), rows, C, Cs, Cp, H.stream())
    H.sync()
    assert_bits(dst[:rows, :C], src[:, :C], f16)  # exact in f32, rounds once
    assert (host(dst[:rows, C:]) == 0).all()
    assert is_sentinel(dst[rows])
    if f16 and C >= 20:  # 65520 (the tie below 2^16), 1e5 and -1e5 overflow
      assert host(dst[0, 13:16]).tolist() == [np.inf, np.inf, -np.inf]


@pytest.mark.parametrize('i', range(len(PITCHES)))
def test_sigmoid_bwd(i, precision):
  f16 = precision
  C, Cr, Cf, Cp = PITCHES[i]
  rows = [31, 1000, 1][i % 3]
  rng = np.random.RandomState(1200 + i)
  for Cs in (Cr, Cf):
    s = np.full((rows, Cs), np.nan, np.float32)
    s[:, :C] = rng.rand(rows, C)
    s[0, :3] = [0.0, 1.0, 0.75]
    dfake = np.zeros((rows, Cp))  # padding channels are zero (the contract)
    dfake[:, :C] = R.round_act(rng.randn(rows, C), f16)
    vals = planted(f16)
    k = min(C - 3, len(vals))
    dfake[rows - 1, 3:3 + k] = vals[:k]
    # an exact tie: (1 + ulp) x 3/4 x 1/4 = 3/16 + 1.5 ulps of [1/8, 1/4), every
    # f32 step exact -> the even neighbour 3/16 + 2 ulps
    u8 = R.ulp_act(1.0, f16) / 8
    dfake[0, 2] = 1 + R.ulp_act(1.0, f16)
    dz = sent_act((rows + 1, Cp), f16)
    dfake_d, s_d = dev_act(dfake, f16), dev32(s)
    _lib.call('cg_sigmoid_bwd', H.p(dfake_d), H.p(s_d), H.p(dz), rows, C, Cs, Cp,
              H.stream())
    H.sync()
    # 1 - s, two products (|s (1 - s)| <= 1/4: no overflow), then the rounding
    assert_act(dz[:rows, :C], R.sigmoid_bwd(dfake[:, :C], s[:, :C]), f16)
    assert host(dz[0, 2]) == 0.1875 + 2 * u8
    assert (host(dz[:rows, C:]) == 0).all()
    assert is_sentinel(dz[rows])


# ---------------------------------------------------------------------------
# cg_colsum
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('rows,C,Cp', [(1, 8, 8), (255, 102, 104),
                                       (256, 2048, 2048), (257, 2050, 2056),
                                       (5000, 102, 104), (5000, 6, 8),
                                       (1, 2056, 2056), (2049 * 256, 5, 8)])
def test_colsum(rows, C, Cp, precision):
  """rows = 2049 * 256 is 2049 blocks of the smallest size, 256 rows; cg_colsum's
  own sizing (rows_per_block grows while 512 blocks remain, up to 4096) already
  takes 1024 rows per block there, so this case runs 513 long blocks and does NOT
  reach the kMaxParts loop -- test_colsum_doubles_rows_per_block does."""
  f16 = precision
  rng = np.random.RandomState(1300 + rows % 997 + Cp)
  x = R.round_act(rng.randn(rows, Cp).astype(np.float32), f16)  # padding: any reals
  tiny, big = R.act_limits(f16)
  vals = [0.0, -0.0, tiny, -tiny, 1024.0]
  x[0, :min(C, 5)] = vals[:min(C, 5)]
  xd = dev_act(x, f16)

  def make_out(zero):
    o = sent32(Cp + 1)
    if zero:
      o[:C] = 0.0
    return [o]

  def launch(o, ws):
    _lib.call('cg_colsum', H.p(xd), H.p(o[0]), rows, C, Cp, H.p(ws), H.stream())

  atom, order = three_forms(launch, make_out)
  want, bar = R.colsum(x[:, :C]), R.sum_bound(x[:, :C], axis=0)
  for o in (atom, order):
    assert_f32(o[0][:C], want, bar, 'colsum')
    assert is_sentinel(o[0][C:])
  if rows > 100000:
    # small integers: every partial sum is exact in f32, so a dropped or doubled
    # row shows whatever the order
    xi = rng.randint(-3, 4, (rows, Cp)).astype(np.float64)
    xd = dev_act(xi, f16)
    atom, order = three_forms(launch, make_out)
    for o in (atom, order):
      np.testing.assert_array_equal(host(o[0][:C]), xi[:, :C].sum(0))


def test_colsum_doubles_rows_per_block(precision):
  """cg_colsum sizes a block at up to 4096 rows on its own (the loop in its
  entry point stops at rows_per_block = 4096); the ordered form keeps at most
  kMaxParts = 2048 partial rows, so its second loop is entered only for rows >
  2048 * 4096, and doubles rows_per_block to 8192.  The narrowest pitch, Cp = 8,
  makes that 134 MB of activations, the smallest input that gets there.  Values
  in {-1, 0, 1}: every partial sum is an integer below 2^24, exact in any order,
  so a dropped or doubled row shows in either form."""
  f16 = precision
  kMaxParts, own_limit = 2048, 4096
  rows, C, Cp = kMaxParts * own_limit + 1, 5, 8
  rng = np.random.RandomState(1399)
  xi = rng.randint(-1, 2, (rows, Cp), dtype=np.int8)
  xd = torch.from_numpy(xi).to(H.DEV).to(R.act_dtype(f16))
  want = xi[:, :C].sum(0, dtype=np.int64).astype(np.float64)
  # (sum |x| < 2^24 per column bounds every partial sum of every subset)
  assert np.abs(xi).sum(0, dtype=np.int64).max() < 2**24

  def make_out(zero):
    o = sent32(Cp + 1)
    if zero:
      o[:C] = 0.0
    return [o]

  def launch(o, ws):
    _lib.call('cg_colsum', H.p(xd), H.p(o[0]), rows, C, Cp, H.p(ws), H.stream())

  atom, order = three_forms(launch, make_out)
  for o in (atom, order):
    np.testing.assert_array_equal(host(o[0][:C]), want)
    assert is_sentinel(o[0][C:])


# ---------------------------------------------------------------------------
# cg_signal_metrics
# ---------------------------------------------------------------------------
def _metrics_forms(real_d, fake_d, rows, C, Cr, Cf, smin, smax):
  def launch(o, ws):
    _lib.call('cg_signal_metrics', H.p(real_d), H.p(fake_d), H.p(o[0]), rows, C, Cr,
              Cf, smin, smax, H.p(ws), H.stream())

  def make_out(zero):
    o = sent32(5)
    if zero:
      o[:4] = 0.0
    return [o]

  atom, order = three_forms(launch, make_out)
  assert float(atom[0][4]) == SENT32 and float(order[0][4]) == SENT32
  return host(atom[0][:4]), host(order[0][:4])


@pytest.mark.parametrize('rows,C,Cr,Cf', [(1, 1, 1, 3), (63, 6, 7, 8),
                                          (150, 8, 8, 10), (150, 9, 10, 12),
                                          (63, 102, 104, 102),
                                          (70000, 102, 102, 103),
                                          (150, 512, 512, 514),
                                          (63, 520, 521, 520),
                                          (150, 1000, 1002, 1000)])
def test_signal_metrics(rows, C, Cr, Cf):
  """C <= 8 lpr: one group per lane; C > 512: the spanning branch.  Pitches: odd,
  even but not a multiple of 4, multiples of 4.  Row 0 of real holds identical
  values (std exactly 0), the last row of fake its maximum, the last row of real
  its minimum, in the last valid channel."""
  rng = np.random.RandomState(1400 + rows % 1000 + C)
  smin, smax = -0.5, 2.5
  real = np.full((rows, Cr), np.nan, np.float32)
  fake = np.full((rows, Cf), np.nan, np.float32)
  real[:, :C] = rng.rand(rows, C)
  fake[:, :C] = rng.rand(rows, C)
  real[0, :C] = 0.625
  real[-1, C - 1] = -0.25 if rows > 1 else 0.625
  fake[-1, C - 1] = 1.75
  atom, order = _metrics_forms(dev32(real), dev32(fake), rows, C, Cr, Cf, smin, smax)
  want = R.signal_metrics(real[:, :C], fake[:, :C], smin, smax)
  bar = R.signal_metrics_bars(real[:, :C], fake[:, :C], smin, smax)
  # (the atomics form leaves the sums: the caller divides by rows)
  assert_f32(atom / rows, want, bar, 'atomics')
  assert_f32(order, want, bar, 'ordered')


def test_signal_metrics_doubles_rows_per_slot():
  """A block covers 4 waves x rpw rows x rows_per_slot, rpw = 64 / LPR rows per
  wave (LPR = 1 for C <= 8), and rows_per_slot stops at 64 on its own; the
  ordered form keeps at most kMaxParts = 2048 partial rows, so it must double
  rows_per_slot once rows > 2048 * 4 * 64 * 64.  The smallest such input is C = 1
  (134 MB of f32; real and fake are two windows of one buffer, one element
  apart).  Values are multiples of 1/4 and the scale is 4: every squared
  difference is 0 or 1 and every partial sum an integer below 2^24, exact in any
  order."""
  kMaxParts, rpw = 2048, 64
  rows = kMaxParts * 4 * rpw * 64 + 1
  buf = np.zeros(rows + 1, np.float32)
  buf[::7] = 0.25
  bd = torch.from_numpy(buf).to(H.DEV)
  real_d, fake_d = bd[:rows], bd[1:]
  # rows i with i % 7 == 0 (real 1, fake 0) or i % 7 == 6 (real 0, fake 1)
  cnt = float(len(range(0, rows, 7)) + len(range(6, rows, 7)))
  assert cnt < 2.0**24
  atom, order = _metrics_forms(real_d, fake_d, rows, 1, 1, 1, 0.0, 4.0)
  # min = max = mean (C = 1), std = 0
  np.testing.assert_array_equal(atom, [cnt, cnt, cnt, 0.0])
  # the mean: float(rows), 1 / rows, the product -- 3 roundings
  assert_f32(order, [cnt / rows] * 3 + [0.0], 3 * U * cnt / rows)


def test_signal_metrics_refusals():
  out = sent32(4)
  x = dev32(np.zeros((4, 8)))
  lib = _lib.load()
  for rows, C, Cr, Cf in ((0, 8, 8, 8), (4, 0, 8, 8), (4, 8, 7, 8), (4, 8, 8, 7)):
    assert lib.cg_signal_metrics(H.p(x), H.p(x), H.p(out), rows, C, Cr, Cf, 0.0,
                                 1.0, None, H.stream()) != 0
  H.sync()
  assert is_sentinel(out)


# ---------------------------------------------------------------------------
# discriminator head
# ---------------------------------------------------------------------------
# (Lt, C, Cp, nB, seg): the three shapes of test_bce_head_matches_float64 (2B
# samples), C = 6 / 102 at Cp = geometry.pitch(C) with nB = 1 / 7 / 768, and the
# tightest pitch the header allows (a multiple of 8: the scalar tail of load8f)
HEAD = [(64, 320, 320, 16, 8), (8, 12, 16, 6, 3), (256, 320, 320, 4, 2),
        (8, 6, geo.pitch(6), 1, 1), (8, 102, geo.pitch(102), 7, 7),
        (4, 102, geo.pitch(102), 768, 384), (128, 6, geo.pitch(6), 768, 256),
        (3, 102, 104, 7, 1), (5, 6, 8, 7, 2)]


def _head_data(rng, Lt, C, Cp, nB, f16):
  tiny, big = R.act_limits(f16)
  h = np.zeros((nB, Lt, Cp))
  h[:, :, :C] = R.round_act(rng.randn(nB, Lt, C), f16)
  h[0, 0, :4] = [0.0, -0.0, tiny, -tiny]
  if nB > 1:
    h[-1, -1, C - 2:C] = [big, -big]
  w = (rng.randn(Lt, C) / np.sqrt(Lt * C)).astype(np.float32)
  # the seed's tie: coef 1.5 x act(w) = 1 + ulp x lrelu' = 1 -> 1.5 + 1.5 ulp
  w[0, C - 1] = 1 + R.ulp_act(1.0, f16)
  h[0, 0, C - 1] = 1.0
  return h, w, R.round_act(w, f16)


@pytest.mark.parametrize('Lt,C,Cp,nB,seg', HEAD)
def test_dense1_fwd_bwd(Lt, C, Cp, nB, seg, precision):
  f16 = precision
  rng = np.random.RandomState(1500 + Lt + C + nB)
  h, w, wq = _head_data(rng, Lt, C, Cp, nB, f16)
  nseg = (nB + seg - 1) // seg
  coef = rng.randn(nseg).astype(np.float32)
  # (the last segment: coef x act(w) reaches 2.5e5 -- beyond fp16's range under
  # either value of lrelu', 1 or 0.3)
  coef[-1] = np.float32(2.5e5 / np.abs(wq).max())
  if nseg > 1:
    coef[0] = 1.5
  if nseg > 2:
    coef[1] = 0.0
  bias = np.float32(0.25)
  hd, wd, bd, cd = dev_act(h, f16), dev32(w), dev32([bias]), dev32(coef)
  out = sent32(nB + 1)
  _lib.call('cg_dense1_fwd', H.p(hd), H.p(wd), H.p(bd), H.p(out), nB, Lt, C, Cp,
            H.stream())
  delta = sent_act((nB + 1, Lt, Cp), f16)
  _lib.call('cg_dense1_bwd', H.p(wd), H.p(cd), H.p(hd), H.p(delta), nB, Lt, C, Cp,
            seg, ALPHA, H.stream())
  out2, delta2 = sent32(nB + 1), sent_act((nB + 1, Lt, Cp), f16)
  _lib.call('cg_dense1_fwd_bwd', H.p(hd), H.p(wd), H.p(bd), H.p(out2), H.p(cd),
            H.p(delta2), nB, Lt, C, Cp, seg, ALPHA, H.stream())
  H.sync()
  # the logit: Lt C products and the bias, one f32 sum in some order
  terms = R.dense1_terms(h[:, :, :C], wq).reshape(nB, -1)
  terms = np.concatenate([terms, np.full((nB, 1), float(bias))], axis=1)
  assert_f32(out[:nB], terms.sum(1), R.sum_bound(terms, axis=1), 'logit')
  # the seeds: two f32 products, then the activation's rounding
  assert_act(delta[:nB, :, :C], R.dense1_bwd(h[:, :, :C], wq, coef, seg, A32), f16)
  assert (host(delta[:nB, :, C:]) == 0).all()
  if nseg > 1:  # the tie goes to the even neighbour
    assert host(delta[0, 0, C - 1]) == 1.5 + 2 * R.ulp_act(1.0, f16)
  if f16:
    assert np.isinf(host(delta[nB - 1])).any()
  # one pass over h: the same bits
  assert torch.equal(bits(out2), bits(out))
  diff = np.argwhere(bits(delta2).numpy() != bits(delta).numpy())
  assert diff.size == 0, (len(diff), diff[:8], host(delta2)[tuple(diff[0])],
                          host(delta)[tuple(diff[0])], coef[diff[0][0] // seg],
                          wq[diff[0][1], min(diff[0][2], C - 1)])
  assert float(out[nB]) == SENT32 and is_sentinel(delta[nB])
  fresh = sent_act((nB, Lt, Cp), f16)
  assert _lib.load().cg_dense1_bwd(H.p(wd), H.p(cd), H.p(hd), H.p(fresh), nB, Lt, C,
                                   Cp, 0, ALPHA, H.stream()) != 0
  H.sync()
  assert is_sentinel(fresh)


@pytest.mark.parametrize('Lt,C,Cp,nB,seg', HEAD)
def test_dense1_wgrad(Lt, C, Cp, nB, seg, precision):
  f16 = precision
  rng = np.random.RandomState(1600 + Lt + C + nB)
  x, _, _ = _head_data(rng, Lt, C, Cp, nB, f16)
  x[:, :, C:] = R.round_act(rng.randn(nB, Lt, Cp - C), f16)  # not part of any sum
  nseg = (nB + seg - 1) // seg
  coef = rng.randn(nseg).astype(np.float32)
  coef[-1] = 0.5  # (times the planted largest finite value: still an f32)
  bc = rng.randn(nseg).astype(np.float32)
  xd, cd, bcd = dev_act(x, f16), dev32(coef), dev32(bc)

  def make_out(zero):
    dw, db = sent32(Lt * C + 1), sent32(2)
    if zero:
      dw[:Lt * C] = 0.0
      db[:1] = 0.0
    return [dw, db]

  def launch(o, ws):
    _lib.call('cg_dense1_wgrad', H.p(xd), H.p(cd), H.p(bcd), H.p(o[0]), H.p(o[1]),
              nB, Lt, C, Cp, seg, H.p(ws), H.stream())

  atom, order = three_forms(launch, make_out)
  terms = R.dense1_wgrad_terms(x[:, :, :C], coef, seg)
  bterms = np.repeat(bc.astype(np.float64), seg)[:nB]
  for o in (atom, order):
    # nB products and their sum, per weight (a product below 2^-126 -- the
    # planted subnormals -- rounds to a multiple of 2^-149 instead); nB
    # coefficients, for the bias
    assert_f32(o[0][:Lt * C], terms.sum(0).reshape(-1),
               R.sum_bound(terms, axis=0).reshape(-1) + nB * 2.0**-149, 'dw')
    assert_f32(o[1][:1], bterms.sum(), R.sum_bound(bterms), 'db')
    assert float(o[0][Lt * C]) == SENT32 and float(o[1][1]) == SENT32


# ---------------------------------------------------------------------------
# Adam and the loss-scale kernels
# ---------------------------------------------------------------------------
B1, B2, EPS, LR = R.f32(0.9), R.f32(0.999), R.f32(1e-7), R.f32(1e-3)


def _adam_data(rng, n):
  p = rng.randn(n).astype(np.float32)
  g = rng.randn(n).astype(np.float32)
  m = (rng.randn(n) * 0.1).astype(np.float32)
  v = (rng.rand(n) * 0.1).astype(np.float32)
  m[0] = v[0] = g[0] = 0.0  # the update must be 0 / eps = 0, not NaN
  if n > 1:
    v[1] = g[1] = 0.0       # m / eps: large, finite
    m[1] = 1e-4
  return p, g, m, v


@pytest.mark.parametrize('dev_lr', [False, True], ids=['host_lr', 'dev_lr'])
@pytest.mark.parametrize('n,t,gs', [(1, 1, 1.0), (255, 3, 0.5), (256, 20000, 3.7),
                                    (257, 3, 3.7), (10007, 20000, 0.5)])
def test_adam(n, t, gs, dev_lr):
  """t = 20000: 0.999^t < 2^-24, so 1 - beta2^t is 1 in f32.  With lr_t_dev the
  host lr_t is a different number: the result shows which one was used."""
  rng = np.random.RandomState(1700 + n)
  p, g, m, v = _adam_data(rng, n)
  lr_t = R.f32(R.adam_lr_t(1e-3, 0.9, 0.999, t))
  gs32 = R.f32(gs)
  pd, gd, md, vd = (dev32(np.r_[a, SENT32]) for a in (p, g, m, v))
  lr_d = dev32([lr_t])
  _lib.call('cg_adam', H.p(pd), H.p(gd), H.p(md), H.p(vd), n,
            123.0 if dev_lr else lr_t, 0.9, 0.999, 1e-7, gs,
            H.p(lr_d) if dev_lr else None, H.stream())
  H.sync()
  pr, mr, vr = R.adam(p, g, m, v, lr_t, B1, B2, EPS, gs32)
  ep, em, ev = R.adam_bars(p, g, m, v, lr_t, B1, B2, EPS, gs32)
  assert_f32(md[:n], mr, em, 'm')
  assert_f32(vd[:n], vr, ev, 'v')
  assert_f32(pd[:n], pr, ep, 'p')
  assert float(pd[0]) == float(p[0]) and float(vd[0]) == 0.0
  for a in (pd, md, vd):
    assert float(a[n]) == SENT32
  ps, ms, vs = sent32(4), sent32(4), sent32(4)
  assert _lib.load().cg_adam(H.p(ps), H.p(gd), H.p(ms), H.p(vs), 0, lr_t, 0.9,
                             0.999, 1e-7, gs, None, H.stream()) != 0
  H.sync()
  assert is_sentinel(ps) and is_sentinel(ms) and is_sentinel(vs)


N_WRAP = 4 * 256 * 2048 + 4  # one f32x4 more than the capped grid covers at once


@pytest.mark.parametrize('n', [4, 1024, N_WRAP])
def test_grad_finite_and_adam_scaled(n):
  rng = np.random.RandomState(1800 + n % 1000)
  p, g, m, v = _adam_data(rng, n)
  S, t = 1024.0, 3
  ls0 = np.array([S, 5.0, t - 1.0, 1.0], np.float32)
  gd = dev32(g)
  # a clean gradient leaves the state alone
  ls = dev32(ls0)
  _lib.call('cg_grad_finite', H.p(gd), n, H.p(ls), H.stream())
  H.sync()
  np.testing.assert_array_equal(host(ls), ls0)
  # one non-finite value: first element, last element, the wrapped tail
  for pos in sorted({0, n - 1, n - 3}):
    for bad in (np.nan, np.inf, -np.inf):
      keep = float(gd[pos])
      gd[pos] = bad
      ls = dev32(ls0)
      _lib.call('cg_grad_finite', H.p(gd), n, H.p(ls), H.stream())
      H.sync()
      gd[pos] = keep
      np.testing.assert_array_equal(host(ls), [S, 5.0, t - 1.0, 0.0], str((pos, bad)))
  # ls[3] == 0: the update is skipped, bit for bit
  ls = dev32([S, 5.0, t - 1.0, 0.0])
  pd, md, vd = dev32(p), dev32(m), dev32(v)
  _lib.call('cg_adam_scaled', H.p(pd), H.p(gd), H.p(md), H.p(vd), n, 1e-3, 0.9,
            0.999, 1e-7, 0.5, H.p(ls), H.stream())
  H.sync()
  for a, b in ((pd, p), (md, m), (vd, v)):
    assert torch.equal(bits(a), bits(torch.from_numpy(b)))
  # ls[3] == 1: Adam on grad * grad_scale / S with lr_t from t = ls[2] + 1
  for tt in (t, 20000):
    ls = dev32([S, 5.0, tt - 1.0, 1.0])
    pd, md, vd = (dev32(np.r_[a, SENT32]) for a in (p, m, v))
    _lib.call('cg_adam_scaled', H.p(pd), H.p(gd), H.p(md), H.p(vd), n, 1e-3, 0.9,
              0.999, 1e-7, 0.5, H.p(ls), H.stream())
    H.sync()
    lr_t = R.adam_lr_t(LR, B1, B2, tt)
    # lr_t on the device: powf within 2 ulps (4 U of beta^t, against 1 - beta^t;
    # halved by the root for beta2), then 1 - x twice, the root, the product and
    # the quotient: 5 U
    rel = 4 * U * B2**tt / (1 - B2**tt) / 2 + 4 * U * B1**tt / (1 - B1**tt) + 5 * U
    pr, mr, vr = R.adam(p, g, m, v, lr_t, B1, B2, EPS, 0.5 / S)
    ep, em, ev = R.adam_bars(p, g, m, v, lr_t, B1, B2, EPS, 0.5 / S, lr_t_rel=rel,
                             g_roundings=2)  # grad_scale / S, then the product
    assert_f32(md[:n], mr, em, 'm')
    assert_f32(vd[:n], vr, ev, 'v')
    assert_f32(pd[:n], pr, ep, 'p')
    assert float(pd[0]) == float(p[0])
    np.testing.assert_array_equal(host(ls), [S, 5.0, tt - 1.0, 1.0])
    for a in (pd, md, vd):
      assert float(a[n]) == SENT32


@pytest.mark.parametrize('n', [2, 6])
def test_grad_finite_refuses_lengths_that_are_not_multiples_of_four(n):
  g = dev32(np.full(8, np.nan))
  ls = sent32(4)
  assert _lib.load().cg_grad_finite(H.p(g), n, H.p(ls), H.stream()) != 0
  H.sync()
  assert is_sentinel(ls)


# ---------------------------------------------------------------------------
# cg_dense1_bce: the whole loss head of --algorithm gan
# ---------------------------------------------------------------------------
# Rows are laid out over the Lt * C valid positions of a sample: positions 0..5
# hold the planted values of act_rows (weight 0), position ONE_HOT has the weight
# 1.0 exactly, every other weight is a random f32 (most of them change when they
# are rounded to the activation type).  A one-hot row -- v at ONE_HOT, zeros of
# both signs elsewhere -- has the logit v + bias exactly, in any order of the sum.
ONE_HOT = 6
S_D, S_G = 1024.0, 256.0  # the fp16 build's loss scales (powers of two)


def _bce_segment(rng, logits, n_rand, Lt, C, Cp, f16, scale):
  n = Lt * C
  v = np.zeros((len(logits) + n_rand, n))
  v[:len(logits), 1] = -0.0        # under a weight of 0 ...
  v[:len(logits), n - 1] = -0.0    # ... and under a random one
  v[:len(logits), ONE_HOT] = logits
  if n_rand:
    v[len(logits):] = act_rows(rng, n_rand, n, f16, scale)
  h = np.zeros((len(v), Lt, Cp))   # padding: as test_dense1_fwd_bwd has it
  h[:, :, :C] = v.reshape(-1, Lt, C)
  return h


def _bce_case(seed, Lt, C, Cp, f16, fake, real, n_rand, bias=0.0):
  """2B = 2 (len(fake) + n_rand) samples [fake | real]: one-hot rows with the
  given logits (less the bias), then n_rand random dense rows per segment, scaled
  so that their logits stay within +-30."""
  assert len(fake) == len(real) and Lt * C >= 8
  rng = np.random.RandomState(seed)
  n = Lt * C
  w = (rng.randn(n) / np.sqrt(n)).astype(np.float32)
  w[:6] = 0.0
  w[ONE_HOT] = 1.0
  h = np.concatenate([_bce_segment(rng, s, n_rand, Lt, C, Cp, f16, 5.0)
                      for s in (fake, real)])
  nan = np.full(n_rand, np.nan)
  d = dict(Lt=Lt, C=C, Cp=Cp, B=len(fake) + n_rand, h=h, w=w, bias=R.f32(bias),
           wq=R.round_act(w, f16).reshape(Lt, C),
           planted=np.r_[np.asarray(fake, np.float64), nan,
                         np.asarray(real, np.float64), nan])
  assert (d['wq'] != w.reshape(Lt, C)).any() or n == 8
  d['hd'] = dev_act(h, f16)
  # exactly Lt * C weights, then NaN: an over-read by any path of load8f shows
  d['wd'] = dev32(np.r_[w.astype(np.float64), np.full(16, np.nan)])
  d['bd'] = dev32([d['bias']])
  return d


def _bce_outputs(d, f16, zero_loss=False):
  """[out, coef_d, coef_g, delta_d, delta_g, loss], one guard element / row each."""
  B, Lt, Cp = d['B'], d['Lt'], d['Cp']
  loss = sent32(3)
  if zero_loss:
    loss[:2] = 0.0
  return [sent32(2 * B + 1), sent32(2 * B + 1), sent32(B + 1),
          sent_act((2 * B + 1, Lt, Cp), f16), sent_act((B + 1, Lt, Cp), f16), loss]


def _bce_launch(d, o, form, scales, ws):
  """form 'all': every pointer; 'disc': delta_g = coef_g = NULL; 'validate': the
  six optional pointers NULL (gan.py's validation call)."""
  out, cd, cg, dd, dg, loss = o
  sd, sg = scales
  if form == 'disc':
    cg = dg = None
  elif form == 'validate':
    cd = cg = dd = dg = sd = sg = None
  _lib.call('cg_dense1_bce', H.p(d['hd']), H.p(d['wd']), H.p(d['bd']), H.p(out),
            H.p(cd), H.p(cg), H.p(dd), H.p(dg), H.p(loss), H.p(sd), H.p(sg), d['B'],
            d['Lt'], d['C'], d['Cp'], ALPHA, H.p(ws), H.stream())


def _bce_scales(f16):
  """bf16: NULL.  fp16: NULL, then device scalars."""
  runs = [((None, None), 1.0, 1.0)]
  if f16:
    runs.append(((dev32([S_D]), dev32([S_G])), S_D, S_G))
  return runs


def _bce_check(d, o, terms, f16, form, S_d, S_g):
  """Every output of one launch.  terms: the first floats of the workspace after
  an ordered launch, None after the atomics form.

  Logits: one-hot rows bit-equal to the planted value (+ bias), dense rows within
  sum_bound of their Lt C products and the bias.  Everything else is compared
  with float64 functions of the logit the launch STORED, inside the bars of
  pointwise_ref.bce_bars -- f32 spacings counted per operation (half a spacing
  per rounding of + * /; expf and log1pf two spacings per call, an allowance
  taken from documentation memory of the HIP math API's accuracy table and not
  from this kernel: tests/test_pointwise_ref.py shows the naive forms miss these
  bars by four orders of magnitude and more)."""
  B, Lt, C, Cp = d['B'], d['Lt'], d['C'], d['Cp']
  n2 = 2 * B
  out, cd, cg, dd, dg, loss = o
  assert float(out[n2]) == SENT32 and float(loss[2]) == SENT32
  x = host(out[:n2])
  assert np.isfinite(x).all()  # (a NaN: the guard behind w was read)
  terms64 = R.dense1_terms(d['h'][:, :, :C], d['wq']).reshape(n2, -1)
  terms64 = np.concatenate([terms64, np.full((n2, 1), d['bias'])], axis=1)
  want = terms64.sum(1)
  assert_f32(out[:n2], want, R.sum_bound(terms64, axis=1), 'logit')
  pl = ~np.isnan(d['planted'])
  np.testing.assert_array_equal(want[pl], d['planted'][pl] + d['bias'])
  np.testing.assert_array_equal(bits(out[:n2]).numpy()[pl],
                                want.astype(np.float32).view(np.int32)[pl])
  r, bar = R.bce_from_logits(x, B, S_d, S_g), R.bce_bars(x, B, S_d, S_g)
  zero = pl & (d['planted'] == 0) & (d['bias'] == 0)  # x = +-0: closed forms
  if terms is not None:
    assert_f32(terms[:n2], r['td'], bar['td'], 'terms of loss[1]')
    assert_f32(terms[n2:3 * B], r['tg'], bar['tg'], 'terms of loss[0]')
    assert torch.isnan(terms[3 * B:]).all()
    t = host(terms)
    assert_f32(t[:n2][zero], np.log(2.0), bar['td'][zero], 'log 2')
    assert_f32(t[n2:3 * B][zero[:B]], np.log(2.0), bar['tg'][zero[:B]], 'log 2')
    assert_f32(loss[:2], r['loss'], bar['loss'], 'loss')
  else:
    assert_f32(loss[:2], r['loss'], bar['loss_atomic'], 'loss (atomics)')
  mask = R.lrelu_grad(d['h'][:, :, :C], A32)
  assert (mask[d['h'][:, :, :C] == 0] == A32).all()  # +0 and -0 take the slope
  g = d['wq'][None] * mask
  sign = np.r_[np.ones(B), -np.ones(B)]
  for name, c, delta, k, on, closed in (
      ('coef_d', cd, dd, n2, form != 'validate', sign * S_d / n2),
      ('coef_g', cg, dg, B, form == 'all', np.full(B, -S_g / n2))):
    if not on:
      assert is_sentinel(c) and is_sentinel(delta), name
      continue
    assert_f32(c[:k], r[name], bar[name], name)
    assert_f32(host(c[:k])[zero[:k]], closed[zero[:k]], bar[name][zero[:k]],
               name + ' at 0')
    # the seeds from the coefficient this launch stored: w lrelu', then the
    # product with the coefficient -- two f32 roundings (2^-149 each where the
    # product is subnormal), then the activation's
    want = host(c[:k])[:, None, None] * g[:k]
    assert_act(delta[:k, :, :C], want, f16,
               f32_err=2 * U * np.abs(want) + 2 * 2.0**-149)
    if Cp > C:  # +0 bit for bit
      assert int(delta[:k, :, C:].view(torch.int16).count_nonzero()) == 0, name
    assert float(c[k]) == SENT32 and is_sentinel(delta[k]), name


def _bce_ordered(d, f16, form, scales):
  ws = H.reduce_ws()
  o = _bce_outputs(d, f16)
  _bce_launch(d, o, form, scales, ws)
  H.sync()
  return o, ws[:3 * d['B'] + 16].clone()


def test_bce_head_planted_logits(precision):
  """Both segments carry every logit of pointwise_ref.bce_planted_logits (in
  opposite orders) and four dense rows.  The three guards of the arithmetic --
  the sign split of the sigmoid, -s(-x) for s(x) - 1, log1p -- each decide one
  segment's seed or term at one sign; past |x| = 87 the f32 results run through
  the subnormals down to 0, where the bars are multiples of 2^-149.  (bf16: the
  largest finite logits make the LOSS bars as large as that term's rounding; the
  losses are pinned by the other tests.)"""
  f16 = precision
  x = R.bce_planted_logits(f16)
  d = _bce_case(1900, 4, 12, 16, f16, x, x[::-1], 4)
  for scales, S_d, S_g in _bce_scales(f16):
    def launch(o, ws):
      _bce_launch(d, o, 'all', scales, ws)
      if ws is not None:
        launch.terms = ws[:3 * d['B'] + 16]
    atom, order = three_forms(launch, lambda zero: _bce_outputs(d, f16, zero))
    _bce_check(d, atom, None, f16, 'all', S_d, S_g)
    _bce_check(d, order, launch.terms.clone(), f16, 'all', S_d, S_g)
    # the dense rows' logits are where the issue wants them
    assert (np.abs(host(order[0][:2 * d['B']])[np.isnan(d['planted'])]) <= 30).all()


# F = Lt Cp: NT = 256 below 8192, 1024 from there on; F / 8 <= 4096 groups stay in
# LDS between the passes, more are read again; C picks the path of load8f
BCE_SHAPES = [(1, 8, 8),         # one lane
              (3, 5, 8),         # scalar weight loads, padded channels
              (5, 10, 16),       # 8-byte weight loads and a scalar tail group
              (4, 12, 16),       # 16-byte weight loads, C < Cp
              (341, 21, 24),     # F = 8184, the last size of NT = 256; 1023 groups
              (256, 32, 32),     # F = 8192, the first size of NT = 1024
              (2049, 6, 8),      # F = 16392: a second trip of the NT = 1024 loop
              (128, 250, 256),   # F / 8 = 4096: the row array exactly full
              (241, 130, 136)]   # F / 8 = 4097: the first size that reads h again


def test_bce_shapes_sit_on_the_dispatch_edges():
  F = [Lt * Cp for Lt, _, Cp in BCE_SHAPES]
  assert 8184 in F and 8192 in F and 4096 * 8 in F and 4097 * 8 in F
  assert any(f > 2 * 1024 * 8 for f in F)          # kNB = 2 loads x 1024 lanes x 8
  assert {C % 4 == 0 for _, C, _ in BCE_SHAPES} == {True, False}
  assert any(C % 2 == 0 and C % 4 for _, C, _ in BCE_SHAPES)


@pytest.mark.parametrize('form', ['all', 'disc', 'validate'])
@pytest.mark.parametrize('Lt,C,Cp', BCE_SHAPES)
def test_bce_head_shapes(Lt, C, Cp, form, precision):
  """B = 2: per segment one one-hot row (logits -0.75 and 20.25 with the bias)
  and one dense row."""
  f16 = precision
  d = _bce_case(2000 + Lt + C, Lt, C, Cp, f16, [-1.0], [20.0], 1, bias=0.25)
  for scales, S_d, S_g in _bce_scales(f16):
    if form == 'validate' and scales[0] is not None:
      continue  # (the form passes no scales: the same launch again)
    o, terms = _bce_ordered(d, f16, form, scales)
    _bce_check(d, o, terms, f16, form, S_d, S_g)
    assert (np.abs(host(o[0][:4])[np.isnan(d['planted'])]) <= 30).all()


@pytest.mark.parametrize('Lt,C,Cp', [(128, 250, 256), (241, 130, 136)])
def test_bce_head_validate_form_has_the_bits_of_the_training_form(Lt, C, Cp,
                                                                  precision):
  """"Same sum order": with the row kept in LDS, with h read again, and in the
  validate form's kernel without a second pass -- the same logits and losses."""
  f16 = precision
  d = _bce_case(2000 + Lt + C, Lt, C, Cp, f16, [-1.0], [20.0], 1, bias=0.25)
  a, _ = _bce_ordered(d, f16, 'all', (None, None))
  v, _ = _bce_ordered(d, f16, 'validate', (None, None))
  assert torch.equal(bits(a[0]), bits(v[0])) and torch.equal(bits(a[5]), bits(v[5]))


BCE_LIST = [0.0, -0.0, 2.0**-10, -2.0**-10, 1.0, -1.0, 20.0, -20.0, 40.0, -40.0,
            88.0, -88.0, 0.5, -3.0, 7.25, -12.5]


@pytest.mark.parametrize('B', BS)
def test_bce_head_batch_sizes(B, precision):
  """dense1_bce_finish strides over b by 256 and reads terms[B + b], terms[2B +
  b]: B around the wave and the block, and B = 1.  Every logit is one of sixteen
  exactly representable values, the segments five positions apart."""
  f16 = precision
  fake = [BCE_LIST[i % 16] for i in range(B)]
  real = [BCE_LIST[(i + 5) % 16] for i in range(B)]
  d = _bce_case(2200 + B, 1, 8, 8, f16, fake, real, 0)
  scales, S_d, S_g = _bce_scales(f16)[-1]

  def launch(o, ws):
    _bce_launch(d, o, 'all', scales, ws)
    if ws is not None:
      launch.terms = ws[:3 * B + 16]

  atom, order = three_forms(launch, lambda zero: _bce_outputs(d, f16, zero))
  _bce_check(d, atom, None, f16, 'all', S_d, S_g)
  _bce_check(d, order, launch.terms.clone(), f16, 'all', S_d, S_g)


def test_bce_head_refusals():
  """Every check of cg_dense1_bce precedes the launch: CG_EINVAL, and every
  output still the sentinel."""
  lib = _lib.load()
  d = _bce_case(2300, 2, 8, 8, False, [1.0], [-1.0], 0)
  o = _bce_outputs(d, False)
  ws = H.reduce_ws()
  p = [H.p(t) for t in (d['hd'], d['wd'], d['bd'])] + [H.p(t) for t in o]
  h, w, bias, out, cd, cg, dd, dg, loss = range(9)

  def rc(B=1, C=8, Cp=8, null=(), ws=ws):
    a = [None if i in null else x for i, x in enumerate(p)]
    return lib.cg_dense1_bce(a[h], a[w], a[bias], a[out], a[cd], a[cg], a[dd], a[dg],
                             a[loss], None, None, B, 2, C, Cp, ALPHA, H.p(ws),
                             H.stream())

  assert rc(Cp=12, C=8) == _lib.CG_EINVAL   # Cp % 8
  assert rc(C=9) == _lib.CG_EINVAL          # C > Cp
  assert rc(B=0) == _lib.CG_EINVAL
  for i in (h, w, bias, out, loss):
    assert rc(null=(i,)) == _lib.CG_EINVAL, i
  assert rc(null=(dd,)) == _lib.CG_EINVAL   # delta_g without delta_d
  # the first B whose 3B terms do not fit the workspace (its size below is NOT
  # launched: 2.8 M blocks)
  B_big = lib.cg_reduce_ws_elems() // 3 + 1
  assert 3 * B_big > lib.cg_reduce_ws_elems() >= 3 * (B_big - 1)
  assert rc(B=B_big) == _lib.CG_EINVAL
  H.sync()
  for t in o:
    assert is_sentinel(t)
  assert torch.isnan(ws[:64]).all()


# ---------------------------------------------------------------------------
# cg_finish_defer / cg_finish_flush
# ---------------------------------------------------------------------------
def _defer_entries(f16):
  """Thirteen ordered reductions -- one more than a batch holds.  Entry 5 needs
  ten column blocks and the cg_ln_lrelu_bwd entries three outputs: every other
  entry's surplus blocks of the batched grid must return early.  The two
  cg_signal_metrics entries queue scale = 1 / rows with different rows."""
  rng = np.random.RandomState(2400)
  ract = lambda *s: dev_act(R.round_act(rng.randn(*s), f16), f16)

  def colsum(rows, C, Cp):
    x = ract(rows, Cp)

    def run(o, ws):
      _lib.call('cg_colsum', H.p(x), H.p(o[0]), rows, C, Cp, H.p(ws), H.stream())

    return dict(name='colsum %d %d %d' % (rows, C, Cp), run=run, reduced=(0,),
                cvalid=C, gx=(Cp + 63) // 64, outs=lambda: [sent32(Cp + 1)])

  def ln_bwd(rows, C, Cp, dbias):
    dh, h, y = ract(rows, Cp), ract(rows, Cp), ract(rows, Cp)
    mean, rstd = dev32(0.5 * rng.randn(rows)), dev32(rng.uniform(0.3, 2.0, rows))
    gamma = dev32(rng.rand(Cp) + 0.5)

    def run(o, ws):
      _lib.call('cg_ln_lrelu_bwd', H.p(dh), H.p(h), H.p(y), H.p(mean), H.p(rstd),
                H.p(gamma), H.p(o[0]), H.p(o[1]), H.p(o[2]),
                H.p(o[3]) if dbias else None, rows, C, Cp, ALPHA, H.p(ws),
                H.stream())

    nred = 3 if dbias else 2
    return dict(name='ln_bwd %d %d %d %d' % (rows, C, Cp, dbias), run=run,
                reduced=tuple(range(1, 1 + nred)), cvalid=C,
                gx=(Cp + 63) // 64,
                outs=lambda: [sent_act((rows + 1, Cp), f16)] +
                [sent32(Cp + 1) for _ in range(nred)])

  def metrics(rows, C, Cr, Cf):
    real, fake = dev32(rng.rand(rows, Cr)), dev32(rng.rand(rows, Cf))

    def run(o, ws):
      _lib.call('cg_signal_metrics', H.p(real), H.p(fake), H.p(o[0]), rows, C, Cr, Cf,
                -0.5, 2.5, H.p(ws), H.stream())

    return dict(name='metrics %d %d' % (rows, C), run=run, reduced=(0,), cvalid=4,
                gx=1, outs=lambda: [sent32(5)])

  entries = [colsum(1, 1, 8), ln_bwd(37, 5, 8, True), metrics(63, 6, 7, 8),
             colsum(300, 70, 72), ln_bwd(1000, 500, 512, False),
             colsum(5000, 600, 608), metrics(3000, 102, 102, 103),
             ln_bwd(300, 8, 8, False), ln_bwd(700, 512, 512, True),
             colsum(2000, 5, 8), ln_bwd(129, 30, 32, True), colsum(257, 102, 104),
             colsum(4097, 16, 16)]
  assert len(entries) == 13
  return entries


def _same_bits(o, ref, what):
  for k, (a, b) in enumerate(zip(o, ref)):
    assert torch.equal(bits(a), bits(b)), (what, k)


def _run_deferred(lib, entries, ref, regions):
  """Queue the thirteen with deferred finishes, checking at every stage what has
  and has not been stored; returns the outputs after the flush."""
  regions.fill_(float('nan'))
  outs = [e['outs']() for e in entries]
  try:
    assert lib.cg_finish_defer(1) == 0
    assert lib.cg_finish_defer(1) == 1
    for e, o, ws in zip(entries[:12], outs, regions):
      e['run'](o, ws)
    H.sync()
    # twelve queued: no sum is stored yet, what is not a sum (dy) is
    for e, o, r in zip(entries[:12], outs, ref):
      for k in range(len(o)):
        if k in e['reduced']:
          assert is_sentinel(o[k]), (e['name'], k)
        else:
          assert torch.equal(bits(o[k]), bits(r[k])), (e['name'], k)
    # the thirteenth finds the batch full: the twelve are added, it is queued
    entries[12]['run'](outs[12], regions[12])
    H.sync()
    for e, o, r in zip(entries[:12], outs, ref):
      _same_bits(o, r, e['name'])
    for k in entries[12]['reduced']:
      assert is_sentinel(outs[12][k]), (entries[12]['name'], k)
    assert lib.cg_finish_flush(H.stream()) == 0
    H.sync()
    for e, o, r in zip(entries, outs, ref):
      _same_bits(o, r, e['name'])
      for k in e['reduced']:  # columns at or past cvalid, and the guard
        assert is_sentinel(o[k][e['cvalid']:]), (e['name'], k)
    assert lib.cg_finish_defer(0) == 0  # the flush left the mode
  finally:
    lib.cg_finish_flush(H.stream())
    H.sync()
  return outs


def test_deferred_finishes_one_by_one(precision):
  """Each of thirteen reductions, finished in batched launches (twelve at the
  thirteenth call, one at the flush), has the bits of its own undeferred launch
  -- whose float64 parity test_colsum, test_ln_bwd and test_signal_metrics hold
  -- in either order of queueing."""
  f16 = precision
  lib = _lib.load()
  entries = _defer_entries(f16)
  # the widest grid (ten column blocks) is neither first nor last in either order
  gx = [e['gx'] for e in entries]
  assert max(gx) == 10 and gx.count(10) == 1 and gx.index(10) == 5
  regions = torch.empty(13, lib.cg_reduce_ws_elems(), dtype=torch.float32,
                        device=H.DEV)
  regions.fill_(float('nan'))
  assert lib.cg_finish_defer(0) == 0
  ref = []
  for e, ws in zip(entries, regions):
    o = e['outs']()
    e['run'](o, ws)
    H.sync()
    for k in e['reduced']:
      assert not is_sentinel(o[k][:e['cvalid']]), e['name']
    ref.append(o)
  outs = _run_deferred(lib, entries, ref, regions)
  # a flush with nothing queued: 0, and no buffer changes
  keep = regions.clone()
  assert lib.cg_finish_flush(H.stream()) == 0
  H.sync()
  for e, o, r in zip(entries, outs, ref):
    _same_bits(o, r, e['name'])
  assert torch.equal(regions.view(torch.int32), keep.view(torch.int32))
  del keep
  # the position in the batch does not matter
  _run_deferred(lib, entries[::-1], ref[::-1], regions)


# ---------------------------------------------------------------------------
# cg_loss_scale_update
# ---------------------------------------------------------------------------
LS_TABLE = [  # (S, good, t, flag, interval)
    (1024.0, 0.0, 4.0, 1.0, 3),        # finite, below the interval
    (1024.0, 2.0, 4.0, 1.0, 3),        # reaching it: doubles, good back to 0
    (1024.0, 0.0, 0.0, 1.0, 1),        # interval 1: doubles every time
    (1024.0, 7.0, 9.0, 1.0, 1),
    (2.0**127, 1999.0, 5.0, 1.0, 2000),  # doubling overflows: S stays, good to 0
    (2.0**127, 3.0, 5.0, 1.0, 2000),
    (1024.0, 5.0, 4.0, 0.0, 3),        # non-finite: halves, t stays, good 0
    (1.0, 5.0, 4.0, 0.0, 3),           # the floor
    (1.5, 5.0, 4.0, 0.0, 3),           # 0.75 -> 1
    (3.0, 2.0, 4.0, 0.0, 1),           # 1.5: not a power of two, above the floor
    (1.5, 2.0, 4.0, 1.0, 3),           # 3
]


@pytest.mark.parametrize('S,good,t,flag,interval', LS_TABLE)
def test_loss_scale_update(S, good, t, flag, interval):
  state = np.array([S, good, t, flag], np.float32)
  ls = dev32(np.r_[state, SENT32])
  _lib.call('cg_loss_scale_update', H.p(ls), interval, H.stream())
  H.sync()
  want = R.loss_scale_update(state, interval)
  assert want[3] == 1.0 and np.isfinite(want).all()
  np.testing.assert_array_equal(bits(ls[:4]).numpy(), want.view(np.int32))
  assert float(ls[4]) == SENT32
  if flag == 0:
    assert want[2] == t and want[1] == 0 and want[0] == max(S / 2, 1.0)
  elif good + 1 >= interval:
    assert want[1] == 0 and want[0] == (S if S == 2.0**127 else 2 * S)


def test_loss_scale_update_refusals():
  lib = _lib.load()
  ls = sent32(4)
  assert lib.cg_loss_scale_update(None, 3, H.stream()) == _lib.CG_EINVAL
  assert lib.cg_loss_scale_update(H.p(ls), 0, H.stream()) == _lib.CG_EINVAL
  H.sync()
  assert is_sentinel(ls)
