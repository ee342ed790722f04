"""Float64 parity of cg_swconv (calciumgan_amd/csrc/swconv.hip, swconv_swp.hip)
and cg_unshuffle_fixup in both precision builds, at the smallest shapes that
reach each dispatch target of swconv_run / swconv_swp_launch.

Every case compares ONE launch with the float64 statement of tests/swconv_ref.py
(tied to autograd of the oracle's layers in tests/test_swconv_ref.py).  Recipes:
rounded reals (one activation ulp plus the derived f32 bar), operands with every
significand bit in use whose sums are exact in f32 and mostly not representable
in the activation type -- exact ties and, in fp16, sums beyond 65504 among them
-- compared bit for bit, special values, subnormal operands.  The weights are
laid out by wgrad_ref.pack (the packer has its own parity tests), so a failure
here is the convolution's.  Every output is over-allocated and holds a sentinel:
rows and guard elements the launch does not own must still hold it afterwards;
split-K and rowsumsq workspaces start as NaN.  Bars: bit-equal or derived in
swconv_ref -- never a measured number.  The parametrisation is built at collection
time from cg_swconv_check: admissible combinations only."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from calciumgan_amd import _lib

import hip_utils as H
import pointwise_ref as R
import swconv_ref as S
import test_hip_pointwise as P
import wgrad_ref as W
from test_hip_pointwise import precision, _back_to_bf16  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

EINVAL = _lib.CG_EINVAL
GUARD = 64
ALPHA = 0.3
A32 = R.f32(ALPHA)
EXACT_ALPHA = 0.25   # the exact recipe's slope: products with it stay exact
LN_EPS = 1e-3
CLASSIC = sorted(_lib.TILES)
SWP = sorted(_lib.SWP_TILES)
LEAN = (13, 14, 15)
LN_CLASSIC = (5, 6, 7, 8)
LN_SWP = (11, 12, 15)


# ---------------------------------------------------------------------------
# descriptors
# ---------------------------------------------------------------------------
def desc_of(G, tile, ks=2, sp=0, pmajor=0, narrow=0, epi=S.EPI_NONE, out_f32=0,
            alpha=ALPHA, CK=32, ksplit=0):
  """cg_conv_desc of geometry G with placeholder pointers (enough for
  cg_swconv_check; Launch fills in the real ones)."""
  d = _lib.ConvDesc()
  d.x = d.w = d.y = 64
  d.nB, d.Lx, d.Cx, d.seg_size = G.nB, G.Lx, G.Cx, G.seg
  d.taps, d.stride, d.off, d.Lu = G.taps, G.stride, G.off, G.Lu
  d.N, d.Ly, d.Cy, d.y_stride, d.y_off = G.N, G.Ly, S.pitch8(G.N), G.y_stride, G.y_off
  d.CK, d.epilogue, d.out_f32, d.alpha = CK, epi, out_f32, alpha
  d.nphase = G.nphase
  d.w_phase_stride = W.packed_elems(G.N, G.taps, G.Cx, CK)
  d.off_phase_step, d.yoff_phase_step = G.off_step, G.yoff_step
  d.tile, d.stage_ksteps, d.split_parity = tile, ks, sp
  d.w_parity_major, d.w_narrow_last = pmajor, narrow
  if G.shifts is not None:
    d.shifts = 64
  if epi == S.EPI_MASK:
    d.mask_src = 64
  if epi == S.EPI_LN:
    d.ln_gamma = d.ln_beta = d.ln_h = d.ln_mean = d.ln_rstd = 64
    d.ln_eps = LN_EPS
  if ksplit:
    d.ksplit, d.split_ws, d.split_ws_elems = ksplit, 64, 1 << 40
  return d


def admits(d):
  return _lib.load().cg_swconv_check(ctypes.byref(d)) == 0


def refused(d):
  lib = _lib.load()
  return (lib.cg_swconv_check(ctypes.byref(d)) == EINVAL and
          lib.cg_swconv(ctypes.byref(d), H.stream()) == EINVAL)


# ---------------------------------------------------------------------------
# dispatch targets: (name, G, keyword arguments of desc_of, exact recipe only)
# ---------------------------------------------------------------------------
MORE_TILES = (1, 4, 6, 8)  # MFMA 16x16x32 and 32x32x16, 64 and 128 columns
CLASSIC_MF = {0: 16, 1: 16, 2: 16, 3: 32, 4: 32, 5: 32, 6: 32, 7: 16, 8: 16}


def rows_of_tile(tile):
  return _lib.tile_shape(tile)[0]


def _targets():
  out = []
  for tile in CLASSIC:
    for ks in (2, 4):
      for G in (S.CLASSIC_DOWN[0], S.CLASSIC_UP[0]):
        out.append(('classic', G, dict(tile=tile, ks=ks), False))
      for G in (S.NON_UNI, S.NON_UNI_UP):
        out.append(('nonuni', G, dict(tile=tile, ks=ks, CK=40), False))
      out.append(('sp', S.CLASSIC_DOWN[0], dict(tile=tile, ks=ks, sp=1, pmajor=1), False))
      for sp in (0, 1):
        out.append(('narrow', S.CLASSIC_DOWN[3],
                    dict(tile=tile, ks=ks, sp=sp, pmajor=1, narrow=1), False))
    # Lu = the tile's rows and twice that
    out.append(('full', S.FULL_TILE[rows_of_tile(tile)], dict(tile=tile), False))
    out.append(('two', S.TWO_TILES[rows_of_tile(tile)], dict(tile=tile), False))
  # 1 / 2 / 8 taps, Lu = 4 and 16 (several samples in a partly empty last tile), Cx = 64
  # / 96, N = 6 / 64 / 102 / 130, the phases' rows the other way round
  for tile in MORE_TILES:
    for G in S.CLASSIC_MORE:
      out.append(('more', G, dict(tile=tile), False))
  for tile in SWP:
    out.append(('swp', S.SWP_UP, dict(tile=tile), False))
    out.append(('full', S.FULL_TILE[rows_of_tile(tile)], dict(tile=tile), False))
    out.append(('swp', S.SWP_DOWN, dict(tile=tile, pmajor=1), False))
    out.append(('swpnarrow', S.SWP_DOWN_NARROW, dict(tile=tile, pmajor=1, narrow=1), False))
  for tile in LN_CLASSIC:
    for ks in (2, 4):
      for G in S.LN_GEOMS:
        out.append(('ln', G, dict(tile=tile, ks=ks, epi=S.EPI_LN), False))
  for tile in LN_SWP:
    for G in S.LN_GEOMS[:2]:
      out.append(('ln', G, dict(tile=tile, epi=S.EPI_LN), False))
  for epi in (S.EPI_NONE, S.EPI_LRELU, S.EPI_MASK):
    for ksplit in (2, 4):
      out.append(('splitk', S.SPLIT_CLASSIC, dict(tile=2, ksplit=ksplit, epi=epi), False))
    out.append(('splitk', S.SPLIT_SWP2, dict(tile=13, ksplit=2, epi=epi, pmajor=1), False))
    out.append(('splitk', S.SPLIT_SWP4, dict(tile=13, ksplit=4, epi=epi, pmajor=1), True))
  out += _sweep_targets()
  return out


SWEEP_TILES = ((0, 2), (0, 4), (1, 2), (1, 4), (2, 2), (2, 4), (4, 2))


def _sweep_targets():
  """Every admitted kernel size other than 24, 8 and 2 (swconv_ref.TAP_SWEEP): the
  tiles nets._conv_desc's static rule picks (0, 1, 2) at both stage depths and one
  32x32x16 tile, with the operand order nets packs (parity-major at stride 2; the
  32x32x16 tile walks the plain order), the narrow last chunk from 6 taps on,
  split-parity staging on tile 1 wherever the check admits it, a three-chunk walk
  with several samples per tile, and the fused LayerNorm at k = 6 and 22."""
  out = []
  for k in S.TAP_SWEEP:
    for tile, ks in SWEEP_TILES:
      pm = int(tile != 4)
      out.append(('taps', S.K_DOWN[k], dict(tile=tile, ks=ks, pmajor=pm), False))
      out.append(('taps', S.K_UP[k], dict(tile=tile, ks=ks), False))
      if k in S.K_DOWN_NARROW:
        out.append(('tapsnarrow', S.K_DOWN_NARROW[k],
                    dict(tile=tile, ks=ks, pmajor=1, narrow=1), False))
    for ks in (2, 4):
      out.append(('tapssp', S.K_DOWN[k], dict(tile=1, ks=ks, sp=1, pmajor=1), False))
      if k in S.K_DOWN_NARROW:
        out.append(('tapssp', S.K_DOWN_NARROW[k],
                    dict(tile=1, ks=ks, sp=1, pmajor=1, narrow=1), False))
    for tile, ks in ((1, 2), (1, 4), (4, 2)):
      out.append(('tapsmulti', S.K_DOWN_MULTI[k], dict(tile=tile, ks=ks, pmajor=int(tile != 4)),
                  False))
  for k, G in sorted(S.K_UP_LN.items()):
    for tile in LN_CLASSIC:
      for ks in (2, 4):
        out.append(('tapsln', G, dict(tile=tile, ks=ks, epi=S.EPI_LN), False))
  return out


def _tid(name, G, kw):
  bits = ['t{}'.format(kw['tile']), 'k{}'.format(kw.get('ks', 2)), name, S.gid(G)]
  for k in ('sp', 'pmajor', 'narrow', 'ksplit', 'epi'):
    if kw.get(k):
      bits.append('{}{}'.format(k, kw[k]))
  return '-'.join(bits)


def dispatch_cases():
  """The admissible targets (the same list in both builds: the check is host
  logic) as pytest params."""
  out = []
  for name, G, kw, exact_only in _targets():
    kw = dict(kw)
    kw.setdefault('epi', S.sweep_epi(G))
    if admits(desc_of(G, **kw)):
      out.append(pytest.param(G, kw, exact_only, id=_tid(name, G, kw)))
  return out


def recipes_of(G, exact_only):
  """The recipes a dispatch case runs (the enumeration test of
  tests/test_swconv_ref.py reads them too)."""
  return ('exact',) if exact_only or G in S.EXACT_ONLY else ('real', 'exact')


# lean forms of the 32-row software-pipelined tiles (cg_debug_lean_epilogue(1)):
# (form, G, desc keywords, extra)
def lean_cases():
  out = []
  for tile in LEAN:
    rows = _lib.tile_shape(tile)[0]
    forms = [('lrelu', S.SWP_UP, dict(epi=S.EPI_LRELU)),
             ('lrelu', S.SWP_DOWN, dict(epi=S.EPI_LRELU, pmajor=1)),
             ('lrelu', S.SWP_DOWN_NARROW, dict(epi=S.EPI_LRELU, pmajor=1, narrow=1)),
             ('mask', S.SWP_DOWN, dict(epi=S.EPI_MASK, pmajor=1)),
             ('mask', S.SWP_DOWN_NARROW, dict(epi=S.EPI_MASK, pmajor=1, narrow=1)),
             ('maskshift', S.SWP_UP, dict(epi=S.EPI_MASK)),
             ('lrelussq', S.FULL_TILE[rows], dict(epi=S.EPI_LRELU))]
    for form, G, kw in forms:
      kw = dict(kw, tile=tile)
      if admits(desc_of(G, **kw)):
        out.append(pytest.param(form, G, kw, id='lean-{}-{}'.format(form, _tid('swp', G, kw))))
  return out


# ---------------------------------------------------------------------------
# data and launches
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(G, f16, recipe, sigmoid=False):
  """Operands of a recipe at a geometry, computed once."""
  if recipe == 'real':
    x, Wl, bias = S.real_recipe(G, f16, sigmoid)
    plants = None
  else:
    x, Wl, bias, plants = S.exact_recipe(G, f16)
  rng = np.random.RandomState(S.seed_of(G) + 5)
  mask = R.round_act(rng.randn(G.nB, G.Ly, G.N), f16)
  mask[:, :, 0] = 0.0
  mask[:, :, 1] = -0.0
  return dict(x=x, Wl=Wl, bias=bias, plants=plants, mask=mask)


@functools.lru_cache(maxsize=64)
def packed(G, f16, recipe, sigmoid, CK, pmajor, narrow):
  """The packed operand (all phases) as float64 values, laid out by wgrad_ref.pack."""
  Wl = case(G, f16, recipe, sigmoid)['Wl']
  d = W.PackDesc(G.taps, G.Cr, G.N, G.Cx, CK, parity_major=pmajor, narrow_last=narrow)
  return np.concatenate([W.pack(Wl[z], d, f16) for z in range(G.nphase)])


def pad_dev(a, Cp, f16, fill=0.0):
  """(nB, L, C) values of the activation type -> device (nB, L, Cp)."""
  t = torch.full((a.shape[0], a.shape[1], Cp), fill, dtype=R.act_dtype(f16), device=H.DEV)
  t[:, :, :a.shape[2]] = P.dev_act(a, f16)
  return t


class Launch(object):
  """One cg_swconv descriptor over fresh, over-allocated sentinel outputs."""

  def __init__(self, G, c, f16, recipe='real', sigmoid=False, bias=True, mask=None,
               row_scale=None, ln=None, ssq=None, out_shifts=None, x=None, **kw):
    self.G, self.f16, self.kw = G, f16, kw
    d = self.d = desc_of(G, **kw)
    self.Cy = d.Cy
    self.xd = pad_dev(c['x'] if x is None else x, G.Cx, f16)
    self.wd = P.dev_act(packed(G, f16, recipe, sigmoid, kw.get('CK', 32),
                               kw.get('pmajor', 0), kw.get('narrow', 0)), f16)
    d.x, d.w = self.xd.data_ptr(), self.wd.data_ptr()
    n = G.nB * G.Ly * d.Cy
    self.n = n
    self.y = (P.sent32(n + GUARD) if d.out_f32 else P.sent_act((n + GUARD,), f16))
    d.y = self.y.data_ptr()
    self.bias = None
    self.h = self.mean = self.rstd = self.ws = self.ssq_ws = None
    if bias:
      self.bias = P.dev32(np.r_[c['bias'], [np.nan] * 8])
      d.bias = self.bias.data_ptr()
    if G.shifts is not None:
      self.sh = torch.tensor(G.shifts, dtype=torch.int32, device=H.DEV)
      d.shifts = self.sh.data_ptr()
    self.mask = None
    if d.epilogue == S.EPI_MASK:
      m = c['mask'] if mask is None else mask
      if isinstance(m, str):  # in place: y holds the mask source
        self.y[:n] = pad_dev(c['mask'], d.Cy, f16).reshape(-1)
        d.mask_src = d.y
      else:
        self.mask = pad_dev(m, d.Cy, f16)
        d.mask_src = self.mask.data_ptr()
    if row_scale is not None:
      self.rs = P.dev32(row_scale)
      d.row_scale = self.rs.data_ptr()
    if d.epilogue == S.EPI_LN:
      gamma, beta, stats = ln
      self.gamma, self.beta = P.dev32(np.r_[gamma, [np.nan] * 8]), P.dev32(
          np.r_[beta, [np.nan] * 8])
      self.h = P.sent_act((n + GUARD,), f16)
      self.mean, self.rstd = P.sent32(G.nB * G.Ly + GUARD), P.sent32(G.nB * G.Ly + GUARD)
      d.ln_gamma, d.ln_beta, d.ln_h = (self.gamma.data_ptr(), self.beta.data_ptr(),
                                       self.h.data_ptr())
      d.ln_mean = self.mean.data_ptr() if stats else None
      d.ln_rstd = self.rstd.data_ptr() if stats else None
    if d.ksplit:
      self.ws = torch.full((d.ksplit * n + GUARD,), float('nan'), device=H.DEV)
      d.split_ws, d.split_ws_elems = self.ws.data_ptr(), d.ksplit * n
    self.ssq = None
    if ssq:
      self.ssq = torch.zeros(G.nB + GUARD, device=H.DEV) if ssq == 'atomic' else P.sent32(
          G.nB + GUARD)
      self.ssq[G.nB:] = P.SENT32
      d.rowsumsq = self.ssq.data_ptr()
      if ssq != 'atomic':
        self.need = _lib.load().cg_rowsumsq_ws_elems(ctypes.byref(d))
        assert self.need > 0
        self.ssq_ws = torch.full((self.need + GUARD,), float('nan'), device=H.DEV)
        d.rowsumsq_ws, d.rowsumsq_ws_elems = self.ssq_ws.data_ptr(), self.need
        d.rowsumsq_defer = int(ssq == 'defer')
    self.side = None
    if out_shifts is not None:
      sh, seg, side_rows = out_shifts
      self.osh = torch.tensor(sh, dtype=torch.int32, device=H.DEV)
      self.side_rows = side_rows
      self.side = P.sent_act((G.nB * side_rows * d.Cy + GUARD,), f16)
      d.out_shifts, d.out_seg_size = self.osh.data_ptr(), seg
      d.side, d.side_rows = self.side.data_ptr(), side_rows

  def run(self):
    assert admits(self.d), 'not admitted by cg_swconv_check'
    rc = _lib.load().cg_swconv(ctypes.byref(self.d), H.stream())
    H.sync()
    return rc

  def view(self, t):
    return t[:self.n].reshape(self.G.nB, self.G.Ly, self.Cy)

  def untouched(self):
    return all(P.is_sentinel(t) for t in (self.y, self.side) if t is not None)

  def check_frame(self, t, own):
    """Guard and un-addressed rows still hold the sentinel; the channel padding of
    every addressed row is +0.  own: (Ly,) or (nB, Ly)."""
    assert P.is_sentinel(t[self.n:])
    v = self.view(t)
    own = np.broadcast_to(own, (self.G.nB, self.G.Ly))
    mine = torch.tensor(own, device=t.device)
    if bool((~mine).any()):
      assert P.is_sentinel(v[~mine])
    pad = v[mine][:, self.G.N:]
    assert int(P.bits(pad).numpy().astype(np.int64).__abs__().sum()) == 0, 'padding not +0'

  def compare(self, t, want, own, exact, err=0.0, what=''):
    """t against the statement on the addressed rows' N real channels."""
    self.check_frame(t, own)
    own = np.broadcast_to(own, (self.G.nB, self.G.Ly))
    got = self.view(t)[torch.tensor(own, device=t.device)][:, :self.G.N]
    want, err = want[own], np.broadcast_to(err, want.shape)[own]
    if t.dtype == torch.float32:
      if exact:
        np.testing.assert_array_equal(P.host(got), want, err_msg=what)
      else:
        P.assert_f32(got, want, err, what)
    elif exact:
      P.assert_bits(got, want, self.f16)
    else:
      P.assert_act(got, want, self.f16, f32_err=err)


def statement(G, c, f16, epi, alpha, bias=True, row_scale=None, ksplit=1, x=None):
  """(y, own, err) of the pointwise epilogues."""
  b = c['bias'] if bias else None
  x = c['x'] if x is None else x
  y, own = S.swconv(G, x, c['Wl'], b, epi, R.f32(alpha), c['mask'], row_scale)
  v = S.place(G, S.linear(G, x, c['Wl'], b))[0]
  err = S.epilogue_bound(S.acc_bound(G, c['x'], c['Wl'], b, ksplit), v, y, epi, row_scale)
  return y, own, err


def ln_params(G):
  rng = np.random.RandomState(S.seed_of(G) + 9)
  gamma = (rng.rand(G.N) + 0.5).astype(np.float32).astype(np.float64)
  beta = (0.1 * rng.randn(G.N)).astype(np.float32).astype(np.float64)
  return gamma, beta


def check_ln_exact(L, c, what):
  """The exact recipe under the fused LayerNorm: the f32 pre-activation is exact, so
  y is its rounding bit for bit (ties to even; fp16: +-2^16 is +-inf) and the
  statistics are those of exactly these values: the bars are the f32 evaluation's
  alone (err = 0).  A row that holds an infinity (fp16: +inf and -inf, the
  overflow plants) has a NaN mean and NaN activations, and no other row does."""
  G, f16 = L.G, L.f16
  gamma, beta = ln_params(G)
  pre, own = S.swconv(G, c['x'], c['Wl'], c['bias'])
  L.compare(L.y, pre, own, True, what=what + ' y')
  got_y = P.host(L.view(L.y))
  for b, t, n, _ in c['plants']['ties']:
    assert pre[b, t, n] != R.round_act(pre[b, t, n], f16)
    assert got_y[b, t, n] == R.round_act(pre[b, t, n], f16)
  bad = ~np.isfinite(R.round_act(pre, f16)).all(axis=-1)
  assert bad.any() == bool(f16) and bad.sum() <= 1
  safe = np.where(bad[:, :, None], 0.0, pre)
  y, h, mean, rstd = S.layernorm(safe, gamma, beta, R.f32(LN_EPS), A32, f16)
  e_h, e_mean, e_rstd = S.layernorm_bounds(safe, 0.0 * safe, gamma, beta, R.f32(LN_EPS), A32,
                                           f16)
  L.check_frame(L.h, own)
  ok = np.broadcast_to(own, bad.shape) & ~bad
  got_h = P.host(L.view(L.h))[:, :, :G.N]
  m = P.host(L.mean[:G.nB * G.Ly]).reshape(G.nB, G.Ly)
  r = P.host(L.rstd[:G.nB * G.Ly]).reshape(G.nB, G.Ly)
  # (ln_rstd of such a row is left open: the kernels clamp a NaN variance to zero)
  assert np.isnan(got_h[bad]).all() and np.isnan(m[bad]).all(), what + ' NaN row'
  rh = R.round_act(h, f16)
  assert (np.abs(got_h[ok] - rh[ok]) <= R.ulp_act(rh[ok], f16) + e_h[ok]).all(), what + ' h'
  P.assert_f32(m[ok], mean[ok], e_mean[ok], what + ' mean')
  P.assert_f32(r[ok], rstd[ok], e_rstd[ok], what + ' rstd')


def check_ln(L, c, stats=True, what='', exact=False):
  """The fused LayerNorm launch against the statement and its derived bars."""
  if exact:
    return check_ln_exact(L, c, what)
  G, f16 = L.G, L.f16
  gamma, beta = ln_params(G)
  pre, own = S.swconv(G, c['x'], c['Wl'], c['bias'])
  err = S.acc_bound(G, c['x'], c['Wl'], c['bias'])
  y, h, mean, rstd = S.layernorm(pre, gamma, beta, R.f32(LN_EPS), A32, f16)
  e_h, e_mean, e_rstd = S.layernorm_bounds(pre, err, gamma, beta, R.f32(LN_EPS), A32, f16)
  L.compare(L.h, h, own, False, e_h, what + ' h')
  ridx = np.broadcast_to(own, (G.nB, G.Ly))
  if stats:
    L.compare(L.y, pre, own, False, err, what + ' y')
    m = P.host(L.mean[:G.nB * G.Ly]).reshape(G.nB, G.Ly)
    r = P.host(L.rstd[:G.nB * G.Ly]).reshape(G.nB, G.Ly)
    P.assert_f32(m[ridx], mean[ridx], e_mean[ridx], what + ' mean')
    P.assert_f32(r[ridx], rstd[ridx], e_rstd[ridx], what + ' rstd')
    assert (m[~ridx] == P.SENT32).all() and (r[~ridx] == P.SENT32).all()
    assert P.is_sentinel(L.mean[G.nB * G.Ly:]) and P.is_sentinel(L.rstd[G.nB * G.Ly:])
  else:
    assert P.is_sentinel(L.y) and P.is_sentinel(L.mean) and P.is_sentinel(L.rstd)


# ---------------------------------------------------------------------------
# every dispatch target
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('G,kw,exact_only', dispatch_cases())
def test_every_dispatch_target(G, kw, exact_only, precision):
  """The nine classic tiles x stage depth x stride, UNI and the CK = 40 walk,
  split-parity, the narrow last chunk with and without split-parity residency, the
  seven software-pipelined tiles x stride 1 / 2 / 2 narrow, the LayerNorm
  instantiations and split-K, and the classic tiles at every kernel size from 4 to 22
  (_sweep_targets) -- rounded reals within the bar, then the exact recipe bit for bit
  (ties round to even; fp16 sums beyond 65504 are +-inf)."""
  f16 = precision
  epi = kw['epi']
  if epi == S.EPI_LN:
    for recipe in recipes_of(G, exact_only):
      c = case(G, f16, recipe)
      L = Launch(G, c, f16, recipe, ln=ln_params(G) + (True,), **kw)
      assert L.run() == 0
      check_ln(L, c, what=recipe, exact=recipe == 'exact')
    return
  mask = 'inplace' if kw.get('ksplit') else None
  for recipe in recipes_of(G, exact_only):
    c = case(G, f16, recipe)
    alpha = ALPHA if recipe == 'real' else EXACT_ALPHA
    L = Launch(G, c, f16, recipe, mask=mask, alpha=alpha, **kw)
    assert L.run() == 0, recipe
    y, own, err = statement(G, c, f16, epi, alpha, ksplit=kw.get('ksplit') or 1)
    L.compare(L.y, y, own, recipe == 'exact', err, recipe)
    if recipe == 'exact':
      # the plants, through the epilogue (a slope of 1/4 keeps a tie a tie)
      got = P.host(L.view(L.y))
      for b, t, n, _ in c['plants']['ties']:
        v = y[b, t, n]
        assert v != R.round_act(v, f16) and got[b, t, n] == R.round_act(v, f16)
      if f16:
        over = [(got[b, t, n], y[b, t, n]) for b, t, n, _ in c['plants']['over']]
        assert all(g == R.round_act(v, f16) for g, v in over)
        assert any(np.isinf(g) for g, _ in over) or epi == S.EPI_MASK
    if kw.get('ksplit'):
      assert bool(torch.isnan(L.ws[L.d.ksplit * L.n:]).all())


@pytest.fixture
def lean():
  was = _lib.load().cg_debug_lean_epilogue(1)
  yield
  _lib.load().cg_debug_lean_epilogue(was)


@pytest.mark.parametrize('form,G,kw', lean_cases())
def test_lean_epilogues(form, G, kw, precision, lean):
  """kEpiLrelu (NONE and LRELU, stride 1 / 2 / 2 narrow), kEpiMask (stride 2),
  kEpiMaskShift (stride 1 with out_shifts) and kEpiLreluSsq (stride 1 with the
  penalty norm, one sample per tile) on tiles 13 - 15."""
  f16 = precision
  epi = kw['epi']
  for recipe in ('real', 'exact'):
    c = case(G, f16, recipe)
    alpha = ALPHA if recipe == 'real' else EXACT_ALPHA
    exact = recipe == 'exact'
    if form == 'maskshift':
      check_out_shifts(G, c, f16, recipe, (2, -1, 0), 1, 2, alpha, epi, kw)
      continue
    L = Launch(G, c, f16, recipe, alpha=alpha, ssq='ordered' if form == 'lrelussq' else None,
               **kw)
    assert L.run() == 0
    y, own, err = statement(G, c, f16, epi, alpha)
    L.compare(L.y, y, own, exact, err, recipe)
    if form == 'lrelussq':
      want = S.rowsumsq(y, own)
      bar = S.rowsumsq_bound(y, 0.0 if exact else err, own)
      P.assert_f32(L.ssq[:G.nB], want, bar, 'rowsumsq')


# ---------------------------------------------------------------------------
# epilogues and features
# ---------------------------------------------------------------------------
FEATURE_TILES = [(1, dict()), (4, dict()), (13, dict(pmajor=1))]


@pytest.mark.parametrize('out_f32', [0, 1])
@pytest.mark.parametrize('epi', [S.EPI_NONE, S.EPI_LRELU, S.EPI_MASK, S.EPI_SIGMOID])
@pytest.mark.parametrize('tile,tkw', FEATURE_TILES, ids=['t1', 't4', 't13'])
def test_epilogues(tile, tkw, epi, out_f32, precision):
  """The four pointwise epilogues with and without bias, activation-typed and f32
  output (N = 102 in a pitch of 104: partial 16-byte column groups, and the f32
  second half past the pitch), on a 16-row MFMA tile, a 32-row one and a
  software-pipelined one; the sigmoid on pre-activations within dense_ref.T_MAX."""
  f16 = precision
  G = S.EPI_GEOM
  sig = epi == S.EPI_SIGMOID
  c = case(G, f16, 'real', sig)
  for bias in (True, False):
    L = Launch(G, c, f16, 'real', sig, bias=bias, tile=tile, epi=epi, out_f32=out_f32, **tkw)
    assert L.run() == 0
    y, own, err = statement(G, c, f16, epi, ALPHA, bias=bias)
    L.compare(L.y, y, own, False, err, 'bias {}'.format(bias))


@pytest.mark.parametrize('tile', [9, 12, 13])
def test_row_scale(tile, precision):
  """y = epi((acc + bias) * row_scale[b]): a negative, a zero and a 2^-20 scale."""
  f16 = precision
  G = S.SWP_DOWN
  c = case(G, f16, 'real')
  rs = np.array([-1.5, 0.0, 2.0**-20])
  for epi in (S.EPI_NONE, S.EPI_LRELU, S.EPI_MASK):
    L = Launch(G, c, f16, row_scale=rs, tile=tile, pmajor=1, epi=epi)
    assert L.run() == 0
    y, own, err = statement(G, c, f16, epi, ALPHA, row_scale=rs)
    L.compare(L.y, y, own, False, err, epi)
  d = Launch(G, c, f16, row_scale=rs, tile=13, pmajor=1).d
  d.tile = 0
  assert refused(d)


@pytest.mark.parametrize('G', S.SHIFT_GEOMS + S.SHIFT_GEOMS_K, ids=S.gid)
def test_shift_edges(G, precision):
  """+-(Lx - 1), mixed signs within a launch, a segment larger than the batch; the
  exact recipe, classic and software-pipelined staging.  Also at 6 and 12 taps
  (classic tiles only; split-parity staging where a parity fills whole stages: 12)."""
  f16 = precision
  c = case(G, f16, 'exact')
  for kw in (dict(tile=1), dict(tile=2, sp=1, pmajor=1), dict(tile=13, pmajor=1)):
    if not admits(desc_of(G, epi=S.EPI_LRELU, **kw)):
      assert (kw['tile'] == 13 and G.taps != 24) or (kw.get('sp') and G.taps % 4)
      continue
    L = Launch(G, c, f16, 'exact', alpha=EXACT_ALPHA, epi=S.EPI_LRELU, **kw)
    assert L.run() == 0
    y, own, err = statement(G, c, f16, S.EPI_LRELU, EXACT_ALPHA)
    L.compare(L.y, y, own, True, what=kw)


@pytest.mark.parametrize('tile', [2, 6, 12, 13])
def test_rowsumsq_forms(tile, precision):
  """The fused penalty norm of a two-phase launch with f32 output, one sample per
  tile (Lu = the tile's rows and twice that): atomics onto zero, the ordered form
  (slots compared with the statement's per-workgroup shares, the finishing sum
  within the derived bar, two runs bit-equal) and rowsumsq_defer (slots only).
  rowsumsq squares the f32 epilogue result BEFORE the store's rounding: the bar
  would not hold for the rounded values in the activation-typed launch below."""
  f16 = precision
  rows, cols = _lib.tile_shape(tile)
  for Lu, out_f32 in ((rows, 1), (2 * rows, 0)):
    G = S.SSQ_GEOMS[Lu]
    c = case(G, f16, 'real')
    y, own, err = statement(G, c, f16, S.EPI_NONE, ALPHA)
    want, bar = S.rowsumsq(y, own), S.rowsumsq_bound(y, err, own)
    runs = []
    for form in ('atomic', 'ordered', 'ordered', 'defer'):
      L = Launch(G, c, f16, tile=tile, out_f32=out_f32, ssq=form)
      assert L.run() == 0, form
      L.compare(L.y, y, own, False, err, form)
      assert P.is_sentinel(L.ssq[G.nB:])
      if form == 'defer':
        assert P.is_sentinel(L.ssq)
      else:
        P.assert_f32(L.ssq[:G.nB], want, bar, form)
      if form != 'atomic':
        assert bool(torch.isnan(L.ssq_ws[L.need:]).all())
        # slot (row tile, phase, column tile) of sample b: its share of the sum
        nt, gn = Lu // rows, -(-G.N // cols)
        slots = P.host(L.ssq_ws[:L.need]).reshape(G.nB, nt, 2, gn)
        for rt in range(nt):
          for z in range(2):
            t = S.rows_of(G, z)[rt * rows:(rt + 1) * rows]
            for bn in range(gn):
              sl = slice(bn * cols, (bn + 1) * cols)
              sub = np.zeros(G.Ly, bool)
              sub[t] = True
              P.assert_f32(slots[:, rt, z, bn], S.rowsumsq(y[:, :, sl], sub),
                           S.rowsumsq_bound(y[:, :, sl], err[:, :, sl], sub), (form, rt, z, bn))
        if form == 'ordered':
          runs.append(L.ssq[:G.nB].clone())
    assert torch.equal(P.bits(runs[0]), P.bits(runs[1]))


def check_out_shifts(G, c, f16, recipe, osh, oseg, side_rows, alpha, epi, kw):
  """cg_conv_desc.out_shifts, then cg_unshuffle_fixup on the result."""
  exact = recipe == 'exact'
  L = Launch(G, c, f16, recipe, alpha=alpha, out_shifts=(osh, oseg, side_rows), **kw)
  assert L.run() == 0
  a = R.f32(alpha)
  y, y_own, side, side_own = S.swconv_out_shifts(G, c['x'], c['Wl'], osh, oseg, side_rows, f16,
                                                 c['bias'], epi, a, c['mask'])
  err = S.acc_bound(G, c['x'], c['Wl'], c['bias'])
  # the bar of a direct row is that of the OUTPUT row t stored there.  MASK: the launch
  # rounds its f32 value to the activation type BEFORE the mask's product, so within
  # err of a rounding boundary it may hold the neighbour (swconv_ref.rounded_spread: one
  # ulp of the UNMASKED value, which the slope scales to more than one ulp of a masked
  # value in a lower binade); everywhere else the two roundings agree and only the f32
  # product with the slope rounds
  pre = S.place(G, S.linear(G, c['x'], c['Wl'], c['bias']))[0]
  pre_at, err_at = np.zeros_like(y), np.zeros_like(y)
  for b in range(G.nB):
    td, r, _, _ = S.out_shift_rows(int(osh[b // oseg]), G.Ly)
    pre_at[b, r], err_at[b, r] = pre[b, td], err[b, td]
  if exact:
    direct_err = 0.0  # (compared bit for bit)
  elif epi == S.EPI_MASK:
    direct_err = (S.rounded_spread(pre_at, err_at, f16) * S.mask_factor(c['mask'], a) +
                  S.U * np.abs(y))
  else:
    direct_err = err_at
  L.compare(L.y, y, y_own, exact, direct_err, 'direct rows')
  sv = L.side[:G.nB * side_rows * L.Cy].reshape(G.nB, side_rows, L.Cy)
  own_t = torch.tensor(side_own, device=sv.device)
  assert P.is_sentinel(sv[~own_t]) and P.is_sentinel(L.side[G.nB * side_rows * L.Cy:])
  got = sv[own_t][:, :G.N]
  if exact:
    P.assert_bits(got, side[side_own], f16)
  else:
    # side rows travel with the rows of y: their bar is that of their own output row
    side_err = np.zeros_like(side)
    for b in range(G.nB):
      _, _, ts, j = S.out_shift_rows(int(osh[b // oseg]), G.Ly)
      side_err[b, j] = err[b, ts]
    P.assert_act(got, side[side_own], f16, f32_err=side_err[side_own])
  assert int(P.bits(sv[own_t][:, G.N:]).numpy().astype(np.int64).__abs__().sum()) == 0
  # the second half: delta = what the launch stored (unowned rows: the sentinel),
  # h = the mask source; compared with the statement applied to the stored values
  delta = L.view(L.y).clone()
  h = L.mask if L.mask is not None else pad_dev(c['mask'], L.Cy, f16)
  sh = torch.tensor(osh, dtype=torch.int32, device=H.DEV)
  rc = _lib.load().cg_unshuffle_fixup(H.p(L.side), H.p(h), H.p(delta), H.p(sh), G.nB, G.Ly,
                                      L.Cy, oseg, side_rows, alpha, H.stream())
  H.sync()
  assert rc == 0
  stored = P.host(L.view(L.y))[:, :, :G.N]
  want = S.unshuffle_fixup(P.host(sv)[:, :, :G.N], c['mask'], stored, osh, oseg, a)
  # one product with the f32 slope and one sum, each rounded once in f32, then the
  # store: one activation ulp + 2 u |want|
  got = delta[:, :, :G.N]
  assert not bool((got == P.SENT).any())
  if exact:
    P.assert_bits(got.contiguous(), want, f16)
  else:
    P.assert_act(got.contiguous(), want, f16, f32_err=2 * S.U * np.abs(want))


@pytest.mark.parametrize('epi', [S.EPI_NONE, S.EPI_MASK])
@pytest.mark.parametrize('tile,side_rows', [(1, 2), (6, 3), (12, 2), (13, 5)])
def test_out_shifts_and_fixup(tile, side_rows, epi, precision):
  """Output-side PhaseShuffle adjoint: direct rows at their source rows (MASK: the
  value rounded to the activation type, then masked with the mask source's row r),
  reflected rows unmasked in `side`, side rows beyond |shift| untouched; then
  cg_unshuffle_fixup.  side_rows = max |shift| and larger."""
  f16 = precision
  G = S.SWP_UP
  for recipe in ('real', 'exact'):
    c = case(G, f16, recipe)
    check_out_shifts(G, c, f16, recipe, (2, -2, 0), 1, side_rows,
                     ALPHA if recipe == 'real' else EXACT_ALPHA, epi, dict(tile=tile, epi=epi))


@pytest.mark.parametrize('epi', [S.EPI_NONE, S.EPI_MASK])
@pytest.mark.parametrize('tile,ks', [(1, 2), (2, 4), (4, 2)])
@pytest.mark.parametrize('k', S.FIXUP_K)
def test_out_shifts_and_fixup_away_from_24_taps(k, tile, ks, epi, precision):
  """The same on the classic tiles at kernel sizes 6 (three taps per phase, both
  phases at one window offset) and 12: the side buffer + cg_unshuffle_fixup form is
  the one the critic's input gradient takes at every kernel size but 24."""
  f16 = precision
  G = S.K_UP[k]
  for recipe in ('real', 'exact'):
    c = case(G, f16, recipe)
    check_out_shifts(G, c, f16, recipe, (2, -2, 0), 1, 2,
                     ALPHA if recipe == 'real' else EXACT_ALPHA, epi,
                     dict(tile=tile, ks=ks, epi=epi))


@pytest.mark.parametrize('tile', [6, 8, 12, 15])
def test_layernorm_forward_only_and_cancellation(tile, precision):
  """ln_mean = ln_rstd = NULL: y, ln_mean and ln_rstd keep the sentinel, ln_h is the
  same.  Then rows with mean / std ~ 50 (50 added to the bias of unit
  pre-activations): the (1 + mean^2 / var) term of the bar -- ~ 2 % of rstd there,
  against ~ 0.1 % at mean 0."""
  f16 = precision
  G = S.LN_GEOMS[0]
  c = case(G, f16, 'real')
  kw = dict(tile=tile, epi=S.EPI_LN)
  La = Launch(G, c, f16, ln=ln_params(G) + (True,), **kw)
  Lb = Launch(G, c, f16, ln=ln_params(G) + (False,), **kw)
  assert La.run() == 0 and Lb.run() == 0
  check_ln(Lb, c, stats=False)
  assert torch.equal(P.bits(La.h), P.bits(Lb.h))
  c50 = dict(c, bias=c['bias'] + 50.0)
  L = Launch(G, c50, f16, ln=ln_params(G) + (True,), **kw)
  assert L.run() == 0
  check_ln(L, c50, what='mean 50')


# ---------------------------------------------------------------------------
# special values
# ---------------------------------------------------------------------------
def check_ieee(L, want, own, err, what):
  """The same NaN pattern and infinities; the finite rest within one ulp + err."""
  L.check_frame(L.y, own)
  got = P.host(L.view(L.y))[:, own][:, :, :L.G.N]
  want, err = want[:, own], err[:, own]
  assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(
      np.isnan(got) != np.isnan(want))[:5])
  r = R.round_act(want, L.f16)
  inf = np.isinf(r)
  assert np.array_equal(got[inf], r[inf]), what
  fin = np.isfinite(r)
  assert fin.any() and (np.abs(got[fin] - r[fin]) <= R.ulp_act(r[fin], L.f16) + err[fin]).all()
  return np.isfinite(got)


SPECIAL_KW = [dict(tile=0), dict(tile=4, ks=4), dict(tile=2, sp=1, pmajor=1),
              dict(tile=9, pmajor=1), dict(tile=13, pmajor=1), dict(tile=13, pmajor=1, lean=1),
              dict(tile=2, ksplit=2)]


@pytest.mark.parametrize('kw', SPECIAL_KW, ids=lambda k: '-'.join(
    '{}{}'.format(a, b) for a, b in sorted(k.items())))
@pytest.mark.parametrize('shifted', [0, 1])
def test_nonfinite_rows_stay_in_their_windows(kw, shifted, precision):
  """inf and NaN in x rows 0 and Lx - 1 and in the last row of sample 0 (sample 1
  shares the row tile: Lu = 64 in tiles of 128 rows and more).  Exactly the outputs
  whose window covers a planted row are non-finite -- with the sign and kind IEEE
  gives in float64 -- every other output matches the statement: rows outside [0, Lx)
  are zeros by selection, never a product with a neighbour's or a clamped row; the
  channel padding [N, Cy) of the poisoned rows (N = 38 of 40) stays +0.  shifted: sample 0 has shift
  1 (its row 0 is read by no shuffled row, its last row twice), sample 1 shift -2."""
  f16 = precision
  kw = dict(kw)
  use_lean = kw.pop('lean', 0)
  G = S.SPECIAL_GEOMS[shifted, 1 if kw.get('ksplit') else 0]  # (two chunks to split)
  c = case(G, f16, 'real')
  x = c['x'].copy()
  x[0, 0, 3], x[0, G.Lx - 1, 4], x[0, G.Lx - 1, 5] = np.inf, np.nan, -np.inf
  x[1, 0, 7], x[2, G.Lx - 1, 6] = np.nan, np.inf
  was = _lib.load().cg_debug_lean_epilogue(use_lean)
  try:
    L = Launch(G, c, f16, x=x, epi=S.EPI_LRELU, **kw)
    assert L.run() == 0
  finally:
    _lib.load().cg_debug_lean_epilogue(was)
  y, own, err = statement(G, c, f16, S.EPI_LRELU, ALPHA, ksplit=kw.get('ksplit') or 1, x=x)
  fin = check_ieee(L, y, own, err, kw)
  assert (~fin).any() and fin.any()
  # the statement agrees with the clean data wherever no window covers a plant
  clean = statement(G, c, f16, S.EPI_LRELU, ALPHA)[0]
  ok = np.isfinite(y)
  assert 0.3 < ok.mean() < 1 and np.allclose(y[ok], clean[ok], rtol=1e-12, atol=0)


@pytest.mark.parametrize('kw', [dict(tile=1), dict(tile=13, pmajor=1),
                                dict(tile=13, pmajor=1, lean=1), dict(tile=2, ksplit=2)],
                         ids=['classic', 'swp', 'lean', 'splitk'])
def test_mask_special_values(kw, precision):
  """mask_src holding -0, +0, NaN, +-subnormal and +-inf: > 0 alone selects 1 (the
  four implementations of the mask epilogue: classic, software-pipelined generic
  and lean, split-K finishing)."""
  f16 = precision
  kw = dict(kw)
  use_lean = kw.pop('lean', 0)
  G = S.SPLIT_CLASSIC if kw.get('ksplit') else S.SWP_DOWN
  c = case(G, f16, 'real')
  tiny = R.act_limits(f16)[0]
  m = c['mask'].copy()
  vals = [-0.0, 0.0, np.nan, tiny, -tiny, np.inf, -np.inf]
  m[:, :, 2:2 + len(vals)] = vals
  assert list(S.mask_factor(vals, 0.5)) == [0.5, 0.5, 0.5, 1.0, 0.5, 1.0, 0.5]
  c = dict(c, mask=m)
  was = _lib.load().cg_debug_lean_epilogue(use_lean)
  try:
    L = Launch(G, c, f16, epi=S.EPI_MASK, **kw)
    assert L.run() == 0
  finally:
    _lib.load().cg_debug_lean_epilogue(was)
  y, own, err = statement(G, c, f16, S.EPI_MASK, ALPHA, ksplit=kw.get('ksplit') or 1)
  L.compare(L.y, y, own, False, err)


@pytest.mark.parametrize('tile', [6, 12])
def test_nan_row_under_layernorm(tile, precision):
  """A row of pre-activations poisoned by one NaN source row: NaN in that row's
  statistics and activations, the padding of its ln_h still +0, every other row
  within the bars."""
  f16 = precision
  G = S.LN_GEOMS[0]
  c = case(G, f16, 'real')
  x = c['x'].copy()
  x[1, 5, 0] = np.nan
  L = Launch(G, c, f16, x=x, ln=ln_params(G) + (True,), tile=tile, epi=S.EPI_LN)
  assert L.run() == 0
  L.check_frame(L.h, True)
  L.check_frame(L.y, True)
  h = P.host(L.view(L.h))[:, :, :G.N]
  mean = P.host(L.mean[:G.nB * G.Ly]).reshape(G.nB, G.Ly)
  pre = S.swconv(G, x, c['Wl'], c['bias'])[0]
  bad = np.isnan(pre).any(axis=2)
  assert bad[1].any() and not bad[0].any() and not bad[2].any() and not bad[1].all()
  assert np.isnan(h[bad]).all() and np.isnan(mean[bad]).all()
  assert np.isfinite(h[~bad]).all() and np.isfinite(mean[~bad]).all()
  gamma, beta = ln_params(G)
  clean = S.swconv(G, c['x'], c['Wl'], c['bias'])[0]
  err = S.acc_bound(G, c['x'], c['Wl'], c['bias'])
  want = S.layernorm(clean, gamma, beta, R.f32(LN_EPS), A32, f16)[1]
  e_h = S.layernorm_bounds(clean, err, gamma, beta, R.f32(LN_EPS), A32, f16)[0]
  r = R.round_act(want, f16)
  assert (np.abs(h[~bad] - r[~bad]) <= R.ulp_act(r[~bad], f16) + e_h[~bad]).all()


SUBNORMAL_KW = [('16x16x32 classic s2', S.CLASSIC_DOWN[0], dict(tile=1)),
                ('16x16x32 classic s1', S.CLASSIC_UP[0], dict(tile=1)),
                ('32x32x16 classic s2', S.CLASSIC_DOWN[0], dict(tile=4)),
                ('32x32x16 classic s1', S.CLASSIC_UP[0], dict(tile=4)),
                ('16x16x32 split-parity', S.CLASSIC_DOWN[0], dict(tile=1, sp=1, pmajor=1)),
                ('16x16x32 swp s2', S.SWP_DOWN, dict(tile=13, pmajor=1)),
                ('16x16x32 swp s1', S.SWP_UP, dict(tile=13))]


def test_subnormal_operands(precision, capsys):
  """Subnormal x against weights of 2^10, one product per output, f32 output: the
  statement keeps them (swconv_ref.FLUSH_SUBNORMAL_OPERANDS = False); a matrix core
  or a staging path that flushed them would store zeros."""
  f16 = precision
  lines = []
  for name, G, kw in SUBNORMAL_KW:
    x, Wl = S.subnormal_recipe(G, f16)
    d = W.PackDesc(G.taps, G.Cr, G.N, G.Cx, 32, parity_major=kw.get('pmajor', 0))
    L = Launch(G, case(G, f16, 'real'), f16, bias=False, x=x, out_f32=1, **kw)
    L.wd = P.dev_act(np.concatenate([W.pack(Wl[z], d, f16) for z in range(G.nphase)]), f16)
    L.d.w = L.wd.data_ptr()
    assert L.run() == 0
    kept, own = S.swconv(G, x, Wl)
    flushed = np.zeros_like(kept)
    got = P.host(L.view(L.y))[:, :, :G.N]
    is_kept = np.array_equal(got[:, own], kept[:, own])
    is_flushed = np.array_equal(got[:, own], flushed[:, own])
    lines.append('{} {}: subnormal operands {}'.format(
        'fp16' if f16 else 'bf16', name,
        'kept' if is_kept else 'flushed' if is_flushed else 'NEITHER'))
    want = flushed if S.FLUSH_SUBNORMAL_OPERANDS else kept
    assert (kept[:, own] != 0).mean() > 0.5
    np.testing.assert_array_equal(got[:, own], want[:, own], err_msg=lines[-1])
  with capsys.disabled():
    print('\n' + '\n'.join(lines))


# ---------------------------------------------------------------------------
# refusals: CG_EINVAL from cg_swconv_check and cg_swconv, nothing written
# ---------------------------------------------------------------------------
def test_refusals(precision):
  """Every clause of swconv_run and swconv_swp_launch the header promises.  Each
  case starts from a descriptor cg_swconv_check admits and then breaks ONE clause
  (the fields named in the case), so the clause under test is the one that
  refuses.  Not reachable on its own, hence absent: nseg > 8 on a
  software-pipelined tile (tile rows = waves x mt x 16 and S >= 16 mt give nseg <=
  waves <= 8: the S clause always fires with it)."""
  f16 = precision
  dummy = P.sent32(64)
  ptr = dummy.data_ptr()
  cases = []

  def broken(what, G, fields, **kw):
    L = Launch(G, case(G, f16, 'real'), f16, **kw)
    assert admits(L.d), what + ': the starting point is not admitted'
    for k, v in fields.items():
      setattr(L.d, k, v)
    cases.append((what, L))

  D_, U_, N_ = S.SWP_DOWN, S.SWP_UP, S.SWP_DOWN_NARROW
  Gl = S.LN_GEOMS[0]
  ln = dict(epi=S.EPI_LN, ln=ln_params(Gl) + (True,))
  lnp = dict(epilogue=S.EPI_LN, ln_gamma=ptr, ln_beta=ptr, ln_h=ptr)
  split = dict(ksplit=2, split_ws=ptr, split_ws_elems=1 << 40)
  osh = dict(out_shifts=((1, -1, 0), 1, 2))
  U64 = S.up(3, 64, 24, 64, 40)
  # the descriptor's own fields
  broken('stride 3', D_, dict(stride=3), tile=1)
  broken('odd taps at stride 2', D_, dict(taps=23), tile=1)
  broken('CK 16', D_, dict(CK=16), tile=1)
  broken('Cx no multiple of CK', S.SPLIT_SWP2, dict(CK=40), tile=1)
  broken('Cy no multiple of 8', D_, dict(Cy=44), tile=1)
  broken('N beyond Cy', D_, dict(N=41), tile=1)
  broken('three phases', U_, dict(nphase=3), tile=1)
  broken('mask epilogue without a source', D_, dict(mask_src=None), tile=1, epi=S.EPI_MASK)
  broken('shifts with seg_size 0', D_, dict(seg_size=0), tile=1)
  broken('tile 16', D_, dict(tile=16), tile=1)
  # rows
  broken('Lu 48 on 64 rows', D_, dict(Lu=48), tile=1)
  broken('Lu 96 on 64 rows', D_, dict(Lu=96), tile=1)
  # MFMA 32x32x16 walks K uniformly: CK = 40 from a 64-row to a 128-row tile
  broken('MF 32 with CK 40', S.NON_UNI, dict(tile=4), tile=1, CK=40)
  # out_shifts
  broken('out_shifts f32', U_, dict(out_f32=1), tile=1, **osh)
  broken('out_shifts rowsumsq', S.FULL_TILE[64], dict(rowsumsq=ptr), tile=1,
         out_shifts=((1, -1), 1, 2))
  broken('out_shifts seg 0', U_, dict(out_seg_size=0), tile=1, **osh)
  broken('out_shifts without side', U_, dict(side=None), tile=1, **osh)
  broken('out_shifts side_rows 0', U_, dict(side_rows=0), tile=1, **osh)
  broken('out_shifts lrelu', U_, dict(epilogue=S.EPI_LRELU), tile=1, **osh)
  broken('out_shifts sigmoid', U_, dict(epilogue=S.EPI_SIGMOID), tile=1, **osh)
  # the fused LayerNorm
  broken('LN at stride 2', D_, lnp, tile=6, pmajor=1, sp=1)
  broken('LN on 64 columns', Gl, dict(tile=4), tile=6, **ln)
  broken('LN on 64 columns, software-pipelined', Gl, dict(tile=13), tile=12, **ln)
  broken('LN N 130', S.LN_GEOMS[1], dict(N=130, Cy=136), tile=6, epi=S.EPI_LN,
         ln=ln_params(S.LN_GEOMS[1]) + (True,))
  broken('LN f32', Gl, dict(out_f32=1), tile=6, **ln)
  broken('LN rowsumsq', S.SSQ_GEOMS[128], dict(rowsumsq=ptr), tile=6, epi=S.EPI_LN,
         ln=ln_params(S.SSQ_GEOMS[128]) + (True,))
  broken('LN without gamma', Gl, dict(ln_gamma=None), tile=6, **ln)
  broken('LN without h', Gl, dict(ln_h=None), tile=6, **ln)
  broken('LN with one statistic', Gl, dict(ln_rstd=None), tile=6, **ln)
  # the penalty norm
  broken('rowsumsq nseg 2', D_, dict(rowsumsq=ptr), tile=2)
  broken('defer without ws', S.FULL_TILE[128], dict(rowsumsq_defer=1), tile=2, ssq='atomic')
  L = Launch(S.FULL_TILE[128], case(S.FULL_TILE[128], f16, 'real'), f16, tile=2, ssq='ordered')
  assert admits(L.d)
  L.d.rowsumsq_ws_elems = L.need - 1
  cases.append(('rowsumsq ws too small', L))
  # stride-2 operand order, split-parity staging, the narrow last chunk
  broken('split-parity without parity-major', D_, dict(w_parity_major=0), tile=1, pmajor=1,
         sp=1)
  broken('split-parity, a parity is no whole stage', S.down(3, 64, 12, 32, 40),
         dict(stage_ksteps=4), tile=1, pmajor=1, sp=1, ks=2)
  broken('narrow one chunk', D_, dict(w_narrow_last=1), tile=1, pmajor=1)
  broken('narrow 4 taps', S.down(3, 64, 4, 38, 40), dict(w_narrow_last=1), tile=1, pmajor=1)
  broken('narrow without parity-major', N_, dict(w_parity_major=0), tile=1, pmajor=1, narrow=1)
  # split-K
  SC = S.SPLIT_CLASSIC
  # (the workspace holds three splits: the chunk count alone refuses)
  broken('split-K 3 of 4 chunks', SC, dict(ksplit=3, split_ws_elems=1 << 40), tile=2, ksplit=2)
  broken('split-K f32', SC, dict(out_f32=1), tile=2, ksplit=2)
  broken('split-K rowsumsq', S.up(2, 128, 24, 64, 40), dict(rowsumsq=ptr), tile=2, ksplit=2)
  broken('split-K out_shifts', U64, split, tile=2, **osh)
  broken('split-K sigmoid', SC, dict(epilogue=S.EPI_SIGMOID), tile=2, ksplit=2)
  broken('split-K without ws', SC, dict(split_ws=None), tile=2, ksplit=2)
  L = Launch(SC, case(SC, f16, 'real'), f16, tile=2, ksplit=2)
  assert admits(L.d)
  L.d.split_ws_elems -= 1
  cases.append(('split-K ws too small', L))
  # row_scale: software-pipelined tiles only, not with split-K or the LayerNorm
  broken('row_scale classic', D_, dict(tile=1), tile=13, pmajor=1, row_scale=np.ones(3))
  broken('row_scale split-K', S.SPLIT_SWP2, dict(row_scale=ptr), tile=13, pmajor=1, ksplit=2)
  broken('row_scale LN', Gl, dict(row_scale=ptr), tile=12, **ln)
  # software-pipelined tiles
  broken('swp CK 64', S.SPLIT_SWP2, dict(CK=64), tile=13, pmajor=1)
  broken('swp Lx 0x3fff', U_, dict(Lx=0x3fff), tile=13)
  broken('swp split-K narrow', N_, split, tile=13, pmajor=1, narrow=1)
  broken('swp tap order', D_, dict(w_parity_major=0), tile=13, pmajor=1)
  broken('swp 8 taps', S.down(3, 64, 8, 32, 40), dict(tile=13), tile=1, pmajor=1)
  broken('swp 4 taps stride 1', S.up(3, 64, 8, 32, 40), dict(tile=13), tile=1)
  # (tile 13: 4 waves x mt 2: S = 16 < 32 with nseg = 8)
  broken('swp S < 16 mt', S.down(3, 16, 24, 32, 40), dict(tile=13), tile=1, pmajor=1)
  for what, L in cases:
    assert refused(L.d), what
    H.sync()
    assert L.untouched(), what
  assert P.is_sentinel(dummy)
