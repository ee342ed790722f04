"""Float64 parity of the convolution weight gradient (cg_wgrad, cg_wgrad_batched:
calciumgan_amd/csrc/wgrad.hip) and of the operand packer (cg_pack_weights,
cg_pack_batched: swconv.hip) in both precision builds, at the smallest shapes
that reach each kernel instantiation and dispatch branch of plan_wgrad.

Every case compares ONE entry point with the float64 statement of
tests/wgrad_ref.py (tied to autograd / numpy_pack in tests/test_wgrad_ref.py,
which also shows that the bar is at most 1/20 of what a dropped K-step, a tap
off by one row or an unshuffled reflected row changes at every shape that runs
rounded reals).  Recipes: rounded reals (the bar), operands with every
significand bit in use whose sums are exact in f32 (bit equality), special
values, fp16 subnormals.  dw and dbias are over-allocated and hold a sentinel
where the call stores, 4.0 where it adds; the partial-sum workspace is NaN.
Bars: bit-equal, or wgrad_ref.acc_bound / dbias_bound -- never a measured number.
Packing is compared byte for byte."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from calciumgan_amd import _lib
from calciumgan_amd import nets

import hip_utils as H
import pointwise_ref as R
import test_hip_pointwise as P
import wgrad_ref as W

pytestmark = pytest.mark.gpu

EINVAL = _lib.CG_EINVAL
GUARD = 64     # floats allocated past the last one a launch may store
START = 4.0    # what dw / dbias hold when the call adds (a multiple of every unit)
# What gfx950 does with fp16 subnormal OPERANDS (profiles/wgrad_parity.txt): the
# MFMA (dw) and the column sums of g (dbias).  False: kept, as the statement says.
FLUSH_SUBNORMAL_OPERANDS = False


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
def to_dev(a, Cp, f16):
  """(nB, L, C) values of the activation type -> (nB, L, Cp), zero channel padding."""
  t = torch.zeros(a.shape[0], a.shape[1], Cp, dtype=R.act_dtype(f16), device=H.DEV)
  t[:, :, :a.shape[2]] = P.dev_act(a, f16)
  return t


@functools.lru_cache(maxsize=None)
def case(G, f16, recipe):
  """Operands and float64 results of a recipe at a geometry, computed once."""
  x, g = (W.real_recipe if recipe == 'real' else W.exact_recipe)(G, f16)
  return dict(x=x, g=g, dw=W.wgrad_of(G, x, g), mag=W.wgrad_of(G, np.abs(x), np.abs(g)))


class Launch(object):
  """One cg_wgrad descriptor over fresh output buffers.  join: 'atomic' (adds onto
  START), 'add' / 'store' (partials), 'direct' (store, one split, no workspace)."""

  def __init__(self, G, x, g, f16, join='atomic', nsplit=0, tile_rows=0, classic=0,
               no_xcd=0, bias_rows=None, Cxp=None, Cgp=None):
    stride, Lx, off = W.stride_of(G)
    self.G, self.join, self.bias_rows = G, join, bias_rows
    self.Cxp, self.Cgp = Cxp or W.pitch_of(G.Cx), Cgp or W.pitch_of(G.Cg)
    self.xd, self.gd = to_dev(x, self.Cxp, f16), to_dev(g, self.Cgp, f16)
    self.stores = join in ('store', 'direct')
    fill = P.SENT32 if self.stores else START
    self.n_dw = G.taps * G.Cx * G.Cg
    self.dw = torch.full((self.n_dw + GUARD,), fill, device=H.DEV)
    self.dw[self.n_dw:] = P.SENT32
    self.db = None
    if bias_rows is not None:
      self.db = torch.full((G.Cg + GUARD,), fill, device=H.DEV)
      self.db[G.Cg:] = P.SENT32
    self.sh = (torch.tensor(G.shifts, dtype=torch.int32, device=H.DEV)
               if G.shifts is not None else None)
    d = nets._wgrad_desc(self.xd, self.gd, self.dw, G.nB, Lx, self.Cxp, G.Lu, self.Cgp,
                         G.taps, stride, off, G.Cx, G.Cg, shifts=self.sh, seg_size=G.seg,
                         dbias=self.db, bias_rows=bias_rows or 0)
    d.nsplit, d.tile_rows, d.classic_staging, d.no_xcd_group = nsplit, tile_rows, classic, no_xcd
    d.store = int(self.stores)
    self.d, self.ws, self.need = d, None, 0
    if join in ('add', 'store'):
      self.need = _lib.load().cg_wgrad_partials_elems(ctypes.byref(d))
      assert self.need > 0, self.need
      self.ws = torch.full((self.need + GUARD,), float('nan'), device=H.DEV)
      d.partials, d.partials_elems = self.ws.data_ptr(), self.need

  def run(self):
    rc = _lib.load().cg_wgrad(ctypes.byref(self.d), H.stream())
    H.sync()
    return rc

  def start(self):
    return 0.0 if self.stores else START

  def out(self):
    """(dw, dbias) as float64; everything past the contract's extent untouched."""
    G = self.G
    assert P.is_sentinel(self.dw[self.n_dw:])
    if self.ws is not None:
      assert bool(torch.isnan(self.ws[self.need:]).all())
    db = None
    if self.db is not None:
      assert P.is_sentinel(self.db[G.Cg:])
      db = P.host(self.db[:G.Cg])
    return P.host(self.dw[:self.n_dw]).reshape(G.taps, G.Cx, G.Cg), db

  def untouched(self):
    fill = P.SENT32 if self.stores else START
    ok = bool((self.dw[:self.n_dw] == fill).all()) and P.is_sentinel(self.dw[self.n_dw:])
    if self.db is not None:
      ok = ok and bool((self.db[:self.G.Cg] == fill).all())
    return ok


def check(L, c, exact, what=''):
  """The launch's outputs against the statement of the case."""
  assert L.run() == 0, what
  dw, db = L.out()
  G, st = L.G, L.start()
  if exact:
    np.testing.assert_array_equal(dw, c['dw'] + st, err_msg=what)
  else:
    P.assert_f32(dw, c['dw'] + st, W._gamma(W.rows_of(G) + W.joins(G)) * (c['mag'] + st), what)
  if db is not None:
    want = W.dbias(c['g'], L.bias_rows) + st
    if exact:
      np.testing.assert_array_equal(db, want, err_msg=what)
    else:
      P.assert_f32(db, want, W.dbias_bound(G, c['g'], L.bias_rows, start=st), what)
  return dw, db


def both_recipes(G, f16, what='', recipes=('real', 'exact'), **kw):
  for recipe in recipes:
    c = case(G, f16, recipe)
    check(Launch(G, c['x'], c['g'], f16, **kw), c, recipe == 'exact',
          '{} {} {}'.format(what, recipe, kw))


# ---------------------------------------------------------------------------
# every kernel instantiation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('gi', [0, 1, 2], ids=['Lu8', 'Lu64', 'Lu128'])
@pytest.mark.parametrize('taps', W.TAPS)
def test_every_instantiation(taps, gi, precision):
  """wgrad_kernel<2, TPW, false, PIPE, TT, ALLT> at every even tap count from 2 to 24:

      taps   2  4  6  8 | 10 12 14 16 | 18 20 22 24
      TPW    1  1  1  1 |  2  2  2  2 |  3  3  3  3
      ALLT   0  0  0  1 |  0  0  0  1 |  0  0  0  2     (at Lu >= 64)

  ALLT = 1 needs taps == 8 TPW and one sample per tile (8, 16 at Lu >= 64), ALLT = 2
  is the ring (24); every other tap count (the last wave owns fewer than TPW live
  taps) and every Lu = 8 case (nseg = 8, no pipe; nB Lu = 72: the second tile holds
  one live sample of eight) take the per-tap guarded body.  Lu = 64: TT 64, pipe.  Lu = 128: TT 128, and TT 64 with
  tile_rows = 64.  The bias gradient rides along over half the rows (a multiple of
  32 at Lu >= 64: the ring keeps it; 36 at Lu = 8: inside a tile and a sample)."""
  f16 = precision
  G = W.instantiation_geoms(taps)[gi]
  half = W.rows_of(G) // 2
  both_recipes(G, f16, 'default', bias_rows=half)
  if gi == 2:
    both_recipes(G, f16, 'tile 64', bias_rows=half, tile_rows=64)
  if taps == 24 and gi > 0:
    # register-staged tiles instead of the ring; the ring refused by bias_rows % 32
    both_recipes(G, f16, 'classic', bias_rows=half, classic=1)
    both_recipes(G, f16, 'bias rows 100', bias_rows=100)
    both_recipes(G, f16, 'ring store', bias_rows=half, join='store', nsplit=2)


def test_more_than_64_shift_segments(precision):
  """65 segments: the ring (whose shifts ride in one 64-lane register) is refused
  and the register-staged body runs; the statement is the same.  Exact recipe only
  (4160 rows: wgrad_ref.SEGS65)."""
  both_recipes(W.SEGS65, precision, recipes=('exact',), bias_rows=2080)
  both_recipes(W.SEGS65, precision, recipes=('exact',), bias_rows=2080, join='store',
               nsplit=9)


@pytest.mark.parametrize('G', W.SHIFT_EDGES, ids=str)
def test_largest_shifts(G, precision):
  """+-(Lx - 1) at Lx = 16 and Lx = 4, a segment larger than the batch, mixed signs in
  one launch, and +-(Lx - 1) on the ring's edge tiles.  Exact recipe only: these
  shapes are not among wgrad_ref.real_geoms()."""
  both_recipes(G, precision, recipes=('exact',), bias_rows=W.rows_of(G))


# ---------------------------------------------------------------------------
# channel edges, the 1-tap form, grouping
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('Cx,Cxp,Cg,Cgp', W.CHANNELS)
def test_channel_edges(Cx, Cxp, Cg, Cgp, precision):
  """Pitch above the real count on both sides; up to gx = 4 cx blocks and gy = 3 cg
  blocks with ragged last blocks (102 = 3 x 32 + 6, 130 = 2 x 64 + 2)."""
  G = W.channel_geom(Cx, Cg)
  both_recipes(G, precision, bias_rows=W.rows_of(G), Cxp=Cxp, Cgp=Cgp)
  both_recipes(G, precision, bias_rows=128, Cxp=Cxp, Cgp=Cgp, join='store', nsplit=3)


@pytest.mark.parametrize('G', W.DENSE, ids=str)
def test_one_tap_form(G, precision):
  """wgrad_kernel<1, 1, true, PIPE, 256, 0>: Lu = 1 and 32 (256 / Lu samples per
  tile, ragged last tile: 300 and 288 rows), Lu = 256 and 512 (pipe).  Atomics over
  the K' splits, and one split stored directly."""
  both_recipes(G, precision)
  both_recipes(G, precision, join='direct', nsplit=1)


@pytest.mark.parametrize('Cx,Cg,mode', W.GROUPING)
def test_xcd_grouping(Cx, Cg, mode, precision):
  """(102, 130): gx 4, gy 3 -> gmode 0; (70, 65): 3 x 2 -> 1; (33, 65): 2 x 2 -> 2; (70,
  130): 3 x 3 -> 3 (wgrad_ref.gmode_of restates plan_wgrad's choice).  Each also
  with no_xcd_group = 1 (plain order)."""
  G = W.geom(4, 64, 8, Cx, Cg, (2, -1), 2)
  stride, Lx, _ = W.stride_of(G)
  assert W.gmode_of(Cx, Cg, G.nB, Lx, W.pitch_of(Cx), W.rows_of(G), W.pitch_of(Cg)) == mode
  both_recipes(G, precision, 'grouped', nsplit=3)
  both_recipes(G, precision, 'plain', nsplit=3, no_xcd=1)


# ---------------------------------------------------------------------------
# joining forms
# ---------------------------------------------------------------------------
def test_joining_forms(precision):
  """18 tiles of 64 rows.  Atomics (twice, each within the bar); partials added /
  stored with 2, 3, 9 and 17 splits (the reduce kernel's zc = 1, 1, 2, 4 threads per
  element), twice and bit-equal; one split stored directly; `store` without a
  workspace at two splits is refused and writes nothing."""
  f16, G = precision, W.JOIN
  for recipe in ('real', 'exact'):
    c = case(G, f16, recipe)
    for _ in range(2):
      check(Launch(G, c['x'], c['g'], f16, bias_rows=576), c, recipe == 'exact', 'atomic')
    for nsplit in (2, 3, 9, 17):
      for join in ('add', 'store'):
        runs = [check(Launch(G, c['x'], c['g'], f16, join=join, nsplit=nsplit,
                             bias_rows=576), c, recipe == 'exact', (join, nsplit))
                for _ in range(2)]
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1],
                                                                         runs[1][1])
    check(Launch(G, c['x'], c['g'], f16, join='direct', nsplit=1, bias_rows=576), c,
          recipe == 'exact', 'direct')
  L = Launch(G, c['x'], c['g'], f16, join='direct', nsplit=2, bias_rows=576)
  assert L.run() == EINVAL and L.untouched()


# ---------------------------------------------------------------------------
# dbias
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('bias_rows', [32, 128, 256, 100])
def test_dbias_rows_ring_and_classic(bias_rows, precision):
  """M = 256 rows, 24 taps: 32, M / 2 and M keep the ring (column sums from the g
  fragments, per 32-row K-step); 100 is refused by the ring and inside a tile.
  Atomics, and the splits' bias partials (bias_part) stored."""
  for kw in (dict(), dict(classic=1), dict(join='store', nsplit=2),
             dict(join='add', nsplit=4, classic=1)):
    both_recipes(W.BIAS_RING, precision, bias_rows=bias_rows, **kw)


@pytest.mark.parametrize('bias_rows', [20, 36, 72])
def test_dbias_rows_inside_a_tile_of_several_samples(bias_rows, precision):
  """Lu = 8, nseg = 8: 20 ends inside a sample, 36 inside the first tile."""
  both_recipes(W.BIAS_NSEG, precision, bias_rows=bias_rows)
  both_recipes(W.BIAS_NSEG, precision, bias_rows=bias_rows, join='store', nsplit=2)


# ---------------------------------------------------------------------------
# special values
# ---------------------------------------------------------------------------
def check_ieee(got, want, bar, what):
  """The same NaN pattern, the same infinities, the finite rest within the bar."""
  assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(
      np.isnan(got) != np.isnan(want))[:5])
  inf = np.isinf(want)
  assert np.array_equal(got[inf], want[inf]), what
  fin = np.isfinite(want)
  assert fin.any() and (np.abs(got[fin] - want[fin]) <= bar[fin]).all(), what


@pytest.mark.parametrize('kw', [dict(), dict(classic=1), dict(join='store', nsplit=3)],
                         ids=['default', 'classic', 'partials'])
@pytest.mark.parametrize('taps', [8, 24])
def test_special_values(taps, kw, precision):
  """Lu = 64, shifts (1, -2, 0); taps 24 takes the ring unless classic.
  (1) NaN / inf in the rows of x no shuffled row reads appear nowhere.
  (2) NaN / inf in g at interior rows >= bias_rows reach dw (exactly the columns
      the statement says) and not dbias.
  (3) NaN in one channel of one sample of x poisons exactly that cx row of every
      tap; +inf in one element of x gives +-inf by the sign of g, in the taps that
      read its row."""
  f16 = precision
  G = W.instantiation_geoms(taps)[1]
  c = case(G, f16, 'real')
  bar = W._gamma(W.rows_of(G) + W.joins(G)) * (c['mag'] + START)
  _, Lx, _ = W.stride_of(G)
  # (1)
  x = c['x'].copy()
  for b in range(G.nB):
    for r in W.unread_rows(G.shifts[b // G.seg], Lx):
      x[b, r, :] = np.nan
      x[b, r, ::3] = np.inf
  assert np.isnan(x).sum() > 0
  L = Launch(G, x, c['g'], f16, bias_rows=96, **kw)
  assert L.run() == 0
  dw, db = L.out()
  P.assert_f32(dw, c['dw'] + L.start(), bar, 'unread rows')
  # (2)
  g = c['g'].copy()
  g[2, 30, 5], g[1, 40, 7], g[1, 41, 8] = np.nan, np.inf, -np.inf
  L = Launch(G, c['x'], g, f16, bias_rows=96, **kw)
  assert L.run() == 0
  dw, db = L.out()
  want = W.wgrad_of(G, c['x'], g)
  assert np.isnan(want[:, :, 5]).all() and np.isinf(want[:, :, 7]).any()
  check_ieee(dw, want + L.start(), bar, 'g specials')
  P.assert_f32(db, W.dbias(g, 96) + L.start(), W.dbias_bound(G, c['g'], 96, start=START))
  # (3)
  x = c['x'].copy()
  x[1, :, 4] = np.nan
  x[2, 50, 9] = np.inf
  L = Launch(G, x, c['g'], f16, bias_rows=96, **kw)
  assert L.run() == 0
  dw, db = L.out()
  want = W.wgrad_of(G, x, c['g'])
  assert np.isnan(want[:, 4, :]).all() and np.isnan(want).sum() == want[:, 4, :].size
  assert np.isinf(want[:, 9, :]).sum() >= (taps // 2) * (G.Cg - 2)
  check_ieee(dw, want + L.start(), bar, 'x specials')


@pytest.mark.parametrize('kw', [dict(), dict(classic=1), dict(join='store', nsplit=2)],
                         ids=['ring', 'classic', 'ring_partials'])
@pytest.mark.parametrize('which', ['x', 'g'])
def test_fp16_subnormal_operands(which, kw):
  """fp16 subnormals in x (times +-2^8 .. 2^12 in g) or in g: every sum is exact in
  f32 and the statement keeps the subnormals, in dw (the MFMA's operands) and in
  dbias = sum of g (the ring sums it with v_dot2 from the g fragments, the
  register-staged body converts and adds) of the same launch.  A unit that
  flushed them would return exact zeros, thousands of bars away
  (test_wgrad_ref.test_subnormal_recipe)."""
  _lib.use('f16')
  G = W.BIAS_RING
  x, g = W.subnormal_recipe(G, which)
  L = Launch(G, x, g, True, bias_rows=128, **kw)
  assert L.run() == 0
  dw, db = L.out()
  fl = W.flush if FLUSH_SUBNORMAL_OPERANDS else (lambda v: v)
  want, wdb = W.wgrad_of(G, fl(x), fl(g)), W.dbias(fl(g), 128)
  st = L.start()
  print('\nfp16 subnormals in {} ({}): dw {} of {} nonzero (statement {}), dbias {} of {} '
        'nonzero (statement {})'.format(
            which, kw, np.count_nonzero(dw - st), dw.size, np.count_nonzero(want),
            np.count_nonzero(db - st), db.size, np.count_nonzero(wdb)))
  P.assert_f32(dw, want + st, W.acc_bound(G, x, g, start=st), 'dw')
  P.assert_f32(db, wdb + st, W.dbias_bound(G, g, 128, start=st), 'dbias')


# ---------------------------------------------------------------------------
# cg_wgrad_batched
# ---------------------------------------------------------------------------
@pytest.fixture(params=[0, 2], ids=['split_forms', 'flex'])
def wgrad_form(request):
  was = _lib.load().cg_debug_wgrad_flex(request.param)
  yield request.param
  _lib.load().cg_debug_wgrad_flex(was)


def run_batched(launches):
  arr = (_lib.WgradDesc * len(launches))(*[L.d for L in launches])
  rc = _lib.load().cg_wgrad_batched(arr, len(launches), H.stream())
  H.sync()
  return rc


def check_batched(launches, cases, exact, what):
  assert run_batched(launches) == 0, what
  for L, c in zip(launches, cases):
    L.run = lambda: 0  # (already run: check() only compares)
    check(L, c, exact, what)


@pytest.mark.parametrize('recipe', ['real', 'exact'])
def test_wgrad_batched(recipe, wgrad_form, precision):
  """Three 24-tap ring layers (64- and 128-row tiles) with partials and dbias: the
  K'-split forms (mode 0) and the flex form (mode 2), each layer against the
  float64 statement; the same batch with atomics; a mixed batch with a 1-tap
  layer (launched one by one); n = 1."""
  f16, exact = precision, recipe == 'exact'
  cases = [case(G, f16, recipe) for G in W.BATCH]
  mk = lambda join, **kw: [Launch(G, c['x'], c['g'], f16, join=join, bias_rows=128, **kw)
                           for G, c in zip(W.BATCH, cases)]
  for join in ('store', 'add'):
    Ls = mk(join)
    if wgrad_form == 2:
      arr = (_lib.WgradDesc * 3)(*[L.d for L in Ls])
      assert _lib.load().cg_wgrad_flex_plan(arr, 3, 2, None, 0, None) > 0
    check_batched(Ls, cases, exact, join)
  check_batched(mk('atomic'), cases, exact, 'atomic')
  check_batched(mk('atomic', classic=1), cases, exact, 'atomic classic')
  Gd = W.DENSE[1]
  cd = case(Gd, f16, recipe)
  Ls = mk('store')
  mixed = [Ls[0], Launch(Gd, cd['x'], cd['g'], f16), Ls[1]]
  check_batched(mixed, [cases[0], cd, cases[1]], exact, 'mixed')
  check_batched(mk('store')[2:], cases[2:], exact, 'n = 1')


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_refusals(precision):
  """CG_EINVAL, outputs untouched."""
  f16 = precision
  G = W.geom(2, 64, 8, 8, 40)
  c = case(G, f16, 'exact')

  def refused(edit, G=G, c=c, **kw):
    L = Launch(G, c['x'], c['g'], f16, bias_rows=64, **kw)
    edit(L.d)
    return L.run() == EINVAL and L.untouched()

  assert refused(lambda d: setattr(d, 'taps', 7))
  assert refused(lambda d: setattr(d, 'taps', 26))
  def stride1(d):
    d.stride, d.taps = 1, 2
  assert refused(stride1)
  assert refused(lambda d: setattr(d, 'Cx', 12))
  assert refused(lambda d: setattr(d, 'Cg', 44))
  assert refused(lambda d: setattr(d, 'Cx_real', 17))  # > Cx = 16
  assert refused(lambda d: setattr(d, 'tile_rows', 128))  # Lu = 64
  def lu96(d):
    d.Lu, d.Lx, d.nB = 96, 192, 1   # (inside the buffers: 96 <= 2 x 64 rows)
  assert refused(lu96)
  assert refused(lambda d: setattr(d, 'partials_elems', d.partials_elems - 1),
                 join='store', nsplit=2)
  # taps 1 needs stride 1
  Gd = W.geom(2, 256, 1, 8, 40)
  cd = case(Gd, f16, 'exact')
  assert refused(lambda d: setattr(d, 'stride', 2), G=Gd, c=cd)


# ---------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------
def pack_source(rng, n, f16):
  """f32 values whose rounding to the activation type is the point: random
  reals, exact ties (both neighbours even / odd), the largest finite value, the
  first f32 that rounds to inf (fp16) and the last that does not, subnormals of
  the type and values below half the smallest one, NaN, +-0, +-inf."""
  s = 11 if f16 else 8
  ulp1 = 2.0**(1 - s)  # ulp at 1
  tiny, big = R.act_limits(f16)
  plant = [1 + ulp1 / 2, 1 + 3 * ulp1 / 2, -(1 + ulp1 / 2), 1 + ulp1 / 2 + 2.0**-23,
           1 + ulp1 / 2 - 2.0**-24, big, -big, tiny, -tiny, 3 * tiny, tiny / 2, -tiny / 2,
           tiny / 2 * (1 + 2.0**-20), 1.5 * tiny, 2.5 * tiny, 0.0, -0.0, np.nan, np.inf,
           -np.inf]
  if f16:
    plant += [65519.996, 65520.0, -65520.0, 65536.0, 1e10, 2.0**-14 - 2.0**-25,
              2.0**-14 - 2.0**-26, 1023 * 2.0**-24]
  plant.append(float(np.finfo(np.float32).max))
  v = rng.randn(n).astype(np.float32)
  with np.errstate(over='ignore'):
    pv = np.array(plant, np.float64).astype(np.float32)
  if n < len(pv):
    v[:] = pv[:n]
    return v
  for row in rng.choice(n, size=(min(4, n // len(pv)), len(pv)), replace=False):
    v[row] = pv
  return v


def pack_descs():
  """(name, wgrad_ref.PackDesc, source elements)."""
  out = []
  for taps in (1, 2, 8, 24):
    for N in (1, 64, 65, 130):
      pm = 1 if taps > 1 and N in (64, 130) else 0
      out.append(('taps{}_N{}_pm{}'.format(taps, N, pm),
                  W.PackDesc(taps, 40, N, 64, parity_major=pm), taps * 40 * N))
  # narrow_last at the edges of its window (CK 32): C_real = Cx - 24 and Cx - 31
  for C in (104, 97):
    out.append(('narrow_C{}'.format(C),
                W.PackDesc(8, C, 65, 128, parity_major=1, narrow_last=1), 8 * C * 65))
  out.append(('narrow_taps24', W.PackDesc(24, 102, 130, 128, parity_major=1, narrow_last=1),
              24 * 102 * 130))
  out.append(('narrow_taps6', W.PackDesc(6, 40, 3, 64, parity_major=1, narrow_last=1),
              6 * 40 * 3))
  # parity-major at every even tap count, narrow_last wherever it has room (6 .. 22;
  # C = 40 of Cx = 64: the last chunk's 8 real channels next to a full chunk)
  for taps in range(2, 25, 2):
    if taps not in (2, 8, 24):
      out.append(('taps{}_pm'.format(taps), W.PackDesc(taps, 40, 65, 64, parity_major=1),
                  taps * 40 * 65))
    if 6 < taps < 24:
      out.append(('narrow_taps{}'.format(taps),
                  W.PackDesc(taps, 40, 3, 64, parity_major=1, narrow_last=1), taps * 40 * 3))
  # two phases out of one 24-tap source: taps 22, 20, .. and 23, 21, ..
  for t0 in (22, 23):
    out.append(('phase_tap0_{}'.format(t0),
                W.PackDesc(12, 33, 70, 64, tap0=t0, tap_step=-2, s_tap=33 * 70),
                24 * 33 * 70))
  # ... and out of a 10-tap one (k = 2 mod 4: phase 0 starts on the EVEN tap 8, phase 1 on
  # 9), 5 taps per phase: ceil16(5 x 4) = 32 groups, 12 of them padding
  for t0 in (8, 9):
    out.append(('phase_k10_tap0_{}'.format(t0),
                W.PackDesc(5, 33, 70, 64, tap0=t0, tap_step=-2, s_tap=33 * 70),
                10 * 33 * 70))
  # a transposed source (s_c and s_n swapped: the LDS-turned form), CK 64
  out.append(('transposed', W.PackDesc(8, 70, 33, 128, CK=64, s_tap=70 * 33, s_c=1, s_n=70),
              8 * 70 * 33))
  out.append(('transposed_pm', W.PackDesc(8, 33, 130, 64, s_tap=33 * 130, s_c=1, s_n=33,
                                          parity_major=1), 8 * 33 * 130))
  return out


PACK = pack_descs()


def c_pack_desc(d, src, dst):
  cd = _lib.PackDesc()
  cd.src, cd.dst = src.data_ptr(), dst.data_ptr()
  for k in ('taps', 'tap0', 'tap_step', 's_tap', 's_c', 's_n', 'C_real', 'N_real', 'Cx', 'CK',
            'parity_major', 'narrow_last'):
    setattr(cd, k, getattr(d, k))
  return cd


def want_bits(src, d, f16):
  """The bytes of wgrad_ref.pack; a NaN (the source holds the default quiet NaN of
  f32, 0x7fc00000) is the default quiet NaN of the type -- the bits a host
  conversion gives a NaN are its own business."""
  v = W.pack(src, d, f16)
  want = torch.tensor(np.where(np.isnan(v), 0.0, v), dtype=torch.float32).to(
      R.act_dtype(f16)).view(torch.int16)
  want[torch.tensor(np.isnan(v))] = 0x7e00 if f16 else 0x7fc0
  return want


def pack_buffers(d, n_src, f16, seed):
  src = pack_source(np.random.RandomState(seed), n_src, f16)
  elems = _lib.load().cg_packed_elems(d.N_real, d.taps, d.Cx, d.CK)
  assert elems == W.packed_elems(d.N_real, d.taps, d.Cx, d.CK)
  return src, torch.tensor(src, device=H.DEV), P.sent_act((elems + GUARD,), f16), elems


def assert_packed(dst, elems, src, d, f16):
  got = P.bits(dst[:elems])
  want = want_bits(src, d, f16)
  bad = torch.nonzero(got != want)
  assert bad.numel() == 0, (bad[:5], got[bad[0]], want[bad[0]])
  assert P.is_sentinel(dst[elems:])


@pytest.mark.parametrize('name,d,n_src', PACK, ids=[p[0] for p in PACK])
def test_pack_weights_bytes(name, d, n_src, precision):
  """cg_pack_weights against wgrad_ref.pack, byte for byte: rounding to nearest
  even (ties), fp16 overflow to inf, subnormals kept, NaN, -0; padding slots are +0
  bits (they are part of the comparison); nothing past cg_packed_elems."""
  f16 = precision
  src, sd, dst, elems = pack_buffers(d, n_src, f16, 11)
  _lib.call('cg_pack_weights', ctypes.byref(c_pack_desc(d, sd, dst)), H.stream())
  H.sync()
  assert_packed(dst, elems, src, d, f16)


def test_pack_refusals(precision):
  """narrow_last just outside its window, without parity_major, with CK 64, without
  room for its 32 groups (taps < 6); C_real > Cx: CG_EINVAL, nothing written."""
  f16 = precision
  base = dict(taps=8, C_real=104, N_real=4, Cx=128, parity_major=1, narrow_last=1)
  for kw in (dict(C_real=96), dict(C_real=105), dict(parity_major=0), dict(CK=64),
             dict(taps=2), dict(taps=4), dict(taps=34), dict(Cx=32, C_real=8),
             dict(narrow_last=0, C_real=129), dict(narrow_last=0, CK=24)):
    d = W.PackDesc(**dict(base, **kw))
    assert not W.pack_admissible(d)
    sd = torch.zeros(40 * 136 * 8, device=H.DEV)
    dst = P.sent_act((128 * 4 * 144 * 8,), f16)
    rc = _lib.load().cg_pack_weights(ctypes.byref(c_pack_desc(d, sd, dst)), H.stream())
    H.sync()
    assert rc == EINVAL and P.is_sentinel(dst), kw


def test_pack_batched_bytes(precision):
  """One launch over all descriptors of test_pack_weights_bytes: the same bytes;
  the sizing pass and cg_pack_plan_bytes agree with the filled plan."""
  f16 = precision
  lib = _lib.load()
  bufs = [pack_buffers(d, n, f16, 20 + i) for i, (_, d, n) in enumerate(PACK)]
  descs = [c_pack_desc(d, b[1], b[2]) for (_, d, _), b in zip(PACK, bufs)]
  n = len(descs)
  arr = (_lib.PackDesc * n)(*descs)
  blocks = lib.cg_pack_plan_build(arr, n, None, 0)
  assert blocks == sum(-(-b[3] // 2048) for b in bufs)
  nbytes = lib.cg_pack_plan_bytes(n, blocks)
  host = torch.zeros(nbytes + 16, dtype=torch.uint8)
  host[nbytes:] = 0xAB
  assert lib.cg_pack_plan_build(arr, n, host.data_ptr(), nbytes - 1) == -1
  assert lib.cg_pack_plan_build(arr, n, host.data_ptr(), nbytes) == blocks
  assert bool((host[nbytes:] == 0xAB).all())
  dev = host[:nbytes].to(H.DEV)
  _lib.call('cg_pack_batched', H.p(dev), n, blocks, H.stream())
  H.sync()
  for (_, d, _), (src, _, dst, elems) in zip(PACK, bufs):
    assert_packed(dst, elems, src, d, f16)
