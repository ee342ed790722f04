"""The folded PhaseShuffle fix-up of cg_swconv (cg_conv_desc.out_shifts with side ==
NULL: calciumgan_amd/csrc/swconv_swp.hip, kEpiMaskShift) in both precision builds.

One launch must leave in y what the launch with a side buffer followed by
cg_unshuffle_fixup leaves: compared (1) with the float64 statement of
tests/swconv_ref.py -- swconv_out_shifts, then unshuffle_fixup on the stored values
-- within derived bars (rounded reals) or bit for bit (the exact recipe), (2) bit for
bit with the two-launch form on the same operands, and (3) frame: every row of y
written, channel padding +0, the guard behind y intact, no side buffer touched.

Geometries (24 taps, two phases of 12): Lu = 32 (a wave holds head AND tail of a
sample, eight samples per 256-row tile, every shift in [-10, 10]); Lu = 64 with
shift segments of two samples over five (a short last segment, the last tile partly
past the batch); Lu = 256 and 512 (one sample per tile; a sample across two
workgroups); side_rows = 15 with shifts of +-15 (a wave's last admissible mirror);
all shifts 0; |shift| <= 3 (|s| = 1: an edge wave in one phase only); N = 102 in a
pitch of 128 (zero tail in the second column tile).  N = 40 in a pitch of 40
everywhere else: narrower than the 64-column tile (open columns).  The
parametrisation is built at collection from cg_swconv_check."""
import ctypes

import numpy as np
import pytest
import torch

from calciumgan_amd import _lib

import hip_utils as H
import pointwise_ref as R
import swconv_ref as S
import test_hip_pointwise as P
import test_hip_swconv as T
from test_hip_pointwise import precision, _back_to_bf16  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GUARD = 64
TILES = (13, 14, 15)
ALL21 = tuple(range(-10, 11)) + (10, -10, 4)

# (name, geometry, out_shifts, out_seg_size, side_rows, pitch of y)
CASES = [
    ('lu32', S.up(24, 32, 24, 32, 40), ALL21, 1, 10, 40),
    ('lu64', S.up(5, 64, 24, 32, 40), (10, -10, 3), 2, 10, 40),
    ('lu256', S.up(3, 256, 24, 32, 40), (10, -10, 1), 1, 10, 40),
    ('lu512', S.up(3, 512, 24, 32, 40), (10, -10, 1), 1, 10, 40),
    ('m15', S.up(4, 32, 24, 32, 40), (15, -15, 1, -14), 1, 15, 40),
    ('zero', S.up(3, 64, 24, 32, 40), (0, 0, 0), 1, 10, 40),
    ('small', S.up(6, 64, 24, 32, 40), (1, -1, 2, -2, 3, -3), 1, 10, 40),
    ('n102', S.up(3, 64, 24, 32, 102), (10, -10, 1), 1, 10, 128),
]


def folded_desc(G, tile, oseg, side_rows, Cy, alpha=T.ALPHA):
  """The folded descriptor with placeholder pointers (cg_swconv_check only)."""
  d = T.desc_of(G, tile=tile, epi=S.EPI_MASK, alpha=alpha)
  d.Cy = Cy
  d.out_shifts, d.out_seg_size, d.side, d.side_rows = 64, oseg, None, side_rows
  return d


def cases():
  out = []
  for name, G, osh, oseg, m, Cy in CASES:
    for tile in TILES:
      if T.admits(folded_desc(G, tile, oseg, m, Cy)):
        out.append(pytest.param(G, osh, oseg, m, Cy, tile, id='{}-t{}'.format(name, tile)))
  return out


PARAMS = cases()


def test_the_tile_14_cases_are_all_collected():
  ids = {p.id for p in PARAMS}
  for name in ('lu32', 'lu64', 'lu256', 'lu512'):
    assert name + '-t14' in ids, sorted(ids)


class Pair(object):
  """Operands of one geometry on the device and the two forms over them."""

  def __init__(self, G, c, f16, recipe, osh, oseg, side_rows, Cy, tile, alpha):
    self.G, self.f16, self.Cy, self.alpha = G, f16, Cy, alpha
    self.oseg, self.side_rows, self.tile = oseg, side_rows, tile
    self.x = T.pad_dev(c['x'], G.Cx, f16)
    self.w = P.dev_act(T.packed(G, f16, recipe, False, 32, 0, 0), f16)
    self.bias = P.dev32(np.r_[c['bias'], [np.nan] * 8])
    self.mask = T.pad_dev(c['mask'], Cy, f16)
    self.osh = torch.tensor(osh, dtype=torch.int32, device=H.DEV)
    self.n = G.nB * G.Ly * Cy

  def launch(self, folded):
    G = self.G
    d = folded_desc(G, self.tile, self.oseg, self.side_rows, self.Cy, self.alpha)
    y = P.sent_act((self.n + GUARD,), self.f16)
    side = P.sent_act((G.nB * self.side_rows * self.Cy + GUARD,), self.f16)
    d.x, d.w, d.y = self.x.data_ptr(), self.w.data_ptr(), y.data_ptr()
    d.bias, d.mask_src = self.bias.data_ptr(), self.mask.data_ptr()
    d.out_shifts = self.osh.data_ptr()
    d.side = None if folded else side.data_ptr()
    lib = _lib.load()
    assert lib.cg_swconv_check(ctypes.byref(d)) == 0
    assert lib.cg_swconv(ctypes.byref(d), H.stream()) == 0
    H.sync()
    if folded:
      assert P.is_sentinel(side)
    else:
      rc = lib.cg_unshuffle_fixup(H.p(side), H.p(self.mask), H.p(y), H.p(self.osh), G.nB,
                                  G.Ly, self.Cy, self.oseg, self.side_rows, self.alpha,
                                  H.stream())
      H.sync()
      assert rc == 0
    return y

  def view(self, y):
    return y[:self.n].reshape(self.G.nB, self.G.Ly, self.Cy)


def statement(G, c, f16, osh, oseg, side_rows, alpha, exact):
  """(want, bar) of y after the fix-up, float64.  Rows no reflected row lands on: the
  masked direct value with the bar of its own output row (acc_bound + one product
  with the slope).  Folded rows: S.unshuffle_fixup on the STORED direct and side
  values; the kernel's stored values may differ from the statement's roundings by
  rounded_spread of their bars, the sum and the product round once each in f32 (a
  fused multiply-add: fewer): spread(direct) + spread(side) mf + 2 u |want|.  Rows
  nothing maps to: zero, no bar."""
  a = R.f32(alpha)
  y, y_own, side, side_own = S.swconv_out_shifts(G, c['x'], c['Wl'], osh, oseg, side_rows, f16,
                                                 c['bias'], S.EPI_MASK, a, c['mask'])
  err = np.zeros_like(y) if exact else S.acc_bound(G, c['x'], c['Wl'], c['bias'])
  u = 0.0 if exact else S.U  # (the exact recipe: nothing rounds before the store)
  sy, ss = R.round_act(y, f16), R.round_act(side, f16)
  fixed = S.unshuffle_fixup(ss, c['mask'], sy, osh, oseg, a)
  want, bar = y.copy(), np.zeros_like(y)
  for b in range(G.nB):
    s = int(osh[b // oseg])
    td, r, ts, j = S.out_shift_rows(s, G.Ly)
    bar[b, r] = err[b, td] + (u * np.abs(y[b, r]) if u else 0.0)
    e_side = err[b, ts]
    n = abs(s)
    for q in range(n):
      ra = G.Ly - 2 - q if s > 0 else n - q
      mf = S.mask_factor(c['mask'][b, ra], a)
      want[b, ra] = fixed[b, ra]
      bar[b, ra] = (S.rounded_spread(y[b, ra], bar[b, ra], f16) +
                    S.rounded_spread(side[b, q], e_side[q], f16) * mf +
                    (2 * u * np.abs(fixed[b, ra]) if u else 0.0))
    zero = np.r_[0:n] if s > 0 else np.r_[G.Ly - n:G.Ly]
    assert not y_own[b, zero].any() and y_own[b].sum() == G.Ly - n
    want[b, zero], bar[b, zero] = fixed[b, zero], 0.0
    assert (fixed[b, zero] == 0).all()
  return want, bar


@pytest.mark.parametrize('G,osh,oseg,side_rows,Cy,tile', PARAMS)
def test_folded_fixup(G, osh, oseg, side_rows, Cy, tile, precision):
  f16 = precision
  for recipe in ('real', 'exact'):
    exact = recipe == 'exact'
    alpha = T.EXACT_ALPHA if exact else T.ALPHA
    c = T.case(G, f16, recipe)
    pr = Pair(G, c, f16, recipe, osh, oseg, side_rows, Cy, tile, alpha)
    two = pr.launch(folded=False)
    one = pr.launch(folded=True)
    # frame: guard intact, every row written, channel padding +0
    assert P.is_sentinel(one[pr.n:]), recipe
    v = pr.view(one)
    assert not bool((v[:, :, :G.N] == P.SENT).any()), recipe
    assert int(P.bits(v[:, :, G.N:]).numpy().astype(np.int64).__abs__().sum()) == 0, recipe
    # the two-launch form, bit for bit
    diff = P.bits(one) != P.bits(two)
    assert not bool(diff.any()), (recipe, np.argwhere(
        diff[:pr.n].reshape(G.nB, G.Ly, Cy).numpy())[:8])
    # the float64 statement
    want, bar = statement(G, c, f16, osh, oseg, side_rows, alpha, exact)
    got = v[:, :, :G.N].contiguous()
    if exact:
      P.assert_bits(got, want, f16)
    else:
      P.assert_act(got, want, f16, f32_err=bar)


def test_folded_and_two_launch_training_end_on_the_same_bits():
  """Three train() calls at cfg2's layer shapes with the default plan (folded where
  the library admits it) and with CALCIUMGAN_FOLD_FIXUP=0 (side buffers +
  cg_unshuffle_fixup): identical outputs and weights."""
  from test_determinism import _run
  shape = (2048, 102, 16, 4)
  a = _run(3, shape)
  b = _run(3, shape, {'CALCIUMGAN_FOLD_FIXUP': '0'})
  assert a['outputs'] == b['outputs'], (a['last'], b['last'])
  assert a['weights'] == b['weights']
