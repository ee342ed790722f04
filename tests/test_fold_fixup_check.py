"""Host side of the folded PhaseShuffle fix-up (cg_conv_desc.out_shifts with side ==
NULL): cg_swconv_check admits it exactly where a reflected row and its target are
registers of one wave -- the mask epilogue of the 32-row software-pipelined tiles,
two interleaved phases, Lu a multiple of 32, side_rows <= 31 -- and refuses it
everywhere else.  No GPU: the dry run dereferences nothing."""
import ctypes

import pytest

from calciumgan_amd import _lib
from calciumgan_amd import geometry as geo

EINVAL = _lib.CG_EINVAL
# cfg2's critic (BASELINE configs[1]): input gradient of layers 2..5, per layer
# (rows per sample and phase, channels in, channels out)
CFG2_DGRAD = [(512, 128, 64), (256, 192, 128), (128, 256, 192), (64, 320, 256)]


def desc(Lu, Cx, N, nB, tile, side_rows=10, epilogue=_lib.EPI_MASK, side=None):
  d = _lib.ConvDesc()
  d.x = d.w = d.y = d.mask_src = 0x1000
  d.nB, d.Lx, d.Cx, d.seg_size = nB, Lu, geo.pitch(Cx), 1
  d.taps, d.stride, d.off, d.Lu = 12, 1, -5, Lu
  d.N, d.Ly, d.Cy, d.y_stride, d.y_off = N, 2 * Lu, geo.pitch(N), 2, 0
  d.CK, d.epilogue, d.alpha = 32, epilogue, 0.3
  d.nphase, d.w_phase_stride, d.off_phase_step, d.yoff_phase_step = 2, 1 << 20, 1, 1
  d.tile, d.stage_ksteps = tile, 2
  d.out_shifts, d.out_seg_size, d.side, d.side_rows = 0x1000, max(1, nB // 3), side, side_rows
  return d


def check(d):
  return _lib.load().cg_swconv_check(ctypes.byref(d))


@pytest.mark.parametrize('nB', [128, 384])
def test_cfg2_critic_layers_are_admitted(nB):
  for Lu, Cx, N in CFG2_DGRAD:
    for tile in (13, 14, 15):
      assert check(desc(Lu, Cx, N, nB, tile)) == 0, (Lu, tile)


def test_refusals():
  ok = desc(64, 320, 256, 128, 14)
  assert check(ok) == 0
  # a 16-row sample: no whole 32-row wave
  assert check(desc(16, 320, 256, 128, 14)) == EINVAL
  assert check(desc(16, 320, 256, 128, 14, side=0x1000)) == EINVAL  # (with a side buffer too)
  # side_rows = 16 MT: a mirror pair may straddle two waves
  assert check(desc(64, 320, 256, 128, 14, side_rows=31)) == 0
  assert check(desc(64, 320, 256, 128, 14, side_rows=32)) == EINVAL
  assert check(desc(64, 320, 256, 128, 14, side_rows=32, side=0x1000)) == 0
  assert check(desc(64, 320, 256, 128, 14, side_rows=0)) == EINVAL
  # classic tiles and the 64-row-wave software-pipelined tiles
  for tile in sorted(_lib.TILES) + [t for t in _lib.SWP_TILES if t not in (13, 14, 15)]:
    assert check(desc(512, 128, 64, 128, tile)) == EINVAL, tile
  assert check(desc(512, 128, 64, 128, 1, side=0x1000)) == 0
  assert check(desc(512, 128, 64, 128, 10, side=0x1000)) == 0
  # other epilogues
  for epi in (_lib.EPI_NONE, _lib.EPI_LRELU, _lib.EPI_SIGMOID):
    assert check(desc(64, 320, 256, 128, 14, epilogue=epi)) == EINVAL, epi
  assert check(desc(64, 320, 256, 128, 14, epilogue=_lib.EPI_NONE, side=0x1000)) == 0
  # the phases' rows the other way round, one phase, a per-sample scale
  d = desc(64, 320, 256, 128, 14)
  d.y_off, d.yoff_phase_step = 1, -1
  assert check(d) == EINVAL
  d = desc(64, 320, 256, 128, 14)
  d.nphase, d.Ly, d.y_stride = 1, 64, 1
  assert check(d) == EINVAL
  d = desc(64, 320, 256, 128, 14)
  d.row_scale = 0x1000
  assert check(d) == EINVAL
