"""GPU tests of cg_population_states and cg_state_neighbours
(csrc/state_neighbours.hip: the Gram tile on v_mfma_f32_16x16x32_bf16 with the
neurons as the K dimension, the k smallest of every row and its count kept in
registers) against their numpy statements spike_metrics.population_states /
state_neighbours -- equality of integers throughout -- and of compute_metrics.py
--state_metrics on both devices.

The kernel's paths: a workgroup owns 128 states of A (32 a wave, two 16-tiles)
and 64-state tiles of B; K is staged in chunks of 128 elements (C > 128: more
than one chunk, A staged again per tile); B is split over workgroups while Sa is
small, with a merge launch.  Covered: Sa and Sb below, at and past 16, 64 and
128; C below one K step of 32, at and past 64 and 128; several row blocks (Sa =
700); several splits (Sb = 2500); the exactness bound itself (C bin^2 = 2^24).
Every output sits between guard words."""
import os

import numpy as np
import pytest
import torch

import compute_metrics as cm
import state_neighbour_cases as SC
from calciumgan_amd import _lib
from calciumgan_amd.gan.utils import spike_metrics as sm

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = -7
GUARD = 1024   # elements of SENTINEL on either side of an output


def _guarded(n, dtype=torch.int32):
  buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
  return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
  return bool((buf[:GUARD] == SENTINEL).all()) and bool(
      (buf[-GUARD:] == SENTINEL).all())


def _check(got, want):
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape, (got.shape, want.shape)
  diff = got != want
  print('%d of %d elements differ' % (int(diff.sum()), diff.size))
  assert not diff.any(), [(tuple(ix), int(got[tuple(ix)]), int(want[tuple(ix)]))
                          for ix in np.argwhere(diff)[:8]]


# -- cg_population_states ----------------------------------------------------------
def _trains(B, T, C, density):
  return (np.random.RandomState(1000 * C + T).uniform(size=(B, T, C)) < density
          ).astype(np.float32)


def _states_of(x, bin):
  """cg_population_states of a float32 device (B, T, C) view into a guarded
  buffer: int32 (S, Cp) of the bf16 values, padding included."""
  B, T, C = x.shape
  S, Cp = B * (T // bin), -(-C // 32) * 32
  buf, out = _guarded(S * Cp, torch.int16)
  _lib.call('cg_population_states', x, B, T, C, x.stride(0), x.stride(1),
            x.stride(2), bin, out, _lib.stream())
  torch.cuda.synchronize()
  assert _guards_intact(buf)
  got = out.view(torch.bfloat16).view(S, Cp).float().cpu().numpy()
  assert (got == np.round(got)).all()
  return got.astype(np.int32)


def _check_states(x, sp, bin):
  C = sp.shape[2]
  got = _states_of(x, bin)
  want = sm.population_states(sp, bin)
  _check(got[:, :C], want)
  assert not got[:, C:].any()
  # the wrapper gives the same set
  dev = sm.population_states_device(x, bin)
  assert (dev.C, dev.bin, len(dev)) == (C, bin, len(want))
  _check(dev.counts().cpu().numpy(), want)
  return want


@pytest.mark.parametrize('shape', [(1, 5, 3, 5, 0.5), (2, 50, 17, 12, 0.5),
                                   (3, 300, 102, 1, 0.5), (3, 300, 102, 12, 0.5),
                                   (3, 300, 102, 12, 0.01),
                                   (1, 127, 130, 127, 1.0)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_population_states_equal_the_statement(shape):
  B, T, C, bin, density = shape
  sp = _trains(B, T, C, density)
  want = _check_states(torch.from_numpy(sp).to(DEV), sp, bin)
  if density == 1.0:
    assert want.max() == 127 == bin


def test_population_states_read_strided_views_in_place():
  B, T, C, bin = 2, 50, 17, 12
  sp = _trains(B, T, C, 0.5)
  buf = torch.full((B, T, 128), 7.0, dtype=torch.float32, device=DEV)
  buf[:, :, :C] = torch.from_numpy(sp).to(DEV)
  x = buf[:, :, :C]
  assert x.stride() == (T * 128, 128, 1)
  _check_states(x, sp, bin)
  rows = torch.from_numpy(np.ascontiguousarray(sp.transpose(0, 2, 1))).to(DEV)
  x = rows.transpose(1, 2)                           # stored (B, C, T)
  assert tuple(x.shape) == (B, T, C) and x.stride() == (C * T, 1, T)
  _check_states(x, sp, bin)


def test_nan_is_a_spike_and_minus_zero_is_not():
  sp = np.zeros((1, 24, 3), np.float32)
  sp[0, 1, 0] = np.nan
  sp[0, 2, 1] = -0.0
  sp[0, 13, 2] = -3.5
  got = _check_states(torch.from_numpy(sp).to(DEV), sp, 12)
  assert got.tolist() == [[1, 0, 0], [0, 0, 1]]


# -- cg_state_neighbours -------------------------------------------------------------
def _device_set(x, bin=SC.BIN):
  x = np.asarray(x)
  S, C = x.shape
  t = torch.zeros(S, -(-C // 32) * 32, dtype=torch.bfloat16, device=DEV)
  t[:, :C] = torch.from_numpy(x.astype(np.float32)).to(DEV).to(torch.bfloat16)
  return sm.DeviceStates(t, C, bin)


def _query(a, b, k, exclude_self=False, radius_b=None, knn=True, within=None):
  """cg_state_neighbours with every output between guards; (knn, within) as
  host arrays, None for what was not asked for."""
  within = (radius_b is not None) if within is None else within
  Sa, Sb = len(a), len(b)
  need = _lib.load().cg_state_neighbours_ws_bytes(Sa, Sb, a.C, a.bin, k)
  assert need >= 4 * (Sa + Sb)
  # (the workspace's contents do not matter: poison)
  ws = torch.full((need // 4 + 4,), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
  kbuf, kout = _guarded(Sa * k)
  wbuf, wout = _guarded(Sa)
  rad = None
  if within:
    rad = torch.from_numpy(np.asarray(radius_b, dtype=np.int32)).to(DEV)
  _lib.call('cg_state_neighbours', a.tensor, Sa, b.tensor, Sb, a.C, a.bin, k,
            1 if exclude_self else 0, rad, kout if knn else None,
            wout if within else None, ws, _lib.stream())
  torch.cuda.synchronize()
  assert _guards_intact(kbuf) and _guards_intact(wbuf)
  if not knn:
    assert bool((kout == SENTINEL).all())
  if not within:
    assert bool((wout == SENTINEL).all())
  return (kout.view(Sa, k).cpu().numpy() if knn else None,
          wout.cpu().numpy() if within else None)


def _compare(xa, xb, k, exclude_self=False, radius_b=None, bin=SC.BIN):
  want_knn, want_within = sm.state_neighbours(xa, xb, k, exclude_self, radius_b)
  a = _device_set(xa, bin)
  b = a if exclude_self else _device_set(xb, bin)
  knn, within = _query(a, b, k, exclude_self, radius_b)
  _check(knn, want_knn)
  if radius_b is not None:
    _check(within, want_within)
  return a, b, knn, within


@pytest.mark.parametrize('density', SC.DENSITIES)
@pytest.mark.parametrize('C', SC.NEURONS)
def test_neighbours_equal_the_statement(C, density):
  kinds = ('zero', 'mixed', 'huge', None)
  n = 0
  for Sa, Sb in SC.PAIRS:
    xa, xb = SC.states(Sa, C, density, 1), SC.states(Sb, C, density, 2)
    for k in SC.KS:
      kind = kinds[n % 4]
      n += 1
      rad = None if kind is None else SC.radii(Sb, kind, C)
      print(Sa, Sb, C, k, kind)
      _compare(xa, xb, k, radius_b=rad)


@pytest.mark.parametrize('S', [1, 2, 17, 128, 129, 300])
def test_self_queries_with_planted_duplicates(S):
  for C, density in ((3, 0.5), (102, 0.01), (130, 0.5)):
    x = SC.with_duplicates(SC.states(S, C, density, 3), seed=S)
    for k in SC.KS:
      _, _, knn, _ = _compare(x, x, k, exclude_self=True,
                              radius_b=SC.radii(S, 'mixed', C))
      if S == 1:
        assert (knn == SC.NONE).all()
      if k >= S:
        assert (knn[:, S - 1:] == SC.NONE).all()
    if S >= 2:
      # a twin at another index counts, at distance 0
      knn = _compare(x, x, 1, exclude_self=True)[2]
      assert (knn[:, 0] == 0).any()
    # the same set without the exclusion: every state finds itself
    assert (_compare(x, x, 1)[2][:, 0] == 0).all()


@pytest.mark.parametrize('shape', [(700, 40, 102), (40, 2500, 102),
                                   (700, 700, 130), (40, 2500, 257)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_several_row_blocks_and_several_splits(shape):
  """Sa = 700: six row blocks of 128.  Sb = 2500 against Sa = 40: 40 tiles of B
  split over 40 workgroups, merged by the second launch."""
  Sa, Sb, C = shape
  for density in SC.DENSITIES:
    xa, xb = SC.states(Sa, C, density, 4), SC.states(Sb, C, density, 5)
    xb = SC.with_duplicates(xb, seed=1)
    for k, kind in ((5, 'mixed'), (8, 'zero'), (1, 'huge')):
      _compare(xa, xb, k, radius_b=SC.radii(Sb, kind, C))
    if Sa == Sb:
      x = SC.with_duplicates(xa, seed=2)
      _compare(x, x, 5, exclude_self=True, radius_b=SC.radii(Sa, 'mixed', C))


@pytest.mark.parametrize('shape', [(129, 300, 102), (40, 2500, 65)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_knn_alone_within_alone_both_and_a_second_call(shape):
  Sa, Sb, C = shape
  xa, xb = SC.states(Sa, C, 0.5, 6), SC.states(Sb, C, 0.5, 7)
  rad = SC.radii(Sb, 'mixed', C)
  want_knn, want_within = sm.state_neighbours(xa, xb, 5, radius_b=rad)
  a, b = _device_set(xa), _device_set(xb)
  both = _query(a, b, 5, radius_b=rad)
  _check(both[0], want_knn)
  _check(both[1], want_within)
  knn_only = _query(a, b, 5)
  assert knn_only[1] is None
  _check(knn_only[0], want_knn)
  within_only = _query(a, b, 5, radius_b=rad, knn=False)
  assert within_only[0] is None
  _check(within_only[1], want_within)
  # a second call gives the same bits
  again = _query(a, b, 5, radius_b=rad)
  assert again[0].tobytes() == both[0].tobytes()
  assert again[1].tobytes() == both[1].tobytes()
  # the wrapper
  knn, within = sm.state_neighbours_device(a, b, 5, radius_b=rad)
  assert knn.dtype == within.dtype == torch.int32 and knn.is_cuda
  _check(knn.cpu().numpy(), want_knn)
  _check(within.cpu().numpy(), want_within)
  knn, within = sm.state_neighbours_device(a, b, 5)
  assert within is None
  _check(knn.cpu().numpy(), want_knn)


def test_the_largest_admitted_sum_and_the_first_refused():
  """C bin^2 = 4096 * 64^2 = 2^24 exactly, states of 63 and 64 throughout: dot
  products within 3 % of 2^24, where an f32 sum past the bound would round."""
  C, bin = _lib.CONSTANTS['CG_STATE_MAX_C'], 64
  assert C * bin * bin == _lib.CONSTANTS['CG_STATE_EXACT_SUM'] == 1 << 24
  rng = np.random.RandomState(5)
  xa = (63 + (rng.uniform(size=(17, C)) < 0.5)).astype(np.int32)
  xb = (63 + (rng.uniform(size=(33, C)) < 0.5)).astype(np.int32)
  xa[3] = 64
  xb[7] = 64            # a . b = 2^24, d2 = 0
  xb[8] = 0             # d2 = |a|^2
  rad = SC.radii(33, 'mixed', C)
  _, _, knn, _ = _compare(xa, xb, 5, radius_b=rad, bin=bin)
  assert knn[3, 0] == 0
  # bin 65 at the same C is refused, with nothing written
  lib = _lib.load()
  a, b = _device_set(xa, 65), _device_set(xb, 65)
  assert lib.cg_state_neighbours_ws_bytes(17, 33, C, 65, 5) == -1
  assert lib.cg_state_neighbours_ws_bytes(17, 33, C, 64, 5) > 0
  ws = torch.full((4096,), SENTINEL, dtype=torch.int32, device=DEV)
  out = torch.full((17 * 5,), SENTINEL, dtype=torch.int32, device=DEV)
  rc = lib.cg_state_neighbours(a.tensor, 17, b.tensor, 33, C, 65, 5, 0, None,
                               out, None, ws, _lib.stream())
  assert rc == _lib.CG_EINVAL
  torch.cuda.synchronize()
  assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
  with pytest.raises(ValueError):
    sm.state_neighbours_device(a, b, 5)
  # the other end of the bound: bin 127 admits C = 1040 and refuses 1041
  assert lib.cg_state_neighbours_ws_bytes(17, 33, 1040, 127, 5) > 0
  assert lib.cg_state_neighbours_ws_bytes(17, 33, 1041, 127, 5) == -1
  xa = (126 + (rng.uniform(size=(17, 1040)) < 0.5)).astype(np.int32)
  xb = (126 + (rng.uniform(size=(33, 1040)) < 0.5)).astype(np.int32)
  _compare(xa, xb, 8, radius_b=SC.radii(33, 'mixed', 1040), bin=127)


def test_scores_are_the_same_dict_on_both_devices():
  ref = sm.population_states(SC.gain_trials(1, trials=12, C=102))
  other = sm.population_states(SC.gain_trials(3, trials=10, C=102, clip=True))
  want = sm.state_scores(ref, other, 5)
  got = sm.state_scores(_device_set(ref), _device_set(other), 5,
                        neighbours=sm.state_neighbours_device)
  print(want)
  assert got == want
  assert got['num_states'] == [480, 400]


# -- compute_metrics.py --------------------------------------------------------------
def test_compute_metrics_state_flag_on_both_devices(tmp_path):
  reports, plain = {}, {}
  for device in ('cpu', 'gpu'):
    os.makedirs(tmp_path / device)
    fake, real_spikes, fake_spikes = SC.run_dir(tmp_path / device)
    args = ['--output_dir', str(tmp_path / device), '--num_processors', '1',
            '--verbose', '0', '--device', device, '--batch_trials', '5']
    hp = cm.build_parser().parse_args(args)
    assert not hasattr(hp, 'state_metrics')
    plain[device] = cm.main(hp)[0]
    reports[device] = cm.main(
        cm.build_parser().parse_args(args + ['--state_metrics']))[0]
  cpu, gpu = reports['cpu'], reports['gpu']
  print('states cpu:', cpu['states'])
  print('states gpu:', gpu['states'])
  assert cpu['states'] == gpu['states']
  assert gpu['states'] == SC.expected_report(real_spikes, fake_spikes)
  assert gpu['states']['generated'] != gpu['states']['floor']
  assert gpu['states']['floor']['num_states'] == [480, 480]
  for device in ('cpu', 'gpu'):
    assert 'states' not in plain[device]
    rest = {k: v for k, v in reports[device].items()
            if k not in ('states', 'elapse')}
    assert rest == {k: v for k, v in plain[device].items() if k != 'elapse'}
