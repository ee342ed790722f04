"""GPU tests of cg_victor_purpura (csrc/victor_purpura.hip: Victor-Purpura edit
distances between the trains of a trial, one 16-lane row per pair) against its
numpy statement spike_metrics.victor_purpura_distance_frames -- bit for bit: the
programme only adds and takes minima -- and of compute_metrics.py
--victor_purpura on both devices.  Every case is one or two launches on valid
input.  Shapes are (B, T, C).

Covered, beside the small cases: the pair kernel past one pass of its grid of
512 x 16 row slots -- slots that walk a second pair of unrelated counts over the
boundary line and the LDS rings the first one left (reuse_3x96x102,
reuse_40x48x27, dg_2x2048x102 in a pitch-128 buffer), also on a workspace that
still holds an earlier call's contents; more than 13 strips of the shorter train
and the boundary line up to row T (long_1x2048x6: 64 strips of 129 blocks beside
pairs a hundred times shorter in the same wave); frame index 16383 at T = 16384,
the largest admitted; the pair index -> (i, j) decode at every one of the
8 386 560 pairs of C = 4096, the largest admitted, against two closed forms; a
workspace of exactly cg_victor_purpura_ws_bytes between 0xFF guards and guard
rows of NaN behind `dist`; T = 16385 and C = 4097 refused with nothing written.

Out of scope: B near the limit of 65 536 trials (the workspace alone is out of
reach of a test of a few seconds); two trains of more than 1024 spikes in one
pair (128 strips: the statement's sweep over their 4096 anti-diagonals is
cheap, a batch that makes the test worth more than long_1x2048x6 is not);
timing."""
import functools
import os

import numpy as np
import pytest
import torch

import compute_metrics as cm
from calciumgan_amd import _lib, nets
from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import h5_helper, spike_metrics
from test_hip_van_rossum import _run_dir
from van_rossum_cases import dg_batch
from victor_purpura_cases import (ROW_SLOTS, counts_difference, crafted_trial,
                                  first_set, grid_case, pair_count, second_set,
                                  unmatched_spikes)

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 2.0**-53


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _trials(B, T, C, seed, density):
  return (np.random.RandomState(seed).uniform(size=(B, T, C)) < density
          ).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
  """name -> (B, T, C) host trains (shared, not to be written to)."""
  if name == 'random_3x96x7':
    sp = _trials(3, 96, 7, seed=41, density=0.25)
    sp[0] = first_set().T        # silent, full and identical trains
  elif name == 'dense_2x40x17':
    sp = _trials(2, 40, 17, seed=42, density=0.5)
    sp[1] = second_set().T
  elif name == 'one_spike':
    sp = np.ones((1, 1, 1), np.float32)
  elif name == 'no_spike':
    sp = np.zeros((1, 1, 1), np.float32)
  elif name == 'dg_3x480x17':
    sp = dg_batch(17, 480, 3)
  elif name == 'crafted_1x200x13':
    sp = np.ascontiguousarray(crafted_trial().T[None])
  else:
    return grid_case(name)
  sp.setflags(write=False)
  return sp


CASES = ('random_3x96x7', 'dense_2x40x17', 'one_spike', 'no_spike', 'dg_3x480x17',
         'crafted_1x200x13', 'reuse_3x96x102', 'reuse_40x48x27', 'long_1x2048x6',
         't16384_1x16384x3')


@functools.lru_cache(maxsize=None)
def _statement(name, q=1.0):
  out = np.stack([spike_metrics.victor_purpura_distance_frames(t.T, q=q)
                  for t in _case(name)])
  out.setflags(write=False)
  return out


def _device(x, q=1.0):
  d = spike_metrics.victor_purpura_distance_device(x, q=q)
  torch.cuda.synchronize()
  assert d.dtype == torch.float64 and d.is_cuda
  assert tuple(d.shape) == (x.shape[0], x.shape[2], x.shape[2])
  return d.cpu().numpy()


def _check_structure(D):
  assert np.array_equal(_bits(D), _bits(D.transpose(0, 2, 1)))
  assert np.all(_bits(np.einsum('bii->bi', D)) == 0)   # +0.0, not -0.0


@pytest.mark.parametrize('name', CASES)
def test_bit_equal_to_the_statement(name):
  sp = _case(name)
  x = torch.from_numpy(sp.copy()).to(DEV)
  D = _device(x)
  want = _statement(name)
  diff = _bits(D) != _bits(want)
  print('%s: %d of %d elements differ' % (name, int(diff.sum()), diff.size))
  assert not diff.any(), np.argwhere(diff)[:8]
  _check_structure(D)
  # two calls give the same bits
  assert np.array_equal(_bits(_device(x)), _bits(D))


@pytest.mark.parametrize('q', [0.0, 48.0, 1000.0])
def test_closed_forms_on_the_crafted_trial(q):
  """q = 0: |n_i - n_j|; q / 24 >= 2: n_i + n_j - 2 |f_i & f_j|."""
  sp = _case('crafted_1x200x13')
  D = _device(torch.from_numpy(sp.copy()).to(DEV), q=q)
  want = counts_difference(sp[0].T) if q == 0 else unmatched_spikes(sp[0].T)
  assert np.array_equal(_bits(D[0]), _bits(want))
  _check_structure(D)


def test_strides_pitch_128_buffer_and_channel_major_storage():
  sp = _case('random_3x96x7')
  want = _device(torch.from_numpy(sp.copy()).to(DEV))
  assert np.array_equal(_bits(want), _bits(_statement('random_3x96x7')))
  buf = torch.full((3, 96, 128), 7.0, dtype=torch.float32, device=DEV)
  buf[:, :, :7] = torch.from_numpy(sp.copy()).to(DEV)
  x = buf[:, :, :7]
  assert x.stride() == (96 * 128, 128, 1)
  assert np.array_equal(_bits(_device(x)), _bits(want))
  rows = torch.from_numpy(np.ascontiguousarray(sp.transpose(0, 2, 1))).to(DEV)
  x = rows.transpose(1, 2)                           # stored (B, C, T)
  assert tuple(x.shape) == (3, 96, 7) and x.stride() == (7 * 96, 1, 96)
  assert np.array_equal(_bits(_device(x)), _bits(want))


@pytest.mark.parametrize('name', ['random_3x96x7', 'crafted_1x200x13'])
def test_nothing_in_the_workspace_needs_zeroing(name):
  """The C entry with a workspace and an output pre-filled with 0xFF bytes."""
  sp = _case(name)
  x = torch.from_numpy(sp.copy()).to(DEV)
  B, T, C = x.shape
  nbytes = _lib.load().cg_victor_purpura_ws_bytes(B, T, C)
  assert nbytes > 0
  ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
  dist = torch.full((B, C, C), float('nan'), dtype=torch.float64, device=DEV)
  _lib.call('cg_victor_purpura', nets._p(x), B, T, C, x.stride(0), x.stride(1),
            x.stride(2), spike_metrics.victor_purpura_cost(1.0), nets._p(dist),
            nets._p(ws), nbytes, nets._stream())
  torch.cuda.synchronize()
  assert np.array_equal(_bits(dist.cpu().numpy()), _bits(_statement(name)))


GUARD = 4096          # bytes of 0xFF on either side of the workspace
GUARD_ROWS = 3        # rows of NaN behind dist


def _entry(x, q=1.0, ws_buf=None):
  """The C entry on a (B, T, C) device tensor read in place, with a workspace of
  exactly cg_victor_purpura_ws_bytes inside a larger buffer of 0xFF bytes (or
  inside `ws_buf`, an earlier call's buffer, as it was left) and `dist` NaN
  with guard rows behind it.  The bytes around the workspace and the guard rows
  must come back untouched.  -> (dist as numpy, the buffer)."""
  B, T, C = x.shape
  nbytes = _lib.load().cg_victor_purpura_ws_bytes(B, T, C)
  assert nbytes > 0
  if ws_buf is None:
    ws_buf = torch.full((GUARD + nbytes + GUARD,), 0xFF, dtype=torch.uint8,
                        device=DEV)
  assert ws_buf.numel() == GUARD + nbytes + GUARD
  ws = ws_buf[GUARD:GUARD + nbytes]
  assert ws.data_ptr() % 8 == 0
  dist = torch.full((B * C + GUARD_ROWS, C), float('nan'), dtype=torch.float64,
                    device=DEV)
  _lib.call('cg_victor_purpura', nets._p(x), B, T, C, x.stride(0), x.stride(1),
            x.stride(2), spike_metrics.victor_purpura_cost(q), nets._p(dist),
            nets._p(ws), nbytes, nets._stream())
  torch.cuda.synchronize()
  assert bool((ws_buf[:GUARD] == 0xFF).all()), 'bytes before the workspace'
  assert bool((ws_buf[GUARD + nbytes:] == 0xFF).all()), 'bytes after the workspace'
  assert bool(torch.isnan(dist[B * C:]).all()), 'guard rows of dist'
  return dist[:B * C].view(B, C, C).cpu().numpy(), ws_buf


def test_dg_trials_of_the_workload_shape_in_a_pitch_128_buffer():
  """(2, 2048, 102) DG trials read through a pitch-128 buffer whose padding
  holds 7.0: 10 302 pairs on 8192 row slots."""
  name = 'dg_2x2048x102'
  sp = _case(name)
  assert pair_count(sp) > ROW_SLOTS
  buf = torch.full((2, 2048, 128), 7.0, dtype=torch.float32, device=DEV)
  buf[:, :, :102] = torch.from_numpy(sp.copy()).to(DEV)
  x = buf[:, :, :102]
  assert x.stride() == (2048 * 128, 128, 1)
  D = _device(x)
  diff = _bits(D) != _bits(_statement(name))
  print('%s: %d of %d elements differ' % (name, int(diff.sum()), diff.size))
  assert not diff.any(), np.argwhere(diff)[:8]
  _check_structure(D)
  assert np.array_equal(_bits(_device(x)), _bits(D))


@pytest.mark.parametrize('name', ['reuse_3x96x102', 'long_1x2048x6'])
def test_workspace_of_exactly_the_size_asked_for_between_guards(name):
  x = torch.from_numpy(_case(name).copy()).to(DEV)
  D, _ = _entry(x)
  diff = _bits(D) != _bits(_statement(name))
  assert not diff.any(), np.argwhere(diff)[:8]


def test_slot_reuse_on_a_workspace_an_earlier_call_left():
  """The second call finds the first call's boundary lines, counts and frames in
  place of 0xFF: the same bits."""
  name = 'reuse_3x96x102'
  x = torch.from_numpy(_case(name).copy()).to(DEV)
  D1, buf = _entry(x)
  left = buf.clone()
  assert bool((left[GUARD:-GUARD] != 0xFF).any())
  D2, buf = _entry(x, ws_buf=buf)
  assert np.array_equal(_bits(D1), _bits(_statement(name)))
  assert np.array_equal(_bits(D2), _bits(D1))


@pytest.mark.parametrize('q', [0.0, 1000.0])
def test_every_pair_index_decodes_at_the_largest_admitted_C(q):
  """(1, 4, 4096): q = 0 gives |n_i - n_j| and q = 1000 gives n_i + n_j - 2
  |f_i & f_j| -- small integers, so exact -- at every one of the 8 386 560
  pairs; `dist` starts as NaN, so an element not written, or written from
  another pair's (i, j), shows."""
  sp = _case('decode_1x4x4096')
  assert sp.shape == (1, 4, 4096)
  want = counts_difference(sp[0].T) if q == 0 else unmatched_spikes(sp[0].T)
  assert np.array_equal(want, np.rint(want))          # no non-integer entry
  D, _ = _entry(torch.from_numpy(sp.copy()).to(DEV), q=q)
  assert not np.isnan(D).any()
  diff = _bits(D[0]) != _bits(want)
  print('q=%g: %d of %d elements differ' % (q, int(diff.sum()), diff.size))
  assert not diff.any(), np.argwhere(diff)[:8]
  _check_structure(D)


@pytest.mark.parametrize('shape', [(1, 16385, 3), (1, 4, 4097)])
def test_shapes_past_the_limits_are_refused_with_nothing_written(shape):
  B, T, C = shape
  lib = _lib.load()
  assert lib.cg_victor_purpura_ws_bytes(B, T, C) == -1
  assert lib.cg_victor_purpura_ws_bytes(B, min(T, 16384), min(C, 4096)) > 0
  x = torch.ones(shape, dtype=torch.float32, device=DEV)
  nbytes = 4 << 20     # (more than either shape would need, were it admitted)
  ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
  dist = torch.full((B, C, C), float('nan'), dtype=torch.float64, device=DEV)
  rc = lib.cg_victor_purpura(nets._p(x), B, T, C, x.stride(0), x.stride(1),
                             x.stride(2), spike_metrics.victor_purpura_cost(1.0),
                             nets._p(dist), nets._p(ws), nbytes, nets._stream())
  torch.cuda.synchronize()
  assert rc == _lib.CG_EINVAL
  assert bool(torch.isnan(dist).all()) and bool((ws == 0xFF).all())
  with pytest.raises(ValueError):
    spike_metrics.victor_purpura_distance_device(x)


def test_wrapper_refuses_host_arrays_wrong_dtype_and_rank():
  with pytest.raises(ValueError):
    spike_metrics.victor_purpura_distance_device(np.zeros((2, 24, 3), np.float32))
  with pytest.raises(ValueError):
    spike_metrics.victor_purpura_distance_device(
        torch.zeros(2, 24, 3, dtype=torch.float64, device=DEV))
  with pytest.raises(ValueError):
    spike_metrics.victor_purpura_distance_device(
        torch.zeros(24, 3, dtype=torch.float32, device=DEV))


def test_compute_metrics_with_the_flag_on_both_devices(tmp_path):
  """victor_purpura_kl is the same number on both devices; every other key
  compares as test_compute_metrics_on_the_device_against_the_host_path compares
  it (firing rates exactly; correlation and van Rossum samples to their
  rounding bounds there, their keys present here)."""
  d = dg.make_dataset(num_neurons=6, sequence_length=480, num_segments=24)
  fakes, hps, reports = {}, {}, {}
  for device in ('cpu', 'gpu'):
    os.makedirs(tmp_path / device)
    fakes[device] = _run_dir(tmp_path / device, d)
    hps[device] = cm.build_parser().parse_args(
        ['--output_dir', str(tmp_path / device), '--num_processors', '1',
         '--verbose', '0', '--device', device, '--batch_trials', '10',
         '--victor_purpura'])
    reports[device] = cm.main(hps[device])[0]
  cpu, gpu = reports['cpu'], reports['gpu']
  assert set(cpu) == set(gpu)
  assert set(gpu) >= {'firing_rate_kl', 'correlation_kl', 'van_rossum_kl',
                      'van_rossum_heatmap_min', 'victor_purpura_kl'}
  print('Victor-Purpura KL cpu / gpu:', cpu['victor_purpura_kl']['mean'],
        gpu['victor_purpura_kl']['mean'])
  assert cpu['victor_purpura_kl'] == gpu['victor_purpura_kl']
  assert np.isfinite(gpu['victor_purpura_kl']['mean'])
  assert cpu['firing_rate_kl'] == gpu['firing_rate_kl']
  sc, sg = (h5_helper.get(fakes[k], 'spikes') for k in ('cpu', 'gpu'))
  assert sc.tobytes() == sg.tobytes() and sc.shape == sg.shape
  # the samples behind the figure hold the same bits, trial by trial
  pairs = cm.device_pairs(hps['gpu'], fakes['gpu'])
  hc = hps['cpu']
  assert len(pairs['victor_purpura']) == hc.num_samples == 24
  for i in range(hc.num_samples):
    for h, g in zip(cm.trial_victor_purpura(hc, fakes['cpu'], i),
                    pairs['victor_purpura'][i]):
      assert np.array_equal(_bits(h), _bits(g)), i
  # correlation and van Rossum samples: the bounds of the existing test
  T = 480
  for i in range(hc.num_samples):
    for h, g in zip(cm.correlation_coefficient(hc, fakes['cpu'], i),
                    pairs['correlation'][i]):
      assert h.shape == g.shape and np.abs(h - g).max() <= 4 * (T // 12) * U
  from test_hip_van_rossum import _distance_tolerance
  iu = np.triu_indices(6, k=1)
  for i in range(hc.num_samples):
    for f, h, g in zip((hc.validation_cache, fakes['cpu']),
                       cm.trial_van_rossum(hc, fakes['cpu'], i),
                       pairs['van_rossum'][i]):
      tol = _distance_tolerance(cm._spikes(hc, f, 'CW', trial=i))
      assert np.all(np.abs(h - g) <= tol[iu]), i
  for neuron in hc.neurons:
    real = cm._spikes(hc, hc.validation_cache, 'NW', neuron=neuron, num_trials=45)
    fake = cm._spikes(hc, fakes['cpu'], 'NW', neuron=neuron, num_trials=45)
    tol = _distance_tolerance(np.concatenate([real, fake]))[len(real):, :len(fake)]
    a = cpu['van_rossum_heatmap_min'][int(neuron)]
    b = gpu['van_rossum_heatmap_min'][int(neuron)]
    assert abs(a - b) <= tol.max() + 2.0**-23 * max(a, b)
  # without the flag the device report has no such key
  plain = cm.build_parser().parse_args(
      ['--output_dir', str(tmp_path / 'gpu'), '--num_processors', '1',
       '--verbose', '0', '--device', 'gpu', '--batch_trials', '10'])
  assert 'victor_purpura_kl' not in cm.main(plain)[0]
  # identical spike sets: exactly zero on the device path
  h5_helper.overwrite(fakes['gpu'], 'spikes', d['spikes'].astype(np.int8))
  z = cm.main(hps['gpu'])[0]
  assert z['victor_purpura_kl']['mean'] == 0
