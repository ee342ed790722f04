"""GPU tests of cg_spike_ccg and cg_spike_population_hist (csrc/spike_ccg.hip:
cross-correlograms on v_mfma_f32_16x16x32_bf16 with time as the K dimension,
population counts per frame) against their numpy statements
spike_metrics.cross_correlogram / population_count_histogram -- equality of
integers throughout -- and of compute_metrics.py --temporal_metrics on both
devices.  Shapes are (B, T, C, max_lag).

The kernel's paths: a workgroup owns a 64 x 64 block of neurons at 8 consecutive
lags and walks T in chunks of 128 frames.  Covered: C below one 16-tile, C not a
multiple of 16, more than one 64-block (102, 1024); T below one k-step of 32,
T not a multiple of the chunk, many chunks; a lag group of one lag (max_lag 0,
8, 24, 256), lags >= T; both fragment shifts parities at every lag."""
import functools
import os

import numpy as np
import pytest
import torch

import compute_metrics as cm
from calciumgan_amd import _lib
from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import h5_helper, spike_metrics
from test_hip_van_rossum import _distance_tolerance, _run_dir
from van_rossum_cases import dg_batch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 2.0**-53
SENTINEL = -7
GUARD = 1024   # int32 elements of SENTINEL on either side of an output

SHAPES = [(1, 5, 3, 8), (2, 50, 17, 8), (3, 480, 6, 24), (2, 1100, 40, 24),
          (1, 2048, 102, 24), (1, 96, 33, 0), (2, 300, 16, 256)]
DENSITIES = [0.01, 0.5]
FIGURES = ('autocorrelogram_mae', 'lag_covariance_mae',
           'lag_covariance_correlation', 'cross_correlogram_mae',
           'population_count_js_bits')


@functools.lru_cache(maxsize=None)
def _trials(B, T, C, density):
  sp = (np.random.RandomState(1000 * C + T).uniform(size=(B, T, C)) < density
        ).astype(np.float32)
  sp.setflags(write=False)
  return sp


@functools.lru_cache(maxsize=None)
def _ccg_statement(B, T, C, max_lag, density):
  out = spike_metrics.cross_correlogram(_trials(B, T, C, density), max_lag)
  out.setflags(write=False)
  return out


def _dev(sp):
  return torch.from_numpy(np.array(sp, dtype=np.float32)).to(DEV)


def _ccg(x, max_lag):
  out = spike_metrics.cross_correlogram_device(x, max_lag)
  torch.cuda.synchronize()
  assert out.dtype == torch.int32 and out.is_cuda
  assert tuple(out.shape) == (x.shape[0], max_lag + 1, x.shape[2], x.shape[2])
  return out.cpu().numpy()


def _hist(x):
  out = spike_metrics.population_count_histogram_device(x)
  torch.cuda.synchronize()
  assert out.dtype == torch.int32 and out.is_cuda
  assert tuple(out.shape) == (x.shape[0], x.shape[2] + 1)
  return out.cpu().numpy()


def _check(got, want):
  diff = got != want
  print('%d of %d elements differ' % (int(diff.sum()), diff.size))
  assert not diff.any(), [(tuple(ix), int(got[tuple(ix)]), int(want[tuple(ix)]))
                          for ix in np.argwhere(diff)[:8]]


def test_a_pair_three_frames_apart_in_different_16_blocks():
  """i fires at t0 only, j at t0 + 3 only: one count at [3][i][j], none at
  [3][j][i] -- a C/D write with rows and columns swapped shows here."""
  T, C, t0, i, j = 70, 40, 29, 3, 21
  sp = np.zeros((1, T, C), np.float32)
  sp[0, t0, i] = 1
  sp[0, t0 + 3, j] = 1
  got = _ccg(_dev(sp), 8)
  assert got[0, 3, i, j] == 1 and got[0, 3, j, i] == 0
  assert got[0, 0, i, i] == 1 and got[0, 0, j, j] == 1
  assert got.sum() == 3
  _check(got, spike_metrics.cross_correlogram(sp, 8))


@pytest.mark.parametrize('density', DENSITIES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_ccg_equals_the_statement(shape, density):
  B, T, C, max_lag = shape
  x = _dev(_trials(B, T, C, density))
  got = _ccg(x, max_lag)
  _check(got, _ccg_statement(B, T, C, max_lag, density))
  # two calls give the same bits
  assert np.array_equal(_ccg(x, max_lag), got)


def test_ccg_of_dg_trials():
  sp = dg_batch(17, 480, 3)
  _check(_ccg(_dev(sp), 24), spike_metrics.cross_correlogram(sp, 24))


def test_no_count_crosses_from_one_sample_to_the_next():
  """Two samples adjacent in memory: a spike in the last frame of sample 0 and
  one in the first frame of sample 1."""
  T, C = 64, 5
  sp = np.zeros((2, T, C), np.float32)
  sp[0, T - 1, 1] = 1
  sp[1, 0, 2] = 1
  x = _dev(sp)
  assert x.is_contiguous()
  got = _ccg(x, 8)
  assert got[0, 0, 1, 1] == 1 and got[1, 0, 2, 2] == 1 and got.sum() == 2
  _check(got, spike_metrics.cross_correlogram(sp, 8))


@pytest.mark.parametrize('T', [32, 128, 256])
def test_a_spike_in_the_last_frame_of_a_multiple_of_32(T):
  C = 4
  sp = np.zeros((1, T, C), np.float32)
  sp[0, T - 1, 0] = 1
  sp[0, T - 6, 3] = 1
  got = _ccg(_dev(sp), 8)
  assert got[0, 5, 3, 0] == 1 and got[0, 5, 0, 3] == 0
  assert got[0, 0, 0, 0] == 1 and got.sum() == 3
  _check(got, spike_metrics.cross_correlogram(sp, 8))


def test_nan_is_a_spike_and_minus_zero_is_not():
  sp = np.zeros((1, 40, 3), np.float32)
  sp[0, 7, 0] = np.nan
  sp[0, 9, 1] = -0.0
  sp[0, 10, 2] = -3.5
  got = _ccg(_dev(sp), 4)
  assert got[0, 0, 0, 0] == 1 and got[0, 0, 1, 1] == 0 and got[0, 3, 0, 2] == 1
  _check(got, spike_metrics.cross_correlogram(sp, 4))
  h = _hist(_dev(sp))
  assert np.array_equal(h[0], [38, 2, 0, 0])
  assert np.array_equal(h, spike_metrics.population_count_histogram(sp))


def test_strides_pitch_128_buffer_and_channel_major_storage():
  B, T, C, max_lag = 2, 50, 17, 8
  sp = _trials(B, T, C, 0.5)
  want = _ccg_statement(B, T, C, max_lag, 0.5)
  want_hist = spike_metrics.population_count_histogram(sp)
  buf = torch.full((B, T, 128), 7.0, dtype=torch.float32, device=DEV)
  buf[:, :, :C] = _dev(sp)
  x = buf[:, :, :C]
  assert x.stride() == (T * 128, 128, 1)
  _check(_ccg(x, max_lag), want)
  _check(_hist(x), want_hist)
  rows = _dev(np.ascontiguousarray(sp.transpose(0, 2, 1)))
  x = rows.transpose(1, 2)                           # stored (B, C, T)
  assert tuple(x.shape) == (B, T, C) and x.stride() == (C * T, 1, T)
  _check(_ccg(x, max_lag), want)
  _check(_hist(x), want_hist)


def _guarded(n):
  """An int32 buffer of SENTINEL with n elements between two guards."""
  buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
  return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
  return bool((buf[:GUARD] == SENTINEL).all()) and bool(
      (buf[-GUARD:] == SENTINEL).all())


@pytest.mark.parametrize('shape', [(2, 50, 17, 8), (2, 300, 16, 256)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_every_element_is_written_and_nothing_beside_the_output(shape):
  B, T, C, max_lag = shape
  x = _dev(_trials(B, T, C, 0.5))
  buf, out = _guarded(B * (max_lag + 1) * C * C)
  _lib.call('cg_spike_ccg', x, B, T, C, x.stride(0), x.stride(1), x.stride(2),
            max_lag, out, _lib.stream())
  hbuf, hout = _guarded(B * (C + 1))
  _lib.call('cg_spike_population_hist', x, B, T, C, x.stride(0), x.stride(1),
            x.stride(2), hout, _lib.stream())
  torch.cuda.synchronize()
  assert _guards_intact(buf) and _guards_intact(hbuf)
  _check(out.view(B, max_lag + 1, C, C).cpu().numpy(),
         _ccg_statement(B, T, C, max_lag, 0.5))
  _check(hout.view(B, C + 1).cpu().numpy(),
         spike_metrics.population_count_histogram(_trials(B, T, C, 0.5)))


def test_the_largest_admitted_C_decodes():
  """(1, 4, 1024), max_lag 0: 256 blocks of 64 x 64 neurons, every element of
  the sentinel-filled output written with its own pair's count."""
  C = _lib.CONSTANTS['CG_CCG_MAX_C']
  assert C == 1024 and _lib.CONSTANTS['CG_CCG_MAX_LAG'] == 256
  sp = _trials(1, 4, C, 0.5)
  x = _dev(sp)
  buf, out = _guarded(C * C)
  _lib.call('cg_spike_ccg', x, 1, 4, C, x.stride(0), x.stride(1), x.stride(2),
            0, out, _lib.stream())
  torch.cuda.synchronize()
  assert _guards_intact(buf)
  _check(out.view(1, 1, C, C).cpu().numpy(),
         spike_metrics.cross_correlogram(sp, 0))
  _check(_hist(x), spike_metrics.population_count_histogram(sp))


def test_refused_arguments_return_einval_and_write_nothing():
  lib = _lib.load()
  B, T, C, L = 2, 20, 5, 3
  x = torch.ones(B, T, C, dtype=torch.float32, device=DEV)
  out = torch.full((B * (L + 1) * C * C,), SENTINEL, dtype=torch.int32,
                   device=DEV)
  hist = torch.full((B * (C + 1),), SENTINEL, dtype=torch.int32, device=DEV)
  st = x.stride()

  def ccg(spikes=x, B=B, T=T, C=C, max_lag=L, o=out):
    return lib.cg_spike_ccg(spikes, B, T, C, st[0], st[1], st[2], max_lag, o,
                            _lib.stream())

  def pop(spikes=x, B=B, T=T, C=C, o=hist):
    return lib.cg_spike_population_hist(spikes, B, T, C, st[0], st[1], st[2], o,
                                        _lib.stream())

  big_t, big_c = (1 << 24) + 1, _lib.CONSTANTS['CG_CCG_MAX_C'] + 1
  for rc in (ccg(spikes=None), ccg(o=None), ccg(B=0), ccg(T=0), ccg(C=0),
             ccg(T=big_t), ccg(C=big_c), ccg(max_lag=-1),
             ccg(max_lag=_lib.CONSTANTS['CG_CCG_MAX_LAG'] + 1),
             pop(spikes=None), pop(o=None), pop(B=0), pop(T=0), pop(C=0),
             pop(T=big_t), pop(C=big_c)):
    assert rc == _lib.CG_EINVAL
  torch.cuda.synchronize()
  assert bool((out == SENTINEL).all()) and bool((hist == SENTINEL).all())
  with pytest.raises(ValueError):
    spike_metrics.cross_correlogram_device(x, 257)
  with pytest.raises(ValueError):
    spike_metrics.cross_correlogram_device(x, -1)
  # the admitted calls on the same buffers do write
  assert ccg() == 0 and pop() == 0
  torch.cuda.synchronize()
  assert not bool((out == SENTINEL).any()) and not bool((hist == SENTINEL).any())


def test_wrappers_refuse_host_arrays_wrong_dtype_and_rank():
  for fn in (lambda a: spike_metrics.cross_correlogram_device(a, 4),
             spike_metrics.population_count_histogram_device,
             lambda a: spike_metrics.temporal_totals_device(a, 4)):
    with pytest.raises(ValueError):
      fn(np.zeros((2, 24, 3), np.float32))
    with pytest.raises(ValueError):
      fn(torch.zeros(2, 24, 3, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
      fn(torch.zeros(24, 3, dtype=torch.float32, device=DEV))


@pytest.mark.parametrize('density', DENSITIES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_population_hist_equals_the_statement(shape, density):
  B, T, C, _ = shape
  sp = _trials(B, T, C, density)
  got = _hist(_dev(sp))
  _check(got, spike_metrics.population_count_histogram(sp))
  assert np.array_equal(got.sum(1), np.full(B, T))


def test_population_hist_one_neuron_and_all_ones():
  sp = _trials(3, 77, 1, 0.5)
  got = _hist(_dev(sp))
  _check(got, spike_metrics.population_count_histogram(sp))
  assert np.array_equal(got[:, 1], sp.sum((1, 2)))
  T, C = 100, 33
  got = _hist(torch.ones(2, T, C, dtype=torch.float32, device=DEV))
  want = np.zeros((2, C + 1), np.int64)
  want[:, C] = T
  _check(got, want)
  got = _ccg(torch.ones(1, T, C, dtype=torch.float32, device=DEV), 9)
  for tau in range(10):
    assert np.all(got[0, tau] == T - tau)


def test_totals_in_three_groups_equal_the_one_group_result():
  B, T, C, max_lag = 5, 50, 17, 8
  sp = _trials(B, T, C, 0.5)
  x = _dev(sp)
  per_trial = (max_lag + 1) * C * C * 4
  one = spike_metrics.temporal_totals_device(x, max_lag)
  three = spike_metrics.temporal_totals_device(x, max_lag,
                                               group_bytes=2 * per_trial)
  torch.cuda.synchronize()
  want = spike_metrics.temporal_totals(sp, max_lag)
  for got in (one, three):
    assert got[0].dtype == got[1].dtype == torch.int64 and got[0].is_cuda
    assert got[2] == want[2] == B
    _check(got[0].cpu().numpy(), want[0])
    _check(got[1].cpu().numpy(), want[1])
  # a budget below one trial still takes a trial at a time
  tiny = spike_metrics.temporal_totals_device(x, max_lag, group_bytes=1)
  _check(tiny[0].cpu().numpy(), want[0])


def test_compute_metrics_temporal_flag_on_both_devices(tmp_path):
  """`temporal` is the same dict on both devices; every other key compares as
  test_compute_metrics_with_the_flag_on_both_devices compares it."""
  d = dg.make_dataset(num_neurons=6, sequence_length=480, num_segments=24)
  fakes, hps, reports = {}, {}, {}
  for device in ('cpu', 'gpu'):
    os.makedirs(tmp_path / device)
    fakes[device] = _run_dir(tmp_path / device, d)
    hps[device] = cm.build_parser().parse_args(
        ['--output_dir', str(tmp_path / device), '--num_processors', '1',
         '--verbose', '0', '--device', device, '--batch_trials', '10',
         '--temporal_metrics'])
    reports[device] = cm.main(hps[device])[0]
  cpu, gpu = reports['cpu'], reports['gpu']
  assert set(cpu) == set(gpu)
  assert set(gpu) == {'firing_rate_kl', 'correlation_kl', 'van_rossum_kl',
                      'van_rossum_heatmap_min', 'temporal', 'elapse'}
  print('temporal cpu:', cpu['temporal'])
  print('temporal gpu:', gpu['temporal'])
  assert cpu['temporal'] == gpu['temporal']
  for name in FIGURES:
    assert np.isfinite(gpu['temporal'][name]), name
  assert gpu['temporal']['max_lag'] == 24
  assert gpu['temporal']['num_trials'] == [24, 24]
  assert cpu['firing_rate_kl'] == gpu['firing_rate_kl']
  sc, sg = (h5_helper.get(fakes[k], 'spikes') for k in ('cpu', 'gpu'))
  assert sc.tobytes() == sg.tobytes() and sc.shape == sg.shape
  # correlation and van Rossum samples: the bounds of the existing test
  pairs = cm.device_pairs(hps['gpu'], fakes['gpu'])
  hc = hps['cpu']
  T = 480
  for i in range(hc.num_samples):
    for h, g in zip(cm.correlation_coefficient(hc, fakes['cpu'], i),
                    pairs['correlation'][i]):
      assert h.shape == g.shape and np.abs(h - g).max() <= 4 * (T // 12) * U
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
  assert not hasattr(plain, 'temporal_metrics')
  assert 'temporal' not in cm.main(plain)[0]
  # identical spike sets: exactly zero on the device path
  h5_helper.overwrite(fakes['gpu'], 'spikes', d['spikes'].astype(np.int8))
  z = cm.main(hps['gpu'])[0]['temporal']
  for name in ('autocorrelogram_mae', 'lag_covariance_mae',
               'cross_correlogram_mae', 'population_count_js_bits'):
    assert z[name] == 0, name
  assert z['lag_covariance_correlation'] == 1
