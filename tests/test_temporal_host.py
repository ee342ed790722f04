"""Host tests of the structure-across-time statistics: the numpy statements
spike_metrics.cross_correlogram / population_count_histogram against a
brute-force triple loop and closed forms, spike_metrics.temporal_scores on
hand-worked totals, and compute_metrics.py --temporal_metrics on the host path.
No GPU: the device kernels are held to these statements in
tests/test_hip_spike_ccg.py."""
import json
import math
import os
import pickle

import numpy as np
import pytest

import compute_metrics as cm
from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import h5_helper, spike_metrics

PLAIN_KEYS = {'firing_rate_kl', 'correlation_kl', 'van_rossum_kl',
              'van_rossum_heatmap_min', 'elapse'}
FIGURES = ('autocorrelogram_mae', 'lag_covariance_mae',
           'lag_covariance_correlation', 'cross_correlogram_mae',
           'population_count_js_bits')


def _brute_force(spikes, max_lag):
  B, T, C = spikes.shape
  ccg = np.zeros((B, max_lag + 1, C, C), np.int64)
  hist = np.zeros((B, C + 1), np.int64)
  for b in range(B):
    for t in range(T):
      on = [c for c in range(C) if spikes[b, t, c] != 0]
      hist[b, len(on)] += 1
      for tau in range(max_lag + 1):
        if t + tau >= T:
          break
        for i in on:
          for j in range(C):
            if spikes[b, t + tau, j] != 0:
              ccg[b, tau, i, j] += 1
  return ccg, hist


def test_statements_equal_a_brute_force_loop():
  spikes = (np.random.RandomState(5).uniform(size=(3, 50, 7)) < 0.3
            ).astype(np.float32)
  ccg = spike_metrics.cross_correlogram(spikes, 8)
  hist = spike_metrics.population_count_histogram(spikes)
  assert ccg.dtype == np.int64 and ccg.shape == (3, 9, 7, 7)
  assert hist.dtype == np.int64 and hist.shape == (3, 8)
  want_ccg, want_hist = _brute_force(spikes, 8)
  assert np.array_equal(ccg, want_ccg)
  assert np.array_equal(hist, want_hist)
  assert np.array_equal(hist.sum(1), [50, 50, 50])
  # plane 0 is symmetric, its diagonal the spike counts
  assert np.array_equal(ccg[:, 0], ccg[:, 0].transpose(0, 2, 1))
  assert np.array_equal(np.einsum('bii->bi', ccg[:, 0]), spikes.sum(1))


def test_an_all_ones_trial():
  T, C, L = 20, 4, 6
  ccg = spike_metrics.cross_correlogram(np.ones((1, T, C), np.float32), L)
  for tau in range(L + 1):
    assert np.all(ccg[0, tau] == T - tau)
  hist = spike_metrics.population_count_histogram(np.ones((1, T, C)))
  assert np.array_equal(hist[0], [0, 0, 0, 0, T])


def test_a_pair_three_frames_apart_counts_in_one_direction():
  T, C, t0, i, j = 30, 5, 11, 1, 3
  spikes = np.zeros((1, T, C), np.float32)
  spikes[0, t0, i] = 1
  spikes[0, t0 + 3, j] = 1
  ccg = spike_metrics.cross_correlogram(spikes, 5)
  assert ccg[0, 3, i, j] == 1 and ccg[0, 3, j, i] == 0
  assert ccg[0, 0, i, i] == 1 and ccg[0, 0, j, j] == 1
  assert ccg.sum() == 3


def test_lags_from_T_on_are_zero_planes():
  spikes = np.ones((2, 5, 3), np.float32)
  ccg = spike_metrics.cross_correlogram(spikes, 8)
  assert ccg.shape == (2, 9, 3, 3)
  assert np.all(ccg[:, 4] == 1) and not ccg[:, 5:].any()


def test_nan_is_a_spike_and_minus_zero_is_not():
  spikes = np.zeros((1, 4, 2), np.float32)
  spikes[0, 1, 0] = np.nan
  spikes[0, 2, 1] = -0.0
  ccg = spike_metrics.cross_correlogram(spikes, 1)
  assert ccg[0, 0, 0, 0] == 1 and ccg.sum() == 1
  assert np.array_equal(spike_metrics.population_count_histogram(spikes)[0],
                        [3, 1, 0])


def test_totals_sum_the_trials():
  spikes = (np.random.RandomState(6).uniform(size=(37, 20, 4)) < 0.4
            ).astype(np.float32)
  ccg, hist, n = spike_metrics.temporal_totals(spikes, 3)
  assert n == 37 and ccg.dtype == hist.dtype == np.int64
  assert np.array_equal(ccg, spike_metrics.cross_correlogram(spikes, 3).sum(0))
  assert np.array_equal(
      hist, spike_metrics.population_count_histogram(spikes).sum(0))


def test_identical_totals_score_zero_and_correlation_one():
  spikes = (np.random.RandomState(7).uniform(size=(5, 40, 6)) < 0.3
            ).astype(np.float32)
  totals = spike_metrics.temporal_totals(spikes, 8)
  s = spike_metrics.temporal_scores(totals, totals, 40)
  for name in ('autocorrelogram_mae', 'lag_covariance_mae',
               'cross_correlogram_mae', 'population_count_js_bits'):
    assert s[name] == 0, name
  assert s['lag_covariance_correlation'] == 1
  assert s['max_lag'] == 8 and s['num_trials'] == [5, 5]
  assert s['population_count_mean'][0] == s['population_count_mean'][1]
  assert s['population_count_mean'][0] == pytest.approx(spikes.sum() / (5 * 40))


def test_a_hand_worked_two_neuron_case():
  """One trial of T = 4 a side, max_lag 1.
  ref:   neuron 0 fires at t = 0, 1, 2; neuron 1 at t = 1, 3
         ccg[0] = [[3, 1], [1, 2]], ccg[1] = [[2, 2], [1, 0]]
         frames with 0, 1, 2 spikes: 0, 3, 1
  other: neuron 0 fires at t = 0, 2; neuron 1 at t = 0, 1, 2, 3
         ccg[0] = [[2, 2], [2, 4]], ccg[1] = [[0, 2], [1, 3]]
         frames with 0, 1, 2 spikes: 0, 2, 2"""
  a = np.array([[1, 0], [1, 1], [1, 0], [0, 1]], np.float32)[None]
  b = np.array([[1, 1], [0, 1], [1, 1], [0, 1]], np.float32)[None]
  ref, other = (spike_metrics.temporal_totals(x, 1) for x in (a, b))
  assert ref[0].tolist() == [[[3, 1], [1, 2]], [[2, 2], [1, 0]]]
  assert other[0].tolist() == [[[2, 2], [2, 4]], [[0, 2], [1, 3]]]
  assert ref[1].tolist() == [0, 3, 1] and other[1].tolist() == [0, 2, 2]
  s = spike_metrics.temporal_scores(ref, other, 4)
  # A(1): ref [2/3, 0/2], other [0/2, 3/4]
  assert s['autocorrelogram_mae'] == pytest.approx((2 / 3 + 3 / 4) / 2)
  # cov(i, j) = ccg[1][i][j] / 3 - p_i p_j; p ref [3/4, 1/2], other [1/2, 1]
  cov_ref = [2 / 3 - 3 / 8, 1 / 3 - 3 / 8]
  cov_other = [2 / 3 - 1 / 2, 1 / 3 - 1 / 2]
  assert s['lag_covariance_mae'] == pytest.approx(
      (abs(cov_ref[0] - cov_other[0]) + abs(cov_ref[1] - cov_other[1])) / 2)
  # two pairs, both sides falling from (0, 1) to (1, 0)
  assert s['lag_covariance_correlation'] == pytest.approx(1.0)
  # tau = 0: 1/4 against 2/4, twice; tau = 1: 2/3 against 2/3, 1/3 against 1/3
  assert s['cross_correlogram_mae'] == pytest.approx((1 / 4 + 1 / 4) / 4)
  p, q = np.array([0, .75, .25]), np.array([0, .5, .5])
  m = (p + q) / 2
  js = 0.5 * sum(x * math.log2(x / y) for x, y in zip(p[1:], m[1:])) + \
      0.5 * sum(x * math.log2(x / y) for x, y in zip(q[1:], m[1:]))
  assert s['population_count_js_bits'] == pytest.approx(js)
  assert s['population_count_mean'] == pytest.approx([1.25, 1.5])
  assert s['max_lag'] == 1 and s['num_trials'] == [1, 1]


def test_the_stated_nan_cases():
  T = 6
  # no neuron fires on both sides: no autocorrelogram value
  a = np.zeros((1, T, 2), np.float32)
  b = np.zeros((1, T, 2), np.float32)
  a[0, 1, 0] = 1
  b[0, 2, 1] = 1
  s = spike_metrics.temporal_scores(spike_metrics.temporal_totals(a, 2),
                                    spike_metrics.temporal_totals(b, 2), T)
  assert math.isnan(s['autocorrelogram_mae'])
  assert np.isfinite(s['lag_covariance_mae'])
  assert math.isnan(s['lag_covariance_correlation'])   # both sides constant 0
  # one neuron: no pair i != j
  one = np.ones((2, T, 1), np.float32)
  s = spike_metrics.temporal_scores(spike_metrics.temporal_totals(one, 2),
                                    spike_metrics.temporal_totals(one, 2), T)
  assert s['autocorrelogram_mae'] == 0
  for name in ('lag_covariance_mae', 'lag_covariance_correlation',
               'cross_correlogram_mae'):
    assert math.isnan(s[name]), name
  assert s['population_count_js_bits'] == 0
  # max_lag 0: no lag-1 plane and no autocorrelogram lag
  two = (np.random.RandomState(8).uniform(size=(2, T, 3)) < 0.5
         ).astype(np.float32)
  s = spike_metrics.temporal_scores(spike_metrics.temporal_totals(two, 0),
                                    spike_metrics.temporal_totals(two, 0), T)
  for name in ('autocorrelogram_mae', 'lag_covariance_mae',
               'lag_covariance_correlation'):
    assert math.isnan(s[name]), name
  assert s['cross_correlogram_mae'] == 0


def test_lags_from_T_on_are_left_out_of_the_cross_correlogram_figure():
  a = (np.random.RandomState(9).uniform(size=(3, 4, 3)) < 0.5).astype(np.float32)
  b = (np.random.RandomState(10).uniform(size=(3, 4, 3)) < 0.5).astype(np.float32)
  short = spike_metrics.temporal_scores(spike_metrics.temporal_totals(a, 3),
                                        spike_metrics.temporal_totals(b, 3), 4)
  long_ = spike_metrics.temporal_scores(spike_metrics.temporal_totals(a, 9),
                                        spike_metrics.temporal_totals(b, 9), 4)
  assert short['cross_correlogram_mae'] == long_['cross_correlogram_mae']
  assert np.isfinite(long_['cross_correlogram_mae'])


def test_scores_refuse_mismatched_totals():
  a = spike_metrics.temporal_totals(np.ones((1, 4, 2), np.float32), 2)
  b = spike_metrics.temporal_totals(np.ones((1, 4, 3), np.float32), 2)
  with pytest.raises(ValueError):
    spike_metrics.temporal_scores(a, b, 4)
  with pytest.raises(ValueError):
    spike_metrics.cross_correlogram(np.ones((4, 2), np.float32), 2)
  with pytest.raises(ValueError):
    spike_metrics.cross_correlogram(np.ones((1, 4, 2), np.float32), -1)


def _run_dir(path, d):
  """A DG run directory: the validation cache with its spikes, one generated
  file with the signals alone (compute_metrics deconvolves them)."""
  gen_dir = path / 'generated'
  os.makedirs(gen_dir)
  val = str(gen_dir / 'validation.h5')
  sig = d['signals'] * (d['info']['signals_max'] - d['info']['signals_min']
                        ) + d['info']['signals_min']
  h5_helper.write(val, {'signals': sig.astype(np.float32),
                        'spikes': d['spikes'].astype(np.int8)})
  fake = str(gen_dir / 'epoch000_signals.h5')
  h5_helper.write(fake, {'signals': sig.astype(np.float32)})
  with open(gen_dir / 'info.pkl', 'wb') as f:
    pickle.dump({0: {'global_step': 1, 'filename': fake}}, f)
  json.dump(dict(generated_dir=str(gen_dir), validation_cache=val,
                 num_neurons=6, sequence_length=480),
            open(path / 'hparams.json', 'w'))
  return fake


def test_compute_metrics_temporal_flag_on_the_host(tmp_path):
  d = dg.make_dataset(num_neurons=6, sequence_length=480, num_segments=24)
  fake = _run_dir(tmp_path, d)
  args = ['--output_dir', str(tmp_path), '--num_processors', '1', '--verbose',
          '0', '--device', 'cpu']
  plain = cm.build_parser().parse_args(args)
  assert not hasattr(plain, 'temporal_metrics') and not hasattr(plain, 'max_lag')
  assert set(cm.main(plain)[0]) == PLAIN_KEYS
  hp = cm.build_parser().parse_args(args + ['--temporal_metrics'])
  assert hp.temporal_metrics is True and not hasattr(hp, 'max_lag')
  report = cm.main(hp)[0]
  assert set(report) == PLAIN_KEYS | {'temporal'}
  t = report['temporal']
  # every neuron fires on both sides, so no figure is NaN
  for f in (hp.validation_cache, fake):
    spikes = np.asarray(h5_helper.get(f, name='spikes'))
    assert spikes.shape == (24, 480, 6)
    assert (spikes.reshape(-1, 6).sum(0) > 0).all()
  for name in FIGURES:
    print(name, t[name])
    assert np.isfinite(t[name]), name
  assert t['max_lag'] == 24 and t['num_trials'] == [24, 24]
  assert all(np.isfinite(v) for v in t['population_count_mean'])
  # the figures are those of the statements on the two files
  totals = [spike_metrics.temporal_totals(
      np.asarray(h5_helper.get(f, name='spikes')), 24)
            for f in (hp.validation_cache, fake)]
  assert t == spike_metrics.temporal_scores(totals[0], totals[1], 480)
  # the report on disk holds it, and --max_lag is read
  on_disk = json.load(open(tmp_path / 'spike_metrics.json'))
  assert on_disk['0']['temporal'] == t
  hp8 = cm.build_parser().parse_args(
      args + ['--temporal_metrics', '--max_lag', '8'])
  assert cm.main(hp8)[0]['temporal']['max_lag'] == 8
