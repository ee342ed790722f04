"""Host tests of the pattern probabilities of the surrogate experiment: the numpy
statements spike_metrics.pattern_codes / pattern_histogram, pattern_scores, and
compute_surrogate_metrics.py --device cpu.  No GPU."""
import json
import os

import numpy as np
import pytest

import compute_surrogate_metrics as csm
from calciumgan_amd.gan.utils import spike_helper, spike_metrics
from pattern_cases import samples, surrogate_dirs


def test_codes_of_hand_written_samples():
  T, C = 6, 2
  x = np.zeros((T * C + 2, T, C), np.float32)
  for t in range(T):
    for c in range(C):
      x[t * C + c, t, c] = 1.0   # sample k: a single spike at (t, c)
  x[T * C + 1] = 1.0             # the last: all ones; the one before: silent
  want = [1 << k for k in range(T * C)] + [0, (1 << (T * C)) - 1]
  codes = spike_metrics.pattern_codes(x)
  assert codes.dtype == np.int64 and codes.tolist() == want
  # any dtype
  for dtype in (np.float64, np.int8, np.bool_, np.int64):
    assert spike_metrics.pattern_codes(x.astype(dtype)).tolist() == want
  # two spikes: (t, c) = (1, 0) and (2, 1) at C = 3
  y = np.zeros((1, 4, 3))
  y[0, 1, 0] = y[0, 2, 1] = 5.0
  assert spike_metrics.pattern_codes(y).tolist() == [(1 << 3) | (1 << 7)]


def test_histogram_sums_to_the_number_of_samples():
  x = samples(777, 3, 3, seed=1)
  h = spike_metrics.pattern_histogram(x)
  assert h.dtype == np.int64 and h.shape == (512,) and h.sum() == 777
  codes = spike_metrics.pattern_codes(x)
  for code in (0, int(codes[5]), 511):
    assert h[code] == (codes == code).sum()


def test_a_transposed_view_counts_like_its_contiguous_copy():
  x = samples(500, 2, 6, seed=2)          # (n, neurons, L)
  view = x.transpose(0, 2, 1)             # (n, L, neurons), not contiguous
  assert not view.flags['C_CONTIGUOUS']
  h = spike_metrics.pattern_histogram(view)
  np.testing.assert_array_equal(
      h, spike_metrics.pattern_histogram(np.ascontiguousarray(view)))
  assert (h != spike_metrics.pattern_histogram(x)).any()


def test_negative_values_negative_zero_and_nan():
  x = np.zeros((4, 2, 2), np.float32)
  x[0, 0, 1] = -3.0           # a spike
  x[1, 1, 0] = -0.0           # none
  x[2, 1, 1] = np.nan         # a spike
  x[3] = [[np.nan, -0.0], [1e-30, -1.0]]
  assert spike_metrics.pattern_codes(x).tolist() == [2, 0, 8, 1 | 4 | 8]


def test_too_many_bits_are_refused():
  spike_metrics.pattern_histogram(np.zeros((2, 24, 1), np.float32))
  with pytest.raises(ValueError):
    spike_metrics.pattern_histogram(np.zeros((2, 5, 5), np.float32))
  with pytest.raises(ValueError):
    spike_metrics.pattern_histogram(np.zeros((2, 6), np.float32))


def test_scores_of_identical_counts():
  h = spike_metrics.pattern_histogram(samples(4000, 3, 2, seed=3))
  s = spike_metrics.pattern_scores(h, h)
  assert s['js_divergence_bits'] == 0.0   # p / m == 1 exactly in every term
  assert s['unseen_mass'] == 0.0
  # Pearson r of a vector with itself, in float64: a few roundings from 1
  assert abs(s['log_prob_correlation'] - 1.0) <= 1e-12
  assert s['patterns_seen'] == [int((h > 0).sum())] * 2
  assert s['firing_probability_mae'] == 0.0 and s['pair_covariance_mae'] == 0.0
  # a multiple of the counts is the same distribution (power of two: exactly)
  assert spike_metrics.pattern_scores(h, 4 * h)['js_divergence_bits'] == 0.0


def test_scores_of_disjoint_supports():
  ref = np.array([1, 1, 0, 0], np.int64)
  cnt = np.array([0, 0, 2, 2], np.int64)
  s = spike_metrics.pattern_scores(ref, cnt)
  assert s['js_divergence_bits'] == 1.0   # every p / m and q / m is exactly 2
  assert s['unseen_mass'] == 1.0
  assert np.isnan(s['log_prob_correlation'])
  assert s['patterns_seen'] == [2, 2]
  # one shared code is still fewer than two points
  s = spike_metrics.pattern_scores(np.array([3, 1, 0, 0]), np.array([0, 1, 1, 2]))
  assert np.isnan(s['log_prob_correlation']) and s['unseen_mass'] == 0.75


def test_marginals_and_pair_covariances_from_the_counts():
  T, C = 2, 2
  a, b = samples(50, T, C, seed=4, rate=0.4), samples(60, T, C, seed=5, rate=0.6)
  s = spike_metrics.pattern_scores(spike_metrics.pattern_histogram(a),
                                   spike_metrics.pattern_histogram(b))
  # directly from the samples: bit k = t C + c is column k of the flat sample
  fa, fb = (x.reshape(len(x), T * C).astype(np.float64) for x in (a, b))
  iu = np.triu_indices(T * C, k=1)
  cov_a, cov_b = (np.cov(f.T, bias=True)[iu] for f in (fa, fb))
  # float64 sums of <= 60 terms of size <= 1: 1e-12 is far above their rounding
  assert abs(s['firing_probability_mae'] -
             np.mean(np.abs(fa.mean(0) - fb.mean(0)))) < 1e-12
  assert abs(s['pair_covariance_mae'] - np.mean(np.abs(cov_a - cov_b))) < 1e-12
  assert s['pair_covariance_mae'] > 0
  # above 16 bits the two figures are not formed
  big = np.zeros(1 << 17, np.int64)
  big[[0, 5, 99999]] = [5, 2, 1]
  s = spike_metrics.pattern_scores(big, big[::-1].copy())
  assert s['firing_probability_mae'] is None and s['pair_covariance_mae'] is None
  assert s['patterns_seen'] == [3, 3]
  for bad in ((big[:3], big[:3]), (big, big[:4]), (big * 0, big), (-big, big)):
    with pytest.raises(ValueError):
      spike_metrics.pattern_scores(*bad)


SCORE_KEYS = {'js_divergence_bits', 'log_prob_correlation', 'unseen_mass',
              'patterns_seen', 'firing_probability_mae', 'pair_covariance_mae'}


def test_cli_on_the_host(tmp_path, capsys):
  n, L, C = 3000, 6, 2
  input_dir, output_dir, signals = surrogate_dirs(str(tmp_path), n, L, C)
  args = ['--input_dir', input_dir, '--output_dir', output_dir, '--verbose', '0']
  report = csm.main(csm.build_parser().parse_args(args))
  with open(os.path.join(output_dir, 'surrogate_metrics.json')) as file:
    stored = json.load(file)
  assert stored == json.loads(json.dumps(report))
  assert set(stored) == {'bits', 'sequence_length', 'num_neurons', 'num_samples',
                         'generated', 'surrogate'}
  assert stored['bits'] == 12
  assert stored['num_samples'] == {'generated': n, 'ground_truth': n,
                                   'surrogate': n}
  for name in ('generated', 'surrogate'):
    assert set(stored[name]) == SCORE_KEYS
    assert 0.0 <= stored[name]['js_divergence_bits'] <= 1.0
    assert np.isfinite(stored[name]['log_prob_correlation'])
  counts = np.load(os.path.join(output_dir, 'pattern_counts.npz'))
  assert sorted(counts.files) == ['generated', 'ground_truth', 'surrogate']
  for name in counts.files:
    assert counts[name].dtype == np.int64 and counts[name].shape == (4096,)
    assert counts[name].sum() == n
  # the generated counts are those of the host deconvolution of the signals
  trains = spike_helper.deconvolve_signals(
      np.ascontiguousarray(signals.transpose(0, 2, 1)).reshape(n * C, L))
  want = spike_metrics.pattern_histogram(
      trains.reshape(n, C, L).transpose(0, 2, 1))
  np.testing.assert_array_equal(counts['generated'], want)
  assert (want > 0).sum() > 100   # (the traces do deconvolve into many patterns)
  assert stored['generated'] == json.loads(json.dumps(
      spike_metrics.pattern_scores(counts['ground_truth'], want)))
  assert not os.path.exists(os.path.join(output_dir, 'pattern_probabilities.pdf'))
  # --plot: the figure, or one line without matplotlib
  capsys.readouterr()
  csm.main(csm.build_parser().parse_args(args + ['--plot', '--format', 'png']))
  figure = os.path.join(output_dir, 'pattern_probabilities.png')
  try:
    import matplotlib  # noqa: F401
    assert os.path.getsize(figure) > 0
  except ImportError:
    assert not os.path.exists(figure)
    assert capsys.readouterr().out.count('\n') == 1


def test_cli_refuses_more_than_16_bits_and_mismatched_shapes(tmp_path):
  input_dir, output_dir, _ = surrogate_dirs(str(tmp_path / 'a'), 10, 9, 2)
  args = csm.build_parser().parse_args(
      ['--input_dir', input_dir, '--output_dir', output_dir])
  with pytest.raises(SystemExit, match='18 bits'):
    csm.main(args)
  assert not os.path.exists(os.path.join(output_dir, 'surrogate_metrics.json'))
  other, _, _ = surrogate_dirs(str(tmp_path / 'b'), 10, 5, 2)
  args = csm.build_parser().parse_args(
      ['--input_dir', other, '--output_dir', output_dir])
  with pytest.raises(SystemExit, match='signals'):
    csm.main(args)
