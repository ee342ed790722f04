"""CPU tests of the spike-statistics chain: OASIS AR(1)
deconvolution (C) against its python restatement and known answers, firing
rate / binned covariance definitions, and the DG metrics report.  Upstream
OASIS / Elephant are un-pinned and absent: PARITY UNPINNED."""
import os
import pickle
from types import SimpleNamespace

import numpy as np

import compute_dg_metrics as cdm
from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import h5_helper, spike_helper, spike_metrics

import spike_stats_cases as SC


def test_oasis_c_matches_python_restatement():
  rng = np.random.RandomState(0)
  for seed in range(4):
    s = (rng.rand(400) < 0.05).astype(np.float64)
    c = np.zeros(400)
    for t in range(400):
      c[t] = s[t] + (0.95 * c[t - 1] if t > 0 else 0.0)
    y = c + 0.3 * rng.randn(400)
    for s_min in (0.0, 0.55):
      c1, s1 = spike_helper.oasis_ar1(y, 0.95, s_min=s_min)
      c2, s2 = spike_helper.oasis_ar1_python(y, 0.95, s_min=s_min)
      np.testing.assert_allclose(c1, c2, rtol=1e-12, atol=1e-12)
      np.testing.assert_allclose(s1, s2, rtol=1e-12, atol=1e-12)


def test_oasis_recovers_noise_free_spikes():
  T, g = 300, 0.95
  s = np.zeros(T)
  s[[20, 21, 90, 200, 260]] = 1.0
  c = np.zeros(T)
  for t in range(T):
    c[t] = s[t] + (g * c[t - 1] if t > 0 else 0.0)
  c_hat, s_hat = spike_helper.oasis_ar1(c, g, s_min=0.55)
  np.testing.assert_allclose(c_hat, c, atol=1e-9)
  np.testing.assert_allclose(s_hat, s, atol=1e-9)
  np.testing.assert_array_equal(spike_helper.oasis_function(c), s)
  # sub-threshold events are suppressed by s_min
  small = c + 0.0
  small[150:] += 0.3 * g**np.arange(150)
  _, s2 = spike_helper.oasis_ar1(small, g, s_min=0.55)
  assert s2[150] < 0.5


def test_deconvolve_signals_on_dg_calcium():
  """Noisy DG calcium (sn = .3): the recovered trains carry the firing rates."""
  rng = np.random.RandomState(1)
  gamma = np.array([-1.0, -1.5, -2.0])
  spikes = dg.sample_spikes(gamma, 0.0, 6000, rng)
  sig = dg.spikes_to_signals(spikes, rng)
  rec = spike_helper.deconvolve_signals(sig)
  assert rec.shape == spikes.shape and rec.dtype == np.float32
  fr_true = spike_metrics.mean_firing_rate(spikes)
  fr_rec = spike_metrics.mean_firing_rate(rec)
  np.testing.assert_allclose(fr_rec, fr_true, rtol=0.25)


def test_firing_rate_and_covariance_definitions():
  sp = np.zeros((2, 48), np.float32)
  sp[0, [0, 5, 13, 30]] = 1
  sp[1, [1, 14, 15, 40, 41, 42]] = 1
  np.testing.assert_allclose(spike_metrics.mean_firing_rate(sp), [2.0, 3.0])
  counts = spike_metrics.bin_counts(sp)  # 12 frames per 500 ms bin
  np.testing.assert_array_equal(counts, [[2, 1, 1, 0], [1, 2, 0, 3]])
  np.testing.assert_allclose(spike_metrics.covariance(sp), np.cov(counts))
  cross = spike_metrics.covariance(sp[:1], sp[1:])
  assert cross.shape == (1, 1)
  np.testing.assert_allclose(cross[0, 0], np.cov(counts)[1, 0])


def _tie_exact_covariance(sp):
  """exact_covariance against batch_statistics by the rule of the GPU test
  test_statistics_against_spike_metrics: entries whose exact value is 0 -- below
  half of the smallest non-zero magnitude 1 / (nb (nb - 1)) on the host -- are
  exactly 0 in the statement, wherever the host has 0 the statement has 0, all
  others agree to rtol = 1e-6."""
  nb = sp.shape[1] // 12
  _, want = spike_metrics.batch_statistics(SC.binary(sp))
  got = SC.exact_covariance(sp)
  assert got.dtype == np.float32 and got.shape == want.shape
  zero = np.abs(want) < 0.5 / (nb * (nb - 1))
  assert np.abs(want[zero]).max() < 1e-12
  assert np.all(got[want == 0] == 0) and np.all(got[zero] == 0)
  np.testing.assert_allclose(got[~zero], want[~zero], rtol=1e-6, atol=0)
  assert (~zero).sum() > 0
  return got


def test_exact_covariance_statement_against_batch_statistics():
  for T, C in SC.GRID:
    _tie_exact_covariance(SC.trains(3, T, C, seed=T + C))
  for name in SC.SHAPES:
    _tie_exact_covariance(SC.stats_case(name))


def test_exact_covariance_by_hand_and_the_planted_trains():
  sp = np.zeros((1, 48, 2), np.float32)
  sp[0, [0, 5, 13, 30], 0] = 1
  sp[0, [1, 14, 15, 40, 41, 42], 1] = 1
  # counts [2, 1, 1, 0] and [1, 2, 0, 3]: S = 4, 6; S_00 = 6, S_01 = 4, S_11 = 14
  want = np.array([[4 * 6 - 16, 4 * 4 - 24, 4 * 14 - 36]], np.float64) / 12.0
  assert np.array_equal(SC.exact_covariance(sp), want.astype(np.float32))
  sp = SC.stats_case('planted_c6_t48')
  assert np.isnan(sp).sum() == 2 and (sp == np.float32(2.0**-149)).sum() == 2
  cov = SC.exact_covariance(sp)
  iu = np.triu_indices(6)
  # a train that fires in every frame, and one that never does, vary with none
  assert np.all(cov[:, (iu[0] == 0) | (iu[0] == 2) | (iu[1] == 2)] == 0)
  assert np.all(cov[:, (iu[0] == 1) & (iu[1] == 1)] > 0)
  rates, _ = spike_metrics.batch_statistics(SC.binary(sp))
  assert np.array_equal(rates[:, :3], [[24.0, 2.0, 0.0], [24.0, 1.5, 0.0]])


def test_statistics_cases_reach_what_they_are_for():
  lds = {n: SC.lds_bytes(*SC.SHAPES[n]) for n in SC.SHAPES}
  assert lds['c300_t2405'] == 61200 and lds['c240_t3029'] == 61440 == SC.STATS_MAX_LDS
  assert [SC.lds_bytes(T, C) for T, C in SC.REFUSED] == [61680, 61500]
  assert all(SC.lds_bytes(T - 12, C) <= SC.STATS_MAX_LDS for T, C in SC.REFUSED)
  assert [SC.split(C) for C in (44, 45, 119, 120, 240, 300)] == [1, 2, 7, 8, 8, 8]
  assert 300 * 301 // 2 == 45150 > 8 * 4 * SC.STATS_THREADS
  assert 2405 % 12 == 5 and 3029 // 12 == 252
  # the error kernel's grid
  assert SC.err_parts(3, 2097152) == 1024 == -(-2097152 // 2048)
  assert SC.err_parts(3, 2097152 + 257) == 1024 < -(-(2097152 + 257) // 2048)
  assert SC.err_parts(0, 5) == 1 and SC.err_parts(2049, 2047) == 2
  for n_fr, n_cov in SC.ERROR_SIZES:
    ra, rb, ca, cb = SC.planted_error_inputs(n_fr, n_cov)
    parts = SC.err_parts(n_fr, n_cov)
    for a, b, n in ((ra, rb, n_fr), (ca, cb, n_cov)):
      idx = np.nonzero(a != b)[0]
      assert sorted(idx) == sorted(SC.planted_indices(n, parts))
      if n:
        assert 0 in idx and n - 1 in idx
      if n > parts * 256:
        assert parts * 256 - 1 in idx and parts * 256 in idx and 255 in idx
    sums = spike_metrics.error_sums(ra, rb, ca, cb)
    # every sum is a float32
    assert np.array_equal(sums, sums.astype(np.float32).astype(np.float64))
    assert (sums[0] > 0) == (n_fr > 0) and (sums[2] > 0) == (n_cov > 0)


def test_dg_metrics_report(tmp_path):
  d = dg.make_dataset(num_neurons=6, sequence_length=480, num_segments=8)
  gen_dir = tmp_path / 'generated'
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
  import json
  json.dump(dict(generated_dir=str(gen_dir), validation_cache=val,
                 num_neurons=6), open(tmp_path / 'hparams.json', 'w'))
  hp = SimpleNamespace(output_dir=str(tmp_path), num_trials=5)
  r = cdm.main(hp)
  # "generated" = the validation calcium itself: the only error is the
  # deconvolution's, so rates agree closely
  assert r['firing_rate']['mae'] < 0.5
  assert r['covariance']['mae'] < 0.2
  # identical inputs -> exactly zero error
  fr, cov = cdm.get_data_statistics(hp, val)
  z = cdm.report(fr, fr, cov, cov)
  assert z['firing_rate']['rmse'] == 0 and z['covariance']['mse'] == 0


def test_oasis_hand_worked_example():
  """Algorithm 3 of Friedrich, Zhou & Paninski (2017) stepped through by hand
  (pools (v, w, t, l); merge while v_i/w_i < g^l_{i-1} v_{i-1}/w_{i-1} + s_min):
  y = [1, .2, .6, .1], g = .5.
    s_min = 0:   t1: .5 > .2 -> merge: v 1.1, w 1.25 (value .88).  t2: .88 g^2 =
                 .22 < .6 -> new pool.  t3: .6 g = .3 > .1 -> merge: v .65, w 1.25
                 (value .52); .22 < .52 -> stop.
                 c = [.88, .44, .52, .26], s = [0, 0, .30, 0].
    s_min = .35: as above until the last test: .22 + .35 > .52 -> merge the two
                 pools: v 1.1 + .65/4 = 1.2625, w 1.25 + 1.25/16 = 1.328125;
                 c = 1.2625/1.328125 * [1, .5, .25, .125], no spike."""
  y = np.array([1.0, 0.2, 0.6, 0.1])
  c, s = spike_helper.oasis_ar1(y, 0.5, s_min=0.0)
  np.testing.assert_allclose(c, [0.88, 0.44, 0.52, 0.26], atol=1e-12)
  np.testing.assert_allclose(s, [0.0, 0.0, 0.30, 0.0], atol=1e-12)
  c, s = spike_helper.oasis_ar1(y, 0.5, s_min=0.35)
  c0 = 1.2625 / 1.328125
  np.testing.assert_allclose(c, c0 * 0.5**np.arange(4), atol=1e-12)
  np.testing.assert_allclose(s, 0.0, atol=1e-12)
  c2, s2 = spike_helper.oasis_ar1_python(y, 0.5, s_min=0.35)
  np.testing.assert_allclose(c2, c, atol=1e-12)


def test_oasis_solves_its_defining_problem():
  """OASIS with s_min = 0, lambda = 0 is an exact solver of the convex problem
  the paper states (its Eq. 3): min_c 1/2 |c - y|^2  s.t.  s_t = c_t - g
  c_{t-1} >= 0.  With c = K s (K lower-triangular Toeplitz of g^k) that is a
  non-negative least-squares problem, solved here independently by
  scipy.optimize.nnls -- a known answer that does not come from OASIS code."""
  from scipy.optimize import nnls
  rng = np.random.RandomState(5)
  g = 0.95
  for T in (40, 120):
    sp = (rng.rand(T) < 0.08).astype(np.float64)
    c = np.zeros(T)
    for t in range(T):
      c[t] = sp[t] + (g * c[t - 1] if t else 0.0)
    y = c + 0.3 * rng.randn(T)
    K = np.tril(g**np.subtract.outer(np.arange(T), np.arange(T)).clip(min=0))
    s_ref, _ = nnls(K, y, maxiter=20 * T)
    c_ref = K @ s_ref
    c_hat, s_hat = spike_helper.oasis_ar1(y, g, s_min=0.0)
    np.testing.assert_allclose(c_hat, c_ref, atol=1e-8)
    # (s[0] is defined as 0 by the reference's convention; the rest agree)
    np.testing.assert_allclose(s_hat[1:], s_ref[1:], atol=1e-8)


def test_van_rossum_and_victor_purpura_known_answers():
  """Closed forms of the two spike-train distances (spike_metrics.py:41-63 ->
  Elephant [ext], tau = 1 s, q = 1 Hz), Elephant's normalisation: a lone spike
  against an empty train is at distance 1 (hand-computed: S_aa = 1, S_ee = 0,
  S_ae = 0); two lone spikes dt apart sqrt(2 (1 - exp(-dt))); identical trains 0;
  Victor-Purpura moves a spike for q dt or deletes + inserts it for 2."""
  T = 24 * 20
  a, b, c, e = (np.zeros(T, np.float32) for _ in range(4))
  a[24] = 1            # spike at 1 s
  b[24 + 12] = 1       # spike at 1.5 s
  c[[24, 24 * 10]] = 1 # spikes at 1 s and 10 s
  d = spike_metrics.van_rossum_distance(np.stack([a, b, c, e]))
  assert d.shape == (4, 4) and np.allclose(np.diag(d), 0)
  np.testing.assert_allclose(d[0, 3], 1.0, rtol=1e-12)
  np.testing.assert_allclose(d[0, 1], np.sqrt(2 * (1 - np.exp(-0.5))), rtol=1e-12)
  # a's spike cancels c's first one: what is left is c's lone second spike
  # (S_aa = 1, S_cc = 2 + 2 e^-9, S_ac = 1 + e^-9 -> D^2 = 1)
  np.testing.assert_allclose(d[0, 2], 1.0, rtol=1e-12)
  np.testing.assert_allclose(d, d.T)
  # the cross block is sliced as the reference slices it
  cross = spike_metrics.van_rossum_distance(np.stack([a, b]), np.stack([c, e]))
  np.testing.assert_allclose(cross, d[2:, :2])
  vp = spike_metrics.victor_purpura_distance(np.stack([a, b, c, e]))
  np.testing.assert_allclose(vp[0, 1], 0.5)      # shift by 0.5 s at q = 1
  np.testing.assert_allclose(vp[0, 3], 1.0)      # delete
  np.testing.assert_allclose(vp[0, 2], 1.0)      # insert the second spike
  far = np.zeros(T, np.float32)
  far[24 * 15] = 1
  np.testing.assert_allclose(
      spike_metrics.victor_purpura_distance(np.stack([a, far]))[0, 1], 2.0)


def test_recorded_data_metrics_report(tmp_path):
  """compute_metrics.py (BASELINE configs[3]'s post-hoc chain) on a run
  directory: deconvolution written back into the generated file, KL of firing
  rate / correlation / van Rossum distances between validation and generated
  spikes.  Generated == the validation calcium: the firing-rate histograms
  differ only by what OASIS misses, correlation and van Rossum KLs stay small;
  a shuffled generated set scores worse; identical spike sets score exactly 0."""
  import compute_metrics as cm
  import json
  d = dg.make_dataset(num_neurons=6, sequence_length=480, num_segments=24)
  gen_dir = tmp_path / 'generated'
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
            open(tmp_path / 'hparams.json', 'w'))
  hp = cm.build_parser().parse_args(['--output_dir', str(tmp_path),
                                     '--num_processors', '1', '--verbose', '0'])
  r = cm.main(hp)[0]
  assert h5_helper.contains(fake, 'spikes')
  got = h5_helper.get(fake, 'spikes')
  assert got.shape == d['spikes'].shape and got.dtype == np.int8
  assert set(r) >= {'firing_rate_kl', 'correlation_kl', 'van_rossum_kl'}
  assert np.isfinite([r['firing_rate_kl']['mean'], r['correlation_kl']['mean'],
                      r['van_rossum_kl']['mean']]).all()
  assert os.path.exists(tmp_path / 'spike_metrics.json')
  # identical spike sets: every KL is exactly zero
  h5_helper.overwrite(fake, 'spikes', d['spikes'].astype(np.int8))
  z = cm.main(hp)[0]
  assert z['firing_rate_kl']['mean'] == 0 and z['van_rossum_kl']['mean'] == 0
  assert z['correlation_kl']['mean'] == 0
  # neurons permuted in the generated set: per-neuron firing rates no longer match
  h5_helper.overwrite(fake, 'spikes',
                      d['spikes'][:, :, ::-1].astype(np.int8).copy())
  w = cm.main(hp)[0]
  assert w['firing_rate_kl']['mean'] > z['firing_rate_kl']['mean']
  # KL helper against a direct numpy evaluation
  rng = np.random.RandomState(0)
  a, b = rng.randn(300), rng.randn(200) + 0.5
  pooled = np.concatenate([a, b])
  lo, hi = pooled.min(), pooled.max()
  edges = np.linspace(lo, hi, cm.NUM_BINS + 1)
  edges[0] -= (hi - lo) * 1e-3   # pandas.cut widens the range by 0.1 % below
  idx = np.clip(np.searchsorted(edges, pooled, side='left') - 1, 0, cm.NUM_BINS - 1)
  p = np.bincount(idx[:300], minlength=cm.NUM_BINS) / 300.0
  q = np.bincount(idx[300:], minlength=cm.NUM_BINS) / 200.0
  np.testing.assert_allclose(cm.pairs_kl_divergence([(a, b)])[0],
                             cm.kl_divergence(p.astype(np.float32),
                                              q.astype(np.float32)), rtol=1e-5)
