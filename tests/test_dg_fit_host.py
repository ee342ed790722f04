"""Host tests of the DG fit (calciumgan_amd/data/dg_fit.py, dg.sample_spikes_corr,
dataset/generate_dg_data.py) against scipy and against outputs of the
REFERENCE's dg package (tests/golden/dg_fit_reference.npz, made by
tests/make_golden_dg_fit.py).  No GPU.

Figures measured when the file was written (profiles/dg_fit_parity.txt):
|bivariate_normal_cdf - scipy| <= 1.4e-14 over the grid; gauss_correlation
equals the golden correlations bit for bit; the fit lies within 1.35 standard
errors of the true latent correlations."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy.stats import multivariate_normal

import dg_fit_cases as cases
from calciumgan_amd import _lib
from calciumgan_amd import build as cg_build
from calciumgan_amd.data import dg, dg_fit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'dataset', 'generate_dg_data.py')
TOL = cases.TOL


def _fitted_golden():
  g = cases.golden()
  stats = dg_fit.recording_statistics(g['trains'].astype(np.float32))
  return g, stats, dg_fit.gauss_correlation(*stats)


@pytest.fixture(scope='module')
def fitted():
  return _fitted_golden()


def test_bivariate_cdf_against_scipy_on_the_grid():
  h, k, r = cases.cdf_grid()
  assert len(h) > 2000 and np.abs(r).max() == 0.99999
  assert (np.abs(h - k) <= 0.004).sum() > 100
  got = dg_fit.bivariate_normal_cdf(h, k, r)
  want = np.array([
      multivariate_normal.cdf([a, b], mean=[0., 0.], cov=[[1., c], [c, 1.]])
      for a, b, c in zip(h, k, r)])
  err = np.abs(got - want)
  worst = int(err.argmax())
  print('eps_cdf = {:.3e} at h {} k {} r {}'.format(
      err.max(), h[worst], k[worst], r[worst]))
  assert got.dtype == np.float64 and err.max() <= 1e-11
  assert err.max() <= cases.EPS_CDF  # what the later bars assume
  # deterministic, and broadcasting over shapes
  np.testing.assert_array_equal(dg_fit.bivariate_normal_cdf(h, k, r), got)
  np.testing.assert_array_equal(
      dg_fit.bivariate_normal_cdf(h[:6].reshape(2, 3), k[:6].reshape(2, 3),
                                  r[:6].reshape(2, 3)), got[:6].reshape(2, 3))
  assert dg_fit.bivariate_normal_cdf(0.0, 0.0, 0.0) == 0.25


def test_recording_statistics_equal_the_reference(fitted):
  g, (rates, gamma, cov), _ = fitted
  assert rates.dtype == gamma.dtype == cov.dtype == np.float64
  assert g['covariance'].dtype == np.float32   # the reference's own dtype
  np.testing.assert_array_equal(gamma[None, :], g['gauss_mean'])
  np.testing.assert_array_equal(cov, g['covariance'].astype(np.float64))
  np.testing.assert_array_equal(
      rates, g['trains'].astype(np.float32).mean(1).astype(np.float64))


def test_rates_of_exactly_zero_and_one_are_nudged():
  from scipy.stats import norm
  spikes = np.zeros((3, 50), np.float32)
  spikes[1] = 1.0
  spikes[2, ::2] = 1.0
  rates, gamma, cov = dg_fit.recording_statistics(spikes)
  np.testing.assert_array_equal(rates, [0.0, 1.0, 0.5])
  np.testing.assert_array_equal(
      gamma, norm.ppf(np.array([1e-4, 1 - 1e-4, 0.5], np.float32)))
  assert abs(gamma[0] + 3.719) < 1e-3 and gamma[2] == 0.0
  assert np.all(cov[:2] == 0) and cov[2, 2] == 0.25


def test_gauss_correlation_against_the_reference(fitted):
  g, (rates, gamma, cov), (corr, status, iterations) = fitted
  C = len(rates)
  want = g['gauss_corr']
  i, j = np.tril_indices(C, -1)
  density = cases.bivariate_density(gamma[i], gamma[j], want[i, j])
  bound = 2 * (TOL + cases.EPS_CDF) / density
  diff = np.abs(corr[i, j] - want[i, j])
  print('max |lambda - reference| = {:.3e}, smallest bound {:.3e}'.format(
      diff.max(), bound.min()))
  assert np.all(diff <= bound)
  np.testing.assert_array_equal(corr, corr.T)
  np.testing.assert_array_equal(np.diag(corr), np.ones(C))
  # the reference bisected every pair to convergence: its matrix has no 0 and
  # no +-0.99999 off the diagonal
  assert np.all(status == 0) and status.dtype == np.int32
  assert not np.any(np.isin(np.abs(want[i, j]), (0.0, dg_fit.BRACKET)))
  assert iterations.dtype == np.int32 and np.all(iterations[i, j] > 10)
  assert np.all(np.diag(iterations) == 0)
  # the residual of every converged pair
  f = dg_fit.pair_function(rates, gamma, cov, i, j, corr[i, j])
  assert np.all(np.abs(f) <= TOL)


def test_recovery_of_the_true_correlation(fitted):
  g, (rates, gamma, cov), (corr, _, _) = fitted
  T = g['trains'].shape[1]
  truth = g['true_corr']
  i, j = np.tril_indices(len(rates), -1)
  density = cases.bivariate_density(gamma[i], gamma[j], truth[i, j])
  se = np.sqrt(np.maximum(rates[i] * rates[j], 1e-6) / T) / density
  z = np.abs(corr[i, j] - truth[i, j]) / se
  print('largest deviation: {:.2f} se'.format(z.max()))
  assert np.all(z <= 5.0)
  assert 0.3 < np.abs(truth[i, j]).max() < 0.6


def test_one_constructed_pair_for_each_early_status():
  rates, gamma, cov, lam = cases.status_system()
  corr, status, iterations = cases.statement('status_system')
  want = {1: 0.0, 2: -dg_fit.BRACKET, 3: dg_fit.BRACKET, 4: 0.0}
  for (i, j), code in cases.STATUS_PAIRS.items():
    assert status[i, j] == status[j, i] == code, (i, j)
    assert corr[i, j] == corr[j, i] == want[code], (i, j)
    assert iterations[i, j] == 0
  # each for its own reason
  f0, f1 = (dg_fit.pair_function(rates, gamma, cov, [2, 3, 4], [0, 1, 2],
                                 np.full(3, s * dg_fit.BRACKET))
            for s in (-1, 1))
  assert abs(f0[0]) < TOL and abs(f1[0]) > 1e-3
  assert abs(f1[1]) < TOL and abs(f0[1]) > 1e-3
  assert f0[2] < -1e-3 and f1[2] < -1e-3
  # every other pair converges to the latent correlation it was built from
  i, j = np.tril_indices(len(rates), -1)
  rest = np.array([(a, b) not in cases.STATUS_PAIRS and
                   (a, b) != cases.CLOSING_PAIR for a, b in zip(i, j)])
  assert np.all(status[i, j][rest] == 0)
  density = cases.bivariate_density(gamma[i], gamma[j], lam[i, j])[rest]
  assert np.all(np.abs(corr[i, j] - lam[i, j])[rest] <=
                2 * (TOL + cases.EPS_CDF) / density)
  for (a, b), v in cases.NEAR_ENDS.items():
    assert abs(corr[a, b] - v) < 1e-5


def test_iteration_limit_and_arguments():
  rates, gamma, cov, _ = cases.status_system()
  corr, status, iterations = cases.statement('status_system', maxiters=3)
  i, j = np.tril_indices(len(rates), -1)
  early = np.array([(a, b) in cases.STATUS_PAIRS for a, b in zip(i, j)])
  assert np.all(status[i, j][~early] == 5)
  assert np.all(iterations[i, j][~early] == 3)
  # the third midpoint: 0, then +-1/2, then +-1/4 or +-3/4 of the bracket
  third = np.abs(corr[i, j][~early]) / dg_fit.BRACKET
  assert np.all(np.isclose(third, 0.25, rtol=1e-12) |
                np.isclose(third, 0.75, rtol=1e-12))
  # a function without a root that the reference bisects all the same: the
  # bracket closes on lambda_1, the pair stops there and reports the limit it
  # would have run to
  a, b = cases.CLOSING_PAIR
  f0, f1 = (dg_fit.pair_function(rates, gamma, cov, [a], [b],
                                 [s * dg_fit.BRACKET])[0] for s in (-1, 1))
  assert f0 < -cases.TOL and f1 < -cases.TOL and f0 * f1 < cases.TOL
  for maxiters in (1000, 100000):
    corr, status, iterations = cases.statement('status_system',
                                               maxiters=maxiters)
    assert status[a, b] == 5 and iterations[a, b] == maxiters
    assert 0 <= dg_fit.BRACKET - corr[a, b] < 1e-15
  for bad in (dict(tol=0.0), dict(tol=-1.0), dict(maxiters=0)):
    with pytest.raises(ValueError):
      dg_fit.gauss_correlation(rates, gamma, cov, **bad)
  with pytest.raises(ValueError):
    dg_fit.gauss_correlation(rates[:1], gamma[:1], cov[:1, :1])


def test_the_statement_held_against_itself_needs_no_excuse():
  rates, gamma, cov, _ = cases.status_system()
  want = cases.statement('status_system')
  report = dg_fit.compare_with_statement(rates, gamma, cov, want, want)
  assert report == dict(pairs=28, excused=0, failures=[])
  # and the rule sees a changed lambda, status or count
  for which, value in ((0, 0.25), (1, 5), (2, 7)):
    other = [np.array(a) for a in want]
    other[which][6, 5] = other[which][5, 6] = value
    assert dg_fit.compare_with_statement(rates, gamma, cov, other,
                                         want)['failures']


def test_nearest_correlation(fitted):
  g = fitted[0]
  M = g['higham_in']
  assert np.linalg.eigvalsh(M).min() < 0
  got = dg_fit.nearest_correlation(M)
  np.testing.assert_array_equal(got, got.T)
  np.testing.assert_allclose(np.diag(got), 1.0, atol=1e-6)
  np.linalg.cholesky(got)
  bound = 10 * 1e-10 * np.abs(g['higham_out']).sum(1).max()
  diff = np.abs(got - g['higham_out']).max()
  print('max |nearest_correlation - reference| = {:.3e}'.format(diff))
  assert diff <= bound
  # a positive definite input is handed back as it is
  pd = np.array(g['true_corr'])
  assert dg_fit.corr_for_sampling(pd) is not None
  np.testing.assert_array_equal(dg_fit.corr_for_sampling(pd), pd)
  np.testing.assert_array_equal(dg_fit.corr_for_sampling(M), got)


def test_sample_spikes_corr_reproduces_the_golden_sample(fitted):
  g, (rates, gamma, cov), (corr, _, _) = fitted
  T = g['trains'].shape[1]
  spikes = dg.sample_spikes_corr(gamma, dg_fit.corr_for_sampling(corr), T,
                                 np.random.RandomState(7))
  assert spikes.shape == (6, T) and spikes.dtype == np.float32
  assert set(np.unique(spikes)) <= {0.0, 1.0}
  # the bars of tests/test_dg_data.py, at this sample's T
  np.testing.assert_allclose(spikes.mean(axis=1), rates, rtol=0.06, atol=2e-3)
  se = np.sqrt(np.outer(rates, rates) / T) * 4 + 2e-3
  assert np.all(np.abs(np.cov(spikes) - cov) < se)
  # the off-diagonal covariances are not merely small: the sample has them
  i, j = np.tril_indices(6, -1)
  assert np.corrcoef(np.cov(spikes)[i, j], cov[i, j])[0, 1] > 0.99


def test_sample_spikes_corr_with_equicorrelation_has_the_law_of_sample_spikes():
  g = cases.golden()
  from scipy.stats import norm
  gamma, rho, T = norm.ppf(g['rates']), 0.05, 200000
  eq = (1 - rho) * np.eye(6) + rho * np.ones((6, 6))
  a = dg.sample_spikes_corr(gamma, eq, T, np.random.RandomState(3))
  b = dg.sample_spikes(gamma, rho, T, np.random.RandomState(4))
  np.testing.assert_allclose(a.mean(1), b.mean(1), rtol=0.06, atol=2e-3)
  se = np.sqrt(np.outer(g['rates'], g['rates']) / T) * 4 + 2e-3
  assert np.all(np.abs(np.cov(a) - np.cov(b)) < se)


def _recording(C, T, seed=11):
  """A (signals, spikes) recording whose trains are correlated and busy enough
  for every pair to have a covariance."""
  rates, gamma, _, lam = cases.random_system(C, seed, spread=0.3)
  rng = np.random.RandomState(seed)
  spikes = dg.sample_spikes_corr(gamma, dg_fit.corr_for_sampling(lam), T, rng)
  return dg.spikes_to_signals(spikes, rng), spikes


def test_tool_end_to_end(tmp_path):
  C, T = 8, 4000
  signals, spikes = _recording(C + 2, T)
  source, out = str(tmp_path / 'recording.pkl'), str(tmp_path / 'dg.pkl')
  with open(source, 'wb') as file:
    pickle.dump({'signals': signals, 'oasis': spikes}, file)
  log = subprocess.run([sys.executable, TOOL, '--input', source, '--output',
                        out], check=True, capture_output=True, text=True).stdout
  assert re.search(r'^\s+28 pairs: converged$', log, re.M), log
  with open(out, 'rb') as file:
    twin = pickle.load(file)
  assert sorted(twin) == ['correlation', 'covariance', 'mean', 'oasis',
                          'signals', 'status']
  for key, shape, dtype in (('signals', (C, T), np.float32),
                            ('oasis', (C, T), np.float32),
                            ('mean', (1, C), np.float64),
                            ('covariance', (C, C), np.float64),
                            ('correlation', (C, C), np.float64),
                            ('status', (C, C), np.int32)):
    assert twin[key].shape == shape and twin[key].dtype == dtype, key
  # the first two rows of the input were dropped; the twin fires, at the
  # recording's rates
  want = spikes[2:].mean(1)
  got = twin['oasis'].mean(1)
  assert got.min() > 0
  assert np.all(np.abs(got - want) <= 5 * np.sqrt(want * (1 - want) / T))
  assert set(np.unique(twin['oasis'])) <= {0.0, 1.0}
  np.testing.assert_array_equal(
      twin['covariance'], dg_fit.recording_statistics(spikes[2:])[2])
  # seeded: a second run writes the same bytes; --is_dg_data keeps all rows
  with open(out, 'rb') as file:
    first = file.read()
  subprocess.run([sys.executable, TOOL, '--input', source, '--output', out],
                 check=True, capture_output=True)
  with open(out, 'rb') as file:
    assert file.read() == first
  # generate_dataset.py --is_dg_data reads the file as it is
  target = str(tmp_path / 'dataset')
  subprocess.run([sys.executable,
                  os.path.join(ROOT, 'dataset', 'generate_dataset.py'),
                  '--input', out, '--output_dir', target, '--sequence_length',
                  '256', '--validation_size', '10', '--is_dg_data',
                  '--normalize'], check=True, capture_output=True)
  with open(os.path.join(target, 'info.pkl'), 'rb') as file:
    info = pickle.load(file)
  assert info['num_neurons'] == C


def test_header_keeps_abi_20_and_declares_the_entry():
  assert _lib.CG_ABI_VERSION == 20
  assert 'dg_fit.hip' in cg_build.SOURCES
  sig = _lib.SIGNATURES['cg_dg_correlation']
  assert len(sig) == 12
  assert _lib.CONSTANTS['CG_DG_FIT_MAX_BLOCKS'] >= 1
  assert _lib.CONSTANTS['CG_DG_FIT_BLOCK_PAIRS'] * 16 == 64
  assert dg_fit.MAX_NEURONS == 4096
