"""Inputs shared by tests/test_dg_fit_host.py and tests/test_hip_dg_fit.py: the
grid on which bivariate_normal_cdf is held against scipy, and systems of
neurons (rates, gamma, cov) whose pairs end in chosen statuses of the DG fit.
Everything is seeded and read-only."""
import functools
import os

import numpy as np
from scipy.stats import norm

from calciumgan_amd.data import dg_fit

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'dg_fit_reference.npz')
# |bivariate_normal_cdf - scipy| over cdf_grid(), as measured
# (profiles/dg_fit_parity.txt: 1.4e-14), rounded up
EPS_CDF = 1e-13
TOL = 1e-10


def cdf_grid():
  """(h, k, r) over |h|, |k| <= 3.8 and |r| <= 0.99999: both signs, the
  thresholds of clipped rates (+-3.72), h near k (where the integrand has its
  narrowest feature), and r up to both ends of the bracket in decades of
  1 - |r|."""
  hs = [-3.8, -3.72, -2.5, -1.0, -0.3, 0.0, 0.4, 1.7, 3.72, 3.8]
  rs = [0.0, 0.3, -0.6, 0.9, -0.99, 0.999, -0.9999]
  rs += [s * (1.0 - 10.0**-k) for k in range(1, 6) for s in (1.0, -1.0)]
  rs += [0.99999, -0.99999]
  H, K, R = [], [], []
  for h in hs:
    for k in hs + [h + 1e-3, h - 0.01, h + 0.004, -h + 0.002]:
      if abs(k) > 3.8:
        continue
      for r in rs:
        H.append(h)
        K.append(k)
        R.append(r)
  return tuple(np.array(v) for v in (H, K, R))


def model_covariance(rates, gamma, lam):
  """cov[i, j] of the DG model with latent correlations lam: Phi_2(gamma_i,
  gamma_j; lam_ij) - fl32(r_i r_j); the diagonal r (1 - r)."""
  C = len(rates)
  i, j = np.tril_indices(C, -1)
  r32 = rates.astype(np.float32)
  c = (dg_fit.bivariate_normal_cdf(gamma[i], gamma[j], lam[i, j]) -
       (r32[i] * r32[j]).astype(np.float64))
  cov = np.diag(rates * (1 - rates))
  cov[i, j] = c
  cov[j, i] = c
  return cov


def _gamma(rates):
  """recording_statistics' thresholds: float32 rates, exact 0 / 1 nudged."""
  mean = rates.astype(np.float32)
  mean[mean == 0.] += 1e-4
  mean[mean == 1.] -= 1e-4
  return np.asarray(norm.ppf(mean), np.float64)


def _freeze(*arrays):
  for a in arrays:
    a.setflags(write=False)
  return arrays


@functools.lru_cache(maxsize=None)
def random_system(C, seed, spread=0.6):
  """(rates, gamma, cov, lam): rates on both sides of 1 / 2 (gamma on both
  sides of 0), latent correlations uniform in +-spread; the covariance is the
  model's, so every pair bisects and recovers lam."""
  rng = np.random.RandomState(seed)
  rates = rng.uniform(0.01, 0.95, C).astype(np.float32).astype(np.float64)
  lam = rng.uniform(-spread, spread, (C, C))
  lam = np.tril(lam, -1) + np.tril(lam, -1).T + np.eye(C)
  gamma = _gamma(rates)
  return _freeze(rates, gamma, model_covariance(rates, gamma, lam), lam)


# pairs (i, j) of status_system() and the status each is built to end in (0:
# every other pair)
STATUS_PAIRS = {(1, 0): 1, (2, 0): 2, (3, 1): 3, (4, 2): 4}
NEAR_ENDS = {(5, 3): 0.9999, (6, 1): -0.9999}
CLOSING_PAIR = (7, 4)


@functools.lru_cache(maxsize=None)
def status_system():
  """Eight neurons: rates from the 1e-4 clip (a silent neuron and one at
  exactly 1e-4) to 0.98, gamma on both sides of 0.  The covariances are the
  model's for latent correlations in +-0.5, except

    (1, 0)  zero                                     -> covariance skip
    (2, 0)  the model's at lambda = -0.99999 (a neuron anti-duplicated in the
            latent: f0 = 0)                          -> lambda_0 returned
    (3, 1)  the model's at lambda = +0.99999 (duplicated: f1 = 0)
                                                     -> lambda_1 returned
    (4, 2)  the model's at +0.99999 plus 0.01: more than any lambda gives
                                                     -> same side, 0
    NEAR_ENDS  the model's at +-0.9999, between neurons with equal and with
            opposite thresholds (any others saturate long before, and end in
            an early return): bisection up to the ends of the bracket

    CLOSING_PAIR  two neurons at the clip, the model's at +0.99999 plus 5e-7:
            f0 = -1e-4 and f1 = -5e-7 lie on one side, but their product is
            below tol, so the reference bisects a function without a root; the
            bracket closes on lambda_1 after some 50 steps and the pair ends at
            the iteration limit                      -> iteration limit

  Neuron 7 never fires: rate 0, gamma = Phi^-1(1e-4); its model covariances
  are those of the nudged threshold, so its pairs bisect too."""
  rng = np.random.RandomState(5)
  rates = np.array([0.3, 0.02, 0.5, 0.7, 1e-4, 0.7, 0.98, 0.0])
  rates = rates.astype(np.float32).astype(np.float64)
  C = len(rates)
  gamma = _gamma(rates)
  lam = rng.uniform(-0.5, 0.5, (C, C))
  lam = np.tril(lam, -1) + np.tril(lam, -1).T + np.eye(C)
  for (i, j), v in list(NEAR_ENDS.items()) + [((2, 0), -dg_fit.BRACKET),
                                               ((3, 1), dg_fit.BRACKET),
                                               ((4, 2), dg_fit.BRACKET),
                                               (CLOSING_PAIR, dg_fit.BRACKET)]:
    lam[i, j] = lam[j, i] = v
  cov = model_covariance(rates, gamma, lam)
  cov[1, 0] = cov[0, 1] = 0.0
  cov[4, 2] = cov[2, 4] = cov[4, 2] + 0.01
  cov[7, 4] = cov[4, 7] = cov[7, 4] + 5e-7
  return _freeze(rates, gamma, cov, lam)


@functools.lru_cache(maxsize=None)
def statement(name, *args, tol=TOL, maxiters=1000):
  """gauss_correlation of a system of this module, computed once."""
  rates, gamma, cov = globals()[name](*args)[:3]
  return _freeze(*dg_fit.gauss_correlation(rates, gamma, cov, tol, maxiters))


def golden():
  return np.load(GOLDEN)


def bivariate_density(h, k, r):
  """phi_2(h, k; r) = d Phi_2 / d r."""
  q = 1.0 - r * r
  return np.exp(-(h * h - 2 * r * h * k + k * k) / (2 * q)) / (
      2 * np.pi * np.sqrt(q))
