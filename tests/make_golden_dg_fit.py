"""Generate tests/golden/dg_fit_reference.npz (run from the repo root:
``python tests/make_golden_dg_fit.py``): outputs of the REFERENCE's dg package
(dataset/dg, numpy + scipy only) on seeded inputs, for tests/test_dg_fit_host.py.
Data only.

(a) a sample of a DG model with known rates and latent correlation, and what
    DGOptimise makes of its float32 trains: gauss_mean, data_tfix_covariance,
    get_gauss_correlation;
(b) Higham().higham_correction of a symmetric unit-diagonal matrix that is not
    positive definite.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'dg_fit_reference.npz')
REFERENCE = os.environ.get('CALCIUMGAN_REFERENCE', '/root/reference')

RATES = np.array([0.02, 0.05, 0.1, 0.2, 0.4, 0.6])
T = 200000


def true_correlation(rng, n=6, rank=2):
  """Low rank plus identity, scaled to a unit diagonal."""
  A = rng.standard_normal((n, rank)) * 0.7
  M = A.dot(A.T) + np.eye(n)
  d = np.sqrt(np.diag(M))
  M = M / np.outer(d, d)
  return 0.5 * (M + M.T)


def non_pd_matrix(rng, n=6):
  """Symmetric, unit diagonal, off-diagonals too large for any Gaussian."""
  M = rng.uniform(-0.9, 0.9, (n, n))
  M = 0.5 * (M + M.T)
  np.fill_diagonal(M, 1.0)
  assert np.linalg.eigvalsh(M).min() < -0.05
  return M


def main():
  dataset = os.path.join(REFERENCE, 'dataset')
  if not os.path.isdir(dataset):
    print('reference not present; keeping the existing golden')
    return
  sys.path.insert(0, dataset)
  from dg.dichot_gauss import DichotGauss, Higham
  from dg.optim_dichot_gauss import DGOptimise
  from scipy.stats import norm
  warnings.simplefilter('ignore')

  rng = np.random.RandomState(20)
  corr = true_correlation(rng)
  gamma = norm.ppf(RATES)[None, :]
  np.random.seed(1234)
  dg = DichotGauss(len(RATES), mean=gamma, corr=corr, make_pd=True)
  spikes = dg.sample(repeats=T)                      # (1, T, n)
  trains = spikes[0].T.astype(np.float32)            # (n, T), the script's dtype
  # generate_dg_data.py:24-32
  data = np.expand_dims(np.transpose(trains, axes=(1, 0)), axis=0)
  opt = DGOptimise(data)
  gauss_mean = np.asarray(opt.gauss_mean)
  covariance = np.asarray(opt.data_tfix_covariance)
  gauss_corr = np.asarray(opt.get_gauss_correlation(set_attr=False))

  M = non_pd_matrix(np.random.RandomState(22))
  higham = np.asarray(Higham().higham_correction(M.copy()))

  np.savez_compressed(
      OUT, rates=RATES, true_corr=corr, trains=trains.astype(np.int8),
      gauss_mean=gauss_mean, covariance=covariance, gauss_corr=gauss_corr,
      higham_in=M, higham_out=higham)
  print('wrote {} ({} bytes)'.format(OUT, os.path.getsize(OUT)))
  print('off-diagonals of the true correlation: {:.3f} .. {:.3f}'.format(
      corr[~np.eye(len(RATES), dtype=bool)].min(),
      corr[~np.eye(len(RATES), dtype=bool)].max()))


if __name__ == '__main__':
  main()
