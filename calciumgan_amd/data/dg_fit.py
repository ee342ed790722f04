"""Fit the dichotomised-Gaussian (DG) model to recorded spike trains: the
latent Gaussian whose thresholded samples have the recording's firing rates and
pairwise covariances.

Numpy statements of the reference's dataset/dg package, and the device form of
the one stage that is expensive:

  recording_statistics   DGOptimise.gauss_mean / data_tfix_covariance
                         (optim_dichot_gauss.py:109-126, :144-154)
  bivariate_normal_cdf   Phi_2(h, k; r), what scipy's multivariate_normal.cdf
                         is to the reference (optim_dichot_gauss.py:11-25)
  gauss_correlation      DGOptimise.get_gauss_correlation with
                         find_root_bisection (optim_dichot_gauss.py:46-94,
                         :156-194): per neuron pair, the latent correlation
                         lambda with Phi_2(g_i, g_j; lambda) = r_i r_j + S_ij
  gauss_correlation_device   the same on the GPU (cg_dg_correlation,
                         csrc/dg_fit.hip), one 16-lane row per pair
  nearest_correlation    Higham.higham_correction (dichot_gauss.py:35-100)
  corr_for_sampling      DichotGauss.do_higham_correction, make_pd=True
  fit                    all of it for one recording

Phi_2 is Plackett's integral

  Phi_2(h, k; r) = Phi(h) Phi(k)
      + 1 / (2 pi) int_0^asin(r) exp(-(h^2 + k^2 - 2 h k sin t) / (2 cos^2 t)) dt

over PANELS = 64 uniform panels of a 16-point Gauss-Legendre rule.  The
integrand has a feature of width |h - k| at t -> pi / 2, which is why one rule
over the whole interval is not enough near |r| = 1.  The 1024 terms are summed
in a fixed order: sixteen groups of 64 consecutive nodes (four panels) one
after the other, then the sixteen partial sums in a tree over neighbours.  That
is the order of the kernel (a lane's own nodes, then the row's DPP tree), so
the two differ only through exp, sin, cos, asin and erfc.
"""
import math

import numpy as np

# 16-point Gauss-Legendre on (0, 1): (x + 1) / 2, and the weights of (-1, 1).
# The same literals stand in csrc/dg_fit.hip.
GL_X = (0.005299532504175031, 0.0277124884633837, 0.06718439880608412,
        0.1222977958224985, 0.19106187779867811, 0.2709916111713863,
        0.35919822461037054, 0.4524937450811813, 0.5475062549188188,
        0.6408017753896295, 0.7290083888286136, 0.8089381222013219,
        0.8777022041775016, 0.9328156011939159, 0.9722875115366163,
        0.994700467495825)
GL_W = (0.027152459411754037, 0.062253523938647706, 0.09515851168249259,
        0.12462897125553403, 0.14959598881657676, 0.16915651939500262,
        0.1826034150449236, 0.18945061045506859, 0.18945061045506859,
        0.1826034150449236, 0.16915651939500262, 0.14959598881657676,
        0.12462897125553403, 0.09515851168249259, 0.062253523938647706,
        0.027152459411754037)
PANELS = 64
LANES = 16                      # partial sums; a DPP row in the kernel
NODES = PANELS * len(GL_X)      # 1024
INV_2PI = 0.15915494309189535   # float64(1 / (2 pi))
BRACKET = 0.99999               # find_root_bisection's lambda_0 / lambda_1
COV_SKIP = 1e-10                # get_gauss_correlation's |S_ij| <= 1e-10
MAX_NEURONS = 4096              # cg_dg_correlation's limit

CONVERGED, COV_SKIPPED, AT_LAMBDA0, AT_LAMBDA1, SAME_SIDE, ITERATION_LIMIT = (
    range(6))
STATUS_NAMES = ('converged', 'covariance skip', 'lambda_0 returned',
                'lambda_1 returned', 'same side -> 0', 'iteration limit')


def _nodes():
  """u in (0, 1) and the weight of node n = 0 .. 1023 (panel n // 16, point
  n % 16): theta = asin(r) u, d theta = asin(r) w."""
  panel = np.repeat(np.arange(PANELS, dtype=np.float64), len(GL_X))
  u = (panel + np.tile(np.array(GL_X), PANELS)) * (1.0 / PANELS)
  w = np.tile(np.array(GL_W), PANELS) * (0.5 / PANELS)
  return u, w


_U, _W = _nodes()
_erfc = np.frompyfunc(math.erfc, 1, 1)


def normal_cdf(x):
  """Phi(x) = erfc(-x / sqrt 2) / 2, float64."""
  x = np.asarray(x, dtype=np.float64)
  return 0.5 * _erfc(-x * math.sqrt(0.5)).astype(np.float64)


def _plackett(pp, hk, hs, r):
  """Phi_2 for flat float64 arrays: pp = Phi(h) Phi(k), hk = h k,
  hs = (h h + k k) / 2."""
  a = np.arcsin(r)
  theta = a[:, None] * _U[None, :]
  s, c = np.sin(theta), np.cos(theta)
  t = _W[None, :] * np.exp((hk[:, None] * s - hs[:, None]) / (c * c))
  t = t.reshape(len(a), LANES, NODES // LANES)
  acc = np.zeros((len(a), LANES))
  for m in range(NODES // LANES):
    acc = acc + t[:, :, m]
  while acc.shape[1] > 1:
    acc = acc[:, 0::2] + acc[:, 1::2]
  return pp + (a * acc[:, 0]) * INV_2PI


def bivariate_normal_cdf(h, k, r):
  """P(X <= h, Y <= k) of a standard bivariate normal with correlation r;
  float64, broadcasting.  For |h|, |k| <= 3.8 and |r| <= 0.99999 it agrees with
  scipy.stats.multivariate_normal.cdf to 1e-11 (profiles/dg_fit_parity.txt)."""
  h, k, r = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64)
                                  for v in (h, k, r)))
  shape = h.shape
  h, k, r = h.ravel(), k.ravel(), r.ravel()
  out = np.empty(h.shape)
  for o in range(0, len(h), 4096):  # (n, 1024) temporaries
    sl = slice(o, o + 4096)
    out[sl] = _plackett(normal_cdf(h[sl]) * normal_cdf(k[sl]), h[sl] * k[sl],
                        (h[sl] * h[sl] + k[sl] * k[sl]) * 0.5, r[sl])
  return out.reshape(shape)


def recording_statistics(spikes):
  """(rates (C,), gamma (C,), cov (C, C)), float64, of (neurons, T) spike
  trains: the reference's gauss_mean and data_tfix_covariance of its (1, T, C)
  layout, computed in the trains' own dtype (float32 in its script) and then
  widened.  gamma is Phi^-1 of the rates with exact 0 / 1 moved by 1e-4; the
  rates themselves are returned as measured, as get_gauss_correlation uses
  them."""
  from scipy.stats import norm
  spikes = np.asarray(spikes)
  if spikes.ndim != 2:
    raise ValueError('spikes must be (neurons, T)')
  if not np.issubdtype(spikes.dtype, np.floating):
    spikes = spikes.astype(np.float32)
  data = np.expand_dims(np.transpose(spikes, axes=(1, 0)), axis=0)
  trials, num_neur = data.shape[1], data.shape[2]
  mean = data.mean(1)
  if np.any(mean < 0) or np.any(mean > 1):
    raise ValueError('mean should have a value between 0 and 1')
  rates = data.mean(1).mean(0)
  mean[mean == 0.] += 1e-4
  mean[mean == 1.] -= 1e-4
  gamma = norm.ppf(mean)
  data_norm = (data - data.mean(1)).reshape(-1, num_neur)
  cov = data_norm.T.dot(data_norm) / (1 * trials)
  return (rates.astype(np.float64), np.asarray(gamma, np.float64).reshape(-1),
          cov.astype(np.float64))


def pair_function(rates, gamma, cov, i, j, lam):
  """f = Phi_2(gamma_i, gamma_j; lam) - r_i r_j - cov[i, j] of
  optim_dichot_gauss.function, for index arrays i, j and an array lam.
  r_i r_j is the float32 product of the rates rounded to float32, widened: the
  reference's script hands DGOptimise float32 trains, and np.prod of their two
  float32 means is a float32 (7.6e-9 from the float64 product for rates 0.4 and
  0.6, against a tolerance of 1e-10).  Rates from recording_statistics are
  float32 values already."""
  rates, gamma, cov = (np.asarray(v, np.float64) for v in (rates, gamma, cov))
  rates = rates.astype(np.float32)
  i, j = np.asarray(i), np.asarray(j)
  lam = np.asarray(lam, np.float64)
  phi = normal_cdf(gamma)
  out = np.empty(len(i))
  for o in range(0, len(i), 4096):
    a, b = i[o:o + 4096], j[o:o + 4096]
    h, k = gamma[a], gamma[b]
    p = _plackett(phi[a] * phi[b], h * k, (h * h + k * k) * 0.5,
                  lam[o:o + 4096])
    out[o:o + 4096] = (p - (rates[a] * rates[b]).astype(np.float64)) - cov[a, b]
  return out


def _check_fit_arguments(C, tol, maxiters):
  if not 2 <= C <= MAX_NEURONS:
    raise ValueError('between 2 and {} neurons'.format(MAX_NEURONS))
  if not tol > 0 or not maxiters >= 1:
    raise ValueError('tol > 0 and maxiters >= 1')


def gauss_correlation(rates, gamma, cov, tol=1e-10, maxiters=1000):
  """(corr float64, status int32, iterations int32), all (C, C): per pair
  i > j, reading cov[i, j], find_root_bisection on the bracket +-0.99999 with
  its three early returns in its order, after get_gauss_correlation's skip of
  |cov| <= 1e-10; both triangles filled, the diagonal 1 / 0 / 0.  status is one
  of CONVERGED .. ITERATION_LIMIT.  A pair whose midpoint has met an end of its
  bracket stops there: further iterations would repeat it up to maxiters, which
  is what `iterations` then reports."""
  rates, gamma, cov = (np.asarray(v, np.float64) for v in (rates, gamma, cov))
  C = len(rates)
  _check_fit_arguments(C, tol, maxiters)
  if gamma.shape != (C,) or cov.shape != (C, C):
    raise ValueError('rates, gamma (C,) and cov (C, C)')
  maxiters = int(maxiters)
  ii, jj = np.tril_indices(C, -1)
  n = len(ii)
  lam = np.zeros(n)
  status = np.full(n, COV_SKIPPED, np.int32)
  its = np.zeros(n, np.int32)

  todo = np.flatnonzero(~(np.abs(cov[ii, jj]) <= COV_SKIP))
  f0 = pair_function(rates, gamma, cov, ii[todo], jj[todo],
                     np.full(len(todo), -BRACKET))
  f1 = pair_function(rates, gamma, cov, ii[todo], jj[todo],
                     np.full(len(todo), BRACKET))
  at0 = np.abs(f0) < tol
  at1 = ~at0 & (np.abs(f1) < tol)
  same = ~at0 & ~at1 & (f0 * f1 > tol)
  status[todo[at0]], lam[todo[at0]] = AT_LAMBDA0, -BRACKET
  status[todo[at1]], lam[todo[at1]] = AT_LAMBDA1, BRACKET
  status[todo[same]] = SAME_SIDE

  act = todo[~(at0 | at1 | same)]      # pairs still bisecting
  lo = np.full(len(act), -BRACKET)
  hi = np.full(len(act), BRACKET)
  it = 0
  while len(act):
    mid = (lo + hi) / 2
    f = pair_function(rates, gamma, cov, ii[act], jj[act], mid)
    stuck = (mid == lo) | (mid == hi)
    hi = np.where(f > 0, mid, hi)
    lo = np.where(f < 0, mid, lo)
    it += 1
    conv = ~(np.abs(f) > tol)
    out_of_time = ~conv & (stuck | (it >= maxiters))
    done = conv | out_of_time
    lam[act[done]] = mid[done]
    its[act[conv]] = it
    its[act[out_of_time]] = maxiters
    status[act[conv]] = np.where(np.abs(f[conv]) <= tol, CONVERGED,
                                 ITERATION_LIMIT)  # (a NaN residual)
    status[act[out_of_time]] = ITERATION_LIMIT
    act, lo, hi = act[~done], lo[~done], hi[~done]

  corr = np.eye(C)
  stat = np.zeros((C, C), np.int32)
  iters = np.zeros((C, C), np.int32)
  for full, flat in ((corr, lam), (stat, status), (iters, its)):
    full[ii, jj] = flat
    full[jj, ii] = flat
  return corr, stat, iters


def gauss_correlation_device(rates, gamma, cov, tol=1e-10, maxiters=1000):
  """`gauss_correlation` on the GPU (cg_dg_correlation): float64 device tensors
  rates, gamma (C,) and cov (C, C) of any strides in; (corr float64, status
  int32, iterations int32) device tensors out, every element written by the
  one launch."""
  import torch
  from .. import _lib as hip
  for t in (rates, gamma, cov):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and
            t.dtype == torch.float64):
      raise ValueError('rates, gamma and cov are float64 device tensors')
  C = rates.shape[0]
  if rates.dim() != 1 or gamma.shape != (C,) or cov.shape != (C, C):
    raise ValueError('rates, gamma (C,) and cov (C, C)')
  _check_fit_arguments(C, tol, maxiters)
  rates, gamma = rates.contiguous(), gamma.contiguous()
  corr = torch.empty((C, C), dtype=torch.float64, device=cov.device)
  status = torch.empty((C, C), dtype=torch.int32, device=cov.device)
  iterations = torch.empty((C, C), dtype=torch.int32, device=cov.device)
  with torch.cuda.device(cov.device):
    hip.call('cg_dg_correlation', rates, gamma, cov, cov.stride(0),
             cov.stride(1), C, float(tol), int(maxiters), corr, status,
             iterations, hip.stream())
  return corr, status, iterations


def nearest_correlation(M, maxiters=1e5, tol=1e-10):
  """Higham.higham_correction: alternating projections onto the positive
  semi-definite matrices and onto unit diagonals, then the reference's repair
  of eigenvalues that are still negative.  numpy.linalg.eigh where the
  reference calls eig: its input is symmetric."""
  M = np.asarray(M, np.float64)

  def projection_s(R):
    eigval, eigvec = np.linalg.eigh(R)
    eigval[eigval < 0.] = 0.
    return eigvec.dot(np.diag(eigval).dot(eigvec.T))

  def projection_u(X):
    return X - np.diag(np.diag(X - np.eye(len(X))))

  it, DS, Yo, Xo, Yn, delta = 0, 0., M, M, M, np.inf
  while it < maxiters and delta > tol:
    R = Yo - DS
    Xn = projection_s(R)
    DS = Xn - R
    Yn = projection_u(Xn)
    del_x = max(np.abs(Xn - Xo).sum(1)) / max(np.abs(Xn).sum(1))
    del_y = max(np.abs(Yn - Yo).sum(1)) / max(np.abs(Yn).sum(1))
    del_xy = max(np.abs(Yn - Xn).sum(1)) / max(np.abs(Yn).sum(1))
    delta = max(del_x, del_y, del_xy)
    Xo, Yo = Xn, Yn
    it += 1
  eigval, eigvec = np.linalg.eigh(Yn)
  if eigval.min() < 0:
    eigval[eigval < 0.] = 1e-6
    Yn = eigvec.dot(np.diag(eigval).dot(eigvec.T))
    std = np.sqrt(np.diag(Yn))
    Yn = Yn / (np.outer(std, std) + 1e-8)   # dichot_gauss.cov_to_corr
    Yn = 0.5 * (Yn + Yn.T)
  return Yn


def _is_pd(M):
  try:
    np.linalg.cholesky(M)
    return True
  except np.linalg.LinAlgError:
    return False


def corr_for_sampling(M):
  """DichotGauss.do_higham_correction with make_pd=True: M itself when its
  Cholesky factorisation succeeds, else its nearest correlation matrix."""
  M = np.asarray(M, np.float64)
  if _is_pd(M):
    return M
  if np.any(M != M.T):                      # dichot_gauss.make_symmetric
    M = np.triu(M) + np.triu(M, 1).T
  return nearest_correlation(M)


def fit(spikes, device='cpu', tol=1e-10, maxiters=1000):
  """The DG model of (neurons, T) spike trains: dict(mean (1, C) = gamma,
  covariance, correlation (the bisection's matrix), status, iterations,
  sampling_correlation (after corr_for_sampling)), numpy arrays.  device 'gpu'
  runs the pair loop as cg_dg_correlation."""
  if device not in ('cpu', 'gpu'):
    raise ValueError("device must be 'cpu' or 'gpu'")
  rates, gamma, cov = recording_statistics(spikes)
  if device == 'gpu':
    import torch
    out = gauss_correlation_device(
        *(torch.from_numpy(v).to('cuda:0') for v in (rates, gamma, cov)),
        tol=tol, maxiters=maxiters)
    corr, status, iterations = (t.cpu().numpy() for t in out)
  else:
    corr, status, iterations = gauss_correlation(rates, gamma, cov, tol,
                                                 maxiters)
  return dict(mean=gamma[None, :], covariance=cov, correlation=corr,
              status=status, iterations=iterations,
              sampling_correlation=corr_for_sampling(corr))


def compare_with_statement(rates, gamma, cov, got, want, tol=1e-10):
  """The rule by which a result `got` = (corr, status, iterations) of another
  implementation (the kernel) is held against the statement's `want`, pair by
  pair (i > j): equal status, and lambda and iterations equal bit for bit.  One
  excuse: the iteration counts differ by exactly 1 and the statement's residual
  at the earlier of the two stops lies within 1e-13 of tol -- a library function
  rounded the other way at the stop test.  Independently, every converged pair
  of `got` has |f_statement(lambda)| <= tol (1 + 1e-3).  Returns dict(pairs,
  excused, failures): failures lists (i, j, reason) and is empty when the rule
  holds; the caller bounds the share of excused pairs."""
  C = len(rates)
  ii, jj = np.tril_indices(C, -1)
  (lam_g, st_g, it_g), (lam_w, st_w, it_w) = (
      tuple(np.asarray(a)[ii, jj] for a in res) for res in (got, want))
  failures = []
  for name, a in zip(('corr', 'status', 'iterations'), got):
    a = np.asarray(a)
    if not np.array_equal(a, a.T):
      failures.append((-1, -1, name + ' is not symmetric'))
  for k in np.flatnonzero(st_g != st_w):
    failures.append((int(ii[k]), int(jj[k]), 'status {} for {}'.format(
        st_g[k], st_w[k])))
  differ = np.flatnonzero((st_g == st_w) & (
      (lam_g.view(np.int64) != lam_w.view(np.int64)) | (it_g != it_w)))
  excused = 0
  if len(differ):
    first_g = it_g[differ] < it_w[differ]
    earlier = np.where(first_g, lam_g[differ], lam_w[differ])
    f = pair_function(rates, gamma, cov, ii[differ], jj[differ], earlier)
    ok = ((np.abs(it_g[differ].astype(np.int64) - it_w[differ]) == 1) &
          (np.abs(np.abs(f) - tol) <= 1e-13))
    excused = int(ok.sum())
    for k, res in zip(differ[~ok], f[~ok]):
      failures.append((int(ii[k]), int(jj[k]),
                       'lambda {!r} after {} for {!r} after {} (residual {!r} '
                       'at the earlier stop)'.format(
                           lam_g[k], it_g[k], lam_w[k], it_w[k], res)))
  conv = np.flatnonzero(st_g == CONVERGED)
  f = pair_function(rates, gamma, cov, ii[conv], jj[conv], lam_g[conv])
  for k, res in zip(conv[~(np.abs(f) <= tol * (1 + 1e-3))],
                    f[~(np.abs(f) <= tol * (1 + 1e-3))]):
    failures.append((int(ii[k]), int(jj[k]),
                     'converged with residual {!r}'.format(res)))
  return dict(pairs=len(ii), excused=excused, failures=failures)
