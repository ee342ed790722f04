"""gan/utils/spike_metrics.py counterparts in numpy (Elephant / Neo are not
installed; they are un-pinned upstream -- PARITY UNPINNED, definitions below
follow Elephant's documented statistics on binary trains at 24 Hz).

spikes: (neurons, T) arrays of {0,1} at FRAME_RATE frames per second."""
import math

import numpy as np

from .spike_helper import FRAME_RATE


def mean_firing_rate(spikes):
  """spike_metrics.py:6-12: spikes per second over [0, T / 24 s) per neuron
  (elephant.statistics.mean_firing_rate of the Neo train built at
  spike_helper.py:8-14)."""
  spikes = np.asarray(spikes)
  duration = spikes.shape[-1] / FRAME_RATE
  return (spikes.sum(axis=-1) / duration).astype(np.float32)


def bin_counts(spikes, binsize_ms=500.0):
  """BinnedSpikeTrain(binsize=500 ms) counts: 12 frames per bin at 24 Hz; the
  trailing partial bin is dropped as Elephant does."""
  spikes = np.asarray(spikes)
  per_bin = int(round(binsize_ms / 1000.0 * FRAME_RATE))
  nb = spikes.shape[-1] // per_bin
  return spikes[..., :nb * per_bin].reshape(spikes.shape[:-1] +
                                            (nb, per_bin)).sum(-1)


def covariance(spikes1, spikes2=None, binsize_ms=500.0):
  """spike_metrics.py:28-38: covariance matrix of the binned counts
  (unbiased, N-1), cross block when spikes2 is given."""
  spikes = spikes1 if spikes2 is None else np.concatenate([spikes1, spikes2], 0)
  cov = np.atleast_2d(np.cov(bin_counts(spikes, binsize_ms)))
  if spikes2 is not None:
    cov = cov[len(spikes1):, :len(spikes2)]
  return cov


def correlation_coefficients(spikes1, spikes2=None, binsize_ms=500.0):
  """spike_metrics.py:15-25 (Pearson r of binned counts; NaN for silent
  trains, like Elephant)."""
  spikes = spikes1 if spikes2 is None else np.concatenate([spikes1, spikes2], 0)
  with np.errstate(invalid='ignore', divide='ignore'):
    r = np.atleast_2d(np.corrcoef(bin_counts(spikes, binsize_ms)))
  if spikes2 is not None:
    r = r[len(spikes1):, :len(spikes2)]
  return r


def spike_times(spikes):
  """spike_helper.py:8-20 (train_to_neo / trains_to_neo without Neo): per train
  the spike times in seconds (frame / 24 Hz); t_stop = T / 24 s."""
  spikes = np.asarray(spikes)
  assert spikes.ndim == 2
  return [np.nonzero(tr)[0] / float(FRAME_RATE) for tr in spikes]


def _exp_sum(a, b, tau):
  """sum_k sum_l exp(-|a_k - b_l| / tau)."""
  if len(a) == 0 or len(b) == 0:
    return 0.0
  return float(np.exp(-np.abs(a[:, None] - b[None, :]) / tau).sum())


def van_rossum_distance(spikes1, spikes2=None, tau=1.0):
  """spike_metrics.py:41-51 -> elephant.spike_train_dissimilarity.van_rossum_dist
  (tau = 1 s default [ext]).  Elephant evaluates the closed form of Houghton &
  Kreuz 2012 on the summed kernel matrix S_ab = sum_k sum_l exp(-|t_k - t_l| /
  tau) and returns D[i, j] = sqrt(S_ii + S_jj - S_ij - S_ji) -- the
  normalisation in which ONE spike against an empty train is at distance 1
  (trains convolved with sqrt(2 / tau) exp(-t / tau) H(t)), without the factor
  1/2 of the plain exp(-t / tau) kernel (round 3 carried that factor:
  van_rossum_heatmap_min in spike_metrics.json was off by sqrt(2); the KL
  statistics do not depend on the normalisation).  Returns the full matrix, or
  the (spikes2 x spikes1) cross block exactly as the reference slices it
  (result[len(spikes1):, :len(spikes2)]).  PARITY UNPINNED (Elephant absent:
  the formula is restated from its published source, not run)."""
  spikes = np.asarray(spikes1) if spikes2 is None else np.concatenate(
      [np.asarray(spikes1), np.asarray(spikes2)], 0)
  # S = A E A^T: E the kernel between ALL spikes of the batch, A the train
  # membership (one matrix product instead of n^2 python-level pair sums: a
  # 102-neuron trial is 5 000 pairs)
  owner, frame = np.nonzero(spikes)
  n = len(spikes)
  t = frame / float(FRAME_RATE)
  E = np.exp(-np.abs(t[:, None] - t[None, :]) / tau)
  A = np.zeros((n, len(t)), np.float64)
  A[owner, np.arange(len(t))] = 1.0
  S = A @ E @ A.T
  d2 = np.diag(S)[:, None] + np.diag(S)[None, :] - 2.0 * S
  result = np.sqrt(np.maximum(d2, 0.0))
  if spikes2 is not None:
    result = result[len(spikes1):, :len(spikes2)]
  return result


def van_rossum_gram_frames(spikes, decay):
  """The summed kernel matrix of `van_rossum_distance` on the frame grid, without
  the kernel between all pairs of spikes: float64 (n, n)
    S_ij = sum_{k in i, l in j} decay^|f_k - f_l| = G_ij + G_ji,  G = M' Sp^T
  with Sp the (n, T) trains and M' the half-weighted causal filter -- per train
  and frame h = s[t] / 2, m' = fl(fl(decay m) + h), M'[t] = m', m = fl(m' + h),
  m = 0 before frame 0, every operation rounded to float64 on its own.  The half
  weights count equal-frame pairs once; the diagonal is S_ii = n_i + 2 sum_{k<l}
  decay^(f_l - f_k).  O(T n^2) and no memory beyond the trial; the statement
  cg_van_rossum (csrc/van_rossum.hip) is tested against: its M' are these bits,
  only the order of the sum over frames differs.  decay 1, 0 and (T <= 40) 0.5
  make every sum exact."""
  s = (np.asarray(spikes) != 0).astype(np.float64)
  assert s.ndim == 2
  n, T = s.shape
  a = np.float64(decay)
  filt = np.empty((n, T), np.float64)
  m = np.zeros(n, np.float64)
  for t in range(T):
    h = 0.5 * s[:, t]
    mp = a * m
    mp = mp + h
    filt[:, t] = mp
    m = mp + h
  G = filt @ s.T
  return G + G.T


def van_rossum_decay(tau=1.0):
  """exp(-1 / (24 tau)): the kernel's decay over one frame, as the host forms it
  for `van_rossum_distance_frames` and for the device call alike."""
  return math.exp(-1.0 / (FRAME_RATE * tau))


def _distance_from_gram(S):
  d = np.diag(S)
  d2 = (d[:, None] + d[None, :]) - 2.0 * S
  return np.sqrt(np.maximum(d2, 0.0))


def van_rossum_distance_frames(spikes1, spikes2=None, tau=1.0):
  """`van_rossum_distance` from `van_rossum_gram_frames`: D_ij =
  sqrt(max(fl(fl(S_ii + S_jj) - 2 S_ij), 0)), the same normalisation (one spike
  against an empty train is at distance 1), the full matrix or the (spikes2 x
  spikes1) cross block sliced exactly as `van_rossum_distance` slices it."""
  spikes = np.asarray(spikes1) if spikes2 is None else np.concatenate(
      [np.asarray(spikes1), np.asarray(spikes2)], 0)
  result = _distance_from_gram(
      van_rossum_gram_frames(spikes, van_rossum_decay(tau)))
  if spikes2 is not None:
    result = result[len(spikes1):, :len(spikes2)]
  return result


def correlation_coefficients_exact(spikes1, spikes2=None, binsize_ms=500.0):
  """`correlation_coefficients` from exact integer sums (what cg_spike_corrcoef
  computes): with the bin counts n_i, S_i = sum n_i, S_ij = sum n_i n_j and nb
  bins, num = nb S_ij - S_i S_j and v_i = nb S_ii - S_i^2 are 64-bit integers,
  converted to float64 exactly BEFORE the product v_i v_j (which does not fit in
  64 bits at large T), and r_ij = num / sqrt(v_i v_j).  NaN where a train's
  counts do not vary, like np.corrcoef; the diagonal is exactly 1 elsewhere."""
  spikes = np.asarray(spikes1) if spikes2 is None else np.concatenate(
      [np.asarray(spikes1), np.asarray(spikes2)], 0)
  counts = np.atleast_2d(bin_counts(spikes != 0, binsize_ms)).astype(np.int64)
  nb = counts.shape[-1]
  sums = counts.sum(-1)
  num = nb * (counts @ counts.T) - sums[:, None] * sums[None, :]
  v = np.diag(num).astype(np.float64)
  with np.errstate(invalid='ignore', divide='ignore'):
    r = num.astype(np.float64) / np.sqrt(v[:, None] * v[None, :])
  if spikes2 is not None:
    r = r[len(spikes1):, :len(spikes2)]
  return r


def victor_purpura_distance(spikes1, spikes2=None, q=1.0):
  """spike_metrics.py:54-63 -> elephant victor_purpura_dist (q = 1 Hz default
  [ext]): minimal cost of turning one train into the other with insert / delete
  (cost 1) and shifts (cost q |dt|); dynamic programme of Victor & Purpura 1996.
  PARITY UNPINNED."""
  spikes = np.asarray(spikes1) if spikes2 is None else np.concatenate(
      [np.asarray(spikes1), np.asarray(spikes2)], 0)
  times = spike_times(spikes)
  n = len(times)
  result = np.zeros((n, n), np.float64)
  for i in range(n):
    for j in range(i + 1, n):
      a, b = times[i], times[j]
      G = np.zeros((len(a) + 1, len(b) + 1))
      G[:, 0] = np.arange(len(a) + 1)
      G[0, :] = np.arange(len(b) + 1)
      for k in range(1, len(a) + 1):
        for l in range(1, len(b) + 1):
          G[k, l] = min(G[k - 1, l] + 1, G[k, l - 1] + 1,
                        G[k - 1, l - 1] + q * abs(a[k - 1] - b[l - 1]))
      result[i, j] = result[j, i] = G[-1, -1]
  if spikes2 is not None:
    result = result[len(spikes1):, :len(spikes2)]
  return result



def victor_purpura_cost(q=1.0):
  """q / 24: the cost of shifting a spike by one frame, as the host forms it for
  `victor_purpura_distance_frames` and for the device call alike."""
  return float(q) / FRAME_RATE


def victor_purpura_distance_frames(spikes1, spikes2=None, q=1.0):
  """`victor_purpura_distance` on the frame grid, in float64, every operation
  rounded on its own: with f_i the ascending frame indices of the non-zero
  entries of train i, n_i their number and qf = victor_purpura_cost(q),
    G[k][0] = k, G[0][l] = l,
    G[k][l] = min(G[k-1][l] + 1, G[k][l-1] + 1,
                  G[k-1][l-1] + fl(qf |f_a[k-1] - f_b[l-1]|)),   D_ab = G[n_a][n_b]
  (the frame difference an exact integer).  `victor_purpura_distance` forms
  q |t_k - t_l| from times in seconds instead: the two agree to rounding.  The
  statement cg_victor_purpura (csrc/victor_purpura.hip) is tested against bit
  for bit -- the programme only adds and takes minima of non-NaN values, so the
  order in which the cells are visited does not matter.  Here all pairs of the
  trial go through one sweep over the anti-diagonals k + l = d, padded to the
  longest train (the padding never feeds a cell that counts) and sorted so that
  the pairs still short of their last diagonal n_a + n_b are a prefix.  The full
  matrix (symmetric, diagonal 0), or the (spikes2 x spikes1) cross block sliced
  exactly as `victor_purpura_distance` slices it."""
  spikes = np.asarray(spikes1) if spikes2 is None else np.concatenate(
      [np.asarray(spikes1), np.asarray(spikes2)], 0)
  s = spikes != 0
  assert s.ndim == 2
  n = len(s)
  qf = victor_purpura_cost(q)
  counts = s.sum(1).astype(np.int64)
  N = int(counts.max()) if n else 0
  result = np.zeros((n, n), np.float64)
  I, J = np.triu_indices(n, k=1)
  if len(I):
    order = np.argsort(-(counts[I] + counts[J]), kind='stable')
    I, J = I[order], J[order]
    na, total = counts[I], counts[I] + counts[J]
    frames = np.zeros((n, max(N, 1)), np.int64)
    for i, train in enumerate(s):
      frames[i, :counts[i]] = np.nonzero(train)[0]
    A = frames[I]                  # A[p, k - 1] = f_a[k - 1]
    Brev = frames[J][:, ::-1]      # Brev[p, N - l] = f_b[l - 1]
    # pairs with n_a + n_b >= d: the first m_ge[d]
    m_ge = np.bincount(total, minlength=2 * N + 2)[::-1].cumsum()[::-1]
    out = np.zeros(len(I), np.float64)
    # g[p, k] = G[k][d - k] of pair p on the diagonal d; d = 0: G[0][0] = 0
    g1 = np.zeros((len(I), N + 1), np.float64)
    g2 = None
    for d in range(1, int(total[0]) + 1):
      m = int(m_ge[d])
      g = np.empty((m, N + 1), np.float64)
      if d <= N:
        g[:, 0] = d
        g[:, d] = d
      k0, k1 = max(1, d - N), min(N, d - 1)
      if k0 <= k1:
        up = g1[:m, k0 - 1:k1] + 1.0
        left = g1[:m, k0:k1 + 1] + 1.0
        df = np.abs(A[:m, k0 - 1:k1] - Brev[:m, N - d + k0:N - d + k1 + 1])
        shift = g2[:m, k0 - 1:k1] + qf * df.astype(np.float64)
        g[:, k0:k1 + 1] = np.minimum(np.minimum(up, left), shift)
      last = int(m_ge[d + 1])      # pairs [last, m) end on this diagonal
      out[last:m] = g[np.arange(last, m), na[last:m]]
      g2, g1 = g1, g
    result[I, J] = out
    result[J, I] = out
  if spikes2 is not None:
    result = result[len(spikes1):, :len(spikes2)]
  return result


# -- a batch of trials at once: the statistics compute_dg_metrics.py reports ----
def batch_statistics(spikes):
  """(rates (B, C), covariances (B, C (C + 1) / 2)) float32 of a batch of binary
  trains (B, T, C): per trial what compute_dg_metrics.get_data_statistics stores
  -- `mean_firing_rate` and the upper triangle (np.triu_indices order) of
  `covariance` of the (C, T) float32 trains."""
  spikes = np.asarray(spikes)
  B, _, C = spikes.shape
  rates = np.zeros((B, C), np.float32)
  covs = np.zeros((B, C * (C + 1) // 2), np.float32)
  iu = np.triu_indices(C)
  for b in range(B):
    trial = spikes[b].T.astype(np.float32)
    rates[b] = mean_firing_rate(trial)
    covs[b] = np.nan_to_num(covariance(trial)[iu])
  return rates, covs


def error_sums(rates_a, rates_b, covs_a, covs_b):
  """float64 (4,): sum |d| and sum d^2 of the firing rates, then of the
  covariances -- the sums behind compute_dg_metrics.report (sums, not means: an
  epoch is formed from its batches)."""
  dr = np.asarray(rates_a, np.float64) - np.asarray(rates_b, np.float64)
  dc = np.asarray(covs_a, np.float64) - np.asarray(covs_b, np.float64)
  return np.array([np.abs(dr).sum(), np.square(dr).sum(), np.abs(dc).sum(),
                   np.square(dc).sum()])


def report_from_sums(sums, n_rates, n_covs):
  """The four figures main.py --spike_metrics logs, by the definitions of
  compute_dg_metrics.report over n_rates / n_covs compared values.  (MAPE is
  a per-trial quantity, not a sum over values: not formed here.)"""
  s = [float(v) for v in sums]
  return {
      'spike_metrics/firing_rate_mae': s[0] / n_rates,
      'spike_metrics/firing_rate_rmse': float(np.sqrt(s[1] / n_rates)),
      'spike_metrics/covariance_mae': s[2] / n_covs,
      'spike_metrics/covariance_mse': s[3] / n_covs,
  }


def batch_statistics_device(spikes):
  """`batch_statistics` on the GPU (cg_spike_stats): float32 device tensor
  (B, T, C) of {0, 1}, any strides, -> device (rates (B, C), covariances
  (B, C (C + 1) / 2)) float32.  Rates equal the host's float32; covariances are
  the exact integer sums divided once (the host's float64 np.cov rounds more
  often: equal to ~1e-7 relative)."""
  import torch
  from ... import _lib as hip
  B, T, C = _trial_batch(spikes)
  rates = torch.empty(B, C, dtype=torch.float32, device=spikes.device)
  covs = torch.empty(B, C * (C + 1) // 2, dtype=torch.float32,
                     device=spikes.device)
  hip.call('cg_spike_stats', spikes, B, T, C, spikes.stride(0),
           spikes.stride(1), spikes.stride(2), rates, covs, hip.stream())
  return rates, covs


def error_sums_device(rates_a, rates_b, covs_a, covs_b):
  """`error_sums` on the GPU (cg_spike_stats_error): float32 device (4,), an
  ordered two-stage reduction -- the same bits every call."""
  import torch
  from ... import _lib as hip
  ts = [rates_a, rates_b, covs_a, covs_b]
  if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
             for t in ts):
    raise ValueError('contiguous float32 device tensors expected')
  if rates_a.shape != rates_b.shape or covs_a.shape != covs_b.shape:
    raise ValueError('the two sets of statistics differ in shape')
  n_r, n_c = rates_a.numel(), covs_a.numel()
  dev = rates_a.device
  ws = torch.empty(hip.load().cg_spike_stats_error_ws_elems(n_r, n_c),
                   dtype=torch.float32, device=dev)
  out = torch.empty(4, dtype=torch.float32, device=dev)
  hip.call('cg_spike_stats_error', rates_a, rates_b, n_r, covs_a, covs_b, n_c,
           out, ws, hip.stream())
  return out


# frames per LDS chunk of cg_van_rossum (csrc/van_rossum.hip: kVrChunk) -- the
# tests put spikes on both sides of every chunk boundary
VAN_ROSSUM_CHUNK = 16


def _trial_batch(spikes, shape='(B, T, C)'):
  """The shape of a batch of trials as every device wrapper takes it."""
  import torch
  if not (torch.is_tensor(spikes) and spikes.is_cuda and
          spikes.dtype == torch.float32 and spikes.dim() == 3):
    raise ValueError('float32 device tensor {} expected'.format(shape))
  return spikes.shape


def _host(x):
  """A device tensor, or anything numpy takes, as a host array; None stays."""
  return None if x is None else np.asarray(x.cpu() if hasattr(x, 'cpu') else x)


def van_rossum_distance_device(spikes, tau=1.0, return_gram=False):
  """`van_rossum_distance_frames` of every trial of a batch on the GPU
  (cg_van_rossum): float32 device tensor (B, T, C) of {0, 1}, any strides, ->
  float64 device (B, C, C) distances between the trial's neurons; return_gram:
  (distances, summed kernel matrices S).  The decay exp(-1 / (24 tau)) is formed
  here on the host.  Symmetric bit for bit, diagonal exactly 0, the same bits
  every call."""
  import torch
  from ... import _lib as hip
  B, T, C = _trial_batch(spikes)
  dist = torch.empty(B, C, C, dtype=torch.float64, device=spikes.device)
  gram = torch.empty_like(dist) if return_gram else None
  hip.call('cg_van_rossum', spikes, B, T, C, spikes.stride(0), spikes.stride(1),
           spikes.stride(2), van_rossum_decay(tau), gram, dist, hip.stream())
  return (dist, gram) if return_gram else dist


def correlation_coefficients_device(spikes):
  """`correlation_coefficients_exact` of every trial of a batch on the GPU
  (cg_spike_corrcoef): float32 device tensor (B, T, C) of {0, 1}, any strides,
  -> float64 device (B, C, C); NaN where a train's bin counts do not vary."""
  import torch
  from ... import _lib as hip
  B, T, C = _trial_batch(spikes)
  corr = torch.empty(B, C, C, dtype=torch.float64, device=spikes.device)
  hip.call('cg_spike_corrcoef', spikes, B, T, C, spikes.stride(0),
           spikes.stride(1), spikes.stride(2), corr, hip.stream())
  return corr


def victor_purpura_distance_device(spikes, q=1.0):
  """`victor_purpura_distance_frames` of every trial of a batch on the GPU
  (cg_victor_purpura): float32 device tensor (B, T, C), non-zero a spike, any
  strides, -> float64 device (B, C, C), the statement's bits.  The cost q / 24
  of a frame is formed here on the host; the workspace (frame indices, counts
  and boundary columns) is allocated per call and needs no initialisation.  No
  host synchronisation."""
  import torch
  from ... import _lib as hip
  B, T, C = _trial_batch(spikes)
  ws = hip.workspace('cg_victor_purpura_ws_bytes', spikes.device, B, T, C)
  dist = torch.empty(B, C, C, dtype=torch.float64, device=spikes.device)
  hip.call('cg_victor_purpura', spikes, B, T, C, spikes.stride(0),
           spikes.stride(1), spikes.stride(2), victor_purpura_cost(q), dist, ws,
           ws.numel(), hip.stream())
  return dist


# -- the histogram counts behind the KL figures of compute_metrics.py ------------
def pair_histograms(real, fake, num_bins=30):
  """What pandas.cut(pooled, bins=num_bins) makes of every (recorded, synthetic)
  pair, as integer counts: float64 host arrays (P, C, C) -> (counts (P, 2,
  num_bins) int32, valid (P, 2) int32, edges (P, num_bins + 1) float64, status
  (P,) int32).  Side 0 of pair p is the set of real[p][i][j], i < j, that are not
  NaN (compute_metrics._upper), side 1 the same from fake; valid holds the two
  set sizes.  With mn, mx the pooled minimum and maximum (a zero maximum taken
  as +0: numpy's own choice between the zeros depends on its reduction order),
    mn == mx:  mn -= (0.001 |mn| if mn != 0 else 0.001),
               mx += (0.001 |mx| if mx != 0 else 0.001)
    otherwise: adj = (mx - mn) 0.001
    step = (mx - mn) / num_bins
    e[k] = fl(fl(k step) + mn)   (step == 0: fl(fl(fl(k / num_bins) (mx - mn)) + mn))
    e[num_bins] = mx;  mn != mx: e[0] -= adj
    id(x) = number of edges < x;  x counts in bin id - 1 when 1 <= id <= num_bins
  -- pandas.core.reshape.tile._nbins_to_bins and _bins_to_cuts with right=True
  and np.linspace restated, every operation rounded to float64 on its own.
  status is a bit set: 1 a side is empty, 2 a pooled value is infinite, 4 two
  edges coincide (looked for only when there is a value and none is infinite);
  pandas raises ValueError for 2 and 4.  With status != 0 the pair's counts and
  edges are zeros.  The statement cg_pair_histogram (csrc/pair_hist.hip) is
  tested against, bit for bit.  No pandas here."""
  real, fake = np.asarray(real), np.asarray(fake)
  if not (real.dtype == fake.dtype == np.float64 and real.ndim == 3 and
          real.shape == fake.shape and real.shape[1] == real.shape[2] >= 2):
    raise ValueError('two float64 arrays (P, C, C), C >= 2, expected')
  num_bins = int(num_bins)
  if num_bins < 1:
    raise ValueError('num_bins < 1')
  P, C = real.shape[:2]
  iu = np.triu_indices(C, k=1)
  counts = np.zeros((P, 2, num_bins), np.int32)
  valid = np.zeros((P, 2), np.int32)
  edges = np.zeros((P, num_bins + 1), np.float64)
  status = np.zeros((P,), np.int32)
  k = np.arange(num_bins + 1).astype(np.float64)
  for p in range(P):
    sides = [m[iu] for m in (real[p], fake[p])]
    sides = [s[~np.isnan(s)] for s in sides]
    valid[p] = [len(s) for s in sides]
    pooled = np.concatenate(sides)
    st = 1 if min(len(s) for s in sides) == 0 else 0
    if len(pooled) and np.isinf(pooled).any():
      st |= 2
    if len(pooled) and not st & 2:
      mn, mx = np.float64(pooled.min()), np.float64(pooled.max()) + 0.0
      flat = mn == mx
      with np.errstate(over='ignore', invalid='ignore'):
        if flat:
          mn = mn - (0.001 * abs(mn) if mn != 0 else 0.001)
          mx = mx + (0.001 * abs(mx) if mx != 0 else 0.001)
        else:
          adj = (mx - mn) * 0.001
        delta = mx - mn
        step = delta / np.float64(num_bins)
        e = (k / np.float64(num_bins)) * delta if step == 0 else k * step
        e = e + mn
        e[num_bins] = mx
        if not flat:
          e[0] = e[0] - adj
      if np.any(e[1:] == e[:-1]):
        st |= 4
    status[p] = st
    if st == 0:
      edges[p] = e
      for s, x in enumerate(sides):
        ids = np.searchsorted(e, x, side='left')
        ids = ids[(ids >= 1) & (ids <= num_bins)]
        counts[p, s] = np.bincount(ids - 1, minlength=num_bins)
  return counts, valid, edges, status


def pair_histograms_device(real, fake, num_bins=30, return_edges=True):
  """`pair_histograms` on the GPU (cg_pair_histogram): float64 device tensors
  (P, C, C), any strides, -> device (counts int32 (P, 2, num_bins), valid int32
  (P, 2), edges float64 (P, num_bins + 1) or None without return_edges, status
  int32 (P,)), the statement's bits.  One launch, no workspace, nothing zeroed
  beforehand, no host synchronisation."""
  import torch
  from ... import _lib as hip
  ok = all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and
           t.dim() == 3 for t in (real, fake))
  if not (ok and real.shape == fake.shape and real.shape[1] == real.shape[2] and
          real.device == fake.device):
    raise ValueError('two float64 device tensors (P, C, C) expected')
  P, C = real.shape[:2]
  num_bins = int(num_bins)
  dev = real.device
  counts = torch.empty(P, 2, num_bins, dtype=torch.int32, device=dev)
  valid = torch.empty(P, 2, dtype=torch.int32, device=dev)
  status = torch.empty(P, dtype=torch.int32, device=dev)
  edges = (torch.empty(P, num_bins + 1, dtype=torch.float64, device=dev)
           if return_edges else None)
  hip.call('cg_pair_histogram', real, real.stride(0), real.stride(1),
           real.stride(2), fake, fake.stride(0), fake.stride(1), fake.stride(2),
           P, C, num_bins, counts, valid, edges, status, hip.stream())
  return counts, valid, edges, status


# -- pattern probabilities of the surrogate experiment ---------------------------
# (compute_surrogate_metrics.py; csrc/patterns.hip)
PATTERN_MAX_BITS = 24   # CG_PATTERN_HIST_MAX_BITS: 2^24 int64 counts are 128 MB
PATTERN_SCORE_BITS = 16  # the marginal / pair figures of pattern_scores


def pattern_codes(spikes):
  """int64 (N,): the binary pattern of every sample of (N, T, C), any dtype and
  any strides (a transposed view is walked in place): a frame is a spike when it
  is != 0 (so a NaN is one and -0.0 is none), and
    code[n] = sum_{t, c} [spikes[n, t, c] != 0] << (t C + c)."""
  spikes = np.asarray(spikes)
  if spikes.ndim != 3:
    raise ValueError('(N, T, C) expected')
  N, T, C = spikes.shape
  if T * C > 62:
    raise ValueError('T C = {} bits do not fit an int64 code'.format(T * C))
  codes = np.zeros(N, np.int64)
  for t in range(T):
    for c in range(C):
      codes |= (spikes[:, t, c] != 0).astype(np.int64) << (t * C + c)
  return codes


def pattern_histogram(spikes):
  """int64 (2^K,), K = T C: the number of samples of (N, T, C) with each
  `pattern_codes` code.  The statement cg_pattern_histogram (csrc/patterns.hip)
  is tested against, for equality.  K > 24 is refused."""
  spikes = np.asarray(spikes)
  if spikes.ndim != 3:
    raise ValueError('(N, T, C) expected')
  K = spikes.shape[1] * spikes.shape[2]
  if not 1 <= K <= PATTERN_MAX_BITS:
    raise ValueError('T C = {} bits: 1 .. {} supported'.format(
        K, PATTERN_MAX_BITS))
  return np.bincount(pattern_codes(spikes), minlength=1 << K).astype(np.int64)


def pattern_histogram_device(spikes):
  """`pattern_histogram` on the GPU (cg_pattern_histogram): float32 device tensor
  (N, T, C), any strides, -> device int64 (2^K,), the statement's counts.
  Nothing is zeroed beforehand (the call's first launch does it), no host
  synchronisation."""
  import torch
  from ... import _lib as hip
  N, T, C = _trial_batch(spikes, '(N, T, C)')
  # (refused: N < 1 or T C outside 1 .. PATTERN_MAX_BITS)
  ws = hip.workspace('cg_pattern_hist_ws_bytes', spikes.device, N, T, C)
  counts = torch.empty(1 << (T * C), dtype=torch.int64, device=spikes.device)
  hip.call('cg_pattern_histogram', spikes, N, T, C, spikes.stride(0),
           spikes.stride(1), spikes.stride(2), counts, ws,
           0 if ws is None else ws.numel(), hip.stream())
  return counts


def _pattern_moments(q, K):
  """(marginals (K,), covariances (K, K)) of the bits under the code
  probabilities q (2^K,): E[b_i] and E[b_i b_j] - E[b_i] E[b_j]."""
  bits = ((np.arange(1 << K)[:, None] >> np.arange(K)[None, :]) & 1).astype(
      np.float64)
  mean = q @ bits
  second = bits.T @ (q[:, None] * bits)
  return mean, second - mean[:, None] * mean[None, :]


def _js_divergence_bits(p, q):
  """Jensen-Shannon divergence in bits of two float64 probability vectors: 1/2
  sum p log2(p / m) + 1/2 sum q log2(q / m), m = (p + q) / 2; a term with a zero
  numerator is 0."""
  m = (p + q) / 2.0
  js = 0.0
  for side in (p, q):
    on = side > 0
    js += 0.5 * float(np.sum(side[on] * np.log2(side[on] / m[on])))
  return js


def pattern_scores(ref_counts, counts):
  """How far the pattern probabilities q = counts / sum(counts) are from p =
  ref_counts / sum(ref_counts); both integer (2^K,).  Host float64, whichever
  device counted:
    js_divergence_bits       1/2 sum p log2(p / m) + 1/2 sum q log2(q / m), m =
                             (p + q) / 2; a term with a zero numerator is 0
    log_prob_correlation     Pearson r of log10 p against log10 q over the codes
                             present on both sides; NaN with fewer than two
    unseen_mass              sum of q over the codes with ref_counts == 0
    patterns_seen            [codes in ref_counts, codes in counts]
    firing_probability_mae   mean |difference| of the K per-bit marginals
    pair_covariance_mae      mean |difference| of the covariances of the bit
                             pairs i < j (NaN for K = 1)
  the last two formed from the counts, for K <= 16 only (None above)."""
  ref = np.asarray(ref_counts)
  cnt = np.asarray(counts)
  if not (ref.ndim == 1 and ref.shape == cnt.shape and len(ref) >= 2 and
          len(ref) & (len(ref) - 1) == 0):
    raise ValueError('two count vectors (2^K,) expected')
  if ref.sum() <= 0 or cnt.sum() <= 0 or (ref < 0).any() or (cnt < 0).any():
    raise ValueError('counts must be non-negative and not all zero')
  K = len(ref).bit_length() - 1
  p = ref.astype(np.float64) / float(ref.sum())
  q = cnt.astype(np.float64) / float(cnt.sum())
  js = _js_divergence_bits(p, q)
  both = (ref > 0) & (cnt > 0)
  r = float('nan')
  if both.sum() >= 2:
    with np.errstate(invalid='ignore', divide='ignore'):
      r = float(np.corrcoef(np.log10(p[both]), np.log10(q[both]))[0, 1])
  scores = {
      'js_divergence_bits': js,
      'log_prob_correlation': r,
      'unseen_mass': float(q[ref == 0].sum()),
      'patterns_seen': [int((ref > 0).sum()), int((cnt > 0).sum())],
      'firing_probability_mae': None,
      'pair_covariance_mae': None,
  }
  if K <= PATTERN_SCORE_BITS:
    mean_p, cov_p = _pattern_moments(p, K)
    mean_q, cov_q = _pattern_moments(q, K)
    iu = np.triu_indices(K, k=1)
    scores['firing_probability_mae'] = float(np.mean(np.abs(mean_p - mean_q)))
    scores['pair_covariance_mae'] = (
        float(np.mean(np.abs(cov_p[iu] - cov_q[iu]))) if K > 1 else float('nan'))
  return scores


# -- structure across time: cross-correlograms and population counts ------------
# (compute_metrics.py --temporal_metrics; csrc/spike_ccg.hip)
CCG_MAX_NEURONS = 1024  # CG_CCG_MAX_C
CCG_MAX_LAG = 256       # CG_CCG_MAX_LAG


def _binary_trials(spikes):
  spikes = np.asarray(spikes)
  if spikes.ndim != 3:
    raise ValueError('(B, T, C) expected')
  # != 0: a NaN is a spike, -0.0 is not
  return (spikes != 0).astype(np.int64)


def cross_correlogram(spikes, max_lag):
  """int64 (B, max_lag + 1, C, C) of trials (B, T, C), a frame a spike when it is
  != 0:
    ccg[b][tau][i][j] = sum_{t = 0}^{T - 1 - tau} s_i(t) s_j(t + tau)
  -- how often neuron j fires tau frames after neuron i.  ccg[b][0][i][i] is the
  spike count n_i, ccg[b][tau][i][i] the autocorrelogram; a lag tau >= T gives
  zeros.  One integer matrix product per lag; the statement cg_spike_ccg
  (csrc/spike_ccg.hip) is tested against, for equality."""
  s = _binary_trials(spikes)
  max_lag = int(max_lag)
  if max_lag < 0:
    raise ValueError('max_lag < 0')
  B, T, C = s.shape
  out = np.zeros((B, max_lag + 1, C, C), np.int64)
  for tau in range(min(max_lag, T - 1) + 1):
    # (B, C, T - tau) @ (B, T - tau, C)
    out[:, tau] = np.matmul(s[:, :T - tau].transpose(0, 2, 1), s[:, tau:])
  return out


def population_count_histogram(spikes):
  """int64 (B, C + 1) of trials (B, T, C): hist[b][k] is the number of frames of
  trial b in which exactly k neurons fire; every row sums to T.  The statement
  cg_spike_population_hist is tested against."""
  s = _binary_trials(spikes)
  B, _, C = s.shape
  out = np.zeros((B, C + 1), np.int64)
  for b in range(B):
    out[b] = np.bincount(s[b].sum(-1), minlength=C + 1)
  return out


def cross_correlogram_device(spikes, max_lag):
  """`cross_correlogram` on the GPU (cg_spike_ccg): float32 device tensor
  (B, T, C), any strides, -> int32 device (B, max_lag + 1, C, C), the
  statement's integers (T <= 2^24, C <= 1024, max_lag <= 256).  One launch, no
  workspace, nothing zeroed beforehand, no host synchronisation."""
  import torch
  from ... import _lib as hip
  B, T, C = _trial_batch(spikes)
  max_lag = int(max_lag)
  if not 0 <= max_lag <= CCG_MAX_LAG:
    raise ValueError('max_lag = {}: 0 .. {} supported'.format(max_lag,
                                                              CCG_MAX_LAG))
  ccg = torch.empty(B, max_lag + 1, C, C, dtype=torch.int32,
                    device=spikes.device)
  hip.call('cg_spike_ccg', spikes, B, T, C, spikes.stride(0), spikes.stride(1),
           spikes.stride(2), max_lag, ccg, hip.stream())
  return ccg


def population_count_histogram_device(spikes):
  """`population_count_histogram` on the GPU (cg_spike_population_hist): float32
  device tensor (B, T, C), any strides, -> int32 device (B, C + 1).  One launch,
  no host synchronisation."""
  import torch
  from ... import _lib as hip
  B, T, C = _trial_batch(spikes)
  hist = torch.empty(B, C + 1, dtype=torch.int32, device=spikes.device)
  hip.call('cg_spike_population_hist', spikes, B, T, C, spikes.stride(0),
           spikes.stride(1), spikes.stride(2), hist, hip.stream())
  return hist


def temporal_totals(spikes, max_lag):
  """(ccg (max_lag + 1, C, C), hist (C + 1,), trials): `cross_correlogram` and
  `population_count_histogram` of trials (B, T, C) summed over the trials, int64,
  and B."""
  B, _, C = np.shape(spikes)
  ccg = np.zeros((int(max_lag) + 1, C, C), np.int64)
  hist = np.zeros((C + 1,), np.int64)
  for i in range(0, B, 16):  # (the per-trial correlograms of 16 trials at a time)
    ccg += cross_correlogram(spikes[i:i + 16], max_lag).sum(0)
    hist += population_count_histogram(spikes[i:i + 16]).sum(0)
  return ccg, hist, int(B)


def temporal_totals_device(spikes, max_lag, group_bytes=256 << 20):
  """`temporal_totals` on the GPU: float32 device tensor (B, T, C) -> (device
  int64 ccg (max_lag + 1, C, C), device int64 hist (C + 1,), B).  The batch is
  walked in groups of as many trials as have their int32 correlograms fit in
  `group_bytes` (one at least); integer sums, so the grouping does not show.
  No host synchronisation."""
  import torch
  B, T, C = _trial_batch(spikes)
  max_lag = int(max_lag)
  per_trial = (max_lag + 1) * C * C * 4
  group = max(int(group_bytes) // per_trial, 1)
  ccg = torch.zeros(max_lag + 1, C, C, dtype=torch.int64, device=spikes.device)
  hist = torch.zeros(C + 1, dtype=torch.int64, device=spikes.device)
  for i in range(0, B, group):
    part = spikes[i:i + group]
    ccg += cross_correlogram_device(part, max_lag).sum(0, dtype=torch.int64)
    hist += population_count_histogram_device(part).sum(0, dtype=torch.int64)
  return ccg, hist, int(B)


def _pearson(a, b):
  """Pearson r of two float64 vectors, NaN with fewer than two values or no
  variance on a side.  sum(da db) / sqrt(sum(da^2) sum(db^2)): exactly 1 for
  equal vectors (sqrt(fl(x x)) == x)."""
  if len(a) < 2:
    return float('nan')
  da, db = a - np.mean(a), b - np.mean(b)
  va, vb = float(da @ da), float(db @ db)
  if va == 0 or vb == 0:
    return float('nan')
  return float(da @ db) / math.sqrt(va * vb)


def _mean_abs_difference(a, b):
  return float(np.mean(np.abs(a - b))) if np.size(a) else float('nan')


def temporal_scores(ref, other, T):
  """How far the structure across time of `other` is from that of `ref`; both
  `temporal_totals` (or `temporal_totals_device`, brought to the host) of trials
  of T frames with the same C and max_lag.  Host float64, whichever device
  counted.  Per side, with N trials, n_i = ccg[0][i][i] and p_i = n_i / (N T):
    autocorrelogram_mae        mean |difference| of A_i(tau) = ccg[tau][i][i] / n_i
                               over tau = 1 .. max_lag and the neurons with n_i > 0
                               on both sides; NaN when there is no such value
    lag_covariance_mae         mean |difference| of cov_ij = ccg[1][i][j] / (N (T -
    lag_covariance_correlation 1)) - p_i p_j over the ordered pairs i != j, and
                               the Pearson r between the two sides' values (NaN
                               with fewer than two pairs or no variance); both
                               NaN when max_lag < 1 or T < 2
    cross_correlogram_mae      mean |difference| of ccg[tau][i][j] / (N (T - tau))
                               over tau = 0 .. max_lag, tau < T, and i != j
    population_count_js_bits   Jensen-Shannon divergence in bits of the two
                               hist / sum(hist)
    population_count_mean      [ref, other] mean number of neurons firing in a
                               frame
    max_lag, num_trials        num_trials as [ref, other]"""
  sides = []
  for ccg, hist, n in (ref, other):
    ccg, hist = (np.asarray(a.cpu() if hasattr(a, 'cpu') else a).astype(np.int64)
                 for a in (ccg, hist))
    if not (ccg.ndim == 3 and ccg.shape[1] == ccg.shape[2] and
            hist.shape == (ccg.shape[1] + 1,) and int(n) >= 1 and
            hist.sum() > 0):
      raise ValueError('totals (ccg (L, C, C), hist (C + 1,), trials) expected')
    sides.append((ccg, hist, int(n)))
  T = int(T)
  if T < 1 or sides[0][0].shape != sides[1][0].shape:
    raise ValueError('the two sides differ in shape, or T < 1')
  L, C = sides[0][0].shape[:2]
  off = ~np.eye(C, dtype=bool)
  auto, cov, cross, pop, mean = [], [], [], [], []
  for ccg, hist, n in sides:
    count = np.diagonal(ccg[0]).astype(np.float64)
    p = count / (float(n) * T)
    with np.errstate(invalid='ignore', divide='ignore'):
      auto.append(np.stack([np.diagonal(ccg[tau]) for tau in range(1, L)]
                           ).astype(np.float64) / count if L > 1 else
                  np.zeros((0, C)))
    cov.append(ccg[1][off].astype(np.float64) / (float(n) * (T - 1)) -
               (p[:, None] * p[None, :])[off] if L > 1 and T > 1 else
               np.zeros(0))
    cross.append(np.concatenate(
        [ccg[tau][off].astype(np.float64) / (float(n) * (T - tau))
         for tau in range(min(L, T))]))
    pop.append(hist.astype(np.float64) / float(hist.sum()))
    mean.append(float(np.arange(C + 1) @ pop[-1]))
  fires = (np.diagonal(sides[0][0][0]) > 0) & (np.diagonal(sides[1][0][0]) > 0)
  return {
      'autocorrelogram_mae': _mean_abs_difference(auto[0][:, fires],
                                                  auto[1][:, fires]),
      'lag_covariance_mae': _mean_abs_difference(cov[0], cov[1]),
      'lag_covariance_correlation': _pearson(cov[0], cov[1]),
      'cross_correlogram_mae': _mean_abs_difference(cross[0], cross[1]),
      'population_count_js_bits': _js_divergence_bits(pop[0], pop[1]),
      'population_count_mean': mean,
      'max_lag': L - 1,
      'num_trials': [sides[0][2], sides[1][2]],
  }


# -- population states: precision, recall and coverage --------------------------
# (compute_metrics.py --state_metrics; csrc/state_neighbours.hip)
STATE_K_STEP = 32          # CG_STATE_K_STEP
STATE_MAX_K = 8            # CG_STATE_MAX_K
STATE_MAX_BIN = 127        # CG_STATE_MAX_BIN
STATE_MAX_NEURONS = 4096   # CG_STATE_MAX_C
STATE_EXACT_SUM = 1 << 24  # CG_STATE_EXACT_SUM: C bin^2 may not exceed it
STATE_NONE = 2**31 - 1     # CG_STATE_NONE: knn entry where fewer than k are admitted


def _state_bin(bin):
  bin = int(bin)
  if not 1 <= bin <= STATE_MAX_BIN:
    raise ValueError('bin = {}: 1 .. {} frames supported'.format(bin,
                                                                 STATE_MAX_BIN))
  return bin


def population_states(spikes, bin=12):
  """int32 (N nb, C) of trials (N, T, C), a frame a spike when it is != 0: row
  n nb + b holds the spike counts of the C neurons in frames b bin .. (b + 1)
  bin - 1 of trial n, nb = T // bin (a trailing partial bin is dropped, as
  `bin_counts` drops it; T < bin raises).  The population state of one bin."""
  s = _binary_trials(spikes)
  bin = _state_bin(bin)
  N, T, C = s.shape
  nb = T // bin
  if nb < 1:
    raise ValueError('trials of {} frames hold no bin of {}'.format(T, bin))
  return s[:, :nb * bin].reshape(N, nb, bin, C).sum(2).reshape(
      N * nb, C).astype(np.int32)


def _state_k(k):
  k = int(k)
  if not 1 <= k <= STATE_MAX_K:
    raise ValueError('k = {}: 1 .. {} supported'.format(k, STATE_MAX_K))
  return k


def state_neighbours(a, b, k, exclude_self=False, radius_b=None, chunk=1024):
  """Neighbour query of the states a (Sa, C) against the states b (Sb, C), with
  d2(x, y) = sum_c (x_c - y_c)^2, an integer:
    knn (Sa, k) int32     the k smallest d2(a_i, b_j) over the admitted j,
                          ascending; STATE_NONE where fewer than k are admitted
    within (Sa,) int32    #{admitted j : d2(a_i, b_j) <= radius_b[j]}, None
                          without radius_b (int (Sb,))
  Every j is admitted, except j == i with exclude_self (a and b the same set):
  by index, so a duplicate of a_i at another index counts, at distance 0.
  Walked in chunks of rows of a; the products are a float64 matmul of integers,
  exact below 2^53.  The statement cg_state_neighbours is tested against, for
  equality."""
  a, b = (np.asarray(x) for x in (a, b))
  k = _state_k(k)
  if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1] or not len(a) or \
      not len(b):
    raise ValueError('states (Sa, C) and (Sb, C) expected')
  if exclude_self and a.shape != b.shape:
    raise ValueError('exclude_self: a and b must be the same set')
  Sa, Sb = len(a), len(b)
  fa, fb = a.astype(np.float64), b.astype(np.float64)
  nb2 = (fb * fb).sum(1)
  if radius_b is not None:
    radius_b = np.asarray(radius_b).astype(np.int64)
    if radius_b.shape != (Sb,):
      raise ValueError('radius_b (Sb,) expected')
  knn = np.full((Sa, k), STATE_NONE, np.int32)
  within = None if radius_b is None else np.zeros((Sa,), np.int32)
  for i0 in range(0, Sa, int(chunk)):
    x = fa[i0:i0 + int(chunk)]
    d2 = ((x * x).sum(1)[:, None] + nb2[None, :] - 2.0 * (x @ fb.T)).astype(
        np.int64)
    admitted = np.ones(d2.shape, bool)
    if exclude_self:
      rows = np.arange(len(x))
      admitted[rows, i0 + rows] = False
    if within is not None:
      within[i0:i0 + len(x)] = ((d2 <= radius_b[None, :]) & admitted).sum(1)
    d2[~admitted] = STATE_NONE
    if Sb < k:
      d2 = np.concatenate(
          [d2, np.full((len(x), k - Sb), STATE_NONE, np.int64)], axis=1)
    knn[i0:i0 + len(x)] = np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1)
  return knn, within


class DeviceStates(object):
  """A set of states on the device as cg_population_states writes it: `tensor`
  bfloat16 (S, C rounded up to STATE_K_STEP) with zeros in the padding, the
  number of neurons C and the bin the counts came from."""
  __slots__ = ('tensor', 'C', 'bin')

  def __init__(self, tensor, C, bin):
    self.tensor, self.C, self.bin = tensor, int(C), int(bin)

  def __len__(self):
    return int(self.tensor.shape[0])

  @classmethod
  def cat(cls, parts):
    import torch
    parts = list(parts)
    if len({(p.C, p.bin) for p in parts}) != 1:
      raise ValueError('sets of one C and one bin expected')
    return cls(torch.cat([p.tensor for p in parts]), parts[0].C, parts[0].bin)

  def counts(self):
    """int32 device (S, C): the states as `population_states` holds them."""
    import torch
    return self.tensor[:, :self.C].to(torch.int32)


def population_states_device(spikes, bin=12):
  """`population_states` on the GPU (cg_population_states): float32 device
  tensor (B, T, C), any strides, read in place -> DeviceStates of B (T // bin)
  states.  One launch, no host synchronisation.  C bin^2 <= 2^24 and C <= 4096
  (the bound under which cg_state_neighbours is exact)."""
  import torch
  from ... import _lib as hip
  B, T, C = _trial_batch(spikes)
  bin = _state_bin(bin)
  if T < bin:
    raise ValueError('trials of {} frames hold no bin of {}'.format(T, bin))
  Cp = -(-C // STATE_K_STEP) * STATE_K_STEP
  states = torch.empty(B * (T // bin), Cp, dtype=torch.bfloat16,
                       device=spikes.device)
  hip.call('cg_population_states', spikes, B, T, C, spikes.stride(0),
           spikes.stride(1), spikes.stride(2), bin, states, hip.stream())
  return DeviceStates(states, C, bin)


def state_neighbours_device(a, b, k, exclude_self=False, radius_b=None,
                            knn=True):
  """`state_neighbours` on the GPU (cg_state_neighbours): DeviceStates a and b
  -> (knn int32 device (Sa, k) or None with knn=False, within int32 device (Sa,)
  or None without radius_b), the statement's integers.  radius_b: int32 (Sb,),
  a device tensor or anything numpy takes.  exclude_self needs `b is a` or the
  same tensor.  No Sa x Sb matrix exists anywhere; no host synchronisation."""
  import torch
  from ... import _lib as hip
  if not (isinstance(a, DeviceStates) and isinstance(b, DeviceStates)):
    raise ValueError('DeviceStates expected')
  if (a.C, a.bin) != (b.C, b.bin):
    raise ValueError('sets of one C and one bin expected')
  k = _state_k(k)
  ta, tb = a.tensor, b.tensor
  if not (ta.is_contiguous() and tb.is_contiguous()):
    raise ValueError('contiguous states expected')
  if exclude_self and not (ta.data_ptr() == tb.data_ptr() and
                           ta.shape == tb.shape):
    raise ValueError('exclude_self: a and b must be the same set')
  Sa, Sb = len(a), len(b)
  dev = ta.device
  if radius_b is not None:
    if not torch.is_tensor(radius_b):
      radius_b = torch.from_numpy(
          np.ascontiguousarray(np.asarray(radius_b).astype(np.int32)))
    radius_b = radius_b.to(device=dev, dtype=torch.int32).contiguous()
    if tuple(radius_b.shape) != (Sb,):
      raise ValueError('radius_b (Sb,) expected')
  elif not knn:
    raise ValueError('nothing asked for: knn=False without radius_b')
  ws = hip.workspace('cg_state_neighbours_ws_bytes', dev, Sa, Sb, a.C, a.bin, k,
                     least=16)
  out = torch.empty(Sa, k, dtype=torch.int32, device=dev) if knn else None
  within = (torch.empty(Sa, dtype=torch.int32, device=dev)
            if radius_b is not None else None)
  hip.call('cg_state_neighbours', ta, Sa, tb, Sb, a.C, a.bin, k,
           1 if exclude_self else 0, radius_b, out, within, ws, hip.stream())
  return out, within


def state_radii(states, k, neighbours=state_neighbours):
  """int32 (S,): the distance d2 from every state of the set to its k-th nearest
  other state of the set (self excluded by index).  The set needs more than k
  states."""
  k = _state_k(k)
  if len(states) <= k:
    raise ValueError('a set of {} states has no {}-th neighbour'.format(
        len(states), k))
  return _host(neighbours(states, states, k, exclude_self=True)[0])[
      :, k - 1].astype(np.int32)


def state_scores(ref, other, k, neighbours=state_neighbours, rad_ref=None):
  """Improved precision and recall (Kynkaanniemi et al. 2019) and coverage
  (Naeem et al. 2020) of the states `other` against the states `ref`, closed
  balls, integer distances.  neighbours(a, b, k, exclude_self=, radius_b=) ->
  (knn, within) is `state_neighbours` (sets as `population_states` gives them)
  or `state_neighbours_device` (DeviceStates); everything after the integers is
  host arithmetic, so both give the same dict bit for bit.  rad_ref:
  `state_radii(ref, k)` where the caller keeps it.
    precision         share of `other` states inside the ball of some ref state
    recall            share of ref states inside the ball of some `other` state
    coverage          share of ref states whose ball holds an `other` state
    exact_match       [share of ref states found in `other`, share of `other`
                      states found in ref] (nearest d2 = 0)
    nearest_distance  [median over ref of the distance to the nearest `other`
                      state, median over `other` of that to the nearest ref one]
    radius_median     [median ball radius of ref, of `other`]
    num_states        [S_ref, S_other]
  The ball of a state reaches to its k-th nearest other state of its own set.
  Both sets need more than k states (ValueError)."""
  k = _state_k(k)
  if len(ref) <= k or len(other) <= k:
    raise ValueError('both sets need more than k = {} states ({} and {})'
                     .format(k, len(ref), len(other)))
  if rad_ref is None:
    rad_ref = state_radii(ref, k, neighbours)
  rad_ref = np.asarray(rad_ref).astype(np.int32)
  rad_other = state_radii(other, k, neighbours)
  knn_o, within_o = (_host(x)
                     for x in neighbours(other, ref, k, radius_b=rad_ref))
  knn_r, within_r = (_host(x)
                     for x in neighbours(ref, other, k, radius_b=rad_other))
  near_r, near_o = knn_r[:, 0].astype(np.int64), knn_o[:, 0].astype(np.int64)

  def root_median(x):
    return float(np.median(np.sqrt(np.asarray(x).astype(np.float64))))

  return {
      'precision': float(np.mean(within_o > 0)),
      'recall': float(np.mean(within_r > 0)),
      'coverage': float(np.mean(near_r <= rad_ref.astype(np.int64))),
      'exact_match': [float(np.mean(near_r == 0)), float(np.mean(near_o == 0))],
      'nearest_distance': [root_median(near_r), root_median(near_o)],
      'radius_median': [root_median(rad_ref), root_median(rad_other)],
      'num_states': [int(len(ref)), int(len(other))],
  }


# -- third-order correlations of binarised population states ---------------------
# (compute_metrics.py --triplet_metrics; csrc/triplets.hip)
TRIPLET_MAX_NEURONS = 512       # CG_TRIPLET_MAX_C
TRIPLET_MAX_WORDS = 2**26 - 1   # CG_TRIPLET_MAX_WORDS: every count below 2^31


def _triplet_bin(bin):
  bin = int(bin)
  if bin < 1:
    raise ValueError('bin = {}: at least one frame'.format(bin))
  return bin


def binary_states(spikes, bin=12):
  """uint8 (N nb, C) of trials (N, T, C), a frame a spike when it is != 0: entry
  (n nb + b, c) is 1 iff neuron c has any spike in frames b bin .. (b + 1) bin -
  1 of trial n, nb = T // bin (a trailing partial bin is dropped; T < bin
  raises).  Binarised on purpose: the counts of binary states need no exactness
  bound."""
  s = _binary_trials(spikes)
  bin = _triplet_bin(bin)
  N, T, C = s.shape
  nb = T // bin
  if nb < 1:
    raise ValueError('trials of {} frames hold no bin of {}'.format(T, bin))
  return s[:, :nb * bin].reshape(N, nb, bin, C).any(2).reshape(
      N * nb, C).astype(np.uint8)


def triplet_index(C):
  """int32 (C(C,3), 3): the (i, j, k), i < j < k, of every rank, in
  lexicographic order (itertools.combinations(range(C), 3))."""
  C = int(C)
  if C < 3:
    raise ValueError('C = {}: three neurons at least'.format(C))
  parts = []
  for i in range(C - 2):
    j, k = np.triu_indices(C - i - 1, 1)
    parts.append(np.stack([np.full(len(j), i), j + i + 1, k + i + 1], 1))
  return np.concatenate(parts).astype(np.int32)


def triplet_counts(states, chunk=1 << 16):
  """(singles (C,), pairs (C, C), triplets (C(C,3),)), int64, of binary states
  (S, C):
    singles[i]  = sum_s x_si
    pairs[i][j] = sum_s x_si x_sj     (symmetric, the singles on the diagonal)
    triplets[r] = sum_s x_si x_sj x_sk   for the r-th i < j < k of triplet_index
  One (C x S)(S x C) float64 product per neuron and chunk of states, exact on
  these integers below 2^53.  The statement cg_triplet_counts is tested
  against, for equality."""
  x = np.asarray(states)
  if x.ndim != 2 or x.shape[1] < 3 or not len(x):
    raise ValueError('states (S, C), C >= 3, expected')
  x = (x != 0).astype(np.float64)
  S, C = x.shape
  pairs = np.zeros((C, C), np.float64)
  ju, ku = np.triu_indices(C, 1)   # ordered by j, then k
  # the pairs j > i are the tail of (ju, ku) from first[i + 1] on
  first = np.concatenate([[0], np.cumsum(C - 1 - np.arange(C))])
  offset = np.concatenate(
      [[0], np.cumsum([len(ju) - first[i + 1] for i in range(C - 2)])])
  triplets = np.zeros((int(offset[-1]),), np.float64)
  for s0 in range(0, S, int(chunk)):
    xs = x[s0:s0 + int(chunk)]
    pairs += xs.T @ xs
    for i in range(C - 2):
      m = (xs * xs[:, i:i + 1]).T @ xs
      sel = slice(first[i + 1], None)
      triplets[offset[i]:offset[i + 1]] += m[ju[sel], ku[sel]]
  pairs = pairs.astype(np.int64)
  return np.diagonal(pairs).copy(), pairs, triplets.astype(np.int64)


def pack_state_words(states, nb):
  """uint32 (C, N wpt) of binary states (N nb, C), the layout of
  cg_binary_words: bit b % 32 of word n wpt + b // 32 of row c is state n nb + b
  of neuron c, wpt = ceil(nb / 32), the tail bits of a trial's last word zero."""
  x = (np.asarray(states) != 0)
  nb = int(nb)
  S, C = x.shape
  if nb < 1 or S % nb:
    raise ValueError('{} states are no whole trials of {}'.format(S, nb))
  N, wpt = S // nb, -(-nb // 32)
  bits = np.zeros((N, wpt * 32, C), np.uint64)
  bits[:, :nb] = x.reshape(N, nb, C)
  bits = bits.reshape(N, wpt, 32, C) << np.arange(32, dtype=np.uint64)[:, None]
  return np.ascontiguousarray(
      bits.sum(2).astype(np.uint32).transpose(2, 0, 1).reshape(C, N * wpt))


def unpack_state_words(words, nb):
  """uint8 (N nb, C): the states of uint32 (C, N wpt) words; what
  `pack_state_words` packed."""
  w = np.asarray(words).astype(np.uint32)
  nb = int(nb)
  wpt = -(-nb // 32)
  C, W = w.shape
  if nb < 1 or W % wpt:
    raise ValueError('{} words are no whole trials of {}'.format(W, wpt))
  N = W // wpt
  bits = (w.reshape(C, N, wpt, 1) >> np.arange(32, dtype=np.uint32)) & 1
  return np.ascontiguousarray(
      bits.reshape(C, N, wpt * 32)[:, :, :nb].transpose(1, 2, 0).reshape(
          N * nb, C).astype(np.uint8))


class DeviceWords(object):
  """Binary states on the device as cg_binary_words writes them: `tensor` int32
  (C, trials wpt), the uint32 words of every neuron (bit b % 32 of word b // 32
  of a trial is the state of its bin b, wpt = ceil(nb / 32)), with the number of
  neurons C, the bin, the bins per trial nb and the number of trials."""
  __slots__ = ('tensor', 'C', 'bin', 'nb', 'trials')

  def __init__(self, tensor, C, bin, nb, trials):
    self.tensor, self.C, self.bin = tensor, int(C), int(bin)
    self.nb, self.trials = int(nb), int(trials)

  def __len__(self):
    """The number of states."""
    return self.nb * self.trials

  @classmethod
  def cat(cls, parts):
    """The sets joined along the words."""
    import torch
    parts = list(parts)
    if len({(p.C, p.bin, p.nb) for p in parts}) != 1:
      raise ValueError('sets of one C, one bin and one trial length expected')
    p = parts[0]
    return cls(torch.cat([q.tensor for q in parts], dim=1), p.C, p.bin, p.nb,
               sum(q.trials for q in parts))

  def states(self):
    """uint8 host (trials nb, C): the states as `binary_states` holds them."""
    return unpack_state_words(
        self.tensor.cpu().numpy().view(np.uint32), self.nb)


def binary_words_device(spikes, bin=12):
  """`binary_states` on the GPU, packed (cg_binary_words): float32 device tensor
  (B, T, C), any strides, read in place -> DeviceWords of B (T // bin) states.
  One launch, no host synchronisation.  3 <= C <= 512."""
  import torch
  from ... import _lib as hip
  B, T, C = _trial_batch(spikes)
  bin = _triplet_bin(bin)
  if T < bin:
    raise ValueError('trials of {} frames hold no bin of {}'.format(T, bin))
  nb = T // bin
  W = B * -(-nb // 32)
  words = torch.empty(C, W, dtype=torch.int32, device=spikes.device)
  hip.call('cg_binary_words', spikes, B, T, C, spikes.stride(0),
           spikes.stride(1), spikes.stride(2), bin, words, W, hip.stream())
  return DeviceWords(words, C, bin, nb, B)


def triplet_counts_device(words):
  """`triplet_counts` on the GPU (cg_triplet_counts): DeviceWords -> ((singles
  (C,), pairs (C, C), triplets (C(C,3),)) int32 device, S), the statement's
  integers and the number of states.  No atomics, no host synchronisation."""
  import torch
  from ... import _lib as hip
  if not isinstance(words, DeviceWords):
    raise ValueError('DeviceWords expected')
  t = words.tensor
  if not t.is_contiguous():
    raise ValueError('contiguous words expected')
  C, W = int(t.shape[0]), int(t.shape[1])
  dev = t.device
  ws = hip.workspace('cg_triplet_counts_ws_bytes', dev, C, W, least=16)
  singles = torch.empty(C, dtype=torch.int32, device=dev)
  pairs = torch.empty(C, C, dtype=torch.int32, device=dev)
  triplets = torch.empty(C * (C - 1) * (C - 2) // 6, dtype=torch.int32,
                         device=dev)
  hip.call('cg_triplet_counts', t, C, W, W, singles, pairs, triplets, ws,
           hip.stream())
  return (singles, pairs, triplets), len(words)


def _triplet_moments(side):
  """(pair covariances over i < j, p_ijk, kappa_ijk) of one side (singles,
  pairs, triplets, S), float64."""
  singles, pairs, triplets, S = side
  S = int(S)
  if S < 1:
    raise ValueError('no states')
  p1 = _host(singles).astype(np.float64) / S
  p2 = _host(pairs).astype(np.float64) / S
  p3 = _host(triplets).astype(np.float64) / S
  C = len(p1)
  if C < 3 or p2.shape != (C, C) or p3.shape != (C * (C - 1) * (C - 2) // 6,):
    raise ValueError('singles (C,), pairs (C, C), triplets (C(C,3),), C >= 3, '
                     'expected')
  ju, ku = np.triu_indices(C, 1)
  cov = p2[ju, ku] - p1[ju] * p1[ku]
  kappa = np.empty_like(p3)
  first = np.concatenate([[0], np.cumsum(C - 1 - np.arange(C))])
  at = 0
  for i in range(C - 2):   # the block of rank (i, j, k), j > i
    j, k = ju[first[i + 1]:], ku[first[i + 1]:]
    n = len(j)
    kappa[at:at + n] = (p3[at:at + n] - p2[i, j] * p1[k] - p2[i, k] * p1[j] -
                        p2[j, k] * p1[i] + 2.0 * p1[i] * p1[j] * p1[k])
    at += n
  return cov, p3, kappa


def triplet_scores(ref, other):
  """How far the third-order structure of `other` is from that of `ref`; each
  side (singles, pairs, triplets, S) as `triplet_counts` or
  `triplet_counts_device` gives them, and its number of states.  Host float64,
  whichever device counted.  With p = n / S:
    c_ij      = p_ij - p_i p_j                                   (i < j)
    kappa_ijk = p_ijk - p_ij p_k - p_ik p_j - p_jk p_i + 2 p_i p_j p_k
  the connected third-order correlation (third joint cumulant) of i < j < k.
    pair_covariance_mae, pair_covariance_correlation   over i < j: the second
                                  order at the same binning, to read the third
                                  order against
    triplet_probability_mae       mean |difference| of p_ijk
    triplet_cumulant_mae, triplet_cumulant_correlation   over all triplets
    triplet_cumulant_top_mae, triplet_cumulant_top_correlation   the same over
                                  the max(2, ceil(Tr / 100)) triplets of largest
                                  |kappa_ref| (stable order: the lower rank first
                                  on ties; NaN when Tr < 2)
    triplet_cumulant_mean_abs     [ref, other]: mean |kappa|
    triplets_observed             [ref, other]: share of triplets with a count
    num_states, num_triplets      [S_ref, S_other], Tr
  A correlation is NaN with fewer than two values or no variance on a side."""
  cov_r, p3_r, k_r = _triplet_moments(ref)
  cov_o, p3_o, k_o = _triplet_moments(other)
  if k_r.shape != k_o.shape:
    raise ValueError('sides of one C expected')
  Tr = len(k_r)
  nan = float('nan')
  if Tr >= 2:
    top = np.argsort(-np.abs(k_r), kind='stable')[:max(2, -(-Tr // 100))]
    top_mae = _mean_abs_difference(k_r[top], k_o[top])
    top_corr = _pearson(k_r[top], k_o[top])
  else:
    top_mae = top_corr = nan
  return {
      'pair_covariance_mae': _mean_abs_difference(cov_r, cov_o),
      'pair_covariance_correlation': _pearson(cov_r, cov_o),
      'triplet_probability_mae': _mean_abs_difference(p3_r, p3_o),
      'triplet_cumulant_mae': _mean_abs_difference(k_r, k_o),
      'triplet_cumulant_correlation': _pearson(k_r, k_o),
      'triplet_cumulant_top_mae': top_mae,
      'triplet_cumulant_top_correlation': top_corr,
      'triplet_cumulant_mean_abs': [float(np.mean(np.abs(k_r))),
                                    float(np.mean(np.abs(k_o)))],
      'triplets_observed': [float(np.mean(p3_r > 0)), float(np.mean(p3_o > 0))],
      'num_states': [int(ref[3]), int(other[3])],
      'num_triplets': int(Tr),
  }


# -- inter-spike intervals and trial-to-trial variability --------------------------
# (compute_metrics.py --interval_metrics; csrc/spike_intervals.hip)
INTERVAL_MAX_NEURONS = 4096     # CG_INTERVAL_MAX_C
INTERVAL_MAX_ISI = 4095         # CG_INTERVAL_MAX_ISI


def _max_isi(max_isi):
  max_isi = int(max_isi)
  if not 1 <= max_isi <= INTERVAL_MAX_ISI:
    raise ValueError('max_isi = {}: 1 .. {} expected'.format(
        max_isi, INTERVAL_MAX_ISI))
  return max_isi


def interval_counts(spikes, max_isi=240):
  """(hist (C, max_isi + 1), moments (C, 6), counts (N, C)), int64, of trials (N,
  T, C), a frame a spike when it is != 0.  Train (n, c) has its spikes at t_1 <
  ... < t_m and the intervals I_k = t_{k+1} - t_k (m - 1 of them, m - 2
  consecutive pairs); no interval runs from one trial into the next.
    hist[c][d - 1]   intervals of neuron c equal to d, 1 <= d <= max_isi, over
                     its trials; hist[c][max_isi] those > max_isi
    moments[c]       spikes, intervals, sum I, sum I^2, consecutive pairs, sum
                     I_k I_{k+1} (an overflow interval with its true length)
    counts[n][c]     spikes of train (n, c)
  The statement cg_spike_intervals is tested against, for equality."""
  s = np.asarray(spikes)
  if s.ndim != 3:
    raise ValueError('(B, T, C) expected')
  s = s != 0   # as _binary_trials: a NaN is a spike, -0.0 is not
  max_isi = _max_isi(max_isi)
  N, T, C = s.shape
  H = max_isi + 1
  counts = s.sum(1).astype(np.int64)
  # every spike as (neuron, trial, frame), sorted in that order
  c, n, t = np.nonzero(s.transpose(2, 0, 1))
  t = t.astype(np.int64)
  same = (c[1:] == c[:-1]) & (n[1:] == n[:-1])   # the spike before: same train
  I = (t[1:] - t[:-1])[same]
  owner = c[1:][same]
  hist = np.bincount(owner * H + np.minimum(I, H) - 1,
                     minlength=C * H).reshape(C, H).astype(np.int64)
  moments = np.zeros((C, 6), np.int64)
  moments[:, 0] = counts.sum(0)
  np.add.at(moments[:, 1], owner, 1)
  np.add.at(moments[:, 2], owner, I)
  np.add.at(moments[:, 3], owner, I * I)
  both = same[1:] & same[:-1]                    # and the one before that
  d = t[1:] - t[:-1]
  np.add.at(moments[:, 4], c[2:][both], 1)
  np.add.at(moments[:, 5], c[2:][both], (d[1:] * d[:-1])[both])
  return hist, moments, counts


def interval_counts_device(words, max_isi=240):
  """`interval_counts` on the GPU (cg_spike_intervals): DeviceWords of bin 1 ->
  (hist (C, max_isi + 1) int32, moments (C, 6) int64, counts (trials, C) int32)
  on the device, the statement's integers.  One call, no atomics in global
  memory, no host synchronisation."""
  import torch
  from ... import _lib as hip
  if not isinstance(words, DeviceWords):
    raise ValueError('DeviceWords expected')
  max_isi = _max_isi(max_isi)
  t = words.tensor
  if words.bin != 1:
    raise ValueError('words of bin 1 expected, not {}'.format(words.bin))
  if not t.is_contiguous():
    raise ValueError('contiguous words expected')
  C, W = int(t.shape[0]), int(t.shape[1])
  trials, wpt = words.trials, -(-words.nb // 32)
  if W != trials * wpt:
    raise ValueError('{} words are no {} trials of {}'.format(W, trials, wpt))
  dev = t.device
  ws = hip.workspace('cg_spike_intervals_ws_bytes', dev, C, trials, wpt, max_isi,
                     least=16)
  hist = torch.empty(C, max_isi + 1, dtype=torch.int32, device=dev)
  moments = torch.empty(C, 6, dtype=torch.int64, device=dev)
  counts = torch.empty(trials, C, dtype=torch.int32, device=dev)
  hip.call('cg_spike_intervals', t, C, trials, wpt, W, max_isi, hist, moments,
           counts, ws, hip.stream())
  return hist, moments, counts


def _interval_side(side):
  hist, moments, counts = (_host(x).astype(np.int64) for x in side)
  if not (hist.ndim == 2 and hist.shape[1] >= 2 and counts.ndim == 2 and
          moments.shape == (len(hist), 6) and counts.shape[1] == len(hist)):
    raise ValueError('hist (C, max_isi + 1), moments (C, 6), counts (N, C) '
                     'expected')
  if len(counts) < 2:
    raise ValueError('{} trial(s): the Fano factor needs two'.format(
        len(counts)))
  m = moments.astype(np.float64)
  nan = np.full(len(hist), np.nan)
  some = m[:, 1] > 0
  mu, var, cv, rho = nan.copy(), nan.copy(), nan.copy(), nan.copy()
  mu[some] = m[some, 2] / m[some, 1]
  var[some] = m[some, 3] / m[some, 1] - mu[some] ** 2
  cv[some] = np.sqrt(np.maximum(var[some], 0.0)) / mu[some]
  serial = some & (m[:, 4] >= 1) & (var > 0)
  rho[serial] = (m[serial, 5] / m[serial, 4] - mu[serial] ** 2) / var[serial]
  x = counts.astype(np.float64)
  mean = x.mean(0)
  d = x - mean
  ss = (d * d).sum(0)
  fano = nan.copy()
  on = mean != 0
  fano[on] = ss[on] / (len(x) - 1) / mean[on]
  varies = ss > 0
  r = np.full((len(hist), len(hist)), np.nan)
  if varies.any():
    v = np.flatnonzero(varies)
    r[np.ix_(v, v)] = (d[:, v].T @ d[:, v]) / np.sqrt(np.outer(ss[v], ss[v]))
  return dict(hist=hist, n=moments[:, 1], pairs=moments[:, 4], mu=mu, var=var,
              cv=cv, rho=rho, serial=serial, fano=fano, on=on, varies=varies,
              r=r, counts=counts)


def interval_scores(ref, other):
  """How far the inter-spike intervals and the trial-to-trial variability of
  `other` are from those of `ref`; each side (hist, moments, counts) as
  `interval_counts` or `interval_counts_device` gives them.  Host float64,
  whichever device counted.  Per neuron, with n intervals: mu = sum I / n,
  sigma^2 = sum I^2 / n - mu^2, CV = sqrt(max(sigma^2, 0)) / mu, rho = (sum I_k
  I_{k+1} / pairs - mu^2) / sigma^2 (the stationary estimator of the lag-1
  serial correlation), F = var(counts, ddof=1) / mean(counts) over the trials.
    isi_js_bits            mean, over the neurons with an interval on both
                           sides, of the Jensen-Shannon divergence in bits of
                           the two hist / n (the overflow bin included)
    isi_js_bits_pooled     the same of the histograms summed over the neurons
    isi_mean_mae           mean |mu_ref - mu_other| in frames, the same neurons
    cv_mae, cv_correlation, cv_mean   over the neurons with two intervals on
                           both sides; cv_mean is [ref, other]
    serial_correlation_mae, serial_correlation_mean   over the neurons with a
                           pair and sigma^2 > 0 on both sides
    adjacent_fraction, overflow_fraction   [ref, other]: share of all intervals
                           equal to 1 frame, and > max_isi
    fano_mae, fano_correlation, fano_mean   over the neurons with a non-zero
                           mean count on both sides
    count_correlation_mae, count_correlation_correlation   Pearson r of the
                           counts of neurons i < j across trials, over the pairs
                           whose two neurons vary on both sides
    silent_trains          [ref, other]: share of trains with no spike
    num_trials, num_intervals, max_isi   [ref, other], [ref, other], as used
  A figure over an empty set is NaN, a correlation with fewer than two values
  or no variance on a side too.  Sides of different C or max_isi, or a side of
  fewer than two trials, raise ValueError."""
  a, b = _interval_side(ref), _interval_side(other)
  if a['hist'].shape != b['hist'].shape:
    raise ValueError('sides of one C and one max_isi expected')
  nan = float('nan')

  def mean(x):
    return float(np.mean(x)) if np.size(x) else nan

  def share(s, column):
    total = int(s['n'].sum())
    return float(s['hist'][:, column].sum()) / total if total else nan

  one = np.flatnonzero((a['n'] >= 1) & (b['n'] >= 1))
  js = [_js_divergence_bits(a['hist'][c] / float(a['n'][c]),
                            b['hist'][c] / float(b['n'][c])) for c in one]
  pa, pb = a['hist'].sum(0), b['hist'].sum(0)
  pooled = (_js_divergence_bits(pa / float(pa.sum()), pb / float(pb.sum()))
            if pa.sum() and pb.sum() else nan)
  two = (a['n'] >= 2) & (b['n'] >= 2)
  ser = a['serial'] & b['serial']
  on = a['on'] & b['on']
  ju, ku = np.triu_indices(len(a['n']), 1)
  vary = a['varies'] & b['varies']
  sel = vary[ju] & vary[ku]
  ra, rb = a['r'][ju[sel], ku[sel]], b['r'][ju[sel], ku[sel]]
  return {
      'isi_js_bits': mean(js),
      'isi_js_bits_pooled': pooled,
      'isi_mean_mae': _mean_abs_difference(a['mu'][one], b['mu'][one]),
      'cv_mae': _mean_abs_difference(a['cv'][two], b['cv'][two]),
      'cv_correlation': _pearson(a['cv'][two], b['cv'][two]),
      'cv_mean': [mean(a['cv'][two]), mean(b['cv'][two])],
      'serial_correlation_mae': _mean_abs_difference(a['rho'][ser],
                                                     b['rho'][ser]),
      'serial_correlation_mean': [mean(a['rho'][ser]), mean(b['rho'][ser])],
      'adjacent_fraction': [share(a, 0), share(b, 0)],
      'overflow_fraction': [share(a, -1), share(b, -1)],
      'fano_mae': _mean_abs_difference(a['fano'][on], b['fano'][on]),
      'fano_correlation': _pearson(a['fano'][on], b['fano'][on]),
      'fano_mean': [mean(a['fano'][on]), mean(b['fano'][on])],
      'count_correlation_mae': _mean_abs_difference(ra, rb),
      'count_correlation_correlation': _pearson(ra, rb),
      'silent_trains': [float(np.mean(a['counts'] == 0)),
                        float(np.mean(b['counts'] == 0))],
      'num_trials': [int(len(a['counts'])), int(len(b['counts']))],
      'num_intervals': [int(a['n'].sum()), int(b['n'].sum())],
      'max_isi': int(a['hist'].shape[1] - 1),
  }
