"""Figures of the calcium traces themselves, before deconvolution (the reference
keeps its TensorFlow trace summaries in a module of this name; they are not
restated here): the per-neuron power spectrum averaged over trials
(compute_metrics.py --spectral_metrics; csrc/trace_psd.hip) and,
in the second half of the module, the distance from every trial to the nearest
stretch of the recording (--novelty_metrics; csrc/nearest_stretch.hip, DESIGN.md
23).

Per trial and neuron, with x the float32 trace of T frames:
  m   = float32(sum_t float64(x_t) / T)
  w_t = float32(0.5 - 0.5 cospi(2 t / T))        periodic Hann, float64 cosine
  y_t = (x_t - m) w_t, the difference and the product each rounded to float32
  X_k = sum_t y_t e^{-2 pi i k t / T},  k = 0 .. T / 2
  totals[k][c] = sum over the trials of |X_k|^2, float64, un-normalised
  S = totals / (trials sum_t w_t^2),  sum_t w_t^2 = 3 T / 8
so that white noise of variance s^2 has S ~ s^2 in every bin.
"""
import math

import numpy as np

from .spike_helper import FRAME_RATE
from .spike_metrics import _host, _trial_batch

# lengths cg_trace_psd takes (csrc/trace_psd.hip): powers of two in this range
PSD_DEVICE_MIN_LENGTH = 32
PSD_DEVICE_MAX_LENGTH = 8192
# a bin below this fraction of its neuron's mean level is left out of the log
# spectral distance
PSD_FLOOR = 1e-12
# upsampling factors of a stack of stride-2 transposed convolutions whose
# periods T / h are looked at by stride_peak_db
STRIDE_PERIODS = (2, 4, 8, 16, 32)
_TRIALS_PER_PASS = 16


def _cospi(x):
  """cos(pi x) of float64 x in [0, 2], exact at the multiples of 1/2: the
  argument is folded into [0, 1/4] before pi comes in."""
  x = np.asarray(x, dtype=np.float64)
  x = np.where(x > 1.0, 2.0 - x, x)            # cos(pi (2 - x)) = cos(pi x)
  sign = np.where(x > 0.5, -1.0, 1.0)
  x = np.where(x > 0.5, 1.0 - x, x)            # cos(pi (1 - x)) = -cos(pi x)
  return sign * np.where(x > 0.25, np.sin(np.pi * (0.5 - x)), np.cos(np.pi * x))


def hann_window(T):
  """float32 (T,): w_t = 0.5 - 0.5 cospi(2 t / T), the cosine in float64, rounded
  once.  Periodic (w_0 = 0, w_{T/2} = 1 for an even T, w_t = w_{T - t})."""
  T = int(T)
  if T < 1:
    raise ValueError('T < 1')
  return (0.5 - 0.5 * _cospi(2.0 * np.arange(T) / T)).astype(np.float32)


def _windowed(x, w):
  """float32 y of a float32 (B, T, C) block: (x - m) w with float32 roundings."""
  m = (x.astype(np.float64).sum(axis=1, keepdims=True) / x.shape[1]).astype(
      np.float32)
  return ((x - m).astype(np.float32) * w[None, :, None]).astype(np.float32)


def trace_power_spectrum(signals, single_precision=False):
  """float64 (T / 2 + 1, C): |X_k|^2 of every neuron of float32 trials (B, T, C),
  summed over the trials (the statement at the top of this module; cg_trace_psd
  is tested against it).  The transform is float64 (numpy's rfft of the float32
  y widened); single_precision=True runs the float32 y through scipy.fft.rfft
  (complex64 pocketfft) and squares in float32 -- the yardstick the device
  kernel's error is held against.  A neuron with a non-finite sample in any
  trial has NaN in all its bins; no other neuron is affected."""
  x = np.asarray(signals)
  if x.ndim != 3 or x.shape[0] < 1 or x.shape[1] < 2 or x.shape[2] < 1:
    raise ValueError('(B, T, C) trials with B, C >= 1 and T >= 2 expected')
  x = x.astype(np.float32, copy=False)
  B, T, C = x.shape
  bad = ~np.isfinite(x).all(axis=(0, 1))
  if bad.any():
    x = np.where(bad[None, None, :], np.float32(0), x)
  w = hann_window(T)
  totals = np.zeros((T // 2 + 1, C), np.float64)
  for i in range(0, B, _TRIALS_PER_PASS):
    y = _windowed(x[i:i + _TRIALS_PER_PASS], w)
    if single_precision:
      import scipy.fft
      X = scipy.fft.rfft(y, axis=1)
      assert X.dtype == np.complex64
      power = X.real * X.real + X.imag * X.imag
      assert power.dtype == np.float32
    else:
      X = np.fft.rfft(y.astype(np.float64), axis=1)
      power = X.real * X.real + X.imag * X.imag
    totals += power.astype(np.float64).sum(axis=0)
  totals[:, bad] = np.nan
  return totals


def trace_power_spectrum_device(signals):
  """`trace_power_spectrum` on the GPU (cg_trace_psd): float32 device tensor
  (B, T, C), any strides, read in place -> float64 device (T / 2 + 1, C).  Two
  launches, nothing zeroed beforehand, no host synchronisation.  The transform
  is float32 there: the result agrees with the statement to float32-transform
  rounding, not bit for bit.

  The kernel takes T a power of two in 32 .. 8192.  Any other length goes
  through `trace_power_spectrum` on the host: the batch goes down and the
  totals come back up as a device tensor."""
  import torch
  from ... import _lib as hip
  B, T, C = _trial_batch(signals)
  if B < 1 or T < 2 or C < 1:
    raise ValueError('(B, T, C) trials with B, C >= 1 and T >= 2 expected')
  if (T & (T - 1)) or not PSD_DEVICE_MIN_LENGTH <= T <= PSD_DEVICE_MAX_LENGTH:
    return torch.from_numpy(trace_power_spectrum(signals.cpu().numpy())).to(
        signals.device)
  ws = hip.workspace('cg_trace_psd_ws_bytes', signals.device, B, T, C)
  totals = torch.empty(T // 2 + 1, C, dtype=torch.float64,
                       device=signals.device)
  hip.call('cg_trace_psd', signals, B, T, C, signals.stride(0),
           signals.stride(1), signals.stride(2), totals, ws, hip.stream())
  return totals


def spectral_totals(signals):
  """(totals float64 (T / 2 + 1, C), trials): `trace_power_spectrum` and B."""
  return trace_power_spectrum(signals), int(np.shape(signals)[0])


def spectral_totals_device(signals, group_bytes=256 << 20):
  """`spectral_totals` on the GPU: float32 device tensor (B, T, C) -> (device
  float64 (T / 2 + 1, C), B).  The batch is walked in groups of as many trials
  as hold `group_bytes` of float32 samples (one at least) and the groups' totals
  are added on the device in float64, in order.  No host synchronisation."""
  B, T, C = signals.shape
  group = max(int(group_bytes) // (T * C * 4), 1)
  totals = None
  for i in range(0, B, group):
    part = trace_power_spectrum_device(signals[i:i + group])
    totals = part if totals is None else totals + part
  return totals, int(B)


def _db(ratio):
  return 10.0 * np.log10(ratio)


def spectral_scores(ref, other, T, frame_rate=FRAME_RATE):
  """How far the power spectra of `other` are from those of `ref`; both
  `spectral_totals` (or `spectral_totals_device`, brought to the host) of trials
  of T frames of the same C neurons.  Host float64, whichever device summed.
  S = totals / (trials 3 T / 8).  Every figure is a mean over the neurons whose
  S is finite with non-zero power over k >= 1 on both sides, NaN if there is
  none; k runs over 1 .. T / 2 unless said:
    log_spectral_distance_db   mean |d| and root mean square of d = 10 log10
    log_spectral_rmse_db       S_other - 10 log10 S_ref over neurons and bins; a
                               bin is left out when either side is below 1e-12 x
    bins_excluded              that side's mean S of the neuron; their number
    total_power_ratio_db       10 log10(sum_k S_other / sum_k S_ref)
    band_power_ratio_db        the same over [1, T/16), [T/16, T/8), [T/8, T/4),
                               [T/4, T/2]: a list of four (a neuron counts in a
                               band where both sides have power there)
    stride_peak_db             {recorded: [...], generated: [...]}: for h in (2,
                               4, 8, 16, 32) with T / h >= 8 and k_h = T / h,
                               10 log10(S[k_h] / median(S[k]: |k - k_h| <= 3,
                               k != k_h, 1 <= k <= T / 2)) -- what the periodic
                               artefacts of stride-2 transposed convolutions
                               raise
    spectral_centroid_hz       [recorded, generated] sum f_k S / sum S, f_k =
                               k frame_rate / T
    num_trials, frame_rate     num_trials as [recorded, generated]"""
  T = int(T)
  if T < 2 or T % 2:
    raise ValueError('an even T >= 2 expected')
  sides = []
  for totals, n in (ref, other):
    totals = np.asarray(totals.cpu() if hasattr(totals, 'cpu') else totals,
                        dtype=np.float64)
    if totals.ndim != 2 or totals.shape[0] != T // 2 + 1 or int(n) < 1:
      raise ValueError('totals ((T / 2 + 1, C), trials) expected')
    sides.append((totals / (int(n) * 3.0 * T / 8.0), int(n)))
  if sides[0][0].shape != sides[1][0].shape:
    raise ValueError('the two sides differ in shape')
  half = T // 2
  nan = float('nan')
  with np.errstate(invalid='ignore', divide='ignore'):
    use = np.ones(sides[0][0].shape[1], bool)
    for S, _ in sides:
      use &= np.isfinite(S).all(axis=0) & (S[1:].sum(axis=0) > 0)
    Sr, So = (S[:, use] for S, _ in sides)
    some = bool(use.any())

    def mean(values):
      values = np.asarray(values, np.float64)
      return float(np.mean(values)) if values.size else nan

    keep = np.ones((half, Sr.shape[1]), bool)
    for S in (Sr, So):
      keep &= S[1:] >= PSD_FLOOR * S[1:].mean(axis=0, keepdims=True)
    d = (_db(So[1:]) - _db(Sr[1:]))[keep]
    bands = []
    for lo, hi in ((1, T // 16), (T // 16, T // 8), (T // 8, T // 4),
                   (T // 4, half + 1)):
      pr, po = Sr[lo:hi].sum(axis=0), So[lo:hi].sum(axis=0)
      both = (pr > 0) & (po > 0)
      bands.append(mean(_db(po[both] / pr[both])) if hi > lo else nan)
    peaks, centroid = [], []
    k = np.arange(half + 1, dtype=np.float64)
    for S in (Sr, So):
      per_h = []
      for h in STRIDE_PERIODS:
        if T // h < 8:
          continue
        kh = T // h
        near = [j for j in range(kh - 3, kh + 4) if j != kh and 1 <= j <= half]
        base = np.median(S[near], axis=0)
        ok = (base > 0) & (S[kh] > 0)
        per_h.append(mean(_db(S[kh][ok] / base[ok])))
      peaks.append(per_h)
      centroid.append(mean((k[1:, None] * frame_rate / T * S[1:]).sum(axis=0) /
                           S[1:].sum(axis=0)) if some else nan)
    return {
        'log_spectral_distance_db': mean(np.abs(d)),
        'log_spectral_rmse_db': math.sqrt(mean(d * d)) if d.size else nan,
        'bins_excluded': int(keep.size - keep.sum()),
        'total_power_ratio_db': mean(_db(So[1:].sum(axis=0) /
                                         Sr[1:].sum(axis=0))),
        'band_power_ratio_db': bands,
        'stride_peak_db': {'recorded': peaks[0], 'generated': peaks[1]},
        'spectral_centroid_hz': centroid,
        'num_trials': [sides[0][1], sides[1][1]],
        'frame_rate': float(frame_rate),
    }


# -- nearest stretch of the recording (compute_metrics.py --novelty_metrics;
# csrc/nearest_stretch.hip) ---------------------------------------
#
# R: the recording, (T_raw, C) float32.  Q: the queries, (N, L, C) float32, L <=
# T_raw.  step >= 1; offsets s_j = j step for j = 0 .. S - 1, S = (T_raw - L) //
# step + 1: every full stretch counts, the last one included.
#   d2[n][j] = sum_{t, c} (float64(Q[n, t, c]) - float64(R[s_j + t, c]))^2
# in float64; a non-finite d2 is NaN.  The expanded form is |q_n|^2 + W_j - 2 sum
# q r with every term float64 (the float32 products are exact there), clamped at
# 0.  Exclusion: `exclude` int32 (N,) of start rows, negative for none; for
# query n the offsets with |s_j - exclude[n]| < exclude_len are left out of the
# minimum (d2 holds them all the same).
#   nearest[n] = the least finite admitted d2[n][j], index[n] the LOWEST j that
#   attains it; NaN and -1 where no admitted entry is finite.
# A non-finite sample of a query spoils that query only, a non-finite row of the
# recording only the offsets whose stretch covers it.
_OFFSETS_PER_PASS = 64


def stretch_offsets(T_raw, L, step=1):
  """S = (T_raw - L) // step + 1, the number of offsets."""
  return (int(T_raw) - int(L)) // int(step) + 1


def _nearest_stretch_args(queries, recording, step, exclude, exclude_len):
  q = np.asarray(queries)
  r = np.asarray(recording)
  if q.ndim != 3 or r.ndim != 2 or q.shape[2] != r.shape[1] or min(q.shape) < 1:
    raise ValueError('(N, L, C) queries and a (T_raw, C) recording expected')
  if q.shape[1] > r.shape[0]:
    raise ValueError('queries of {} rows, a recording of {}'.format(
        q.shape[1], r.shape[0]))
  if int(step) < 1 or int(exclude_len) < 0:
    raise ValueError('step >= 1 and exclude_len >= 0 expected')
  q = q.astype(np.float32, copy=False)
  r = np.ascontiguousarray(r, dtype=np.float32)
  if exclude is not None:
    exclude = np.asarray(exclude).astype(np.int64)
    if exclude.shape != (q.shape[0],):
      raise ValueError('exclude: one start row per query expected')
  return q, r, int(step), exclude, int(exclude_len)


def nearest_stretch(queries, recording, step=1, exclude=None, exclude_len=0,
                    return_profile=False, expanded=False):
  """(nearest float64 (N,), index int64 (N,)[, d2 float64 (N, S)]) of the
  definitions above.  The default is the direct difference form, walked in
  chunks of offsets: the statement cg_nearest_stretch and the expanded form are
  tested against.  expanded=True is the three-term form, a float64 matmul over
  chunks of the Toeplitz operand (a strided view of the recording: nothing of
  size S x K is kept), within 4 K 2^-53 (|q_n|^2 + W_j) of the direct form."""
  q, r, step, exclude, exclude_len = _nearest_stretch_args(
      queries, recording, step, exclude, exclude_len)
  N, L, C = q.shape
  K, S = L * C, stretch_offsets(r.shape[0], L, step)
  q64 = q.astype(np.float64)
  flat = r.astype(np.float64).reshape(-1)
  # row j: the K elements of stretch j, as they lie in the recording
  toeplitz = np.lib.stride_tricks.sliding_window_view(flat, K)[::step * C]
  assert toeplitz.shape == (S, K)
  if expanded:
    qf = q64.reshape(N, K)
    q2 = (qf * qf).sum(axis=1)
  nearest = np.full(N, np.inf)
  index = np.full(N, -1, np.int64)
  profile = np.empty((N, S), np.float64) if return_profile else None
  with np.errstate(invalid='ignore', over='ignore'):
    for j0 in range(0, S, _OFFSETS_PER_PASS):
      rows = toeplitz[j0:j0 + _OFFSETS_PER_PASS]
      if expanded:
        w = (rows * rows).sum(axis=1)
        d2 = (q2[:, None] + w[None, :]) - 2.0 * (qf @ rows.T)
        d2 = np.where(d2 < 0.0, 0.0, d2)
      else:
        d2 = np.empty((N, len(rows)), np.float64)
        for i, row in enumerate(rows):
          d = q64 - row.reshape(1, L, C)
          d2[:, i] = (d * d).reshape(N, K).sum(axis=1)
      d2 = np.where(np.isfinite(d2), d2, np.nan)
      if return_profile:
        profile[:, j0:j0 + len(rows)] = d2
      admitted = np.isfinite(d2)
      if exclude is not None:
        s = (j0 + np.arange(len(rows), dtype=np.int64)) * step
        admitted &= ~((exclude[:, None] >= 0) &
                      (np.abs(s[None, :] - exclude[:, None]) < exclude_len))
      cand = np.where(admitted, d2, np.inf)
      at = cand.argmin(axis=1)            # (the first of equals)
      least = cand[np.arange(N), at]
      better = admitted[np.arange(N), at] & ((index < 0) | (least < nearest))
      nearest = np.where(better, least, nearest)
      index = np.where(better, j0 + at, index)
  nearest = np.where(index < 0, np.nan, nearest)
  return (nearest, index, profile) if return_profile else (nearest, index)


def nearest_stretch_device(queries, recording, step=1, exclude=None,
                           exclude_len=0, return_profile=False):
  """`nearest_stretch` on the GPU (cg_nearest_stretch): float32 device tensors
  (N, L, C) and (T_raw, C), any strides, read in place -> device (nearest
  float64 (N,), index int32 (N,)[, d2 float64 (N, S)]).  exclude: None, or one
  int32 start row per query (a device tensor is taken as it is).  Five launches,
  nothing zeroed beforehand, no host synchronisation.  Agrees with the statement
  within 4 K 2^-53 (|q_n|^2 + W_j), and bit for bit where the sums are exact."""
  import torch
  from ... import _lib as hip
  for t, dim in ((queries, 3), (recording, 2)):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and
            t.dim() == dim):
      raise ValueError('float32 device tensors (N, L, C) and (T_raw, C) expected')
  N, L, C = queries.shape
  T_raw = recording.shape[0]
  if min(N, L, C) < 1 or recording.shape[1] != C or L > T_raw:
    raise ValueError('(N, L, C) queries and a (T_raw >= L, C) recording expected')
  if int(step) < 1 or int(exclude_len) < 0:
    raise ValueError('step >= 1 and exclude_len >= 0 expected')
  if exclude is not None:
    if not torch.is_tensor(exclude):
      exclude = torch.as_tensor(np.asarray(exclude).astype(np.int32))
    exclude = exclude.to(device=queries.device, dtype=torch.int32).contiguous()
    if exclude.shape != (N,):
      raise ValueError('exclude: one start row per query expected')
  dev = queries.device
  ws = hip.workspace('cg_nearest_stretch_ws_bytes', dev, N, L, C, T_raw,
                     int(step))
  S = stretch_offsets(T_raw, L, step)
  nearest = torch.empty(N, dtype=torch.float64, device=dev)
  index = torch.empty(N, dtype=torch.int32, device=dev)
  d2 = (torch.empty(N, S, dtype=torch.float64, device=dev)
        if return_profile else None)
  hip.call('cg_nearest_stretch', queries, N, L, C, queries.stride(0),
           queries.stride(1), queries.stride(2), recording, T_raw,
           recording.stride(0), recording.stride(1), int(step), exclude,
           int(exclude_len), d2, nearest, index, ws, hip.stream())
  return (nearest, index, d2) if return_profile else (nearest, index)


def nearest_stretch_totals_device(queries, recording, step=1, exclude=None,
                                  exclude_len=0, group_bytes=256 << 20):
  """`nearest_stretch_device` with the queries walked in groups of as many
  trials as hold `group_bytes` of float32 samples (one at least): device
  (nearest float64 (N,), index int32 (N,)), the bits of the single call (a
  query's result does not depend on its neighbours).  No host
  synchronisation."""
  import torch
  N, L, C = queries.shape
  group = max(int(group_bytes) // (L * C * 4), 1)
  if exclude is not None and not torch.is_tensor(exclude):
    exclude = torch.as_tensor(np.asarray(exclude).astype(np.int32))
  parts = [
      nearest_stretch_device(queries[i:i + group], recording, step,
                             None if exclude is None else exclude[i:i + group],
                             exclude_len) for i in range(0, N, group)
  ]
  return (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))


def recorded_starts(S, n, step):
  """The start rows of the n recorded stretches --novelty_metrics measures:
  v_i = step floor(i (S - 1) / max(n - 1, 1)), on the offset grid, spread over
  the recording."""
  i = np.arange(int(n), dtype=np.int64)
  return int(step) * ((i * (int(S) - 1)) // max(int(n) - 1, 1))


def novelty_scores(recorded, generated, L, C, step, offsets=None):
  """How close the generated trials come to the recording, read against how
  close the recording comes to itself.  `recorded` and `generated` are (nearest,
  index) of `nearest_stretch` (either device): of stretches of the recording
  with their own neighbourhood excluded, and of generated trials.  With rms =
  sqrt(nearest / (L C)), the distance per sample, NaNs left out:

    nearest_rms            {recorded, generated}: [min, median, max]
    nearest_rms_ratio      median generated / median recorded
    copied_fraction        share of generated trials below the recorded minimum
    below_recorded_median  share below the recorded median; about 0.5 for a
                           perfect generator
    distinct_stretches     distinct nearest offsets among the generated trials /
                           their number: a collapse onto one stretch shows here
    step, offsets          as used (offsets: S, None if not given)
    num_trials, undefined  [recorded, generated]; undefined counts the NaNs

  A figure whose side is empty is NaN."""
  nan = float('nan')
  sides = []
  for nearest, index in (recorded, generated):
    nearest = _host(nearest).astype(np.float64).reshape(-1)
    index = _host(index).astype(np.int64).reshape(-1)
    if nearest.shape != index.shape:
      raise ValueError('(nearest, index) of equal lengths expected')
    ok = ~np.isnan(nearest)
    sides.append((np.sqrt(nearest[ok] / (float(L) * float(C))), index[ok],
                  int(nearest.size), int((~ok).sum())))
  (rec, _, n_rec, bad_rec), (gen, gen_at, n_gen, bad_gen) = sides

  def spread(x):
    return ([float(x.min()), float(np.median(x)), float(x.max())]
            if x.size else [nan, nan, nan])

  both = rec.size > 0 and gen.size > 0
  return {
      'nearest_rms': {'recorded': spread(rec), 'generated': spread(gen)},
      'nearest_rms_ratio': (float(np.median(gen) / np.median(rec))
                            if both else nan),
      'copied_fraction': float((gen < rec.min()).mean()) if both else nan,
      'below_recorded_median': (float((gen < np.median(rec)).mean())
                                if both else nan),
      'distinct_stretches': (float(len(np.unique(gen_at))) / gen_at.size
                             if gen_at.size else nan),
      'step': int(step),
      'offsets': None if offsets is None else int(offsets),
      'num_trials': [n_rec, n_gen],
      'undefined': [bad_rec, bad_gen],
  }
