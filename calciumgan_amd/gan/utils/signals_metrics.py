"""Figures of the calcium traces themselves, before deconvolution (the reference
keeps its TensorFlow trace summaries in a module of this name; they are not
restated here): the per-neuron power spectrum averaged over trials.
compute_metrics.py --spectral_metrics; csrc/trace_psd.hip, DESIGN.md 22.

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
  if not (torch.is_tensor(signals) and signals.is_cuda and
          signals.dtype == torch.float32 and signals.dim() == 3):
    raise ValueError('float32 device tensor (B, T, C) expected')
  B, T, C = signals.shape
  if B < 1 or T < 2 or C < 1:
    raise ValueError('(B, T, C) trials with B, C >= 1 and T >= 2 expected')
  if (T & (T - 1)) or not PSD_DEVICE_MIN_LENGTH <= T <= PSD_DEVICE_MAX_LENGTH:
    return torch.from_numpy(trace_power_spectrum(signals.cpu().numpy())).to(
        signals.device)
  nbytes = hip.load().cg_trace_psd_ws_bytes(B, T, C)
  if nbytes < 0:
    raise ValueError('cg_trace_psd: unsupported shape {}'.format((B, T, C)))
  ws = torch.empty(nbytes, dtype=torch.uint8, device=signals.device)
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
