"""gan/utils/spike_helper.py counterpart: OASIS AR(1) deconvolution
(g = 0.95, s_min = 0.55, threshold 0.5; spike_helper.py:23-54) on the host.

The arithmetic lives in csrc/oasis_ar1.c (gcc, built by
calciumgan_amd.build.build_host); `oasis_ar1_python` is the same algorithm in
pure python, kept as the cross-check the tests use.  OASIS upstream is an
un-pinned git clone (setup.sh:43) and absent here: PARITY UNPINNED."""
import ctypes
import os

import numpy as np

FRAME_RATE = 24.0  # spike_helper.py:8
_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, '..', '..', 'csrc', 'libcalciumgan_host.so')
_lib = None


def _load():
  global _lib
  if _lib is None:
    if not os.path.exists(_LIB_PATH):
      from ... import build
      build.build_host(verbose=False)
    lib = ctypes.CDLL(os.path.abspath(_LIB_PATH))
    dp = ctypes.POINTER(ctypes.c_double)
    lib.cg_oasis_ar1.argtypes = [dp, ctypes.c_int, ctypes.c_double,
                                 ctypes.c_double, ctypes.c_double, dp, dp]
    lib.cg_deconvolve.argtypes = [dp, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_double, ctypes.c_double,
                                  ctypes.c_double,
                                  ctypes.POINTER(ctypes.c_float)]
    lib.cg_oasis_pow_table.argtypes = [ctypes.c_double, ctypes.c_int, dp]
    fp = ctypes.POINTER(ctypes.c_float)
    lib.cg_oasis_ar1_flat.argtypes = [fp, ctypes.c_int, ctypes.c_float,
                                      ctypes.c_float, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_double, dp, fp,
                                      dp, dp]
    _lib = lib
  return _lib


def oasis_ar1(y, g, lam=0.0, s_min=0.0):
  """(c, s) of the AR(1) active-set deconvolution of one trace."""
  y = np.ascontiguousarray(y, dtype=np.float64)
  c = np.empty_like(y)
  s = np.empty_like(y)
  dp = ctypes.POINTER(ctypes.c_double)
  rc = _load().cg_oasis_ar1(y.ctypes.data_as(dp), len(y), g, lam, s_min,
                            c.ctypes.data_as(dp), s.ctypes.data_as(dp))
  if rc:
    raise RuntimeError('cg_oasis_ar1 failed: {}'.format(rc))
  return c, s


def oasis_ar1_python(y, g, lam=0.0, s_min=0.0):
  """Pure-python restatement (pools as lists) of the same algorithm."""
  y = np.asarray(y, dtype=np.float64)
  T = len(y)
  P = [[y[0] - lam * (1 - g), 1.0, 0, 1]]
  for t in range(1, T):
    P.append([y[t] - lam * (1 if t == T - 1 else (1 - g)), 1.0, t, 1])
    while len(P) > 1 and (P[-2][0] / P[-2][1] * g**P[-2][3] + s_min >
                          P[-1][0] / P[-1][1]):
      v, w, _, l = P.pop()
      gl = g**P[-1][3]
      P[-1][0] += v * gl
      P[-1][1] += w * gl * gl
      P[-1][3] += l
  c = np.empty(T)
  for v, w, t, l in P:
    c[t:t + l] = max(v / w, 0.0) * g**np.arange(l)
  s = np.zeros(T)
  s[1:] = c[1:] - g * c[:-1]
  return c, s


def oasis_function(signal, threshold=0.5):
  """spike_helper.py:23-29."""
  _, train = oasis_ar1(signal, g=0.95, s_min=.55)
  return np.where(train > threshold, 1.0, 0.0)


def deconvolve_signals(signals, threshold=0.5):
  """spike_helper.py:32-54: (rows, T) calcium traces -> float32 {0,1} trains."""
  if hasattr(signals, 'detach'):
    signals = signals.detach().cpu().numpy()
  signals = np.ascontiguousarray(signals, dtype=np.float64)
  assert signals.ndim == 2
  out = np.empty(signals.shape, dtype=np.float32)
  rc = _load().cg_deconvolve(
      signals.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), signals.shape[0],
      signals.shape[1], 0.95, 0.55, threshold,
      out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
  if rc:
    raise RuntimeError('cg_deconvolve failed: {}'.format(rc))
  return out


# -- on the device (csrc/spikes.hip) -------------------------------------------
OASIS_G, OASIS_S_MIN = 0.95, 0.55  # spike_helper.py:24


def oasis_pow_table(g, n):
  """float64 (n,): pow(g, l) for l < n by the libm call cg_oasis_ar1 makes (the
  device kernel reads its powers from this table: device pow is another
  function, and numpy's vectorised power may be a SIMD variant)."""
  out = np.empty(n, dtype=np.float64)
  rc = _load().cg_oasis_pow_table(
      g, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
  if rc:
    raise RuntimeError('cg_oasis_pow_table failed: {}'.format(rc))
  return out


def oasis_ar1_flat(x, g, s_min=0.0, threshold=0.5, scale=1.0, offset=0.0):
  """(c, s, spikes) of one float32 trace by the device kernel's per-lane loop
  (csrc/oasis_flat.h) compiled for the host: the CPU check of that loop against
  `oasis_ar1`."""
  x = np.ascontiguousarray(x, dtype=np.float32)
  T = len(x)
  gpow = oasis_pow_table(g, T + 1)
  c, s = np.empty(T), np.empty(T)
  spikes = np.empty(T, dtype=np.float32)
  dp, fp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
  rc = _load().cg_oasis_ar1_flat(x.ctypes.data_as(fp), T, scale, offset, g,
                                 s_min, threshold, gpow.ctypes.data_as(dp),
                                 spikes.ctypes.data_as(fp), c.ctypes.data_as(dp),
                                 s.ctypes.data_as(dp))
  if rc:
    raise RuntimeError('cg_oasis_ar1_flat failed: {}'.format(rc))
  return c, s, spikes


_DEVICE_CACHE = {}  # (kind, device, ...) -> tensor


def _device_pow_table(device, g, T):
  """gpow[0 .. T] on `device`, uploaded once per (device, g) and grown on
  demand -- never from inside a launch."""
  import torch
  key = ('gpow', str(device), float(g))
  t = _DEVICE_CACHE.get(key)
  if t is None or t.numel() < T + 1:
    t = _DEVICE_CACHE[key] = torch.from_numpy(oasis_pow_table(g, T + 1)).to(device)
  return t


def _device_workspace(device, nbytes):
  """The pool-stack workspace, one per device, grown on demand and kept (535 MB
  for a cfg2 batch).  Calls share it: they must be ordered on one stream."""
  import torch
  key = ('ws', str(device))
  t = _DEVICE_CACHE.get(key)
  if t is None or t.numel() * 8 < nbytes:
    t = _DEVICE_CACHE[key] = torch.empty((nbytes + 7) // 8, dtype=torch.float64,
                                         device=device)
  return t


def deconvolve_signals_device(signals, threshold=0.5, scale=1.0, offset=0.0,
                              g=OASIS_G, s_min=OASIS_S_MIN, return_cs=False):
  """`deconvolve_signals` on the GPU, bit for bit: a float32 device tensor of
  (rows, T) traces, or of (B, L, C) with the traces along axis 1 (any strides:
  a channel-padded generator output is read in place), -> float32 {0, 1} trains
  of the same logical shape.  The traces deconvolved are (double)(signals *
  scale + offset) with float32 product and sum, i.e. utils.denormalize of the
  float32 array with scale = max - min, offset = min.  return_cs: also the
  float64 (traces, T) calcium and spike-size arrays (tests)."""
  import torch
  from ... import _lib as hip
  if not (torch.is_tensor(signals) and signals.is_cuda):
    raise ValueError('deconvolve_signals_device needs a device tensor '
                     '(deconvolve_signals is the host path)')
  if signals.dtype != torch.float32 or signals.dim() not in (2, 3):
    raise ValueError('float32 (rows, T) or (B, L, C) expected')
  dev = signals.device
  out = torch.empty(signals.shape, dtype=torch.float32, device=dev)
  if signals.dim() == 2:
    rows, T = signals.shape
    n_outer, n_inner = 1, rows
    sx = (0, signals.stride(1), signals.stride(0))
    so = (0, out.stride(1), out.stride(0))
  else:
    n_outer, T, n_inner = signals.shape
    sx = (signals.stride(0), signals.stride(1), signals.stride(2))
    so = (out.stride(0), out.stride(1), out.stride(2))
  traces = n_outer * n_inner
  if traces == 0 or T == 0:
    raise ValueError('empty input')
  lib = hip.load()
  nbytes = lib.cg_oasis_ws_bytes(traces, T)
  if nbytes < 0:
    raise ValueError('cg_oasis_ws_bytes: unsupported shape')
  ws = _device_workspace(dev, nbytes)
  gpow = _device_pow_table(dev, g, T)
  c = s = None
  if return_cs:
    c = torch.empty(traces, T, dtype=torch.float64, device=dev)
    s = torch.empty(traces, T, dtype=torch.float64, device=dev)
  hip.call('cg_oasis_ar1_batched', signals, n_outer, n_inner, T, sx[0], sx[1],
           sx[2], scale, offset, g, s_min, threshold, gpow, out, so[0], so[1],
           so[2], c, s, ws, nbytes, hip.stream())
  return (out, c, s) if return_cs else out
