"""The shared case table of the recording-window tests (tests/test_recording_host.py,
tests/test_hip_window_batch.py): seeded (T, C) float32 recordings as numpy
arrays, the start rows of a batch of windows, the memory layouts the device test
gives the recording and the output, and the error figures an FFT case is held to.

Shapes are the smallest at which each mechanism of csrc/windows.hip can break:
  L and G       every accepted L, 32 .. 8192 (fewest stages / the radix-2 stage
                of an odd log2 L, an even number of radix-4 stages, the radix-2
                stage on a quarter-full image at 128 and on the first full one
                at 512, the cfg2 length, the LDS limit): every geometry of the
                FFT kernel, G = min(16, 8192 / L) in {16, 8, 4, 2, 1} neurons
                per workgroup with its swizzle rows_mask = 32 / G - 1; C in {1,
                3, G + 1, 102} (ragged groups); the 8192-point cases have B = 2
                or 3
  grid stride   FFT: L 32, C 17, B 600: 1200 workgroups' worth > 1024; plain:
                L 64, C 65, B 600: 3000 items of 1024 elements > 2048 workgroups
  renumbering   FFT items = B x groups: the 8 edge starts make it a multiple of
                8 below the grid (the renumbered walk; 24 items at L 1024, C
                17), the 3 impulse starts do not
  starts        0; odd starts; overlapping windows; the same start twice; the
                last valid start T - L; one start beyond it and one negative
                (edge rows repeat)
  plain paths   16-byte rows (C % 4 == 0, padded pitches of 12 included), the
                16-byte flat span (C 17 / 102 at starts with start * C % 4 == 0),
                one by one (odd starts, a (C, T)-stored transposed view, pitches
                of 9), and a span whose length is no multiple of 4 (L 33, C 3)
  raw layouts   contiguous (T, C), a channel-padded pitch, a (C, T)-stored
                transposed view
  outputs       contiguous and padded pitch (the padding must stay NaN)
  affine        one case with (sub, div) = (-1.25, 3.7)
  inputs        an all-zero trace among non-zero ones (its spectrum must be
                exactly zero), unit impulses at t0 in {1, L / 4 + 1, L - 1} (a
                wrong twiddle index moves them), DG traces, normal deviates"""
import functools

import numpy as np

from calciumgan_amd.data import dg

from ifft_cases import higham_bound  # noqa: F401  (the FFT cases' first bar)

FFT_MAX_GRID = 1024   # csrc/windows.hip: kWinFftMaxGrid
PLAIN_MAX_GRID = 2048  # csrc/windows.hip: kWinMaxGrid
PLAIN_ITEM = 1024     # csrc/windows.hip: kWinItemElems


def group(L):
  """Neurons per workgroup of the FFT kernel of csrc/windows.hip."""
  return min(16, 8192 // L)


def _dg(T, C, seed):
  return np.ascontiguousarray(dg.make_recording(C, T, seed)[0].T)


def _normal(T, C, seed):
  return np.random.RandomState(seed).standard_normal((T, C)).astype(np.float32)


def _zero_trace(T, C, seed):
  x = _normal(T, C, seed)
  x[:, 2] = 0.0
  return x


def _impulses(L):
  """Three windows back to back, window b with a unit impulse of neuron 0 (and
  -2 of neuron 1) at t0 = (1, L / 4 + 1, L - 1)[b]."""
  x = np.zeros((3 * L, 2), dtype=np.float32)
  for b, t0 in enumerate((1, L // 4 + 1, L - 1)):
    x[b * L + t0, 0] = 1.0
    x[b * L + t0, 1] = -2.0
  return x


def _edge_starts(T, L):
  return np.array([0, 1, 3, 4, 4, T - L, T - L + 5, -3], dtype=np.int32)


def _many_starts(T, L, B, seed):
  return np.random.RandomState(seed).randint(-5, T - L + 6, size=B).astype(
      np.int32)


def _case(L, C, raw, starts=None, lin='contig', lout='contig', sub=0.0, div=1.0,
          fft=True):
  return dict(L=L, C=C, raw=raw, starts=starts, lin=lin, lout=lout, sub=sub,
              div=div, fft=fft)


# name -> case; raw: builder of the (T, C) recording; starts: builder from
# (T, L), default _edge_starts; lin: 'contig', 'padded' (channel pitch C + 3),
# 'padded4' (pitch C + 4), 'transposed' (stored (C, T)); lout: 'contig',
# 'padded' (pitch + 3), 'padded4' (pitch + 4); fft: the case is also an FFT case
_TABLE = {
    'l32_c1_dg': _case(32, 1, lambda: _dg(72, 1, 1)),
    'l32_c17_normal': _case(32, 17, lambda: _normal(72, 17, 2)),
    'l32_c102_normal': _case(32, 102, lambda: _normal(72, 102, 3)),
    'l32_impulses': _case(32, 2, lambda: _impulses(32),
                          lambda T, L: np.array([0, L, 2 * L], np.int32)),
    'l32_c17_grid_stride': _case(32, 17, lambda: _normal(200, 17, 4),
                                 lambda T, L: _many_starts(T, L, 600, 5)),
    'l33_c3_plain_tail': _case(33, 3, lambda: _normal(80, 3, 6), fft=False),
    'l64_c3_dg': _case(64, 3, lambda: _dg(104, 3, 7)),
    'l64_c17_normal': _case(64, 17, lambda: _normal(104, 17, 8)),
    'l64_impulses': _case(64, 2, lambda: _impulses(64),
                          lambda T, L: np.array([0, L, 2 * L], np.int32)),
    'l64_c5_transposed': _case(64, 5, lambda: _normal(104, 5, 9),
                               lin='transposed'),
    'l64_c65_plain_grid_stride': _case(
        64, 65, lambda: _normal(300, 65, 10),
        lambda T, L: _many_starts(T, L, 600, 11), fft=False),
    'l128_c17_normal': _case(128, 17, lambda: _normal(200, 17, 23)),
    'l128_impulses': _case(128, 2, lambda: _impulses(128),
                           lambda T, L: np.array([0, L, 2 * L], np.int32)),
    'l256_c8_dg': _case(256, 8, lambda: _dg(300, 8, 12)),
    'l256_c8_dg_affine': _case(256, 8, lambda: _dg(300, 8, 12), sub=-1.25,
                               div=3.7),
    'l256_c17_normal': _case(256, 17, lambda: _normal(300, 17, 13)),
    'l256_impulses': _case(256, 2, lambda: _impulses(256),
                           lambda T, L: np.array([0, L, 2 * L], np.int32)),
    'l256_c6_padded_in': _case(256, 6, lambda: _dg(300, 6, 14), lin='padded'),
    'l256_c8_padded4_in': _case(256, 8, lambda: _dg(300, 8, 15), lin='padded4'),
    'l256_c6_padded_out': _case(256, 6, lambda: _normal(300, 6, 16),
                                lout='padded'),
    'l256_c8_padded4_out': _case(256, 8, lambda: _normal(300, 8, 17),
                                 lout='padded4'),
    'l256_c4_zero_trace': _case(256, 4, lambda: _zero_trace(300, 4, 18)),
    'l512_c17_dg': _case(512, 17, lambda: _dg(580, 17, 24)),
    'l512_impulses': _case(512, 2, lambda: _impulses(512),
                           lambda T, L: np.array([0, L, 2 * L], np.int32)),
    # G = 8: C = G + 1; 8 starts x 3 groups = 24 items at C = 17
    'l1024_c9_normal': _case(1024, 9, lambda: _normal(1094, 9, 25)),
    'l1024_c17_dg': _case(1024, 17, lambda: _dg(1094, 17, 26)),
    'l1024_impulses': _case(1024, 2, lambda: _impulses(1024),
                            lambda T, L: np.array([0, L, 2 * L], np.int32)),
    'l1024_c5_transposed': _case(1024, 5, lambda: _normal(1094, 5, 27),
                                 lin='transposed'),
    'l2048_c102_dg': _case(2048, 102, lambda: _dg(2100, 102, 19)),
    'l2048_c5_normal': _case(2048, 5, lambda: _normal(2100, 5, 20)),
    'l2048_impulses': _case(2048, 2, lambda: _impulses(2048),
                            lambda T, L: np.array([0, L, 2 * L], np.int32)),
    # G = 2: C = G + 1
    'l4096_c3_dg': _case(4096, 3, lambda: _dg(4166, 3, 28)),
    'l4096_impulses': _case(4096, 2, lambda: _impulses(4096),
                            lambda T, L: np.array([0, L, 2 * L], np.int32)),
    'l4096_c2_normal': _case(4096, 2, lambda: _normal(4166, 2, 29),
                             lout='padded'),
    'l8192_c1_dg': _case(8192, 1, lambda: _dg(8260, 1, 21),
                         lambda T, L: np.array([1, T - L + 5], np.int32)),
    'l8192_c2_normal': _case(8192, 2, lambda: _normal(8260, 2, 22),
                             lambda T, L: np.array([7, T - L], np.int32)),
    'l8192_impulses': _case(8192, 2, lambda: _impulses(8192),
                            lambda T, L: np.array([0, L, 2 * L], np.int32)),
}
CASES = tuple(_TABLE)
FFT_CASES = tuple(n for n in CASES if _TABLE[n]['fft'])


def fft_items(name):
  """Workgroup items of the FFT kernel for the case: windows x neuron groups."""
  c = case(name)
  return len(c['starts']) * (-(-c['C'] // group(c['L'])))


@functools.lru_cache(maxsize=None)
def case(name):
  """dict(raw (T, C) float32 read-only, starts int32 (B,) read-only, L, C, lin,
  lout, sub, div, fft)."""
  c = dict(_TABLE[name])
  raw = np.ascontiguousarray(c['raw'](), dtype=np.float32)
  assert raw.ndim == 2 and raw.shape[1] == c['C']
  starts = (c['starts'] or _edge_starts)(raw.shape[0], c['L'])
  starts = np.ascontiguousarray(starts, dtype=np.int32)
  raw.setflags(write=False)
  starts.setflags(write=False)
  c.update(raw=raw, starts=starts)
  return c


@functools.lru_cache(maxsize=None)
def windows(name):
  """(B, L, C) float32: the windows themselves, written out with np.pad (not
  with the statement's clip): a start before the recording or past T - L
  repeats the edge row."""
  c = case(name)
  raw, L = c['raw'], c['L']
  T = raw.shape[0]
  pad = L + int(np.abs(c['starts']).max()) + 8
  padded = np.pad(raw, ((pad, pad), (0, 0)), mode='edge')
  out = np.stack([padded[pad + int(s):pad + int(s) + L] for s in c['starts']])
  assert out.shape == (len(c['starts']), L, raw.shape[1]) and T > L
  out.setflags(write=False)
  return out


@functools.lru_cache(maxsize=None)
def reference(name):
  """(B, L, C) complex128: the float64 forward FFT along time of the float32
  windows."""
  y = np.fft.fft(windows(name).astype(np.float64), axis=1)
  y.setflags(write=False)
  return y


def as_complex(y):
  """(B, L, 2C) [real | imag] -> (B, L, C) complex128."""
  y = np.asarray(y, dtype=np.float64)
  C = y.shape[2] // 2
  return y[..., :C] + 1j * y[..., C:]


def trace_errors(y, name):
  """e = ||z - z64||_2 / ||z64||_2 of the complex spectrum per (window, neuron)
  as a (B, C) float64 array, NaN where z64 is all zero -- and there z must be
  exactly zero."""
  z64 = reference(name)
  z = as_complex(y) if not np.iscomplexobj(y) else np.asarray(y, np.complex128)
  assert z.shape == z64.shape, (z.shape, z64.shape)
  norm = np.sqrt((np.abs(z64) ** 2).sum(axis=1))
  err = np.sqrt((np.abs(z - z64) ** 2).sum(axis=1))
  zero = norm == 0
  assert not z.transpose(0, 2, 1)[zero].any(), name
  with np.errstate(invalid='ignore', divide='ignore'):
    return np.where(zero, np.nan, err / norm)


@functools.lru_cache(maxsize=None)
def single_precision_errors(name):
  """The same errors of scipy.fft.fft on the complex64 input (single-precision
  pocketfft: the stand-in for the reference's tf.signal.fft)."""
  import scipy.fft
  y = scipy.fft.fft(windows(name).astype(np.complex64), axis=1)
  assert y.dtype == np.complex64
  return trace_errors(y, name)


def check_accuracy(y, name):
  """Both conditions of ifft_cases.check_accuracy on a (B, L, 2C) un-normalised
  result; returns (max e, max e_ref)."""
  L = case(name)['L']
  e = trace_errors(y, name)
  e_ref = single_precision_errors(name)
  if np.isnan(e).all():
    return 0.0, 0.0
  worst, worst_ref = float(np.nanmax(e)), float(np.nanmax(e_ref))
  print('%s: max e %.3g, max e_ref %.3g (ratio %.2f), Higham bound %.3g' % (
      name, worst, worst_ref, worst / worst_ref if worst_ref else np.inf,
      higham_bound(L)))
  assert worst <= higham_bound(L), (name, worst, higham_bound(L))
  assert worst <= 4 * worst_ref, (name, worst, worst_ref)
  return worst, worst_ref
