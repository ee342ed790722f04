"""The shared case table of the inverse-FFT tests (tests/test_fft_host.py,
tests/test_hip_ifft.py): seeded (B, T, 2C) float32 spectra in the [real | imag]
layout of utils.fft_channels, as numpy arrays, with the memory layout the device
test gives them, and the two error figures every case is held to.

Shapes are the smallest at which each mechanism of csrc/ifft.hip can break:
every accepted T, 32 .. 8192 (fewest stages / the radix-2 stage of an odd log2
T, an even number of radix-4 stages, the radix-2 stage on a quarter-full image
at 128 and on the first full one at 512, the cfg2 length, the LDS limit), which
is every geometry G = min(16, 8192 / T) in {16, 8, 4, 2, 1} with its row swizzle
rows_mask = 32 / G - 1; C in {1, 3, G + 1, 102} (ragged groups); B x groups a
multiple of 8 below the 1024-workgroup grid (the renumbered walk of the items),
no multiple of 8, and past one pass of the grid."""
import functools

import numpy as np

from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import utils

MAX_GRID = 1024  # csrc/ifft.hip: kIfftMaxGrid


def group(T):
  """Neurons per workgroup of csrc/ifft.hip."""
  return min(16, 8192 // T)


def _dg(B, T, C, seed):
  """fft_channels of B DG segments (normalised traces of make_dataset)."""
  d = dg.make_dataset(num_neurons=C, sequence_length=T, num_segments=B, seed=seed)
  return utils.fft_channels(d['signals'])


def _normal(B, T, C, seed):
  return np.random.RandomState(seed).standard_normal((B, T, 2 * C)).astype(
      np.float32)


def _bins(T):
  """One sample per k0 in {1, T/4 + 1, T - 1}: neuron 0 has a real 1 in bin k0,
  neuron 1 an imaginary 1 (a wrong twiddle index in one stage moves it)."""
  ks = (1, T // 4 + 1, T - 1)
  x = np.zeros((len(ks), T, 4), dtype=np.float32)
  for b, k0 in enumerate(ks):
    x[b, k0, 0] = 1.0
    x[b, k0, 3] = 1.0
  return x


def _zero_trace(B, T, C, seed):
  x = _normal(B, T, C, seed)
  x[:, :, 2] = 0.0
  x[:, :, C + 2] = 0.0
  return x


# name -> (spectra builder, C, scale, offset, input layout, output layout)
# input layouts: 'contig', 'padded' (channel pitch > 2C), 'permuted' (stored
# (B, 2C, T), viewed (B, T, 2C)); output: 'contig' or 'padded' (pitch > C)
_TABLE = {
    't32_c1_dg': (lambda: _dg(3, 32, 1, 1), 1, 1.0, 0.0, 'contig', 'contig'),
    't32_c17_normal': (lambda: _normal(2, 32, 17, 2), 17, 1.0, 0.0, 'contig',
                       'contig'),
    't32_bins': (lambda: _bins(32), 2, 1.0, 0.0, 'contig', 'contig'),
    't64_c3_dg': (lambda: _dg(2, 64, 3, 3), 3, 1.0, 0.0, 'contig', 'contig'),
    't64_c17_normal': (lambda: _normal(2, 64, 17, 15), 17, 1.0, 0.0, 'contig',
                       'contig'),
    't64_bins': (lambda: _bins(64), 2, 1.0, 0.0, 'contig', 'contig'),
    't64_zeros': (lambda: np.zeros((2, 64, 6), np.float32), 3, 1.0, 0.0,
                  'contig', 'contig'),
    't64_c5_permuted': (lambda: _normal(3, 64, 5, 4), 5, 1.0, 0.0, 'permuted',
                        'contig'),
    't128_c17_normal': (lambda: _normal(2, 128, 17, 16), 17, 1.0, 0.0, 'contig',
                        'contig'),
    't128_bins': (lambda: _bins(128), 2, 1.0, 0.0, 'contig', 'contig'),
    't256_c8_dg': (lambda: _dg(2, 256, 8, 5), 8, 1.0, 0.0, 'contig', 'contig'),
    't256_c8_dg_affine': (lambda: _dg(2, 256, 8, 5), 8, 0.37, -1.25, 'contig',
                          'contig'),
    't256_c17_normal': (lambda: _normal(2, 256, 17, 6), 17, 1.0, 0.0, 'contig',
                        'contig'),
    't256_bins': (lambda: _bins(256), 2, 1.0, 0.0, 'contig', 'contig'),
    't256_c6_padded_in': (lambda: _dg(2, 256, 6, 7), 6, 1.0, 0.0, 'padded',
                          'contig'),
    't256_c6_padded_out': (lambda: _normal(2, 256, 6, 8), 6, 1.0, 0.0, 'contig',
                           'padded'),
    't256_c4_zero_trace': (lambda: _zero_trace(2, 256, 4, 9), 4, 1.0, 0.0,
                           'contig', 'contig'),
    't512_c17_dg': (lambda: _dg(2, 512, 17, 17), 17, 1.0, 0.0, 'contig',
                    'contig'),
    't512_bins': (lambda: _bins(512), 2, 1.0, 0.0, 'contig', 'contig'),
    # G = 8: C = G + 1
    't1024_c9_normal': (lambda: _normal(2, 1024, 9, 18), 9, 1.0, 0.0, 'contig',
                        'contig'),
    't1024_bins': (lambda: _bins(1024), 2, 1.0, 0.0, 'contig', 'contig'),
    # 3 samples x 8 groups = 24 items: a multiple of 8 below the grid cap
    't1024_c64_renumbered': (lambda: _normal(3, 1024, 64, 19), 64, 1.0, 0.0,
                             'contig', 'contig'),
    't1024_c5_permuted': (lambda: _normal(3, 1024, 5, 20), 5, 1.0, 0.0,
                          'permuted', 'padded'),
    't2048_c102_dg': (lambda: _dg(2, 2048, 102, 10), 102, 1.0, 0.0, 'contig',
                      'contig'),
    't2048_c5_normal': (lambda: _normal(2, 2048, 5, 11), 5, 1.0, 0.0, 'contig',
                        'contig'),
    't2048_bins': (lambda: _bins(2048), 2, 1.0, 0.0, 'contig', 'contig'),
    # G = 2: C = G + 1
    't4096_c3_dg': (lambda: _dg(2, 4096, 3, 21), 3, 1.0, 0.0, 'contig',
                    'contig'),
    't4096_bins': (lambda: _bins(4096), 2, 1.0, 0.0, 'contig', 'contig'),
    't4096_c2_affine': (lambda: _dg(2, 4096, 2, 22), 2, 0.37, -1.25, 'contig',
                        'contig'),
    't8192_c1_dg': (lambda: _dg(2, 8192, 1, 12), 1, 1.0, 0.0, 'contig',
                    'contig'),
    't8192_c2_normal': (lambda: _normal(2, 8192, 2, 13), 2, 1.0, 0.0, 'contig',
                        'contig'),
    't8192_bins': (lambda: _bins(8192), 2, 1.0, 0.0, 'contig', 'contig'),
    # 600 samples x 2 groups of 16 neurons = 1200 workgroups' worth > 1024
    't32_c17_grid_stride': (lambda: _normal(600, 32, 17, 14), 17, 1.0, 0.0,
                            'contig', 'contig'),
}
CASES = tuple(_TABLE)


def items(name):
  """Workgroup items of csrc/ifft.hip for the case: samples x neuron groups."""
  x, C = case(name)[:2]
  return x.shape[0] * (-(-C // group(x.shape[1])))


@functools.lru_cache(maxsize=None)
def case(name):
  """(x (B, T, 2C) float32 read-only, C, scale, offset, input layout, output
  layout)."""
  build, C, scale, offset, lin, lout = _TABLE[name]
  x = np.ascontiguousarray(build(), dtype=np.float32)
  assert x.ndim == 3 and x.shape[2] == 2 * C
  x.setflags(write=False)
  return x, C, scale, offset, lin, lout


def denormalised(name):
  """The transform's float32 input: x * scale + offset, float32 product, then
  float32 sum (what the kernel forms)."""
  x, _, scale, offset, _, _ = case(name)
  return (x * np.float32(scale)).astype(np.float32) + np.float32(offset)


def _complex(name, dtype):
  x = denormalised(name)
  C = x.shape[2] // 2
  z = np.empty(x.shape[:2] + (C,), dtype=dtype)
  z.real = x[..., :C]
  z.imag = x[..., C:]
  return z


@functools.lru_cache(maxsize=None)
def reference(name):
  """(B, T, C) float64: the real part of the complex128 inverse FFT of the
  float32 input."""
  y = np.fft.ifft(_complex(name, np.complex128), axis=1).real
  y.setflags(write=False)
  return y


def trace_errors(y, name):
  """e = ||y - y64||_2 / ||y64||_2 per (sample, neuron) as a (B, C) float64
  array, NaN where y64 is all zero -- and there y must be exactly zero."""
  y64 = reference(name)
  y = np.asarray(y, dtype=np.float64)
  assert y.shape == y64.shape, (y.shape, y64.shape)
  norm = np.sqrt((y64 * y64).sum(axis=1))
  err = np.sqrt(((y - y64) ** 2).sum(axis=1))
  zero = norm == 0
  assert not y.transpose(0, 2, 1)[zero].any(), name
  with np.errstate(invalid='ignore', divide='ignore'):
    return np.where(zero, np.nan, err / norm)


@functools.lru_cache(maxsize=None)
def single_precision_errors(name):
  """The same errors of scipy.fft.ifft on the complex64 input (single-precision
  pocketfft: the stand-in for the reference's tf.signal.ifft)."""
  import scipy.fft
  z = _complex(name, np.complex64)
  y = scipy.fft.ifft(z, axis=1)
  assert y.dtype == np.complex64
  return trace_errors(y.real, name)


def higham_bound(T):
  """log2(T) eta, eta = mu + gamma_4 (sqrt(2) + mu), gamma_4 = 4u / (1 - 4u),
  u = 2^-24, mu = 2u: Higham's bound on the relative 2-norm error of a radix-2
  float32 FFT with twiddles good to 2 ulp (Accuracy and Stability of Numerical
  Algorithms, 2nd ed., theorem 24.2); a higher radix that fuses radix-2 stages
  meets it too."""
  u = 2.0 ** -24
  mu = 2 * u
  gamma4 = 4 * u / (1 - 4 * u)
  return np.log2(T) * (mu + gamma4 * (np.sqrt(2.0) + mu))


def check_accuracy(y, name):
  """Both conditions on a (B, T, C) result; returns (max e, max e_ref)."""
  T = case(name)[0].shape[1]
  e = trace_errors(y, name)
  e_ref = single_precision_errors(name)
  if np.isnan(e).all():
    return 0.0, 0.0
  worst, worst_ref = float(np.nanmax(e)), float(np.nanmax(e_ref))
  print('%s: max e %.3g, max e_ref %.3g (ratio %.2f), Higham bound %.3g' % (
      name, worst, worst_ref, worst / worst_ref if worst_ref else np.inf,
      higham_bound(T)))
  assert worst <= higham_bound(T), (name, worst, higham_bound(T))
  assert worst <= 4 * worst_ref, (name, worst, worst_ref)
  return worst, worst_ref
