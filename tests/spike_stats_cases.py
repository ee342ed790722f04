"""Inputs and exact statements shared by tests/test_spike_stats.py (CPU) and the
GPU tests of cg_spike_stats / cg_spike_corrcoef / cg_spike_stats_error
(tests/test_hip_spikes.py, tests/test_hip_van_rossum.py).  Batches are (B, T, C)
float32; an entry that is not zero is a spike."""
import functools

import numpy as np

BIN_FRAMES = 12            # 500 ms at 24 Hz
STATS_THREADS = 256        # threads of a workgroup of the statistics kernels
STATS_MAX_LDS = 60 * 1024  # bytes of bin counts and sums a workgroup may hold
ERR_THREADS = 256
ERR_MAX_PARTS = 1024


def trains(B, T, C, seed):
  """A rate per neuron from U(0.02, 0.3); neuron 0 is silent."""
  rng = np.random.RandomState(seed)
  rate = rng.uniform(0.02, 0.3, (1, 1, C))
  sp = (rng.uniform(size=(B, T, C)) < rate).astype(np.float32)
  sp[:, :, 0] = 0.0  # a silent neuron
  return sp


def lds_bytes(T, C):
  """What cg_spike_stats / cg_spike_corrcoef ask of the LDS: C int32 sums and
  one byte per (bin, neuron)."""
  return C * 4 + (T // BIN_FRAMES) * C


def split(C):
  """Workgroups that share a trial's C (C + 1) / 2 pairs."""
  P = C * (C + 1) // 2
  return min(max(-(-P // (STATS_THREADS * 4)), 1), 8)


# (T, C) of the existing tests, kept
GRID = tuple((T, C) for C in (6, 102) for T in (24, 250, 2048))
# name -> (T, C): what each reaches is said in `stats_case`
SHAPES = {
    'c300_t2405': (2405, 300),
    'c240_t3029': (3029, 240),
    'c44_t48': (48, 44),
    'c45_t48': (48, 45),
    'c119_t48': (48, 119),
    'c120_t48': (48, 120),
    'c130_t250': (250, 130),
    'planted_c6_t48': (48, 6),
}
# one byte class over the LDS limit: refused on the host
REFUSED = ((3036, 240), (2412, 300))
CORRCOEF_CASES = ('c300_t2405', 'c240_t3029')


@functools.lru_cache(maxsize=None)
def stats_case(name):
  """name -> (2, T, C) float32 (shared, read-only).
  c300_t2405      nb = 200, 61 200 B of LDS, 5 trailing frames; the second trip
                  of the loops over c += 256; P = 45 150 pairs, `split` capped
                  at 8;
  c240_t3029      nb = 252, exactly 61 440 B, the most that is admitted;
  c44 / c45       P = 990 / 1035: `split` 1 -> 2;
  c119 / c120     P = 7140 / 7260: `split` 7 -> 8;
  c130_t250       read as stored, channel-major and as a slice of a wider
                  buffer by the GPU test;
  planted_c6_t48  neuron 0 fires in every frame (12 a bin: S_00 = 144 nb,
                  covariance exactly 0); neuron 1 "fires" 2.0, -1.0, the
                  smallest float32 subnormal and NaN (each counts); neuron 2
                  holds -0.0 alone (none counts); neurons 3-5 ordinary."""
  T, C = SHAPES[name]
  sp = trains(2, T, C, seed=T + C)
  if name == 'planted_c6_t48':
    sp[:, :, 0] = 1.0
    sp[:, :, 1] = 0.0
    sp[0, [0, 13, 14, 47], 1] = [2.0, -1.0, np.float32(2.0**-149), np.nan]
    sp[1, [11, 12, 30], 1] = [np.nan, np.float32(2.0**-149), -1.0]
    sp[:, :, 2] = -0.0
    assert np.signbit(sp[:, :, 2]).all()
  sp.setflags(write=False)
  return sp


def binary(sp):
  """The host's rule: float32 {0, 1}, 1 where `spikes != 0`."""
  return (np.asarray(sp) != 0).astype(np.float32)


def exact_covariance(sp):
  """The covariances cg_spike_stats states: from the integer 500-ms bin counts
  n of a trial, S_ij = sum_bin n_i n_j and S_i = sum_bin n_i are integers, and
    cov_ij = float32(float64(nb S_ij - S_i S_j) / float64(nb (nb - 1)))
  -- the numerator and the denominator are integers below 2^53, so this rounds
  twice.  (B, T, C) -> (B, C (C + 1) / 2) float32, np.triu_indices order."""
  sp = np.asarray(sp)
  B, T, C = sp.shape
  nb = T // BIN_FRAMES
  assert nb >= 2
  counts = (sp[:, :nb * BIN_FRAMES] != 0).reshape(B, nb, BIN_FRAMES, C).sum(
      2).astype(np.int64)                                   # (B, nb, C)
  S = counts.sum(1)                                          # (B, C)
  Sij = np.einsum('bni,bnj->bij', counts, counts)            # (B, C, C) int64
  num = nb * Sij - S[:, :, None] * S[:, None, :]
  assert Sij.dtype == np.int64 and np.abs(num).max() < 2**53
  iu = np.triu_indices(C)
  cov = num[:, iu[0], iu[1]].astype(np.float64) / np.float64(nb * (nb - 1))
  return cov.astype(np.float32)


# -- cg_spike_stats_error ---------------------------------------------------------
def err_parts(n_fr, n_cov):
  """Workgroups of the error kernel: one per 2048 elements of the longer side,
  1024 at most; beyond 1024 x 2048 elements a thread strides over more than
  eight."""
  n = max(n_fr, n_cov)
  return min(max(-(-n // (ERR_THREADS * 8)), 1), ERR_MAX_PARTS)


# (n_fr, n_cov): nothing, one element, both sides past one workgroup, the last
# size the grid is not capped at, the first it is capped at (ceil(n / 2048) =
# 1025 workgroups wanted; the ninth stride is partial), the rates the long side
ERROR_SIZES = ((0, 5), (1, 0), (2049, 2047), (3, 2097152), (3, 2097152 + 257),
               (2097409, 7))
RANDOM_ERROR_SIZES = ((2049, 2047), (3, 2097409))


def planted_indices(n, parts):
  """Indices of a side of n elements at which the two sets differ: the ends, the
  middle, the last element of the first workgroup's first trip and of the whole
  grid's, and the first elements of the second and of the last trip."""
  stride = parts * ERR_THREADS
  want = [0, n - 1, n // 2, ERR_THREADS - 1, stride - 1, stride,
          (n - 1) // stride * stride]
  out = []
  for i in want:
    if 0 <= i < n and i not in out:
      out.append(i)
  return out


@functools.lru_cache(maxsize=None)
def planted_error_inputs(n_fr, n_cov):
  """(rates_a, rates_b, covs_a, covs_b) float32: each pair equal everywhere but
  at `planted_indices`, where b = 1 and a = 1 + 2^-k with another k = 0, 1, ...
  at every index.  The differences 2^-k and their squares 4^-k are distinct
  powers of two spanning less than 24 bits, so every partial sum of either, in
  any order, is a float32: the four sums are exact."""
  parts = err_parts(n_fr, n_cov)
  rng = np.random.RandomState(n_fr % 1000 + n_cov % 1000)
  out = []
  for n, scale in ((n_fr, 3.0), (n_cov, 0.3)):
    b = (rng.uniform(-1, 1, n) * scale).astype(np.float32)
    a = b.copy()
    idx = planted_indices(n, parts)
    assert len(idx) <= 12                 # 4^-11: 23 bits below 4^0
    for k, i in enumerate(idx):
      b[i] = 1.0
      a[i] = np.float32(1.0 + 2.0**-k)
      assert np.float64(a[i]) - np.float64(b[i]) == 2.0**-k
    a.setflags(write=False)
    b.setflags(write=False)
    out += [a, b]
  return tuple(out)


@functools.lru_cache(maxsize=None)
def random_error_inputs(n_fr, n_cov):
  """The inputs of test_error_sums_against_numpy_and_bitwise_repeatable at other
  sizes: rates uniform in [0, 3), covariances 0.3 N(0, 1)."""
  rng = np.random.RandomState(n_fr % 1000 + 7)
  out = [rng.uniform(0, 3, n_fr).astype(np.float32),
         rng.uniform(0, 3, n_fr).astype(np.float32),
         (rng.randn(n_cov) * 0.3).astype(np.float32),
         (rng.randn(n_cov) * 0.3).astype(np.float32)]
  for a in out:
    a.setflags(write=False)
  return tuple(out)


def error_bars(n_fr, n_cov, sums):
  """Bound on |device - float64| of the four error sums `sums` (float64 of the
  float32 inputs): (d + 2) 2^-24 times the sum of the magnitudes of the terms --
  the terms are not negative, so that is the sum itself -- with d the depth of
  the kernel's summation of that side: the elements a thread adds, six levels of
  the wave sum, three additions that join the four waves and `parts` rows in the
  finishing kernel; the 2 stands for the rounded subtraction and the rounded
  square."""
  parts = err_parts(n_fr, n_cov)
  bars = []
  for n, pair in ((n_fr, sums[:2]), (n_cov, sums[2:])):
    d = -(-n // (parts * ERR_THREADS)) + 6 + 3 + parts
    bars += [(d + 2) * 2.0**-24 * float(s) for s in pair]
  return np.array(bars)
