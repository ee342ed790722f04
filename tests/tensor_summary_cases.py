"""Shared inputs of the cg_tensor_summary tests (tests/test_tensor_summary_host.py
on the CPU, tests/test_hip_tensor_summary.py on the GPU).

A case is one flat float32 buffer and the segment tables into it.  Segments sit
at odd and at 4-aligned offsets in turn and every element outside a segment is
NaN: a read past a segment would flag it.  CHUNK is the kernel's per-workgroup
chunk (csrc/summary.hip: kTsChunk); segments of CHUNK - 1, CHUNK + 1 and
2 CHUNK + 1 elements end, begin and span its tiles."""
import functools
import math
from types import SimpleNamespace

import numpy as np

CHUNK = 4096
NUM_BUCKETS = 30
LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025,
           CHUNK - 1, CHUNK + 1, 2 * CHUNK + 1, 70001)
F32_MAX = np.finfo(np.float32).max
F32_TINY = np.float32(2.0**-149)  # the smallest float32 subnormal

# (b): the pairs (lo, hi) and how many of the 93 values a float32 evaluation of
# the bucket index puts elsewhere than the statement does
INEXACT = (((0.0, 1.0), 6), ((-0.0541, 0.0541), 25), ((-0.3, 0.7), 17))


def lay_out(segments, first_odd=True):
  """-> (buffer, offsets, lengths): the segments at odd / 4-aligned offsets in
  turn, NaN in between and at both ends."""
  offsets, pos = [], 8
  for i, seg in enumerate(segments):
    pos = (pos + 3) // 4 * 4
    if (i % 2 == 0) == first_odd:
      pos += 1 + 2 * (i % 4 == 0)  # 1 or 3 past a multiple of 4
    offsets.append(pos)
    pos += len(seg) + 2
  buf = np.full(pos + 8, np.nan, np.float32)
  for o, seg in zip(offsets, segments):
    buf[o:o + len(seg)] = seg
  return buf, offsets, [len(s) for s in segments]


def exact_boundaries():
  """(a) k/16 - 1, k = 0 .. 30: over 30 buckets the width is 1/16, every value
  sits on a left edge and the last on the clamped top edge."""
  return (np.arange(31, dtype=np.float64) / 16 - 1).astype(np.float32)


def inexact_widths(lo, hi):
  """(b) the float32 values at lo + (j / 30)(hi - lo), j = 0 .. 30 (lo and hi
  the float32 values of the pair), each with its two float32 neighbours,
  clipped to [lo, hi]: 93 values within an ulp of the bucket edges."""
  lo32, hi32 = np.float32(lo), np.float32(hi)
  j = np.arange(31, dtype=np.float64)
  c = (float(lo32) + (j / 30) * (float(hi32) - float(lo32))).astype(np.float32)
  v = np.concatenate([np.nextafter(c, np.float32(-np.inf)), c,
                      np.nextafter(c, np.float32(np.inf))])
  return np.clip(v, lo32, hi32).astype(np.float32)


def float32_index(x, k=NUM_BUCKETS):
  """The bucket index evaluated in float32: what a kernel that does not widen
  to float64 would count."""
  x = np.asarray(x, np.float32)
  mn, mx = x.min(), x.max()
  w = np.float32((mx - mn) / np.float32(k))
  return np.minimum(np.floor((x - mn) / w).astype(np.int64), k - 1)


def statement_index(x, k=NUM_BUCKETS):
  d = np.asarray(x).astype(np.float64)
  mn, mx = d.min(), d.max()
  w = (mx - mn) / np.float64(k)
  return np.minimum(np.floor((d - mn) / w).astype(np.int64), k - 1)


def constants(n):
  """(c) a fresh bias, a fresh gamma, -2.5, and zeros of both signs."""
  zeros = np.zeros(n, np.float32)
  zeros[::2] = -0.0
  return [np.zeros(n, np.float32), np.ones(n, np.float32),
          np.full(n, -2.5, np.float32), zeros]


def extremes(n, rng):
  """(d) float32 subnormals of both signs with +FLT_MAX and -FLT_MAX."""
  v = (rng.randint(-2**22, 2**22, size=n).astype(np.float64) *
       float(F32_TINY)).astype(np.float32)
  assert (np.abs(v) < np.finfo(np.float32).tiny).all()
  v[n // 3], v[2 * n // 3] = F32_MAX, -F32_MAX
  return v


def glorot_uniform(rng, shape, fan_in, fan_out):
  limit = math.sqrt(6.0 / (fan_in + fan_out))
  return rng.uniform(-limit, limit, size=shape).astype(np.float32)


def small_model_weights(rng):
  """(f) initial weights at the shapes of the model tests/test_main_e2e.py
  trains (--num_units 8 --kernel_size 24 --noise_dim 32 --layer_norm on
  (256, 16) signals): glorot_uniform kernels, zero biases and betas, unit
  gammas; generator, then discriminator."""
  from calciumgan_amd import geometry as geo
  hp = SimpleNamespace(num_units=8, kernel_size=24, strides=2, noise_dim=32,
                       num_channels=16, signal_shape=(256, 16))
  k, C = hp.kernel_size, hp.num_channels
  w0 = geo.calculate_noise_shape(hp.signal_shape, hp.noise_dim, geo.NUM_CONVS,
                                 hp.strides)[0]
  nflat = w0 * hp.noise_dim
  out = [glorot_uniform(rng, (hp.noise_dim, nflat), hp.noise_dim, nflat),
         np.zeros(nflat, np.float32)]
  for lay in geo.generator_layers(hp):
    out += [glorot_uniform(rng, (k, 1, lay.cout, lay.cin), k * lay.cout,
                           k * lay.cin), np.zeros(lay.cout, np.float32),
            np.ones(lay.cout, np.float32), np.zeros(lay.cout, np.float32)]
  out += [glorot_uniform(rng, (C, C), C, C), np.zeros(C, np.float32)]
  for lay in geo.discriminator_layers(hp):
    out += [glorot_uniform(rng, (k, lay.cin, lay.cout), k * lay.cin,
                           k * lay.cout), np.zeros(lay.cout, np.float32)]
  flat = geo.discriminator_layers(hp)[-1]
  flat = flat.lout * flat.cout
  out += [glorot_uniform(rng, (flat, 1), flat, 1), np.zeros(1, np.float32)]
  return [w.reshape(-1) for w in out]


CASES = ('lengths', 'lengths_aligned_first', 'forty', 'boundaries', 'inexact',
         'constant', 'extreme', 'nonfinite', 'glorot')


@functools.lru_cache(maxsize=None)
def case(name):
  """-> (buffer, offsets, lengths), read-only."""
  rng = np.random.RandomState(sorted(CASES).index(name) + 20)
  first_odd = True
  if name in ('lengths', 'lengths_aligned_first'):
    # every length at an odd offset in one of the two cases, aligned in the other
    segs = [rng.uniform(-0.05, 0.05, n).astype(np.float32) for n in LENGTHS]
    first_odd = name == 'lengths'
  elif name == 'forty':
    sizes = [LENGTHS[i % 14] for i in range(35)] + [CHUNK + 1, 5000, 2 * CHUNK]
    segs = [rng.normal(0.1 * i, 1 + i, n).astype(np.float32)
            for i, n in enumerate(sizes)]
  elif name == 'boundaries':
    a = exact_boundaries()
    # alone, and repeated past one chunk (every count times 133)
    segs = [a, np.tile(a, 133), a[::-1].copy()]
  elif name == 'inexact':
    segs = [inexact_widths(*pair) for pair, _ in INEXACT]
    segs += [np.tile(segs[1], 45)]  # 4185 values: two tiles
  elif name == 'constant':
    segs = [c for n in (1, 5, 257, CHUNK + 1, 70001) for c in constants(n)]
  elif name == 'extreme':
    segs = [extremes(1025, rng), extremes(CHUNK + 3, rng),
            np.array([F32_MAX, -F32_MAX], np.float32),
            np.array([F32_TINY, -F32_TINY, 0.0], np.float32)]
  elif name == 'nonfinite':
    segs = [rng.uniform(-1, 1, n).astype(np.float32)
            for n in (100, 257, 300, CHUNK + 5, 64)]
    segs[1][200] = np.nan
    segs[3][CHUNK + 1] = np.inf
    segs[3][7] = -np.inf
  elif name == 'glorot':
    segs = small_model_weights(rng)
  else:
    raise KeyError(name)
  buf, offsets, lengths = lay_out(segs, first_odd)
  if name == 'forty':
    # segments may repeat and overlap: two more table entries into the same
    # data, 40 in all
    offsets += [offsets[3], offsets[37] + 100]
    lengths += [lengths[3], 4200]
  if name == 'glorot':
    # as FlatParams lays them out: every tensor 4-aligned, zeros in between
    sizes = [len(s) for s in segs]
    offsets = list(np.cumsum([0] + [(n + 3) // 4 * 4 for n in sizes[:-1]]))
    buf = np.zeros(offsets[-1] + (sizes[-1] + 3) // 4 * 4, np.float32)
    for o, s in zip(offsets, segs):
      buf[o:o + len(s)] = s
    offsets = [int(o) for o in offsets]
  buf.setflags(write=False)
  return buf, tuple(offsets), tuple(lengths)


def segments(name):
  buf, offsets, lengths = case(name)
  return [buf[o:o + n] for o, n in zip(offsets, lengths)]


def statement_rows(values, k=NUM_BUCKETS):
  """(stats [8], buckets [k][3]) of one segment as cg_tensor_summary lays them
  out, from the numpy statements: {n, mn, mx, sum, mean, sq, stddev,
  nonfinite}; the single bucket of equal values in row 0 above zeros; NaN
  statistics and zero rows for a segment with a NaN or an infinity."""
  from calciumgan_amd.gan.utils import summary_helper as sh
  d = np.asarray(values).astype(np.float64).reshape(-1)
  n = np.float64(d.size)
  bad = int((~np.isfinite(d)).sum())
  buckets = np.zeros((k, 3), np.float64)
  if bad:
    return np.array([n] + [np.nan] * 6 + [bad], np.float64), buckets
  st = sh.variable_statistics(values)
  total = d.sum()
  c = d - total / n
  rows = sh.histogram_buckets(values, k)
  buckets[:len(rows)] = rows
  return np.array([n, st['min'], st['max'], total, st['mean'], (c * c).sum(),
                   st['stddev'], 0], np.float64), buckets


@functools.lru_cache(maxsize=None)
def statement(name, k=NUM_BUCKETS):
  """-> (stats (nseg, 8), buckets (nseg, k, 3)) of a case, read-only."""
  rows = [statement_rows(seg, k) for seg in segments(name)]
  out = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
  for a in out:
    a.setflags(write=False)
  return out
