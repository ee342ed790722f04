"""Shared cases of the interval tests (test_spike_intervals_host.py,
test_hip_spike_intervals.py): spike trains, raw word matrices, the loop over
single trains the numpy statement is held to, the three constructions that show
what the figures see and a run directory.  Everything compared is an integer or
a dict."""
import functools
import json

import numpy as np

import triplet_cases
from calciumgan_amd.gan.utils import spike_metrics

# (B, T, C, density)
TRAINS = [
    (1, 3, 1, .5),         # one partly filled word, one neuron
    (2, 50, 3, .5),        # tail bits in the second word
    (2, 64, 5, .5),        # exactly two words, no tail
    (1, 33, 4, .5),        # one bit into a second word
    (3, 300, 102, .01),    # the report's neuron count, sparse
]
MAX_ISIS = [1, 24, 240, 4095]

# raw word matrices of the counting kernel: a wave walks a trial in chunks of 64
# words (63, 64, 65: below, at and past one; 129: a third chunk with one word)
WORD_NEURONS = [1, 3, 17, 102, 512]
WORDS_PER_TRIAL = [1, 2, 63, 64, 65, 129]
WORD_TRIALS = [1, 2, 7]
KINDS = ['dense', 'sparse', 'rare', 'ones', 'zeros', 'edges', 'boundary', 'ends']
SPLIT_CASE = (3, 4000, 2)   # C, trials, wpt: the trials split, with the merge


def trains(B, T, C, density):
  return (np.random.RandomState(1000 * C + T).uniform(size=(B, T, C)) < density
          ).astype(np.float32)


def _random_words(rng, shape, ands):
  w = rng.randint(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
  for _ in range(ands):
    w &= rng.randint(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
  return w


@functools.lru_cache(maxsize=None)
def words(C, trials, wpt, kind='dense'):
  """uint32 (C, trials wpt), read-only:
    dense, sparse, rare   random bits of density 1/2, 1/16, 1/1024 (whole lanes
                          and whole chunks empty between two spikes)
    ones, zeros
    edges      bits 0 and 31 of every word: intervals 31 and 1 in turn, across
               the word boundaries
    boundary   the last bit of the trials 0, 2, ... and the first bit of the
               trials 1, 3, ...: neighbours in memory, one spike a trial, no
               interval
    ends       frame 0 and the last frame of every trial"""
  rng = np.random.RandomState(7919 * C + 31 * trials + wpt)
  shape = (C, trials, wpt)
  if kind in ('dense', 'sparse', 'rare'):
    w = _random_words(rng, shape, {'dense': 0, 'sparse': 3, 'rare': 9}[kind])
  elif kind == 'ones':
    w = np.full(shape, 0xffffffff, np.uint32)
  elif kind == 'edges':
    w = np.full(shape, 0x80000001, np.uint32)
  else:
    w = np.zeros(shape, np.uint32)
    if kind == 'boundary':
      w[:, 0::2, -1] |= np.uint32(0x80000000)
      w[:, 1::2, 0] |= np.uint32(1)
    elif kind == 'ends':
      w[:, :, 0] |= np.uint32(1)
      w[:, :, -1] |= np.uint32(0x80000000)
    elif kind != 'zeros':
      raise ValueError(kind)
  w = np.ascontiguousarray(w.reshape(C, trials * wpt))
  w.setflags(write=False)
  return w


def spikes_of_words(w, trials):
  """uint8 (trials, 32 wpt, C): the frames of uint32 (C, trials wpt) words."""
  C, W = w.shape
  wpt = W // trials
  return spike_metrics.unpack_state_words(w, 32 * wpt).reshape(
      trials, 32 * wpt, C)


@functools.lru_cache(maxsize=None)
def word_counts(C, trials, wpt, kind='dense', max_isi=240):
  """The statement's (hist, moments, counts) of `words(C, trials, wpt, kind)`:
  computed once, shared, read-only."""
  out = spike_metrics.interval_counts(
      spikes_of_words(words(C, trials, wpt, kind), trials), max_isi)
  for x in out:
    x.setflags(write=False)
  return out


def train_loop(spikes, max_isi):
  """The definition, one train at a time, in Python integers."""
  x = np.asarray(spikes)
  N, T, C = x.shape
  hist = [[0] * (max_isi + 1) for _ in range(C)]
  moments = [[0] * 6 for _ in range(C)]
  counts = [[0] * C for _ in range(N)]
  for n in range(N):
    for c in range(C):
      at = [t for t in range(T) if x[n, t, c] != 0]   # NaN != 0, -0.0 == 0
      I = [b - a for a, b in zip(at, at[1:])]
      counts[n][c] = len(at)
      m = moments[c]
      m[0] += len(at)
      m[1] += len(I)
      m[2] += sum(I)
      m[3] += sum(i * i for i in I)
      m[4] += max(len(I) - 1, 0)
      m[5] += sum(i * j for i, j in zip(I, I[1:]))
      for i in I:
        hist[c][min(i, max_isi + 1) - 1] += 1
  return (np.array(hist, np.int64).reshape(C, max_isi + 1),
          np.array(moments, np.int64).reshape(C, 6),
          np.array(counts, np.int64).reshape(N, C))


def identities(spikes, got):
  """The four identities of the statement's integers."""
  hist, moments, counts = got
  s = np.asarray(spikes) != 0
  m = s.sum(1)                                          # (N, C) spikes a train
  T = s.shape[1]
  first = np.where(m > 0, s.argmax(1), 0)
  last = np.where(m > 0, T - 1 - s[:, ::-1].argmax(1), 0)
  assert np.array_equal(counts, m)
  assert np.array_equal(hist.sum(1), moments[:, 1])
  assert np.array_equal(moments[:, 1], np.maximum(m - 1, 0).sum(0))
  assert np.array_equal(moments[:, 2], (last - first).sum(0))
  assert np.array_equal(moments[:, 4], np.maximum(m - 2, 0).sum(0))
  assert np.array_equal(moments[:, 0], counts.sum(0))


# -- what the figures see: 60 trials x 2048 frames x 8 neurons --------------------
SEEN = (60, 2048, 8)


def _trains_of_intervals(draw, seed, shape=SEEN):
  """Trials (N, T, C), uint8: train (n, c) has its first spike at a uniform
  frame below 40 and then the intervals draw(rng) gives (an int array, long
  enough), up to the end of the trial."""
  N, T, C = shape
  rng = np.random.RandomState(seed)
  x = np.zeros(shape, np.uint8)
  for n in range(N):
    for c in range(C):
      t = rng.randint(40) + np.concatenate([[0], np.cumsum(draw(rng))])
      x[n, t[t < T], c] = 1
  return x


def gamma_trains(seed, shape=SEEN):
  """Gamma-renewal trains, shape 4, mean interval about 39 frames (intervals
  rounded up to whole frames): CV 0.5 before the rounding."""
  return _trains_of_intervals(
      lambda rng: np.ceil(rng.gamma(4.0, 39.0 / 4.0, size=400)).astype(np.int64),
      seed, shape)


def bernoulli_trains(seed, p=1.0 / 39.5, shape=SEEN, gain_sigma=0.0):
  """Bernoulli trains of probability p a frame: CV sqrt(1 - p), Fano 1 - p.
  gain_sigma: p times a log-normal gain of mean 1 drawn per trial and shared by
  its neurons, which spreads the counts across trials and nothing else."""
  rng = np.random.RandomState(seed)
  gain = np.exp(gain_sigma * rng.randn(shape[0], 1, 1) - 0.5 * gain_sigma ** 2)
  return (rng.uniform(size=shape) < p * gain).astype(np.uint8)


def alternating_trains(seed, shuffled=False, shape=SEEN):
  """Intervals short (5 .. 14 frames) and long (60 .. 99) in turn; shuffled: the
  same intervals of every train in a random order -- the same histogram, mean
  and CV, no serial correlation."""
  def draw(rng):
    I = np.empty(200, np.int64)
    I[0::2] = rng.randint(5, 15, size=100)
    I[1::2] = rng.randint(60, 100, size=100)
    return I

  x = _trains_of_intervals(draw, seed, shape)
  if not shuffled:
    return x
  rng = np.random.RandomState(seed + 1000)
  N, T, C = shape
  out = np.zeros_like(x)
  for n in range(N):
    for c in range(C):
      t = np.flatnonzero(x[n, :, c])
      I = np.diff(t)
      rng.shuffle(I)
      out[n, t[0] + np.concatenate([[0], np.cumsum(I)]), c] = 1
  return out


def side(spikes, max_isi=240):
  return spike_metrics.interval_counts(spikes, max_isi)


# -- compute_metrics.py --------------------------------------------------------------
run_dir = triplet_cases.run_dir


def same(a, b):
  """Equality of two reports, a NaN equal to a NaN: floats print exactly."""
  return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


def expected_report(real, fake, max_isi=240):
  """The `intervals` dict compute_metrics.py should write for these spikes."""
  ref = side(real[0::2], max_isi)
  floor = spike_metrics.interval_scores(ref, side(real[1::2], max_isi))
  generated = spike_metrics.interval_scores(ref, side(fake[1::2], max_isi))
  return dict(generated=generated, floor=floor, max_isi=max_isi)
