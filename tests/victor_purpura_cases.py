"""Inputs and closed forms shared by tests/test_victor_purpura_host.py and
tests/test_hip_victor_purpura.py.  Trains are (n, T) float32 of {0, 1}; the
named cases of `grid_case` are whole batches (B, T, C)."""
import functools

import numpy as np

from van_rossum_cases import dg_batch, random_trains

QS = (1.0, 0.375, 7.3)
# trains of the crafted trial: counts on both sides of every 16- and 64-column
# strip boundary of the kernel
CRAFTED_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def first_set():
  """(7, 96) at density 0.25 with one silent train, one full train and two
  identical trains."""
  sp = random_trains(7, 96, 0.25, seed=31)
  sp[0] = 0.0
  sp[1] = 1.0
  sp[3] = sp[2]
  return sp


def second_set():
  """(17, 40) at density 0.5."""
  return random_trains(17, 40, 0.5, seed=32)


def crafted_trial():
  """(13, 200): trains holding exactly CRAFTED_COUNTS spikes at random frames,
  one all-ones train (200 spikes) and one train identical to another (the copy
  of the 33-spike train is the thirteenth: eleven counts, the full train and a
  copy do not fit in twelve); the 1-spike train fires at frame 0, the 15-spike
  train holds frame T - 1 and the 16-spike train holds both ends."""
  T = 200
  rng = np.random.RandomState(33)
  sp = np.zeros((len(CRAFTED_COUNTS) + 2, T), np.float32)
  for i, n in enumerate(CRAFTED_COUNTS):
    sp[i, rng.permutation(T)[:n]] = 1.0
  sp[1] = 0.0
  sp[1, 0] = 1.0
  for i, ends in ((2, [T - 1]), (3, [0, T - 1])):
    inner = rng.permutation(np.arange(1, T - 1))[:CRAFTED_COUNTS[i] - len(ends)]
    sp[i] = 0.0
    sp[i, list(ends) + list(inner)] = 1.0
  sp[11] = 1.0
  sp[12] = sp[7]
  assert tuple(int(v) for v in sp[:11].sum(1)) == CRAFTED_COUNTS
  return sp


def counts_difference(sp):
  """q = 0: shifts are free, D = |n_i - n_j|."""
  n = (np.asarray(sp) != 0).sum(1).astype(np.float64)
  return np.abs(n[:, None] - n[None, :])


def unmatched_spikes(sp):
  """q / 24 >= 2: a shift by a frame costs what delete + insert cost, so only
  coincident spikes are kept: D = n_i + n_j - 2 |f_i & f_j| (0 on the
  diagonal)."""
  s = (np.asarray(sp) != 0).astype(np.float64)
  n = s.sum(1)
  return n[:, None] + n[None, :] - 2.0 * (s @ s.T)


# -- batches past one pass of the pair kernel's grid ------------------------------
# cg_victor_purpura runs at most 512 workgroups of 16 row slots; a slot walks
# the pairs p, p + 8192, ... and keeps its boundary column in one workspace line
ROW_SLOTS = 512 * 16
GRID_CASES = ('reuse_3x96x102', 'reuse_40x48x27', 'long_1x2048x6',
              't16384_1x16384x3', 'dg_2x2048x102', 'decode_1x4x4096')


def _uniform_trials(B, T, C, seed, density):
  return (np.random.RandomState(seed).uniform(size=(B, T, C)) < density
          ).astype(np.float32)


@functools.lru_cache(maxsize=None)
def grid_case(name):
  """name -> (B, T, C) float32 trains (shared, read-only).
  reuse_3x96x102    a density per train from U(0.02, 0.9), train 0 of every
                    trial silent and train 1 full: 15 453 pairs on 8192 slots,
                    so 7261 slots walk a second pair whose counts have nothing
                    to do with the first one's;
  reuse_40x48x27    density 0.5; 351 pairs a trial is no multiple of the four
                    rows of a wave, so a wave's rows straddle trials;
  long_1x2048x6     2048, 1024 (every second frame), ~0.3 T, exactly 17, one (at
                    frame 2047) and no spikes: the longest pair is 2048 against
                    1024 -- 64 strips of 129 blocks, the boundary line used up
                    to row T of its pitch T + 1 -- beside pairs a hundred times
                    shorter in the same wave;
  t16384_1x16384x3  density 0.02 with spikes planted at frames 0, 16383 (the
                    largest index the uint16 storage must hold) and 255 / 256;
  dg_2x2048x102     the workload's shape: two DG trials, 10 302 pairs;
  decode_1x4x4096   density 0.5 at the largest admitted C: 8 386 560 pairs."""
  if name == 'reuse_3x96x102':
    B, T, C = 3, 96, 102
    rng = np.random.RandomState(51)
    density = rng.uniform(0.02, 0.9, size=(B, 1, C))
    sp = (rng.uniform(size=(B, T, C)) < density).astype(np.float32)
    sp[:, :, 0] = 0.0
    sp[:, :, 1] = 1.0
  elif name == 'reuse_40x48x27':
    sp = _uniform_trials(40, 48, 27, seed=52, density=0.5)
  elif name == 'long_1x2048x6':
    T = 2048
    rng = np.random.RandomState(53)
    sp = np.zeros((1, T, 6), np.float32)
    sp[0, :, 0] = 1.0
    sp[0, ::2, 1] = 1.0
    sp[0, :, 2] = rng.uniform(size=T) < 0.3
    sp[0, np.sort(rng.permutation(T)[:17]), 3] = 1.0
    sp[0, T - 1, 4] = 1.0
    assert tuple(int(v) for v in sp[0].sum(0)[[0, 1, 3, 4, 5]]) == (
        2048, 1024, 17, 1, 0)
  elif name == 't16384_1x16384x3':
    sp = _uniform_trials(1, 16384, 3, seed=54, density=0.02)
    sp[0, [0, 16383], 0] = 1.0
    sp[0, [255, 256], 1] = 1.0
    sp[0, [256, 16383], 2] = 1.0
  elif name == 'dg_2x2048x102':
    sp = dg_batch(102, 2048, 2)
  elif name == 'decode_1x4x4096':
    sp = _uniform_trials(1, 4, 4096, seed=55, density=0.5)
  else:
    raise KeyError(name)
  sp.setflags(write=False)
  return sp


def pair_count(sp):
  B, _, C = sp.shape
  return B * C * (C - 1) // 2


def double_loop_pair(a, b, qf):
  """The plain double loop of spike_metrics.victor_purpura_distance for one pair
  of trains (T,), with the frame-grid cost fl(qf |f_k - f_l|) of the statement
  in place of q |t_k - t_l| in seconds: the statement's operations, cell by
  cell, so its bits."""
  fa = [int(f) for f in np.nonzero(a)[0]]
  fb = [int(f) for f in np.nonzero(b)[0]]
  prev = [float(l) for l in range(len(fb) + 1)]
  for k in range(1, len(fa) + 1):
    f = fa[k - 1]
    row = [float(k)]
    left = row[0]
    for l in range(1, len(fb) + 1):
      left = min(prev[l] + 1.0, left + 1.0, prev[l - 1] + qf * abs(f - fb[l - 1]))
      row.append(left)
    prev = row
  return prev[-1]
