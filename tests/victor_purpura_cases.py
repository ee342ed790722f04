"""Inputs and closed forms shared by tests/test_victor_purpura_host.py and
tests/test_hip_victor_purpura.py.  Trains are (n, T) float32 of {0, 1}."""
import numpy as np

from van_rossum_cases import random_trains

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
