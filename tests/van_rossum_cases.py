"""Inputs and reference statements shared by tests/test_van_rossum_host.py and
tests/test_hip_van_rossum.py."""
import functools

import numpy as np

from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import spike_metrics


def random_trains(n, T, density, seed):
  return (np.random.RandomState(seed).uniform(size=(n, T)) < density
          ).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _dg(C, T, trials):
  d = dg.make_dataset(num_neurons=C, sequence_length=T, num_segments=trials)
  return np.ascontiguousarray(d['spikes'], dtype=np.float32)  # (trials, T, C)


def dg_batch(C, T, trials):
  """(trials, T, C) float32 DG spike trains (a copy)."""
  return _dg(C, T, trials).copy()


def dg_trial(C, T):
  """(C, T) float32: one DG trial."""
  return np.ascontiguousarray(_dg(C, T, 1)[0].T)


def gram_reference(spikes, tau=1.0):
  """S = A E A^T as spike_metrics.van_rossum_distance forms it."""
  owner, frame = np.nonzero(spikes)
  t = frame / float(spike_metrics.FRAME_RATE)
  E = np.exp(-np.abs(t[:, None] - t[None, :]) / tau)
  A = np.zeros((len(spikes), len(t)), np.float64)
  A[owner, np.arange(len(t))] = 1.0
  return A @ E @ A.T


def correlation_cases():
  """name -> (n, T) trains: the inputs of the correlation tests, CPU and GPU."""
  rng = np.random.RandomState(21)
  special = (rng.uniform(size=(5, 480)) < 0.2).astype(np.float32)
  special[0] = 0.0           # silent
  special[1] = 1.0           # full
  special[3] = special[2]    # identical trains
  return {
      'dg102': dg_trial(102, 2048),
      'dg6': dg_trial(6, 480),
      'dense': random_trains(40, 2048, 0.5, seed=4),
      'full98': random_trains(40, 2048, 0.98, seed=5),
      'two_bins': random_trains(17, 24, 0.3, seed=6),
      'special': special,
  }
