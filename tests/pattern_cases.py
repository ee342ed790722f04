"""Inputs shared by tests/test_pattern_hist_host.py and
tests/test_hip_pattern_hist.py: spike samples (N, T, C) and the directories
compute_surrogate_metrics.py reads."""
import os
import pickle

import numpy as np


def samples(N, T, C, seed=0, rate=0.3):
  """float32 (N, T, C) of {0, 1}, each frame a spike with probability `rate`."""
  rng = np.random.RandomState(seed)
  return (rng.random_sample((N, T, C)) < rate).astype(np.float32)


def calcium(trains, rng, g=0.95, noise=0.05):
  """float32 (n, L, C) AR(1) traces c[t] = g c[t - 1] + s[t] of the (n, L, C)
  trains, plus a little noise: what OASIS turns back into (nearly) the trains."""
  c = trains.astype(np.float64).copy()
  for t in range(1, c.shape[1]):
    c[:, t] += g * c[:, t - 1]
  return (c + noise * rng.standard_normal(c.shape)).astype(np.float32)


def surrogate_dirs(root, n=3000, L=6, C=2, seed=7):
  """(input_dir, output_dir) under `root` as compute_surrogate_metrics.py wants
  them: ground_truth.pkl / surrogate.pkl with 'spikes' (n, C, L), generated.pkl
  with 'signals' (n, L, C).  Returns also the generated signals."""
  rng = np.random.RandomState(seed)
  input_dir, output_dir = os.path.join(root, 'in'), os.path.join(root, 'out')
  os.makedirs(input_dir)
  os.makedirs(output_dir)
  for name in ('surrogate', 'ground_truth'):
    spikes = (rng.random_sample((n, C, L)) < 0.3).astype(np.float32)
    with open(os.path.join(input_dir, name + '.pkl'), 'wb') as file:
      pickle.dump({'spikes': spikes}, file)
  trains = (rng.random_sample((n, L, C)) < 0.3).astype(np.float32)
  signals = calcium(trains, rng)
  with open(os.path.join(output_dir, 'generated.pkl'), 'wb') as file:
    pickle.dump({'signals': signals}, file)
  return input_dir, output_dir, signals
