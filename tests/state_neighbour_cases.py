"""Shared cases of the population-state tests (test_state_neighbours_host.py,
test_hip_state_neighbours.py): sets of states, the double loop the numpy
statement is held to, the clipped-gain construction and a small DG run
directory.  Everything compared is an integer or a dict."""
import functools
import json
import os
import pickle

import numpy as np

from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import h5_helper, spike_metrics

NONE = 2**31 - 1

# (Sa, Sb): every size of the issue's list on either side, around one MFMA tile
# (16), one tile of B (64 .. 128) and one row block of A (128)
PAIRS = [(1, 1), (1, 300), (15, 17), (16, 300), (17, 16), (127, 129),
         (128, 128), (129, 15), (300, 127), (300, 1)]
NEURONS = [1, 3, 63, 64, 65, 102, 130, 257]
KS = [1, 5, 8]
DENSITIES = [0.01, 0.5]
BIN = 12


@functools.lru_cache(maxsize=None)
def states(S, C, density, seed, bin=BIN):
  """int32 (S, C) of counts 0 .. bin, binomial(bin, density)."""
  rng = np.random.RandomState(100003 * seed + 1009 * C + S)
  x = rng.binomial(bin, density, size=(S, C)).astype(np.int32)
  x.setflags(write=False)
  return x


def with_duplicates(x, seed=0):
  """A copy of the set in which a quarter of the rows repeat other rows (at
  least one pair where the set has two rows)."""
  x = np.array(x)
  rng = np.random.RandomState(seed)
  n = len(x)
  if n >= 2:
    for _ in range(max(n // 4, 1)):
      i, j = rng.choice(n, 2, replace=False)
      x[i] = x[j]
  return x


def radii(Sb, kind, C, seed=0):
  """int32 (Sb,): all 0, all huge, or mixed (0, typical distances, huge)."""
  if kind == 'zero':
    return np.zeros(Sb, np.int32)
  if kind == 'huge':
    return np.full(Sb, NONE, np.int32)
  rng = np.random.RandomState(seed + Sb)
  r = rng.randint(0, 6 * C + 2, size=Sb).astype(np.int32)
  r[rng.uniform(size=Sb) < 0.2] = 0
  r[rng.uniform(size=Sb) < 0.1] = NONE
  return r


def double_loop(a, b, k, exclude_self=False, radius_b=None):
  """The definition, one pair at a time."""
  knn = np.full((len(a), k), NONE, np.int64)
  within = np.zeros(len(a), np.int64)
  for i in range(len(a)):
    found = []
    for j in range(len(b)):
      if exclude_self and j == i:
        continue
      d2 = sum((int(p) - int(q)) ** 2 for p, q in zip(a[i], b[j]))
      found.append(d2)
      if radius_b is not None and d2 <= int(radius_b[j]):
        within[i] += 1
    found = sorted(found)[:k]
    knn[i, :len(found)] = found
  return knn, (within if radius_b is not None else None)


def gain_trials(seed, trials=100, T=480, C=102, clip=False):
  """Spike trains (trials, T, C) of C neurons of rate 0.08 a frame times a gain
  shared by all neurons and drawn per bin of 12 frames, lognormal(0, 0.6);
  clip: the gain is cut at exp(0.3), so the high-gain population states -- a
  part of the repertoire -- are never produced."""
  r = np.random.RandomState(seed)
  gain = np.exp(0.6 * r.randn(trials, T // 12, 1))
  if clip:
    gain = np.minimum(gain, np.exp(0.3))
  rate = 0.08 * np.repeat(gain, 12, axis=1) * np.ones((1, 1, C))
  return (r.uniform(size=(trials, T, C)) < rate).astype(np.float32)


def run_dir(path, trials=24, T=480, C=6):
  """A DG run directory: the validation cache with its spikes and one generated
  file that holds the signals and the spikes of another seed.  Returns
  (generated file, recorded spikes, generated spikes), spikes (trials, T, C)."""
  real = dg.make_dataset(num_neurons=C, sequence_length=T, num_segments=trials,
                         seed=21)
  other = dg.make_dataset(num_neurons=C, sequence_length=T, num_segments=trials,
                          seed=22)
  gen_dir = path / 'generated'
  os.makedirs(gen_dir)
  val = str(gen_dir / 'validation.h5')
  h5_helper.write(val, {'signals': np.asarray(real['signals'], np.float32),
                        'spikes': real['spikes'].astype(np.int8)})
  fake = str(gen_dir / 'epoch000_signals.h5')
  h5_helper.write(fake, {'signals': np.asarray(other['signals'], np.float32),
                         'spikes': other['spikes'].astype(np.int8)})
  with open(gen_dir / 'info.pkl', 'wb') as f:
    pickle.dump({0: {'global_step': 1, 'filename': fake}}, f)
  with open(path / 'hparams.json', 'w') as f:
    json.dump(dict(generated_dir=str(gen_dir), validation_cache=val,
                   num_neurons=C, sequence_length=T), f)
  return fake, real['spikes'], other['spikes']


def expected_report(real, fake, k=5, bin=BIN):
  """The `states` dict compute_metrics.py should write for these spikes."""
  ref = spike_metrics.population_states(real[0::2], bin)
  floor = spike_metrics.state_scores(
      ref, spike_metrics.population_states(real[1::2], bin), k)
  generated = spike_metrics.state_scores(
      ref, spike_metrics.population_states(fake[1::2], bin), k)
  return dict(generated=generated, floor=floor, k=k, bin_frames=bin)
