"""Shared cases of the third-order tests (test_triplets_host.py,
test_hip_triplets.py): spike trains, raw word matrices, the triple loop the
numpy statement is held to and the XOR construction whose structure no pair
figure sees.  Everything compared is an integer or a dict."""
import functools
import itertools
import json
import os
import pickle

import numpy as np

from calciumgan_amd.gan.utils import h5_helper, spike_metrics

# (B, T, C, bin, density)
TRAINS = [
    (1, 3, 3, 1, .5),        # one partly filled word, one triplet
    (2, 50, 17, 12, .5),     # a partial bin holding spikes that must not count
    (2, 64, 5, 1, .5),       # exactly two words, no tail
    (1, 33, 4, 1, .5),       # one bit into a second word
    (3, 300, 102, 1, .5),    # the report's neuron count, dense
    (3, 300, 102, 12, .01),  # and sparse
    (1, 127, 130, 127, 1.0),  # nb = 1, C past 128
]

# raw word matrices of the counting kernel: tiles of 16 neurons (3, 4, 16: one
# tile; 17, 33: a second and a third with one neuron; 102: the report; 130: nine
# tiles), chunks of 64 words (63, 64, 65)
WORD_NEURONS = [3, 4, 16, 17, 33, 102, 130]
WORD_COUNTS = [1, 2, 63, 64, 65]
SPLIT_CASE = (5, 5000)     # one tile triple: the words split, with the merge
LARGEST_CASE = (512, 4)    # the largest output


def trains(B, T, C, density):
  return (np.random.RandomState(1000 * C + T).uniform(size=(B, T, C)) < density
          ).astype(np.float32)


@functools.lru_cache(maxsize=None)
def words(C, W, kind='dense'):
  """uint32 (C, W): random words of density 1/2 ('dense') or 1/16 ('sparse'),
  all ones or all zeros."""
  rng = np.random.RandomState(7919 * C + W)
  if kind == 'ones':
    w = np.full((C, W), 0xffffffff, np.uint32)
  elif kind == 'zeros':
    w = np.zeros((C, W), np.uint32)
  else:
    w = rng.randint(0, 1 << 32, size=(C, W), dtype=np.uint64).astype(np.uint32)
    if kind == 'sparse':
      for _ in range(3):
        w &= rng.randint(0, 1 << 32, size=(C, W), dtype=np.uint64).astype(
            np.uint32)
  w.setflags(write=False)
  return w


@functools.lru_cache(maxsize=None)
def word_counts(C, W, kind='dense'):
  """The statement's (singles, pairs, triplets) of `words(C, W, kind)`: computed
  once, shared, read-only."""
  out = spike_metrics.triplet_counts(
      spike_metrics.unpack_state_words(words(C, W, kind), 32 * W))
  for x in out:
    x.setflags(write=False)
  return out


def triple_loop(states):
  """The definition, one triplet at a time."""
  x = np.asarray(states).astype(np.int64)
  C = x.shape[1]
  singles = np.array([x[:, i].sum() for i in range(C)])
  pairs = np.array([[(x[:, i] * x[:, j]).sum() for j in range(C)]
                    for i in range(C)])
  triplets = np.array([(x[:, i] * x[:, j] * x[:, k]).sum()
                       for i, j, k in itertools.combinations(range(C), 3)])
  return singles, pairs, triplets


XOR_NEURONS, XOR_TRIOS = 24, 4


def xor_states(seed, S=4000, broken=False):
  """uint8 (S, 24): four trios (3 t, 3 t + 1, 3 t + 2) with s_i and s_j fair
  coins and s_k = s_i XOR s_j -- pairwise independent, kappa = -1/8 -- and twelve
  independent neurons at 0.1.  broken: s_k is a fair coin of its own, which
  leaves every rate and every pair covariance what it was."""
  rng = np.random.RandomState(seed)
  x = (rng.uniform(size=(S, XOR_NEURONS)) < 0.1).astype(np.uint8)
  for t in range(XOR_TRIOS):
    a, b = (rng.uniform(size=(2, S)) < 0.5).astype(np.uint8)
    own = (rng.uniform(size=S) < 0.5).astype(np.uint8)
    x[:, 3 * t], x[:, 3 * t + 1] = a, b
    x[:, 3 * t + 2] = own if broken else a ^ b
  return x


def side(states):
  return spike_metrics.triplet_counts(states) + (len(states),)


def gain_trials(seed, trials=24, T=480, C=7):
  """Spike trains (trials, T, C), int8: rate 0.04 a frame times a gain shared by
  all neurons and drawn per 12 frames, so that pairs and triplets of neurons are
  active together more often than their rates give."""
  r = np.random.RandomState(seed)
  gain = np.exp(0.7 * r.randn(trials, T // 12, 1))
  rate = 0.04 * np.repeat(gain, 12, axis=1) * np.ones((1, 1, C))
  return (r.uniform(size=(trials, T, C)) < rate).astype(np.int8)


def run_dir(path, trials=24, T=480, C=7):
  """A run directory: the validation cache with its spikes and one generated
  file that holds signals and the spikes of another seed.  Returns (generated
  file, recorded spikes, generated spikes), spikes (trials, T, C)."""
  real, other = gain_trials(31, trials, T, C), gain_trials(32, trials, T, C)
  gen_dir = path / 'generated'
  os.makedirs(gen_dir)
  val = str(gen_dir / 'validation.h5')
  fake = str(gen_dir / 'epoch000_signals.h5')
  for name, spikes, seed in ((val, real, 1), (fake, other, 2)):
    signals = np.random.RandomState(seed).uniform(size=spikes.shape)
    h5_helper.write(name, {'signals': (signals + spikes).astype(np.float32),
                           'spikes': spikes})
  with open(gen_dir / 'info.pkl', 'wb') as f:
    pickle.dump({0: {'global_step': 1, 'filename': fake}}, f)
  with open(path / 'hparams.json', 'w') as f:
    json.dump(dict(generated_dir=str(gen_dir), validation_cache=val,
                   num_neurons=C, sequence_length=T), f)
  return fake, real, other


def same(a, b):
  """Equality of two reports, a NaN equal to a NaN: floats print exactly."""
  return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


def expected_report(real, fake, bin=12):
  """The `triplets` dict compute_metrics.py should write for these spikes."""
  ref = side(spike_metrics.binary_states(real[0::2], bin))
  floor = spike_metrics.triplet_scores(
      ref, side(spike_metrics.binary_states(real[1::2], bin)))
  generated = spike_metrics.triplet_scores(
      ref, side(spike_metrics.binary_states(fake[1::2], bin)))
  return dict(generated=generated, floor=floor, bin_frames=bin)
