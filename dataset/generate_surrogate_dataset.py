#!/usr/bin/env python
"""The surrogate dataset of the MLP experiment (the reference's
dataset/generate_surrogate_data.py): a dichotomised-Gaussian population of 2
neurons over a few time steps, numpy only.

  python dataset/generate_surrogate_dataset.py --output_dir dataset/surrogate

Model (generate_surrogate_data.py:55-57 as dataset/dg/dichot_gauss.py:145-179
reads it): per time bin z ~ N(0, [[1, .3], [.3, 1]]), spike = [z + mean > 0]
with the GAUSSIAN mean [0.6, 0.8], independent across bins and samples.
Calcium by spikes_to_signals' AR(1) recipe (:33-47: g 0.95 from t = 2 on, noise
0.3).  Written, with the reference's keys and (n, neurons, L) float32 shapes:
  surrogate.pkl     {'spikes'}             num_samples draws
  ground_truth.pkl  {'spikes'}             num_samples further draws
  training.pkl      {'spikes', 'signals'}  training_size of the ground truth,
                                           drawn with replacement (:71)
main.py reads training.pkl when the input directory's name contains
'surrogate' (8192 samples train, the rest validate).
"""
import argparse
import os
import pickle
import shutil
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from calciumgan_amd.data import dg  # noqa: E402

NUM_NEURONS = 2
GAUSS_MEAN = np.array([0.6, 0.8])
GAUSS_CORR = 0.3


def generate_dg_spikes(num_samples, sequence_length, rng):
  """(num_samples, 2, L) float32 in {0, 1}.  Bins are independent, so one draw
  of num_samples * L bins is cut into the samples."""
  bins = dg.sample_spikes(GAUSS_MEAN, GAUSS_CORR, num_samples * sequence_length,
                          rng)
  return np.ascontiguousarray(
      bins.reshape(NUM_NEURONS, num_samples, sequence_length).transpose(1, 0, 2))


def spikes_to_signals(spikes, rng, g=0.95, sn=0.3):
  """generate_surrogate_data.py:33-47 over all samples at once: (n, neurons, L)
  spikes -> float32 signals."""
  c = spikes.astype(np.float32).copy()
  for j in range(2, c.shape[2]):
    c[:, :, j] += np.float32(g) * c[:, :, j - 1]
  return (c + sn * rng.standard_normal(c.shape)).astype(np.float32)


def generate(output_dir, num_samples, training_size, sequence_length,
             seed=1234):
  if os.path.exists(output_dir):
    shutil.rmtree(output_dir)
  os.makedirs(output_dir)
  rng = np.random.RandomState(seed)  # generate_surrogate_data.py:11

  def dump(name, content):
    with open(os.path.join(output_dir, name), 'wb') as file:
      pickle.dump(content, file)

  dump('surrogate.pkl',
       {'spikes': generate_dg_spikes(num_samples, sequence_length, rng)})
  ground_truth = generate_dg_spikes(num_samples, sequence_length, rng)
  dump('ground_truth.pkl', {'spikes': ground_truth})
  indices = rng.choice(len(ground_truth), size=training_size)
  training_spikes = ground_truth[indices]
  dump('training.pkl', {'spikes': training_spikes,
                        'signals': spikes_to_signals(training_spikes, rng)})


def build_parser():
  """generate_surrogate_data.py:78-84: the same flags and defaults."""
  parser = argparse.ArgumentParser()
  parser.add_argument('--output_dir', default='surrogate', type=str)
  parser.add_argument('--num_samples', default=2 * 10**6, type=int)
  parser.add_argument('--training_size', default=9192, type=int)
  parser.add_argument('--sequence_length', default=6, type=int)
  return parser


if __name__ == '__main__':
  a = build_parser().parse_args()
  generate(a.output_dir, a.num_samples, a.training_size, a.sequence_length)
  print('saved surrogate.pkl, ground_truth.pkl and training.pkl to {}'.format(
      a.output_dir))
