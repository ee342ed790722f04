#!/usr/bin/env python
"""Pattern probabilities of the surrogate experiment (Spike-GAN's figure 2; the
reference keeps this step outside its tree): a sample of L time steps x C
neurons is one of 2^(L C) binary spike patterns, few enough to count.  The
numerical probability of every pattern in the generated samples is compared
with its probability in the ground truth, and the surrogate draw -- a second,
independent draw from the generating model -- against the same ground truth
gives the scatter that sampling alone produces.

  python compute_surrogate_metrics.py --input_dir dataset/surrogate \
      --output_dir runs/surrogate [--device gpu] [--batch_samples 262144]
      [--plot] [--format pdf|png] [--dpi 120]

Read: <output_dir>/generated.pkl ('signals', (n, L, C), denormalised: what
main.py --model mlp writes when training ends), <input_dir>/ground_truth.pkl and
<input_dir>/surrogate.pkl ('spikes', (n, neurons, L)).  The generated signals
are deconvolved as everywhere else: OASIS AR(1), g 0.95, s_min 0.55, > 0.5.

Written: <output_dir>/surrogate_metrics.json (spike_metrics.pattern_scores of
the generated and of the surrogate counts against the ground truth's) and
<output_dir>/pattern_counts.npz (the three int64 count vectors); with --plot
and matplotlib, pattern_probabilities.<format>.

--device gpu deconvolves (cg_oasis_ar1_batched) and counts
(cg_pattern_histogram) on the device in batches of --batch_samples; the
per-batch counts are added there and only the three count vectors come to the
host.  Both are exact, so the two devices write the same files.
"""
import argparse
import json
import os
import pickle

import numpy as np

from calciumgan_amd.gan.utils import spike_helper, spike_metrics

MAX_BITS = spike_metrics.PATTERN_SCORE_BITS


def _load(filename, key):
  with open(filename, 'rb') as file:
    array = np.asarray(pickle.load(file)[key])
  if array.ndim != 3:
    raise SystemExit('{}: {!r} is not a 3-d array'.format(filename, key))
  return array


def counts_host(generated, recorded, batch_samples):
  """[counts of the deconvolved generated signals (n, L, C), counts of each
  (n, neurons, L) array of `recorded`], int64 (2^K,) on the host."""
  del batch_samples
  n, L, C = generated.shape
  traces = np.ascontiguousarray(generated.transpose(0, 2, 1)).reshape(n * C, L)
  trains = spike_helper.deconvolve_signals(traces).reshape(n, C, L)
  return [spike_metrics.pattern_histogram(x.transpose(0, 2, 1))
          for x in [trains] + list(recorded)]


def counts_device(generated, recorded, batch_samples):
  """`counts_host` through the device kernels, a batch of samples at a time."""
  import torch
  device = torch.device('cuda', torch.cuda.current_device())

  def batches(array):
    for i in range(0, len(array), batch_samples):
      yield torch.from_numpy(np.ascontiguousarray(
          array[i:i + batch_samples], dtype=np.float32)).to(device)

  def total(parts):
    counts = None
    for part in parts:
      counts = part if counts is None else counts + part
    return counts

  out = [total(spike_metrics.pattern_histogram_device(
      spike_helper.deconvolve_signals_device(x)) for x in batches(generated))]
  for array in recorded:  # (n, neurons, L), read in place as (n, L, neurons)
    out.append(total(spike_metrics.pattern_histogram_device(x.permute(0, 2, 1))
                     for x in batches(array)))
  return [c.cpu().numpy() for c in out]


def plot(counts, filename, dpi):
  """Log-log scatter of each pattern's probability against the ground truth's.
  Returns False (after one line) when matplotlib is not installed."""
  try:
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
  except ImportError:
    print('matplotlib is not installed: no figure written')
    return False
  truth = counts['ground_truth'] / counts['ground_truth'].sum()
  figure, axes = plt.subplots(1, 2, figsize=(9, 4.5), sharex=True, sharey=True)
  for axis, name in zip(axes, ('generated', 'surrogate')):
    q = counts[name] / counts[name].sum()
    both = (truth > 0) & (q > 0)
    low = min(truth[both].min(), q[both].min()) if both.any() else 1e-6
    axis.loglog(truth[both], q[both], '.', markersize=3, alpha=0.6)
    axis.loglog([low, 1.0], [low, 1.0], 'k-', linewidth=0.8)
    axis.set_xlabel('probability in the ground truth')
    axis.set_ylabel('probability in the {} samples'.format(name))
    axis.set_title(name)
  figure.tight_layout()
  figure.savefig(filename, dpi=dpi)
  plt.close(figure)
  return True


def main(hparams):
  # (float32 as generate_dataset stores them: what both devices deconvolve)
  generated = _load(os.path.join(hparams.output_dir, 'generated.pkl'),
                    'signals').astype(np.float32, copy=False)
  recorded = [_load(os.path.join(hparams.input_dir, name + '.pkl'), 'spikes')
              for name in ('ground_truth', 'surrogate')]
  _, L, C = generated.shape
  for array in recorded:
    if array.shape[1:] != (C, L):
      raise SystemExit('generated.pkl holds (n, {}, {}) signals, the input '
                       'directory (n, {}, {}) spikes'.format(
                           L, C, array.shape[1], array.shape[2]))
  if min(len(generated), len(recorded[0]), len(recorded[1])) < 1:
    raise SystemExit('an empty file')
  if L * C > MAX_BITS:
    raise SystemExit('{} time steps x {} neurons are {} bits: the report '
                     'covers up to {} (2^{} patterns)'.format(
                         L, C, L * C, MAX_BITS, MAX_BITS))
  if hparams.batch_samples < 1:
    raise SystemExit('--batch_samples < 1')
  count = counts_device if hparams.device == 'gpu' else counts_host
  names = ('generated', 'ground_truth', 'surrogate')
  counts = dict(zip(names, count(generated, recorded, hparams.batch_samples)))
  report = {
      'bits': L * C,
      'sequence_length': L,
      'num_neurons': C,
      'num_samples': {name: int(counts[name].sum()) for name in names},
      'generated': spike_metrics.pattern_scores(counts['ground_truth'],
                                                counts['generated']),
      'surrogate': spike_metrics.pattern_scores(counts['ground_truth'],
                                                counts['surrogate']),
  }
  with open(os.path.join(hparams.output_dir, 'surrogate_metrics.json'),
            'w') as file:
    json.dump(report, file, indent=2, sort_keys=True)
  np.savez(os.path.join(hparams.output_dir, 'pattern_counts.npz'), **counts)
  if hparams.plot:
    plot(counts, os.path.join(hparams.output_dir, 'pattern_probabilities.' +
                              hparams.format), hparams.dpi)
  if hparams.verbose:
    for name in ('generated', 'surrogate'):
      print('{} against the ground truth'.format(name))
      for key, value in sorted(report[name].items()):
        print('\t{}\t{}'.format(key, value))
  return report


def build_parser():
  parser = argparse.ArgumentParser()
  parser.add_argument('--input_dir', default='dataset/surrogate')
  parser.add_argument('--output_dir', default='runs/surrogate')
  parser.add_argument('--device', default='cpu', choices=['cpu', 'gpu'],
                      help='gpu: deconvolution and counting on the device')
  parser.add_argument('--batch_samples', default=262144, type=int,
                      help='--device gpu: samples per batch')
  parser.add_argument('--plot', action='store_true')
  parser.add_argument('--format', default='pdf', choices=['pdf', 'png'])
  parser.add_argument('--dpi', default=120, type=int)
  parser.add_argument('--verbose', default=1, type=int)
  return parser


if __name__ == '__main__':
  main(build_parser().parse_args())
