#!/usr/bin/env python
"""Write the dataset directory of a recording for main.py (counterpart of the
reference's dataset/spike_train_inference.py + dataset/generate_tfrecords.py,
same flags, no TensorFlow).

  python dataset/generate_dataset.py --input raw_data/signals.pkl \
      --output_dir dataset/recording --sequence_length 2048 --normalize

--input is a pickle {'signals': (neurons, T), 'oasis': (neurons, T)}; without
'oasis' the spike trains are inferred as spike_train_inference.py does (OASIS
AR(1), g 0.95, s_min 0.55, then > 0.5), on the host.

By default the directory holds the recording itself (recording.npy beside
info.pkl, calciumgan_amd/data/recording.py) and every training step cuts its
windows on the GPU; --materialize arrays|tfrecords writes every window out as
the reference does (train.npy / validation.npy, or its TFRecord shards).
"""
import argparse
import os
import pickle
import sys
from shutil import rmtree

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from calciumgan_amd.data import recording
from calciumgan_amd.gan.utils import dataset_helper


def load_pickle(filename, is_dg_data=False):
  """(signals, spikes) as (neurons, T) float32 (generate_tfrecords.py:61-72:
  the first two rows are dropped unless --is_dg_data)."""
  with open(filename, 'rb') as file:
    data = pickle.load(file)
  signals = np.array(data['signals'], dtype=np.float32)
  if 'oasis' in data:
    spikes = np.array(data['oasis'], dtype=np.float32)
  else:
    from calciumgan_amd.gan.utils import spike_helper
    print('inferring spike trains (OASIS AR(1), g 0.95, s_min 0.55)...')
    spikes = spike_helper.deconvolve_signals(signals)
  if not is_dg_data:
    signals, spikes = signals[2:], spikes[2:]
  assert signals.shape == spikes.shape
  return signals, spikes


def build_parser():
  p = argparse.ArgumentParser()
  p.add_argument('--input', default='raw_data/ST260_Day4_signals4Bryan.pkl')
  p.add_argument('--output_dir', default='tfrecords')
  p.add_argument('--sequence_length', default=2048, type=int)
  p.add_argument('--stride', default=2, type=int)
  p.add_argument('--normalize', action='store_true')
  p.add_argument('--fft', action='store_true')
  p.add_argument('--conv2d', action='store_true')
  p.add_argument('--replace', action='store_true')
  p.add_argument('--validation_size', default=1000, type=float)
  p.add_argument('--is_dg_data', action='store_true')
  p.add_argument('--device', default='cpu', choices=['cpu', 'gpu'],
                 help='where the spectra of an --fft set are walked for their '
                 'min / max, and where --materialize cuts the windows')
  p.add_argument('--materialize', default='none',
                 choices=['none', 'arrays', 'tfrecords'],
                 help='none: the recording directory; arrays / tfrecords: every '
                 'window written out')
  p.add_argument('--num_per_shard', default=0, type=int,
                 help='segments per TFRecord shard (0: one shard per mode)')
  return p


def main(a):
  if a.conv2d:
    raise SystemExit('--conv2d datasets are not supported: the models here are '
                     'the 1-D ones')
  if not os.path.exists(a.input):
    raise SystemExit('input file {} does not exist'.format(a.input))
  if os.path.exists(a.output_dir):
    if not a.replace:
      raise SystemExit('output directory {} already exists'.format(a.output_dir))
    rmtree(a.output_dir)
  signals, spikes = load_pickle(a.input, a.is_dg_data)
  device = 'cuda:0' if a.device == 'gpu' else None
  rec = recording.build(signals, spikes, a.sequence_length, stride=a.stride,
                        normalize=a.normalize, fft=a.fft,
                        validation_size=int(a.validation_size), device=device)
  if a.materialize == 'none':
    info = recording.write(a.output_dir, rec)
  else:
    sig, spk = recording.materialize(rec, device=device)
    info = {k: v for k, v in rec['info'].items()
            if k not in ('recording', 'minmax_by')}
    info = dataset_helper.write_dataset(
        a.output_dir, sig, spk, info, int(a.validation_size),
        tfrecords=a.materialize == 'tfrecords', num_per_shard=a.num_per_shard)
  print('saved {} train + {} validation segments of shape {} to {} ({})'.format(
      info['train_size'], info['validation_size'], info['signal_shape'],
      a.output_dir, 'recording' if a.materialize == 'none' else a.materialize))
  return info


if __name__ == '__main__':
  main(build_parser().parse_args())
