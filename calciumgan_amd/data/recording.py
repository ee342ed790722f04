"""Recording datasets: the dataset directory of a recording that stays whole.

The reference builds its training set with dataset/generate_tfrecords.py: a
(neurons, T) recording is cut into overlapping windows (--stride 2), each
optionally replaced by its spectrum (--fft), min/max-normalised, and every
window is written out -- each row of the recording about L / 2 times.  Here
the directory holds the recording itself (``recording.npy``: raw (T, C) float32,
spikes (T, C) int8, the start rows of the train and validation windows) beside
the reference's ``info.pkl``, and dataset_helper.RecordingDataset cuts each
step's windows on the device (csrc/windows.hip, cg_window_batch).

Normalisation statement: sub = signals_min, div = float(signals_max) -
float(signals_min) -- the difference in float64, rounded to float32 where it
is applied -- which is what dg.make_dataset computes for its segments."""
import os
import pickle

import numpy as np

from ..gan.utils import dataset_helper

FILENAME = 'recording.npy'
MINMAX_BATCH = 64  # windows per step of the walk over an FFT set's spectra


def window_starts(T, sequence_length, stride=2, max_segments=None):
  """generate_tfrecords.py:82-86: i = 0, stride, ... while i + L < T."""
  starts = np.arange(0, T - sequence_length, stride)
  if max_segments is not None:
    starts = starts[:max_segments]
  return starts


def normalisation(info):
  """(sub, div) of the windows of a recording with this info."""
  if not info['normalize']:
    return 0.0, 1.0
  return (float(info['signals_min']),
          float(info['signals_max']) - float(info['signals_min']))


def _spectra_minmax(raw, starts, L, device):
  """min / max over the spectra of all windows, walked in batches."""
  lo, hi = np.inf, -np.inf
  if device is None:
    for i in range(0, len(starts), MINMAX_BATCH):
      s = dataset_helper.window_batch(raw, starts[i:i + MINMAX_BATCH], L, True)
      lo, hi = min(lo, float(s.min())), max(hi, float(s.max()))
    return lo, hi
  import torch
  dev_raw = torch.from_numpy(raw).to(device)
  dev_starts = torch.from_numpy(starts.astype(np.int32)).to(device)
  los, his = [], []
  for i in range(0, len(starts), MINMAX_BATCH):
    s = dataset_helper.window_batch_device(dev_raw, dev_starts[i:i + MINMAX_BATCH],
                                           L, True)
    los.append(torch.amin(s))
    his.append(torch.amax(s))
  return float(torch.stack(los).amin()), float(torch.stack(his).amax())


def build(signals, spikes, sequence_length, stride=2, normalize=True, fft=False,
          validation_size=1000, max_segments=None, seed=1234, device=None):
  """(C, T) signals and spike trains, as the reference's pickles hold them, ->
  the recording dict: raw (T, C) float32, spikes (T, C) int8, train_starts /
  validation_starts (in the permuted order of write_dataset's split: the last
  `validation_size` of RandomState(seed).permutation(n) validate) and info with
  the reference's keys plus recording=True.

  signals_min / signals_max: over the rows the windows cover; for `fft` over
  the spectra of all windows, walked in batches without keeping them -- on
  `device` through cg_window_batch, else by the numpy statement
  (info['minmax_by'] says which).  The two differ by float32 roundings of the
  transform, so a set built on the host and trained on the device may leave
  [0, 1] by a rounding."""
  signals = np.asarray(signals, dtype=np.float32)
  spikes = np.asarray(spikes)
  assert signals.ndim == 2 and signals.shape == spikes.shape
  assert stride >= 1
  L = int(sequence_length)
  raw = np.ascontiguousarray(signals.T)
  raw_spikes = np.ascontiguousarray(spikes.T).astype(np.int8)
  T, C = raw.shape
  starts = window_starts(T, L, stride, max_segments)
  n = len(starts)
  if n < 1 or not 0 <= validation_size < n:
    raise ValueError('{} windows of {} rows in a recording of {}, {} of them '
                     'for validation'.format(n, L, T, validation_size))
  perm = np.random.RandomState(seed).permutation(n)
  train_size = n - int(validation_size)
  num_channels = 2 * C if fft else C
  info = dict(
      signal_shape=(L, num_channels),
      spike_shape=(L, C),
      sequence_length=L,
      num_neurons=C,
      num_channels=num_channels,
      normalize=bool(normalize),
      stride=int(stride),
      fft=bool(fft),
      conv2d=False,
      train_size=train_size,
      validation_size=int(validation_size),
      num_train_shards=1,
      num_validation_shards=1,
      buffer_size=train_size,
      recording=True)
  if normalize:
    if fft:
      lo, hi = _spectra_minmax(raw, starts, L, device)
      info['minmax_by'] = 'host' if device is None else 'device'
    else:
      covered = raw[:int(starts[-1]) + L]
      lo, hi = float(covered.min()), float(covered.max())
      info['minmax_by'] = 'host'
    info['signals_min'], info['signals_max'] = lo, hi
  return dict(raw=raw, spikes=raw_spikes, train_starts=starts[perm[:train_size]],
              validation_starts=starts[perm[train_size:]], info=info)


def write(output_dir, rec):
  """recording.npy (a pickled dict, as train.npy / validation.npy are) beside
  info.pkl."""
  os.makedirs(output_dir, exist_ok=True)
  with open(os.path.join(output_dir, FILENAME), 'wb') as f:
    pickle.dump({k: rec[k] for k in ('raw', 'spikes', 'train_starts',
                                     'validation_starts')}, f, protocol=4)
  with open(os.path.join(output_dir, 'info.pkl'), 'wb') as f:
    pickle.dump(dict(rec['info']), f)
  return rec['info']


def load(input_dir):
  with open(os.path.join(input_dir, FILENAME), 'rb') as f:
    rec = pickle.load(f)
  with open(os.path.join(input_dir, 'info.pkl'), 'rb') as f:
    rec['info'] = pickle.load(f)
  return rec


def materialize(rec, device=None):
  """(signals, spikes) of ALL windows in start order, float32 (N, L, channels)
  and (N, L, C): what the reference's generator would have written, cut by the
  same two functions the training loop uses (tests, and generate_dataset.py
  --materialize)."""
  info = rec['info']
  L, fft = info['sequence_length'], info['fft']
  sub, div = normalisation(info)
  starts = np.sort(np.concatenate([rec['train_starts'],
                                   rec['validation_starts']]))
  spikes = np.asarray(dataset_helper.LazyWindows(rec['spikes'], starts, L))
  if device is None:
    return dataset_helper.window_batch(rec['raw'], starts, L, fft, sub,
                                       div), spikes
  import torch
  dev_raw = torch.from_numpy(rec['raw']).to(device)
  dev_starts = torch.from_numpy(starts.astype(np.int32)).to(device)
  parts = [
      dataset_helper.window_batch_device(
          dev_raw, dev_starts[i:i + MINMAX_BATCH], L, fft, sub, div).cpu().numpy()
      for i in range(0, len(starts), MINMAX_BATCH)
  ]
  return np.concatenate(parts), spikes
