"""gan/utils/utils.py counterparts: run utilities around the hot path
(hparams persistence, checkpoints, generated-sample files).  On-disk layouts
follow SURVEY Appendix C."""
import json
import os
import pickle
import subprocess
from glob import glob

import numpy as np

from . import h5_helper


def normalize(x, x_min, x_max):
  """utils.py:25-27."""
  return (x - x_min) / (x_max - x_min)


def denormalize(x, x_min, x_max):
  """utils.py:30-32."""
  return x * (x_max - x_min) + x_min


def _to_numpy(x):
  if hasattr(x, 'detach'):
    x = x.detach().cpu().numpy()
  return np.asarray(x)


def fft_channels(signals):
  """generate_tfrecords.py:30-42 (--fft): (N, L, C) float32 traces -> (N, L, 2C)
  float32 spectra.  Per (n, c) the complex64 FFT along L; real parts in
  channels [0, C), imaginary parts in [C, 2C) (neuron c's imaginary part is
  channel C + c, not interleaved)."""
  signals = np.asarray(signals, dtype=np.float32)
  assert signals.ndim == 3
  z = np.fft.fft(signals.astype(np.complex64), axis=1)
  return np.concatenate([z.real, z.imag], axis=-1).astype(np.float32)


def ifft_channels(x):
  """utils.py:35-46: (N, L, 2C) float32 spectra in the [real | imag] layout of
  `fft_channels` -> (N, L, C) float32, the real part of the complex64 inverse
  FFT along L of x[..., c] + 1j * x[..., C + c].  (numpy 2.x keeps complex64 in
  np.fft: the precision class of the reference's tf.signal.ifft.)"""
  x = np.asarray(x, dtype=np.float32)
  assert x.ndim == 3 and x.shape[-1] % 2 == 0
  C = x.shape[-1] // 2
  z = np.empty(x.shape[:2] + (C,), dtype=np.complex64)
  z.real = x[..., :C]
  z.imag = x[..., C:]
  return np.ascontiguousarray(np.fft.ifft(z, axis=1).real, dtype=np.float32)


IFFT_DEVICE_MIN_LENGTH, IFFT_DEVICE_MAX_LENGTH = 32, 8192


def ifft_channels_device(x, num_neurons, scale=1.0, offset=0.0):
  """`ifft_channels` of x * scale + offset on the GPU (csrc/ifft.hip,
  cg_ifft_channels): a float32 device tensor (B, L, >= 2 num_neurons) with any
  strides -- a channel-padded generator output or a permuted view is read in
  place; channels [0, num_neurons) are the real parts, [num_neurons, 2
  num_neurons) the imaginary parts -- -> float32 device (B, L, num_neurons),
  contiguous.  The spectrum inverted is x * scale + offset with float32 product
  and sum, i.e. utils.denormalize of the float32 array with scale = max - min,
  offset = min.  No host sync.

  The kernel takes L a power of two in 32 .. 8192.  Any other length (the tile
  rule admits L = 2048 k with k not a power of two) is inverted by
  `ifft_channels` on the host, silently: the batch goes down and the traces come
  back up as a device tensor."""
  import torch
  from ... import _lib as hip
  if not (torch.is_tensor(x) and x.is_cuda):
    raise ValueError('ifft_channels_device needs a device tensor '
                     '(ifft_channels is the host path)')
  C = int(num_neurons)
  if x.dtype != torch.float32 or x.dim() != 3 or C < 1 or x.shape[2] < 2 * C:
    raise ValueError('float32 (B, L, >= 2 num_neurons) expected')
  B, L = x.shape[0], x.shape[1]
  if B == 0 or L == 0:
    raise ValueError('empty input')
  if (L & (L - 1)) or not IFFT_DEVICE_MIN_LENGTH <= L <= IFFT_DEVICE_MAX_LENGTH:
    host = x[:, :, :2 * C].cpu().numpy()
    host = host * np.float32(scale) + np.float32(offset)
    return torch.from_numpy(ifft_channels(host)).to(x.device)
  y = torch.empty((B, L, C), dtype=torch.float32, device=x.device)
  hip.call('cg_ifft_channels', x, B, L, C, x.stride(0), x.stride(1),
           x.stride(2), scale, offset, y, y.stride(0), y.stride(1), y.stride(2),
           hip.stream())
  return y


def _reverse_fft(hparams, x):
  """reverse_preprocessing of an FFT dataset (utils.py:49-63 with hparams.fft):
  denormalise, then the inverse transform per (sample, neuron).  A device
  tensor is denormalised and inverted on the device (`ifft_channels_device`)
  and only the (N, L, num_neurons) traces come to the host."""
  if hasattr(x, 'is_cuda') and x.is_cuda:
    scale, offset = 1.0, 0.0
    if hparams.normalize:
      scale = hparams.signals_max - hparams.signals_min
      offset = hparams.signals_min
    x = ifft_channels_device(x.detach(), hparams.num_neurons, scale=scale,
                             offset=offset)
    return x.cpu().numpy()
  x = _to_numpy(x)
  if hparams.normalize:
    x = denormalize(x, x_min=hparams.signals_min, x_max=hparams.signals_max)
  return ifft_channels(x)


def reverse_preprocessing(hparams, x):
  """utils.py:49-63 (1-D): denormalise, and on an FFT dataset (hparams.fft)
  invert the spectra to (N, L, num_neurons) traces."""
  if getattr(hparams, 'fft', False):
    return _reverse_fft(hparams, x)
  x = _to_numpy(x)
  if hparams.normalize:
    x = denormalize(x, x_min=hparams.signals_min, x_max=hparams.signals_max)
  return x


def get_current_git_hash():
  """utils.py:66-69, tolerant of running outside a git checkout (the
  reference crashes there -- SURVEY Appendix D.7)."""
  try:
    return subprocess.check_output(['git', 'describe', '--always'],
                                   stderr=subprocess.DEVNULL).strip().decode()
  except Exception:  # noqa
    return 'unknown'


def _jsonable(v):
  if isinstance(v, (np.integer,)):
    return int(v)
  if isinstance(v, (np.floating,)):
    return float(v)
  if isinstance(v, np.ndarray):
    return v.tolist()
  if isinstance(v, tuple):
    return list(v)
  return v


def save_hparams(hparams):
  """utils.py:72-75."""
  hparams.git_hash = get_current_git_hash()
  os.makedirs(hparams.output_dir, exist_ok=True)
  with open(os.path.join(hparams.output_dir, 'hparams.json'), 'w') as file:
    json.dump({k: _jsonable(v) for k, v in hparams.__dict__.items()}, file)


def load_hparams(hparams):
  """utils.py:78-84."""
  filename = os.path.join(hparams.output_dir, 'hparams.json')
  with open(filename, 'r') as file:
    content = json.load(file)
  for key, value in content.items():
    if not hasattr(hparams, key):
      setattr(hparams, key, value)


def save_fake_signals(hparams, epoch, signals):
  """utils.py:93-113: append denormalised (N, L, C) float32 signals to
  generated/epoch{:03d}_signals.h5 and record it in generated/info.pkl."""
  signals = reverse_preprocessing(hparams, signals)
  filename = os.path.join(hparams.generated_dir,
                          'epoch{:03d}_signals.h5'.format(epoch))
  h5_helper.write(filename, {'signals': signals.astype(np.float32)})
  info_filename = os.path.join(hparams.generated_dir, 'info.pkl')
  info = {}
  if os.path.exists(info_filename):
    with open(info_filename, 'rb') as file:
      info = pickle.load(file)
  if epoch not in info:
    info[epoch] = {'global_step': hparams.global_step, 'filename': filename}
    with open(info_filename, 'wb') as file:
      pickle.dump(info, file)


def save_models(hparams, gan, epoch):
  """utils.py:116-132: checkpoints/epoch-{:03d}.pkl with Keras-order weight
  lists; the step counters are plain ints (the reference pickles tf.Variables,
  SURVEY 5.4)."""
  if not os.path.exists(hparams.ckpt_dir):
    os.makedirs(hparams.ckpt_dir)
  filename = os.path.join(hparams.ckpt_dir, 'epoch-{:03d}.pkl'.format(epoch))
  ckpt = {
      'epoch': epoch,
      'gen_weights': gan.generator.get_weights(),
      'dis_weights': gan.discriminator.get_weights(),
      'gen_steps': int(gan.gen_optimizer.iterations),
      'dis_steps': int(gan.dis_optimizer.iterations)
  }
  average = getattr(gan, 'average', None)
  if average is not None:
    # --ema_decay: the averaged generator next to the raw one, and how many
    # updates it has had (the warm-up of its decay depends on the count)
    ckpt['gen_ema_weights'] = average.get_weights()
    ckpt['ema_updates'] = int(average.updates)
  with open(filename, 'wb') as file:
    pickle.dump(ckpt, file)
  if hparams.verbose:
    print('Saved checkpoint to {}'.format(filename))


def load_models(hparams, gan):
  """utils.py:135-152: resume from the lexicographically last epoch-*."""
  if not hasattr(hparams, 'ckpt_dir'):
    hparams.ckpt_dir = os.path.join(hparams.output_dir, 'checkpoints')
  hparams.start_epoch = 0
  filenames = glob(os.path.join(hparams.ckpt_dir, 'epoch-*'))
  if filenames:
    filename = sorted(filenames)[-1]
    with open(filename, 'rb') as file:
      ckpt = pickle.load(file)
    hparams.start_epoch = ckpt['epoch'] + 1
    gan.generator.set_weights(ckpt['gen_weights'])
    gan.discriminator.set_weights(ckpt['dis_weights'])
    gan.gen_optimizer.iterations = int(ckpt['gen_steps'])
    gan.dis_optimizer.iterations = int(ckpt['dis_steps'])
    average = getattr(gan, 'average', None)
    if average is not None:
      # (a checkpoint of a run without --ema_decay: averaging starts from the
      # loaded weights; without the flag the keys are ignored)
      have = 'gen_ema_weights' in ckpt and 'ema_updates' in ckpt
      average.set_weights(ckpt['gen_ema_weights'] if have else
                          ckpt['gen_weights'])
      average.updates = int(ckpt['ema_updates']) if have else 0
    if hparams.verbose:
      print('\n\nRestored checkpoint at {}\n\n'.format(filename))


def generate_dataset(hparams, gan, num_samples=1000):
  """utils.py:191-207: sample the generator in batches of 100 into
  <output_dir>/generated.pkl."""
  generated = np.zeros((num_samples,) + tuple(hparams.signal_shape),
                       dtype=np.float32)
  batch_size = 100
  for i in range(0, num_samples, batch_size):
    noise = gan.get_noise(batch_size)
    signals = _to_numpy(gan.generate(noise, denorm=True))
    generated[i:i + batch_size] = signals[:num_samples - i]
  filename = os.path.join(hparams.output_dir, 'generated.pkl')
  with open(filename, 'wb') as file:
    pickle.dump({'signals': generated}, file)
  if hparams.verbose:
    print('save {} samples to {}'.format(num_samples, filename))


def get_array_format(shape, hparams):
  """utils.py:155-165: 'N' samples / 'W' sequence length / 'C' channels."""
  assert len(shape) <= 3
  return ''.join('W' if s == hparams.sequence_length else
                 'C' if s == hparams.num_neurons else 'N' for s in shape)


def set_array_format(array, data_format, hparams):
  """utils.py:168-184."""
  assert len(array.shape) == len(data_format)
  current_format = get_array_format(array.shape, hparams)
  assert set(current_format) == set(data_format)
  if data_format == current_format:
    return array
  return np.transpose(array, axes=[current_format.index(s) for s in data_format])


def remove_nan(array):
  """utils.py:187-188."""
  return array[np.logical_not(np.isnan(array))]
