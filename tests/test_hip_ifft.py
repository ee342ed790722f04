"""GPU tests of cg_ifft_channels (csrc/ifft.hip: the inverse FFT along time of
generated [real | imag] spectra, one workgroup per sample and group of
neurons) on the cases of ifft_cases.py -- every case one launch on valid input,
held to the float64 inverse transform of its float32 input by the two
conditions of ifft_cases.check_accuracy -- of its wrapper
utils.ifft_channels_device, and of the FFT-dataset wiring: GAN.spike_statistics,
reverse_preprocessing of a device tensor, main.py on a make_dataset(fft=True)
directory and compute_metrics.py on what it wrote.

Measured on one MI355X (max over the traces of each T's cases, e against the
float64 transform, e_ref the same for single-precision pocketfft):
DESIGN.md "FFT datasets"."""
import json
import os

import numpy as np
import pytest
import torch

import ifft_cases as IC
import main as cli
import oracle as O
from calciumgan_amd import _lib
from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import (dataset_helper, h5_helper, spike_helper,
                                      spike_metrics, utils)

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _input(name):
  """The case's spectra on the device in the case's memory layout: a (B, T, 2C)
  view."""
  x, C, _, _, lin, _ = IC.case(name)
  B, T, _ = x.shape
  t = torch.from_numpy(np.array(x)).to(DEV)
  if lin == 'padded':
    buf = torch.full((B, T, 2 * C + 4), float('nan'), device=DEV)
    buf[:, :, :2 * C] = t
    view = buf[:, :, :2 * C]
    assert view.stride() == (T * (2 * C + 4), 2 * C + 4, 1)
    return view
  if lin == 'permuted':
    view = t.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert view.stride() == (2 * C * T, 1, T)
    return view
  assert lin == 'contig' and t.is_contiguous()
  return t


def _launch(name, x):
  """The C entry into the case's output layout; returns (y view, whole
  buffer)."""
  _, C, scale, offset, _, lout = IC.case(name)
  B, T, _ = x.shape
  pitch = C + 3 if lout == 'padded' else C
  buf = torch.full((B, T, pitch), float('nan'), device=DEV)
  y = buf[:, :, :C]
  _lib.call('cg_ifft_channels', x, B, T, C, x.stride(0), x.stride(1),
            x.stride(2), scale, offset, y, y.stride(0), y.stride(1), y.stride(2),
            _lib.stream())
  torch.cuda.synchronize()
  return y, buf


@pytest.mark.parametrize('name', IC.CASES)
def test_against_the_float64_transform(name):
  x_host, C, scale, offset, _, lout = IC.case(name)
  x = _input(name)
  y, buf = _launch(name, x)
  got = y.cpu().numpy()
  assert not np.isnan(got).any()
  if lout == 'padded':
    assert bool(torch.isnan(buf[:, :, C:]).all())  # the padding is untouched
  IC.check_accuracy(got, name)
  if not x_host.any() and offset == 0:
    assert not got.any()
  # determinism: a second launch gives the same bits
  again = _launch(name, x)[0].cpu().numpy()
  assert again.tobytes() == got.tobytes()
  # the wrapper: a contiguous (B, T, C) device tensor with the same bits
  dev = utils.ifft_channels_device(x, C, scale=scale, offset=offset)
  assert dev.is_cuda and dev.dtype == torch.float32 and dev.is_contiguous()
  assert tuple(dev.shape) == got.shape
  assert dev.cpu().numpy().tobytes() == got.tobytes()


@pytest.mark.parametrize('name', ['t128_c17_normal', 't512_c17_dg',
                                  't1024_c64_renumbered', 't4096_c3_dg'])
def test_the_f16_library_holds_the_same_kernel(name):
  """The float32 kernel of the other precision build, at the lengths the case
  table gained: under both conditions, and the bf16 build's bits."""
  x = _input(name)
  want = _launch(name, x)[0].cpu().numpy()
  _lib.use('f16')
  try:
    got = _launch(name, x)[0].cpu().numpy()
  finally:
    _lib.use('bf16')
  IC.check_accuracy(got, name)
  assert got.tobytes() == want.tobytes()


def test_other_lengths_take_the_host_statement():
  rng = np.random.RandomState(5)
  x = rng.standard_normal((2, 96, 6)).astype(np.float32)
  got = utils.ifft_channels_device(torch.from_numpy(x).to(DEV), 3)
  assert got.is_cuda and tuple(got.shape) == (2, 96, 3)
  assert got.cpu().numpy().tobytes() == utils.ifft_channels(x).tobytes()
  # denormalised as the kernel would: float32 product, float32 sum
  got = utils.ifft_channels_device(torch.from_numpy(x).to(DEV), 3, scale=0.37,
                                   offset=-1.25)
  want = utils.ifft_channels(
      (x * np.float32(0.37)).astype(np.float32) + np.float32(-1.25))
  assert got.cpu().numpy().tobytes() == want.tobytes()
  # the wrapper refuses host arrays, other dtypes, ranks and too few channels
  t = torch.from_numpy(x).to(DEV)
  for bad in ((x, 3), (torch.from_numpy(x), 3), (t.double(), 3), (t[0], 3),
              (t, 4), (t, 0)):
    with pytest.raises(ValueError):
      utils.ifft_channels_device(*bad)


def test_invalid_arguments_are_refused_and_nothing_is_written():
  x = torch.zeros((2, 16384, 6), device=DEV)
  y = torch.full((2, 16384, 3), -7.0, device=DEV)
  lib = _lib.load()

  def call(x=x, y=y, B=2, T=64, C=3):
    return lib.cg_ifft_channels(x, B, T, C, T * 6, 6, 1, 1.0, 0.0, y, T * 3, 3, 1,
                                _lib.stream())

  E = _lib.CG_EINVAL
  for kw in (dict(T=96), dict(T=16384), dict(B=0), dict(x=None), dict(y=None),
             dict(T=16), dict(C=0), dict(B=-2)):
    assert call(**kw) == E, kw
  torch.cuda.synchronize()
  assert bool((y == -7.0).all())


# -- wiring ------------------------------------------------------------------------
def _fft_gan(algorithm, L, neurons):
  from calciumgan_amd.gan.algorithms import get_algorithm
  from calciumgan_amd.gan.models import get_models
  hp = O.make_hparams(L, 2 * neurons, 8, m=2)
  hp.verbose = 0
  hp.algorithm = algorithm
  hp.normalize = True
  hp.fft = True
  hp.num_neurons = neurons
  hp.signals_min, hp.signals_max = -17.5, 141.25
  gen, dis = get_models(hp, None)
  return hp, get_algorithm(hp, gen, dis, None)


@pytest.mark.parametrize('algorithm', ['wgan-gp', 'gan'])
def test_gan_spike_statistics_is_the_chain_written_out(algorithm):
  B, L, C = 6, 256, 8
  hp, gan = _fft_gan(algorithm, L, C)
  d = dg.make_dataset(num_neurons=C, sequence_length=L, num_segments=B, fft=True)
  fake = gan.validate(np.ascontiguousarray(d['signals']))[0]
  assert tuple(fake.shape) == (B, L, 2 * C)
  kept = gan.spike_real_statistics(d['spikes'])
  out = gan.spike_statistics(fake, real_stats=kept)
  scale, offset = hp.signals_max - hp.signals_min, hp.signals_min
  traces = utils.ifft_channels_device(fake, C, scale=scale, offset=offset)
  assert tuple(traces.shape) == (B, L, C)
  spikes = spike_helper.deconvolve_signals_device(traces)
  rates, covs = spike_metrics.batch_statistics_device(spikes)
  sums = spike_metrics.error_sums_device(kept[0], rates, kept[1], covs)
  torch.cuda.synchronize()
  for i, k in enumerate(('firing_rate_abs_sum', 'firing_rate_sq_sum',
                         'covariance_abs_sum', 'covariance_sq_sum')):
    assert torch.equal(out[k], sums[i]), k
  assert float(out['firing_rate_count']) == B * C
  assert float(out['covariance_count']) == B * C * (C + 1) // 2
  assert all(np.isfinite(float(v)) for v in out.values())
  # with the ground-truth trains instead of kept statistics: the same
  again = gan.spike_statistics(fake, d['spikes'])
  assert all(torch.equal(out[k], again[k]) for k in out)
  # reverse_preprocessing of a device tensor: the device path, then the host
  got = utils.reverse_preprocessing(hp, fake)
  assert isinstance(got, np.ndarray) and got.shape == (B, L, C)
  assert got.tobytes() == traces.cpu().numpy().tobytes()
  # and it is the host statement's answer to float32 rounding
  host = utils.reverse_preprocessing(hp, fake.cpu())
  norm = np.sqrt((host.astype(np.float64) ** 2).sum(1))
  err = np.sqrt(((got.astype(np.float64) - host) ** 2).sum(1))
  assert (err <= 2 * IC.higham_bound(L) * norm).all()


# -- main.py on an FFT dataset (shapes of tests/test_main_e2e.py) ------------------
def _scalars(path):
  return [json.loads(l) for l in open(path)]


def test_main_on_an_fft_dataset_and_compute_metrics(tmp_path):
  import compute_metrics as cm
  n, L, C = 70, 256, 8
  d = dg.make_dataset(num_neurons=C, sequence_length=L, num_segments=n, fft=True)
  info = {k: v for k, v in d['info'].items() if k != 'rates_hz'}
  ds = str(tmp_path / 'ds')
  dataset_helper.write_dataset(ds, d['signals'], d['spikes'], info,
                               validation_size=6)
  out = str(tmp_path / 'run')
  a = cli.build_parser().parse_args([
      '--input_dir', ds, '--output_dir', out, '--model', 'calciumgan',
      '--algorithm', 'wgan-gp', '--batch_size', '8', '--num_units', '8', '--m',
      '2', '--layer_norm', '--epochs', '1', '--save_generated', 'last',
      '--spike_metrics', '--verbose', '0'])
  a.global_step = 0
  a.surrogate_ds = False
  cli.main(a)
  assert a.fft is True and a.num_channels == 2 * C and a.num_neurons == C
  gen = h5_helper.get(os.path.join(out, 'generated', 'epoch000_signals.h5'),
                      'signals')
  assert gen.shape == (6, L, C) and np.isfinite(gen).all()
  # validation.h5: the traces of the validation spectra, by the host statement
  idx = np.random.RandomState(1234).permutation(n)[n - 6:]
  want = utils.ifft_channels(utils.denormalize(
      d['signals'][idx], info['signals_min'], info['signals_max']))
  val = h5_helper.get(os.path.join(out, 'generated', 'validation.h5'), 'signals')
  assert val.shape == (6, L, C) and val.tobytes() == want.tobytes()
  va = _scalars(os.path.join(out, 'validation', 'scalars.jsonl'))
  tags = {r['tag'] for r in va}
  assert {'spike_metrics/firing_rate_mae', 'spike_metrics/firing_rate_rmse',
          'spike_metrics/covariance_mae', 'spike_metrics/covariance_mse',
          'signals_metrics/std'} <= tags
  assert all(np.isfinite(r['value']) for r in va)
  # compute_metrics.py reads files that now hold traces
  mhp = cm.build_parser().parse_args(['--output_dir', out, '--num_processors',
                                      '1', '--verbose', '0'])
  rep = cm.main(mhp)
  assert list(rep) == [0]
  spikes = h5_helper.get(os.path.join(out, 'generated', 'epoch000_signals.h5'),
                         'spikes')
  assert spikes.shape == (6, L, C) and set(np.unique(spikes)) <= {0, 1}
  saved = json.load(open(os.path.join(out, 'spike_metrics.json')))
  for k in ('firing_rate_kl', 'correlation_kl', 'van_rossum_kl'):
    assert np.isfinite(saved['0'][k]['mean']), (k, saved['0'][k])
