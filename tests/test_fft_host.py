"""CPU tests of FFT datasets (the reference's generate_tfrecords.py --fft):
the numpy statements utils.fft_channels / ifft_channels the kernel of
csrc/ifft.hip is tested against, dg.make_dataset(fft=True) through both
writers, reverse_preprocessing / cache_validation_set on such a dataset, and
the C ABI entry cg_ifft_channels under version 20 with its argument checks
(which return before any HIP call)."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import ifft_cases
from calciumgan_amd import _lib
from calciumgan_amd import build as cg_build
from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import dataset_helper, h5_helper, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'calciumgan_hip.h')
U = 2.0 ** -24  # float32 unit roundoff


def _rel(a, b):
  """||a - b||_2 / ||b||_2 along time per (sample, neuron)."""
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return np.sqrt(((a - b) ** 2).sum(1)) / np.sqrt((b * b).sum(1))


# -- known answers ---------------------------------------------------------------
@pytest.mark.parametrize('L,t0', [(32, 0), (32, 5), (256, 77)])
def test_fft_of_a_unit_impulse(L, t0):
  x = np.zeros((1, L, 2), np.float32)
  x[0, t0, 1] = 1.0
  s = utils.fft_channels(x)
  assert s.shape == (1, L, 4) and s.dtype == np.float32
  k = np.arange(L)
  # e^{-2 pi i k t0 / L} for neuron 1: real in channel 1, imaginary in 2 + 1
  np.testing.assert_allclose(s[0, :, 1], np.cos(2 * np.pi * k * t0 / L),
                             atol=8 * U)
  np.testing.assert_allclose(s[0, :, 3], -np.sin(2 * np.pi * k * t0 / L),
                             atol=8 * U)
  assert not s[0, :, 0].any() and not s[0, :, 2].any()


def test_fft_of_a_constant_is_dc_only():
  L = 64
  x = np.full((2, L, 3), 0.75, np.float32)
  s = utils.fft_channels(x)
  assert s.shape == (2, L, 6)
  np.testing.assert_allclose(s[:, 0, :3], 0.75 * L, rtol=4 * U)
  assert np.abs(s[:, 1:, :3]).max() <= 0.75 * L * 4 * U
  assert np.abs(s[:, :, 3:]).max() <= 0.75 * L * 4 * U


@pytest.mark.parametrize('L,k0', [(32, 1), (64, 17), (256, 255)])
def test_ifft_of_a_single_bin(L, k0):
  x = np.zeros((1, L, 4), np.float32)
  x[0, k0, 0] = 1.0   # neuron 0: real 1 in bin k0
  x[0, k0, 3] = 1.0   # neuron 1: imaginary 1 in bin k0
  y = utils.ifft_channels(x)
  assert y.shape == (1, L, 2) and y.dtype == np.float32
  t = np.arange(L)
  np.testing.assert_allclose(y[0, :, 0], np.cos(2 * np.pi * k0 * t / L) / L,
                             atol=8 * U / L)
  # Re(i e^{i a}) = -sin a
  np.testing.assert_allclose(y[0, :, 1], -np.sin(2 * np.pi * k0 * t / L) / L,
                             atol=8 * U / L)


def test_layout_is_real_block_then_imaginary_block():
  """Neuron c's imaginary part is channel C + c, not interleaved."""
  L, C = 32, 3
  rng = np.random.RandomState(0)
  for c in range(C):
    x = np.zeros((1, L, C), np.float32)
    x[0, :, c] = rng.standard_normal(L)
    s = utils.fft_channels(x)
    z = np.fft.fft(x[0, :, c].astype(np.float64))
    used = np.zeros(2 * C, bool)
    used[[c, C + c]] = True
    assert not s[0][:, ~used].any()
    np.testing.assert_allclose(s[0, :, c], z.real, atol=1e-5)
    np.testing.assert_allclose(s[0, :, C + c], z.imag, atol=1e-5)
    assert np.abs(s[0, :, C + c]).max() > 0.1
    # and back: only channel c of the traces
    y = utils.ifft_channels(s)
    assert y.shape == (1, L, C)
    np.testing.assert_allclose(y, x, atol=1e-5)


def test_round_trip_on_dg_traces():
  """ifft_channels(fft_channels(x)) against x at L = 256, C = 8.  The error bar
  comes from the float64 inverse of the SAME float32 spectrum: y64 differs from
  x by the forward transform's error e_fwd (a float32 FFT, Higham's bound, plus
  the rounding of the stored spectrum), and the float32 inverse differs from
  y64 by the inverse's own Higham bound -- no hand-picked constant."""
  L, C = 256, 8
  x = dg.make_dataset(num_neurons=C, sequence_length=L, num_segments=4)['signals']
  s = utils.fft_channels(x)
  y = utils.ifft_channels(s)
  assert y.shape == x.shape and y.dtype == np.float32
  z = s[..., :C].astype(np.complex128) + 1j * s[..., C:].astype(np.complex128)
  y64 = np.fft.ifft(z, axis=1).real
  bound = ifft_cases.higham_bound(L)
  e_fwd = _rel(y64, x)
  e_inv = _rel(y, y64)
  e_rt = _rel(y, x)
  print('forward %.3g, inverse %.3g, round trip %.3g, Higham %.3g' % (
      e_fwd.max(), e_inv.max(), e_rt.max(), bound))
  assert e_fwd.max() <= bound + U
  assert e_inv.max() <= bound
  assert (e_rt <= e_inv * (1 + e_fwd) + e_fwd + U).all()
  assert e_rt.max() <= 2 * bound + 2 * U


def test_the_case_table_meets_its_own_conditions_with_the_statement():
  """utils.ifft_channels (complex64 numpy) is held to the two conditions the
  device kernel is held to, on the small cases."""
  for name in ifft_cases.CASES:
    x = ifft_cases.denormalised(name)
    if x.size > 1 << 18:
      continue
    ifft_cases.check_accuracy(utils.ifft_channels(x), name)


def test_the_cases_cover_the_mechanisms():
  cases = {n: ifft_cases.case(n) for n in ifft_cases.CASES}
  Ts = {c[0].shape[1] for c in cases.values()}
  assert Ts == {32, 64, 128, 256, 512, 1024, 2048, 4096, 8192}
  assert {ifft_cases.group(T) for T in Ts} == {16, 8, 4, 2, 1}
  for T in Ts:
    G = ifft_cases.group(T)
    Cs = {c[1] for c in cases.values() if c[0].shape[1] == T}
    assert G + 1 in Cs, T      # a ragged second group
    if T in (128, 512, 1024, 4096):
      assert 't%d_bins' % T in cases
  for G in (8, 4, 2):          # a last group that is not full
    assert any(ifft_cases.group(c[0].shape[1]) == G and c[1] > G and c[1] % G
               for c in cases.values()), G
  x, C = cases['t32_c17_grid_stride'][:2]
  groups = -(-C // ifft_cases.group(32))
  assert x.shape[0] * groups > ifft_cases.MAX_GRID
  # the walk of the items: renumbered when the grid (the item count, below the
  # cap) is a multiple of 8, as they come otherwise
  items = {n: ifft_cases.items(n) for n in cases}
  assert items['t1024_c64_renumbered'] == 24
  assert any(i % 8 == 0 and i < ifft_cases.MAX_GRID for i in items.values())
  assert any(i % 8 and i < ifft_cases.MAX_GRID for i in items.values())
  assert cases['t1024_c5_permuted'][4:] == ('permuted', 'padded')
  assert cases['t4096_c2_affine'][2:4] == (0.37, -1.25)
  assert cases['t2048_c102_dg'][0].shape == (2, 2048, 204)
  assert {c[4] for c in cases.values()} == {'contig', 'padded', 'permuted'}
  assert {c[5] for c in cases.values()} == {'contig', 'padded'}
  assert cases['t256_c8_dg_affine'][2:4] == (0.37, -1.25)
  src = open(os.path.join(ROOT, 'calciumgan_amd', 'csrc', 'ifft.hip')).read()
  assert 'kIfftMaxGrid = %d;' % ifft_cases.MAX_GRID in src


# -- the dataset generator ---------------------------------------------------------
def _info(d):
  return {k: v for k, v in d['info'].items() if k != 'rates_hz'}


def test_make_dataset_fft():
  L, C, n = 64, 5, 12
  d0 = dg.make_dataset(num_neurons=C, sequence_length=L, num_segments=n)
  d = dg.make_dataset(num_neurons=C, sequence_length=L, num_segments=n, fft=True)
  i0, i = d0['info'], d['info']
  assert i0['fft'] is False and i0['num_channels'] == C
  assert i['fft'] is True and i['num_channels'] == 2 * C
  assert i['num_neurons'] == C and i['sequence_length'] == L
  assert tuple(i['signal_shape']) == (L, 2 * C)
  assert tuple(i['spike_shape']) == (L, C)
  assert set(i) == set(i0)
  assert d['signals'].shape == (n, L, 2 * C) and d['signals'].dtype == np.float32
  # the spikes are untouched
  assert np.array_equal(d['spikes'], d0['spikes'])
  # normalize holds over the spectra
  assert d['signals'].min() == 0.0 and d['signals'].max() == 1.0
  assert i['signals_min'] < 0 < i['signals_max']
  # and they are the spectra of the traces, transformed before normalisation
  traces = utils.denormalize(d0['signals'], i0['signals_min'], i0['signals_max'])
  want = utils.fft_channels(traces)
  got = utils.denormalize(d['signals'], i['signals_min'], i['signals_max'])
  spec_range = i['signals_max'] - i['signals_min']
  trace_range = i0['signals_max'] - i0['signals_min']
  np.testing.assert_allclose(
      got, want, rtol=0, atol=4 * U * (spec_range + L * trace_range))
  # (one float32 rounding of a trace value moves a bin by at most L of them;
  # normalising and denormalising a bin rounds it twice at the spectra's range)


@pytest.mark.parametrize('tfrecords', [False, True])
def test_fft_dataset_through_both_writers(tmp_path, tfrecords):
  L, C, n, nval = 32, 3, 10, 4
  d = dg.make_dataset(num_neurons=C, sequence_length=L, num_segments=n, fft=True)
  path = str(tmp_path / 'ds')
  full = dataset_helper.write_dataset(path, d['signals'], d['spikes'], _info(d),
                                      validation_size=nval, tfrecords=tfrecords,
                                      num_per_shard=4)
  assert full['fft'] is True and full['num_channels'] == 2 * C
  hp = SimpleNamespace(input_dir=path, output_dir=str(tmp_path / 'run'),
                       noise_dim=4, batch_size=4, save_generated='')
  train_ds, validation_ds = dataset_helper.get_dataset(hp)
  assert hp.fft is True and hp.num_channels == 2 * C and hp.num_neurons == C
  assert hp.signal_shape == (L, 2 * C) and hp.spike_shape == (L, C)
  idx = np.random.RandomState(1234).permutation(n)
  for ds, ii in ((train_ds, idx[:n - nval]), (validation_ds, idx[n - nval:])):
    assert np.array_equal(np.asarray(ds.signals), d['signals'][ii])
    assert np.array_equal(np.asarray(ds.spikes), d['spikes'][ii])


# -- reverse_preprocessing / cache_validation_set ------------------------------------
def _hparams(fft, C, normalize=True):
  return SimpleNamespace(normalize=normalize, fft=fft, conv2d=False,
                         num_neurons=C, signals_min=-3.5, signals_max=17.25)


def test_reverse_preprocessing():
  rng = np.random.RandomState(3)
  C = 3
  x = rng.uniform(0, 1, (2, 32, 2 * C)).astype(np.float32)
  hp = _hparams(True, C)
  got = utils.reverse_preprocessing(hp, x)
  want = utils.ifft_channels(utils.denormalize(x, hp.signals_min, hp.signals_max))
  assert got.shape == (2, 32, C) and got.dtype == np.float32
  assert got.tobytes() == want.tobytes()
  # a host torch tensor takes the same path
  import torch
  assert utils.reverse_preprocessing(hp, torch.from_numpy(x)).tobytes() == \
      want.tobytes()
  # not normalised: the inverse transform alone
  got = utils.reverse_preprocessing(_hparams(True, C, normalize=False), x)
  assert got.tobytes() == utils.ifft_channels(x).tobytes()
  # without fft: today's result bit for bit, attribute present or not
  plain = utils.denormalize(x, hp.signals_min, hp.signals_max)
  assert plain.dtype == np.float32 and plain.shape == x.shape
  assert utils.reverse_preprocessing(_hparams(False, C), x).tobytes() == \
      plain.tobytes()
  bare = SimpleNamespace(normalize=True, signals_min=-3.5, signals_max=17.25)
  assert utils.reverse_preprocessing(bare, x).tobytes() == plain.tobytes()
  bare.normalize = False
  assert utils.reverse_preprocessing(bare, x) is x


def test_cache_validation_set_holds_traces_for_an_fft_dataset(tmp_path):
  L, C, n = 32, 3, 6
  d = dg.make_dataset(num_neurons=C, sequence_length=L, num_segments=n, fft=True)
  i = d['info']
  hp = SimpleNamespace(normalize=True, fft=True, conv2d=False, num_neurons=C,
                       signals_min=i['signals_min'], signals_max=i['signals_max'],
                       batch_size=4,
                       validation_cache=str(tmp_path / 'validation.h5'))
  dataset_helper.cache_validation_set(hp, {'signals': d['signals'],
                                           'spikes': d['spikes']})
  sig = h5_helper.get(hp.validation_cache, 'signals')
  want = utils.ifft_channels(utils.denormalize(d['signals'], hp.signals_min,
                                               hp.signals_max))
  assert sig.shape == (n, L, C) and sig.dtype == np.float32
  assert sig.tobytes() == want.tobytes()
  assert h5_helper.get(hp.validation_cache, 'spikes').shape == (n, L, C)
  # without fft the cache is what it was: denormalised, same shape
  hq = SimpleNamespace(normalize=True, fft=False, signals_min=hp.signals_min,
                       signals_max=hp.signals_max, batch_size=4,
                       validation_cache=str(tmp_path / 'plain.h5'))
  dataset_helper.cache_validation_set(hq, {'signals': d['signals'],
                                           'spikes': d['spikes']})
  plain = h5_helper.get(hq.validation_cache, 'signals')
  want = d['signals'] * (hq.signals_max - hq.signals_min) + hq.signals_min
  assert plain.tobytes() == want.astype(np.float32).tobytes()


def test_generator_cli_has_the_flag(tmp_path):
  import pickle
  import subprocess
  import sys
  out = str(tmp_path / 'ds')
  subprocess.check_call([
      sys.executable, os.path.join(ROOT, 'dataset', 'generate_dg_dataset.py'),
      '--output_dir', out, '--sequence_length', '32', '--num_neurons', '3',
      '--num_segments', '8', '--validation_size', '2', '--fft'])
  info = pickle.load(open(os.path.join(out, 'info.pkl'), 'rb'))
  assert info['fft'] is True and info['num_channels'] == 6
  assert tuple(info['signal_shape']) == (32, 6)
  assert tuple(info['spike_shape']) == (32, 3)


# -- header and binding -------------------------------------------------------------
def test_header_signature_and_both_libraries_carry_the_entry_point():
  cg_build.build(verbose=False)
  text = open(HEADER).read()
  src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  m = re.search(r'\bint\s+cg_ifft_channels\s*\(([^()]*)\)\s*;', src)
  assert m, 'no prototype of cg_ifft_channels'
  assert ' '.join(m.group(1).split()) == (
      'const float* x, int B, int T, int C, long long s_b, long long s_t, '
      'long long s_c, float scale, float offset, float* y, long long y_sb, '
      'long long y_st, long long y_sc, void* stream')
  assert 'ifft.hip' in cg_build.SOURCES
  sig = _lib.SIGNATURES['cg_ifft_channels']
  assert len(sig) == 14
  assert [t for t in sig[1:9]] == [ctypes.c_int] * 3 + [ctypes.c_longlong] * 3 + [
      ctypes.c_float] * 2
  assert issubclass(sig[0], _lib.DataPtr) and issubclass(sig[9], _lib.DataPtr)
  for precision in ('bf16', 'f16'):
    lib = _lib.load(precision)
    assert hasattr(lib, 'cg_ifft_channels'), precision
    assert lib.cg_abi_version() == 20
  assert '#define CG_ABI_VERSION 20' in text
  assert _lib.CG_ABI_VERSION == 20


def test_nothing_is_launched_for_invalid_arguments():
  """(host-side argument checks: they return before any HIP call)"""
  lib = _lib.load()
  q = ctypes.c_void_p(0x1000)
  E = _lib.CG_EINVAL

  def call(x=q, y=q, B=2, T=64, C=3):
    return lib.cg_ifft_channels(x, B, T, C, T * 2 * C, 2 * C, 1, 1.0, 0.0, y,
                                T * C, C, 1, None)

  assert call(x=None) == E and call(y=None) == E
  assert call(B=0) == E and call(B=-1) == E
  assert call(C=0) == E and call(C=-3) == E
  for T in (96, 16384, 16, 0, -64, 8191, 1 << 20):
    assert call(T=T) == E, T
