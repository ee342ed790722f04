"""CPU tests of recording datasets (calciumgan_amd/data/recording.py: the
recording stays whole and every batch of windows is cut out of it): the numpy
statement dataset_helper.window_batch the kernel of csrc/windows.hip is tested
against, recording.build / materialize against dg.make_dataset, the directory
round trip, RecordingDataset against ArrayDataset on the materialised directory,
both generator CLIs, and the C ABI entry cg_window_batch under version 20 with
its argument checks (which return before any HIP call)."""
import ctypes
import os
import pickle
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import window_cases as WC
from calciumgan_amd import _lib
from calciumgan_amd import build as cg_build
from calciumgan_amd.data import dg, recording
from calciumgan_amd.gan.utils import dataset_helper, spike_helper, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'calciumgan_hip.h')


# -- the statement ------------------------------------------------------------------
@pytest.mark.parametrize('name', WC.CASES)
def test_the_statement_is_segment_plus_the_normalisation(name):
  c = WC.case(name)
  raw, starts, L = c['raw'], c['starts'], c['L']
  T = raw.shape[0]
  sub, div = np.float32(c['sub']), np.float32(c['div'])
  got = dataset_helper.window_batch(raw, starts, L, sub=c['sub'], div=c['div'])
  assert got.dtype == np.float32 and got.shape == (len(starts), L, c['C'])
  # every window, those past an end included, written out with np.pad
  want = (WC.windows(name) - sub) / div
  assert got.tobytes() == want.astype(np.float32).tobytes()
  # the windows inside the recording are dg.segment's
  seg = dg.segment(raw, L, stride=1)
  inside = [b for b, s in enumerate(starts) if 0 <= s < T - L]
  assert inside
  for b in inside:
    assert np.array_equal(got[b], (seg[starts[b]] - sub) / div)
  if (c['sub'], c['div']) == (0.0, 1.0):
    assert got.tobytes() == WC.windows(name).tobytes()


def test_the_statement_with_fft_is_fft_channels_of_the_windows():
  c = WC.case('l256_c8_dg_affine')
  got = dataset_helper.window_batch(c['raw'], c['starts'], c['L'], fft=True,
                                    sub=c['sub'], div=c['div'])
  want = (utils.fft_channels(WC.windows('l256_c8_dg_affine')) -
          np.float32(c['sub'])) / np.float32(c['div'])
  assert got.dtype == np.float32 and got.shape == (8, 256, 16)
  assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize('name', WC.FFT_CASES)
def test_the_fft_cases_meet_their_own_conditions_with_the_statement(name):
  """The numpy statement (complex64 numpy) is held to the two conditions the
  device kernel is held to."""
  c = WC.case(name)
  WC.check_accuracy(
      dataset_helper.window_batch(c['raw'], c['starts'], c['L'], fft=True), name)


def test_the_cases_cover_the_mechanisms():
  cases = {n: WC.case(n) for n in WC.CASES}
  fft = {n: cases[n] for n in WC.FFT_CASES}
  Ls = {c['L'] for c in fft.values()}
  assert Ls == {32, 64, 128, 256, 512, 1024, 2048, 4096, 8192}
  assert {WC.group(L) for L in Ls} == {16, 8, 4, 2, 1}
  for L in Ls:
    assert WC.group(L) + 1 in {c['C'] for c in fft.values() if c['L'] == L}, L
    if L in (128, 512, 1024, 4096):
      assert 'l%d_impulses' % L in fft
  for G in (8, 4, 2):          # a last group that is not full
    assert any(WC.group(c['L']) == G and c['C'] > G and c['C'] % G
               for c in fft.values()), G
  # the walk of the FFT kernel's items: renumbered when the grid (the item
  # count, below the cap) is a multiple of 8, as they come otherwise
  items = {n: WC.fft_items(n) for n in fft}
  assert items['l1024_c17_dg'] == 24
  assert any(i % 8 == 0 and i < WC.FFT_MAX_GRID for i in items.values())
  assert any(i % 8 and i < WC.FFT_MAX_GRID for i in items.values())
  assert cases['l1024_c5_transposed']['lin'] == 'transposed'
  assert cases['l4096_c2_normal']['lout'] == 'padded'
  assert {1, 3, 102} <= {c['C'] for c in fft.values()}
  c = cases['l32_c17_grid_stride']
  assert len(c['starts']) * -(-17 // WC.group(32)) > WC.FFT_MAX_GRID
  c = cases['l64_c65_plain_grid_stride']
  assert len(c['starts']) * -(-64 * 65 // WC.PLAIN_ITEM) > WC.PLAIN_MAX_GRID
  src = open(os.path.join(ROOT, 'calciumgan_amd', 'csrc', 'windows.hip')).read()
  assert 'kWinFftMaxGrid = %d;' % WC.FFT_MAX_GRID in src
  assert 'kWinMaxGrid = %d;' % WC.PLAIN_MAX_GRID in src
  assert WC.PLAIN_ITEM == 4 * 256 and 'kWinThreads = 256;' in src
  c = cases['l256_c8_dg']
  T, L = c['raw'].shape[0], c['L']
  s = list(c['starts'])
  assert 0 in s and any(v % 2 for v in s) and len(set(s)) < len(s)
  assert T - L in s and max(s) > T - L and min(s) < 0
  assert {c['lin'] for c in cases.values()} == {'contig', 'padded', 'padded4',
                                                'transposed'}
  assert {c['lout'] for c in cases.values()} == {'contig', 'padded', 'padded4'}
  assert (cases['l256_c8_dg_affine']['sub'],
          cases['l256_c8_dg_affine']['div']) == (-1.25, 3.7)
  assert (33 * 3) % 4 and not cases['l33_c3_plain_tail']['fft']
  assert not cases['l256_c4_zero_trace']['raw'][:, 2].any()
  assert all(len(cases[n]['starts']) <= 3 for n in cases if n.startswith('l8192'))


# -- build / materialize against make_dataset ---------------------------------------
N, L0, C0 = 70, 256, 8


def _dg_recording(fft, validation_size=6):
  signals, spikes, _ = dg.make_recording(C0, L0 + 2 * N, 1234, 0.05)
  return recording.build(signals, spikes, L0, stride=2, fft=fft,
                         validation_size=validation_size, max_segments=N)


@pytest.mark.parametrize('fft', [False, True])
def test_build_and_materialize_are_make_dataset_byte_for_byte(fft):
  d = dg.make_dataset(num_neurons=C0, sequence_length=L0, num_segments=N, fft=fft)
  rec = _dg_recording(fft)
  sig, spk = recording.materialize(rec)
  assert sig.dtype == np.float32 and spk.dtype == np.float32
  assert sig.tobytes() == d['signals'].tobytes()
  assert spk.tobytes() == d['spikes'].tobytes()
  info = rec['info']
  assert info['signals_min'] == d['info']['signals_min']
  assert info['signals_max'] == d['info']['signals_max']
  assert info['minmax_by'] == 'host' and info['recording'] is True
  for k in ('signal_shape', 'spike_shape', 'sequence_length', 'num_neurons',
            'num_channels', 'normalize', 'stride', 'fft', 'conv2d'):
    assert info[k] == d['info'][k], k
  assert info['train_size'] == N - 6 and info['validation_size'] == 6
  assert info['buffer_size'] == N - 6
  # the split is write_dataset's: the windows in permuted order
  idx = np.random.RandomState(1234).permutation(N)
  assert np.array_equal(rec['train_starts'], 2 * idx[:N - 6])
  assert np.array_equal(rec['validation_starts'], 2 * idx[N - 6:])
  assert rec['raw'].shape == (L0 + 2 * N, C0) and rec['raw'].dtype == np.float32
  assert rec['spikes'].shape == rec['raw'].shape and rec['spikes'].dtype == np.int8


def test_build_without_normalisation_and_its_refusals():
  signals, spikes, _ = dg.make_recording(3, 100, 5, 0.05)
  rec = recording.build(signals, spikes, 32, stride=3, normalize=False,
                        validation_size=4)
  assert 'signals_min' not in rec['info'] and rec['info']['normalize'] is False
  assert recording.normalisation(rec['info']) == (0.0, 1.0)
  starts = np.sort(np.concatenate([rec['train_starts'], rec['validation_starts']]))
  assert np.array_equal(starts, np.arange(0, 100 - 32, 3))
  sig, _ = recording.materialize(rec)
  assert sig.tobytes() == dg.segment(signals.T, 32, 3).tobytes()
  with pytest.raises(ValueError):
    recording.build(signals, spikes, 100)
  with pytest.raises(ValueError):
    recording.build(signals, spikes, 32, validation_size=1000)


def test_write_load_round_trip(tmp_path):
  rec = _dg_recording(True)
  path = str(tmp_path / 'rec')
  recording.write(path, rec)
  assert sorted(os.listdir(path)) == ['info.pkl', 'recording.npy']
  back = recording.load(path)
  assert set(back) == {'raw', 'spikes', 'train_starts', 'validation_starts',
                       'info'}
  for k in ('raw', 'spikes', 'train_starts', 'validation_starts'):
    assert back[k].dtype == rec[k].dtype and np.array_equal(back[k], rec[k]), k
  assert back['info'] == rec['info']


# -- RecordingDataset against ArrayDataset ------------------------------------------
def _hparams(input_dir, tmp_path, save_generated=''):
  return SimpleNamespace(input_dir=input_dir, output_dir=str(tmp_path / 'run'),
                         noise_dim=4, batch_size=8, save_generated=save_generated)


@pytest.mark.parametrize('fft', [False, True])
def test_a_recording_directory_yields_the_batches_of_the_materialised_one(
    tmp_path, fft):
  rec = _dg_recording(fft, validation_size=5)  # 65 train: 8 batches of 8 and 1
  rdir, adir = str(tmp_path / 'rec'), str(tmp_path / 'arrays')
  recording.write(rdir, rec)
  sig, spk = recording.materialize(rec)
  info = {k: v for k, v in rec['info'].items()
          if k not in ('recording', 'minmax_by')}
  dataset_helper.write_dataset(adir, sig, spk, info, validation_size=5)
  hr, ha = _hparams(rdir, tmp_path), _hparams(adir, tmp_path)
  got, want = dataset_helper.get_dataset(hr), dataset_helper.get_dataset(ha)
  for k in ('train_size', 'validation_size', 'signal_shape', 'spike_shape',
            'sequence_length', 'num_neurons', 'num_channels', 'normalize', 'fft',
            'signals_min', 'signals_max', 'train_steps', 'validation_steps'):
    assert getattr(hr, k) == getattr(ha, k), k
  assert isinstance(got[0], dataset_helper.RecordingDataset)
  assert isinstance(want[0], dataset_helper.ArrayDataset)
  for r_ds, a_ds in zip(got, want):
    assert len(r_ds) == len(a_ds)
    for epoch in range(2):
      r_batches, a_batches = list(r_ds), list(a_ds)
      assert len(r_batches) == len(a_batches) == len(a_ds)
      sizes = [len(s) for s, _ in r_batches]
      assert sizes[-1] == len(r_ds.starts) % 8 != 0   # the short last batch
      for (rs, rk), (as_, ak) in zip(r_batches, a_batches):
        assert isinstance(rs, np.ndarray) and rs.dtype == np.float32
        assert rs.tobytes() == np.asarray(as_).tobytes()
        assert rk.shape == ak.shape and rk.dtype == np.float32
        assert len(rk) == len(ak)
        assert np.asarray(rk).tobytes() == np.asarray(ak).tobytes()
        assert np.array_equal(rk[0], np.asarray(ak)[0])
  # the training set is reshuffled every epoch, the validation set never
  a, b = [list(got[1])[0][0] for _ in range(2)]
  assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('fft', [False, True])
def test_the_validation_cache_of_a_recording_directory(tmp_path, fft):
  from calciumgan_amd.gan.utils import h5_helper
  rec = _dg_recording(fft)
  rdir = str(tmp_path / 'rec')
  recording.write(rdir, rec)
  hp = _hparams(rdir, tmp_path, save_generated='last')
  dataset_helper.get_dataset(hp)
  val = h5_helper.get(hp.validation_cache, 'signals')
  spk = h5_helper.get(hp.validation_cache, 'spikes')
  vs = rec['validation_starts']
  raw_windows = dataset_helper.window_batch(rec['raw'], vs, L0)
  assert val.shape == (6, L0, C0) and spk.shape == (6, L0, C0)
  assert np.array_equal(spk, dataset_helper.window_batch(
      rec['spikes'].astype(np.float32), vs, L0))
  if fft:
    # the raw windows themselves, exact
    assert val.tobytes() == raw_windows.tobytes()
  else:
    # what an array directory's cache holds: the normalised windows, denormalised
    sub, div = recording.normalisation(rec['info'])
    norm = dataset_helper.window_batch(rec['raw'], vs, L0, sub=sub, div=div)
    want = norm * (hp.signals_max - hp.signals_min) + hp.signals_min
    assert val.tobytes() == want.astype(np.float32).tobytes()
    np.testing.assert_allclose(val, raw_windows, rtol=0, atol=4e-7 * div)


# -- the CLIs -----------------------------------------------------------------------
def _pickle(tmp_path, with_oasis=True):
  signals, spikes, _ = dg.make_recording(5, 140, 7, 0.05)
  data = {'signals': signals}
  if with_oasis:
    data['oasis'] = spikes
  path = str(tmp_path / 'signals.pkl')
  with open(path, 'wb') as f:
    pickle.dump(data, f)
  return path, signals, spikes


def _cli(*args):
  subprocess.check_call([sys.executable,
                         os.path.join(ROOT, 'dataset', 'generate_dataset.py')] +
                        list(args))


@pytest.mark.parametrize('is_dg', [False, True])
def test_generate_dataset_drops_the_first_two_rows_unless_dg(tmp_path, is_dg):
  path, signals, spikes = _pickle(tmp_path)
  out = str(tmp_path / 'ds')
  _cli('--input', path, '--output_dir', out, '--sequence_length', '32',
       '--normalize', '--validation_size', '4', *(['--is_dg_data'] if is_dg else []))
  rec = recording.load(out)
  keep = slice(None) if is_dg else slice(2, None)
  assert np.array_equal(rec['raw'], signals[keep].T)
  assert np.array_equal(rec['spikes'], spikes[keep].T.astype(np.int8))
  info = rec['info']
  assert info['num_neurons'] == (5 if is_dg else 3) and info['recording'] is True
  assert info['stride'] == 2 and info['normalize'] is True and not info['fft']
  n = len(np.arange(0, 140 - 32, 2))
  assert (info['train_size'], info['validation_size']) == (n - 4, 4)
  want = recording.build(signals[keep], spikes[keep], 32, validation_size=4)
  assert info == want['info']
  # an existing directory is refused without --replace
  with pytest.raises(subprocess.CalledProcessError):
    _cli('--input', path, '--output_dir', out, '--sequence_length', '32')
  with pytest.raises(subprocess.CalledProcessError):
    _cli('--input', path, '--output_dir', str(tmp_path / 'c2d'), '--conv2d')


def test_generate_dataset_infers_missing_spike_trains_and_materialises(tmp_path):
  path, signals, _ = _pickle(tmp_path, with_oasis=False)
  out, arr = str(tmp_path / 'ds'), str(tmp_path / 'arrays')
  common = ['--input', path, '--sequence_length', '32', '--normalize', '--fft',
            '--validation_size', '4', '--is_dg_data']
  _cli('--output_dir', out, *common)
  rec = recording.load(out)
  want = spike_helper.deconvolve_signals(signals)
  assert want.any()
  assert np.array_equal(rec['spikes'], want.T.astype(np.int8))
  assert rec['info']['fft'] is True and rec['info']['num_channels'] == 10
  # --materialize arrays: write_dataset's directory of the same windows
  _cli('--output_dir', arr, '--materialize', 'arrays', *common)
  assert sorted(os.listdir(arr)) == ['info.pkl', 'train.npy', 'validation.npy']
  sig, spk = recording.materialize(rec)
  idx = np.random.RandomState(1234).permutation(len(sig))
  train = pickle.load(open(os.path.join(arr, 'train.npy'), 'rb'))
  assert train['signals'].tobytes() == sig[idx[:-4]].tobytes()
  assert train['spikes'].tobytes() == spk[idx[:-4]].tobytes()
  info = pickle.load(open(os.path.join(arr, 'info.pkl'), 'rb'))
  assert 'recording' not in info and info['fft'] is True
  assert info['signals_min'] == rec['info']['signals_min']


def test_generate_dg_dataset_recording_flag(tmp_path):
  out = str(tmp_path / 'ds')
  subprocess.check_call([
      sys.executable, os.path.join(ROOT, 'dataset', 'generate_dg_dataset.py'),
      '--output_dir', out, '--sequence_length', '32', '--num_neurons', '3',
      '--num_segments', '12', '--validation_size', '2', '--recording'])
  rec = recording.load(out)
  d = dg.make_dataset(num_neurons=3, sequence_length=32, num_segments=12)
  sig, spk = recording.materialize(rec)
  assert sig.tobytes() == d['signals'].tobytes()
  assert spk.tobytes() == d['spikes'].tobytes()
  assert rec['info']['train_size'] == 10 and rec['info']['recording'] is True


# -- header and binding -------------------------------------------------------------
def test_header_signature_and_both_libraries_carry_the_entry_point():
  cg_build.build(verbose=False)
  text = open(HEADER).read()
  src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  m = re.search(r'\bint\s+cg_window_batch\s*\(([^()]*)\)\s*;', src)
  assert m, 'no prototype of cg_window_batch'
  assert ' '.join(m.group(1).split()) == (
      'const float* raw, long long T_raw, int C, long long r_st, long long r_sc, '
      'const int* starts, int B, int L, int fft, float sub, float div, '
      'float* y, long long y_sb, long long y_st, long long y_sc, void* stream')
  assert 'windows.hip' in cg_build.SOURCES
  assert 'fft_stages.h' in cg_build.HEADERS
  sig = _lib.SIGNATURES['cg_window_batch']
  assert len(sig) == 16
  assert [issubclass(sig[i], _lib.DataPtr) for i in (0, 5, 11)] == [True] * 3
  assert sig[5].dtype is __import__('torch').int32
  assert sig[9:11] == [ctypes.c_float] * 2
  for precision in ('bf16', 'f16'):
    lib = _lib.load(precision)
    assert hasattr(lib, 'cg_window_batch'), precision
    assert lib.cg_abi_version() == 20
  assert '#define CG_ABI_VERSION 20' in text


def test_nothing_is_launched_for_invalid_arguments():
  """(host-side argument checks: they return before any HIP call)"""
  lib = _lib.load()
  q = ctypes.c_void_p(0x1000)
  E = _lib.CG_EINVAL

  def call(raw=q, starts=q, y=q, T=100, C=3, B=2, L=64, fft=0, div=1.0):
    ch = 2 * C if fft else C
    return lib.cg_window_batch(raw, T, C, C, 1, starts, B, L, fft, 0.0, div, y,
                               L * ch, ch, 1, None)

  for fft in (0, 1):
    assert call(raw=None, fft=fft) == E and call(starts=None, fft=fft) == E
    assert call(y=None, fft=fft) == E
    assert call(T=0, fft=fft) == E and call(T=-5, fft=fft) == E
    assert call(C=0, fft=fft) == E and call(C=-3, fft=fft) == E
    assert call(B=0, fft=fft) == E and call(B=-1, fft=fft) == E
    assert call(L=0, fft=fft) == E and call(L=-64, fft=fft) == E
    assert call(div=0.0, fft=fft) == E and call(div=-0.0, fft=fft) == E
  for L in (96, 16384, 16, 8191, 1 << 20, 33):
    assert call(L=L, fft=1) == E, L
