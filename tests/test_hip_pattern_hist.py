"""GPU tests of cg_pattern_histogram (csrc/patterns.hip: the number of samples
with each of the 2^(T C) binary spike patterns) against its numpy statement
spike_metrics.pattern_histogram, for equality; of deconvolve_signals_device at
the surrogate experiment's T = 6; and of compute_surrogate_metrics.py --device
gpu against --device cpu.  Every case is a call on valid input.  Shapes are
(N, T, C)."""
import functools
import os

import numpy as np
import pytest
import torch

import compute_surrogate_metrics as csm
from calciumgan_amd import _lib, nets
from calciumgan_amd.gan.utils import spike_helper, spike_metrics
from pattern_cases import calcium, samples, surrogate_dirs

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
MAX_BITS, LDS_BITS, BLOCK_SAMPLES, MAX_BLOCKS = (
    _lib.CONSTANTS['CG_PATTERN_HIST_' + n]
    for n in ('MAX_BITS', 'LDS_BITS', 'BLOCK_SAMPLES', 'MAX_BLOCKS'))
POISON = -0x0123456789abcdef


def _split(K):
  """(T, C) with T C = K: two neurons where K is even."""
  return (K // 2, 2) if K % 2 == 0 else (K, 1)


@functools.lru_cache(maxsize=None)
def _case(N, T, C, seed=0, rate=0.3):
  """(samples, the statement's counts), computed once and read-only."""
  x = samples(N, T, C, seed, rate)
  want = spike_metrics.pattern_histogram(x)
  x.setflags(write=False)
  want.setflags(write=False)
  return x, want


def _launch(x, counts=None):
  """The C entry on a device tensor (N, T, C) of any strides; the output buffer
  is filled with a non-zero pattern beforehand."""
  N, T, C = x.shape
  if counts is None:
    counts = torch.full((1 << (T * C),), POISON, dtype=torch.int64, device=DEV)
  _lib.call('cg_pattern_histogram', x, N, T, C, x.stride(0), x.stride(1),
            x.stride(2), counts, None, 0, nets._stream())
  torch.cuda.synchronize()
  return counts.cpu().numpy()


def _check(x_host, want, what):
  x = torch.from_numpy(np.array(x_host, dtype=np.float32)).to(DEV)
  got = _launch(x)
  assert got.dtype == np.int64 and got.sum() == len(x_host), what
  np.testing.assert_array_equal(got, want, err_msg=str(what))
  dev = spike_metrics.pattern_histogram_device(x)
  assert dev.is_cuda and dev.dtype == torch.int64
  np.testing.assert_array_equal(dev.cpu().numpy(), want, err_msg=str(what))
  return x, got


def test_the_constants_are_those_the_cases_assume():
  assert MAX_BITS == spike_metrics.PATTERN_MAX_BITS == 24
  assert 1 <= LDS_BITS < MAX_BITS and BLOCK_SAMPLES >= 64 and MAX_BLOCKS >= 1
  assert _lib.CG_ABI_VERSION == 20
  assert _lib.load().cg_pattern_hist_ws_bytes(3, 6, 2) >= 0


@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 6, 2)])
def test_smallest_shapes(shape):
  for rate in (0.0, 0.5, 1.0):
    _check(*_case(*shape, seed=1, rate=rate), (shape, rate))


def test_more_than_one_pass_of_the_grid():
  N = 2 * BLOCK_SAMPLES * MAX_BLOCKS + 37
  x, want = _case(N, 3, 1, seed=2)
  assert want.sum() == N and (want > 0).all()
  _check(x, want, N)


@pytest.mark.parametrize('K', [LDS_BITS, LDS_BITS + 1])
def test_the_last_lds_and_the_first_global_case(K):
  T, C = _split(K)
  x, want = _case(5000, T, C, seed=3, rate=0.25)
  assert (want > 0).sum() > 1000
  _check(x, want, K)


def test_the_largest_code():
  x = samples(1000, 6, 4, seed=4, rate=0.5)
  x[-1] = 1.0   # the last table entry is reached
  x[-2] = 0.0
  want = spike_metrics.pattern_histogram(x)
  assert want.shape == (1 << MAX_BITS,) and want[-1] == 1 and want[0] == 1
  _check(x, want, 24)


def test_every_sample_the_same_pattern():
  N, T, C = 200000, 6, 2
  one = samples(1, T, C, seed=5, rate=0.5)
  x = np.broadcast_to(one, (N, T, C))
  code = int(spike_metrics.pattern_codes(one)[0])
  assert 0 < code < 4095
  want = np.zeros(4096, np.int64)
  want[code] = N
  _, got = _check(x, want, 'all equal')
  assert got[code] == N
  # the same through a stride-0 view of the one sample
  view = torch.from_numpy(one).to(DEV).expand(N, T, C)
  assert view.stride(0) == 0
  np.testing.assert_array_equal(_launch(view), want)


def test_permuted_and_negative_strides():
  N, T, C = 3001, 6, 2
  stored = samples(N, C, T, seed=6)        # (n, neurons, L)
  view = stored.transpose(0, 2, 1)         # the (n, L, neurons) view
  want = spike_metrics.pattern_histogram(view)
  d = torch.from_numpy(stored).to(DEV).permute(0, 2, 1)
  assert d.stride() == (T * C, 1, T) and not d.is_contiguous()
  np.testing.assert_array_equal(_launch(d), want)
  np.testing.assert_array_equal(
      spike_metrics.pattern_histogram_device(d).cpu().numpy(), want)
  # channel-padded rows: C = 2 of 5 stored, every other sample
  padded = samples(2 * N, T, 5, seed=7)
  want = spike_metrics.pattern_histogram(padded[::2, :, 1:3])
  d = torch.from_numpy(padded).to(DEV)[::2, :, 1:3]
  assert d.stride() == (2 * T * 5, 5, 1)
  np.testing.assert_array_equal(_launch(d), want)
  # time and samples walked backwards.  torch has no negative strides: the C
  # entry is given the last sample's last time step and negative strides
  x, _ = _case(N, T, C, seed=8)
  want = spike_metrics.pattern_histogram(x[::-1, ::-1, :])
  d = torch.from_numpy(x.copy()).to(DEV)
  counts = torch.full((1 << (T * C),), POISON, dtype=torch.int64, device=DEV)
  first = d.data_ptr() + 4 * ((N - 1) * T * C + (T - 1) * C)
  _lib.call('cg_pattern_histogram', first, N, T, C, -T * C, -C, 1, counts, None,
            0, nets._stream())
  torch.cuda.synchronize()
  np.testing.assert_array_equal(counts.cpu().numpy(), want)


@pytest.mark.parametrize('K', [12, 24])
def test_packed_samples_read_whole_and_frame_by_frame(K):
  """A sample whose frames fill K consecutive elements, K a multiple of 4 and
  16-byte aligned, is read with 16-byte loads; one element further into the
  same buffer the alignment is gone and every frame is loaded on its own."""
  T, C = _split(K)
  N = 2 * BLOCK_SAMPLES + 5
  stored = samples(N, C, T, seed=15, rate=0.4)       # (n, neurons, L)
  want = spike_metrics.pattern_histogram(stored.transpose(0, 2, 1))
  flat = torch.zeros(N * K + 4, dtype=torch.float32, device=DEV)
  for shift in (0, 1, 4):
    flat.fill_(1.0)   # (elements around the samples would count as spikes)
    flat[shift:shift + N * K] = torch.from_numpy(stored).to(DEV).reshape(-1)
    view = flat[shift:shift + N * K].view(N, C, T).permute(0, 2, 1)
    assert view.data_ptr() % 16 == (4 * shift) % 16
    np.testing.assert_array_equal(_launch(view), want, err_msg=str(shift))
  # samples a multiple of 4 elements apart, and 5 apart
  for pitch in (K + 4, K + 5):
    rows = torch.ones(N, pitch, dtype=torch.float32, device=DEV)
    rows[:, :K] = torch.from_numpy(stored).to(DEV).reshape(N, K)
    view = rows[:, :K].view(N, C, T).permute(0, 2, 1)
    assert view.stride(0) == pitch
    np.testing.assert_array_equal(_launch(view), want, err_msg=str(pitch))


def test_nan_and_negative_zero_frames():
  x = samples(2000, 3, 2, seed=9).copy()
  rng = np.random.RandomState(10)
  x[rng.random_sample(x.shape) < 0.2] = np.nan     # spikes
  x[rng.random_sample(x.shape) < 0.2] = -0.0       # none
  x[rng.random_sample(x.shape) < 0.1] = -2.5       # spikes
  x[rng.random_sample(x.shape) < 0.1] = np.inf     # spikes
  want = spike_metrics.pattern_histogram(x)
  assert np.isnan(x).any() and np.signbit(x[x == 0]).any()
  _check(x, want, 'nan / -0.0')
  # every frame NaN: the all-active pattern; every frame -0.0: the silent one
  for value, code in ((np.nan, 63), (-0.0, 0)):
    got = _launch(torch.full((100, 3, 2), value, dtype=torch.float32, device=DEV))
    assert got[code] == 100 and got.sum() == 100


def test_garbage_in_the_output_buffer_and_the_same_bits_twice():
  for K in (12, LDS_BITS + 1):
    T, C = _split(K)
    x, want = _case(5000, T, C, seed=11)
    d = torch.from_numpy(x.copy()).to(DEV)
    counts = torch.from_numpy(np.random.RandomState(K).randint(
        -2**62, 2**62, size=1 << K, dtype=np.int64)).to(DEV)
    first = _launch(d, counts).copy()
    np.testing.assert_array_equal(first, want)
    # the buffer now holds the counts themselves: they are not added to
    second = _launch(d, counts)
    np.testing.assert_array_equal(second, first)


def test_invalid_arguments_are_refused_and_nothing_is_written():
  N, T, C = 64, 6, 2
  x = torch.from_numpy(samples(N, T, C, seed=12)).to(DEV)
  counts = torch.full((1 << (T * C),), POISON, dtype=torch.int64, device=DEV)
  lib = _lib.load()

  def call(x=x, N=N, T=T, C=C, counts=counts, ws_bytes=0):
    return lib.cg_pattern_histogram(x, N, T, C, T * C, C, 1, counts, None,
                                    ws_bytes, nets._stream())

  need = lib.cg_pattern_hist_ws_bytes(N, T, C)
  E = _lib.CG_EINVAL
  for kw in (dict(x=None), dict(counts=None), dict(N=0), dict(N=-1), dict(T=0),
             dict(C=0), dict(T=-6, C=-2), dict(T=5, C=5), dict(T=25, C=1),
             dict(T=1, C=25), dict(T=1 << 16, C=1 << 16),
             dict(ws_bytes=need - 1)):
    assert call(**kw) == E, kw
  torch.cuda.synchronize()
  assert bool((counts == POISON).all())
  for shape in ((N, 0, C), (N, 5, 5), (0, T, C)):
    assert lib.cg_pattern_hist_ws_bytes(*shape) < 0
  assert call() == 0
  torch.cuda.synchronize()
  assert int(counts.sum()) == N
  # the wrapper refuses host arrays, other dtypes, ranks and K > 24
  for bad in (samples(4, 2, 2), x.double(), x[0], x.reshape(2, 32, 12),
              x[:0]):
    with pytest.raises(ValueError):
      spike_metrics.pattern_histogram_device(bad)


def test_deconvolution_of_six_step_traces_equals_the_host():
  n, L, C = 1000, 6, 2
  rng = np.random.RandomState(13)
  signals = calcium(samples(n, L, C, seed=14), rng, noise=0.3)
  want = spike_helper.deconvolve_signals(
      np.ascontiguousarray(signals.transpose(0, 2, 1)).reshape(n * C, L))
  want = want.reshape(n, C, L).transpose(0, 2, 1)
  assert 0.05 < want.mean() < 0.6
  got = spike_helper.deconvolve_signals_device(torch.from_numpy(signals).to(DEV))
  assert got.shape == (n, L, C)
  np.testing.assert_array_equal(got.cpu().numpy(), want)
  np.testing.assert_array_equal(
      spike_metrics.pattern_histogram_device(got).cpu().numpy(),
      spike_metrics.pattern_histogram(want))


def test_cli_on_the_device_writes_what_the_host_writes(tmp_path):
  input_dir, output_dir, _ = surrogate_dirs(str(tmp_path), 3000)
  files = {}
  for device in ('cpu', 'gpu'):
    # (three batches a file on the device, the last one short)
    csm.main(csm.build_parser().parse_args(
        ['--input_dir', input_dir, '--output_dir', output_dir, '--device',
         device, '--batch_samples', '1024', '--verbose', '0']))
    with open(os.path.join(output_dir, 'surrogate_metrics.json'), 'rb') as file:
      report = file.read()
    counts = dict(np.load(os.path.join(output_dir, 'pattern_counts.npz')))
    files[device] = (report, counts)
    os.remove(os.path.join(output_dir, 'surrogate_metrics.json'))
    os.remove(os.path.join(output_dir, 'pattern_counts.npz'))
  assert files['gpu'][0] == files['cpu'][0]
  assert sorted(files['gpu'][1]) == sorted(files['cpu'][1]) == [
      'generated', 'ground_truth', 'surrogate']
  for name, want in files['cpu'][1].items():
    got = files['gpu'][1][name]
    assert got.dtype == np.int64 and got.sum() == 3000
    np.testing.assert_array_equal(got, want)
