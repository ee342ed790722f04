"""CPU tests of the on-device spike statistics (csrc/spikes.hip): the C ABI
carries the new entry points, the host-filled power table is libm's, the
per-lane loop of the device kernel -- compiled for the host from the same
header -- equals cg_oasis_ar1 bit for bit, the numpy statement of "statistics of
a batch + error sums" equals compute_dg_metrics, and the new flag parses."""
import ctypes
import ctypes.util
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import compute_dg_metrics as cdm
import main as cli
from calciumgan_amd import _lib
from calciumgan_amd import build as cg_build
from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import h5_helper, spike_helper, spike_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'calciumgan_hip.h')
NEW = ('cg_oasis_ws_bytes', 'cg_oasis_ar1_batched', 'cg_spike_stats',
       'cg_spike_stats_error_ws_elems', 'cg_spike_stats_error')


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_header_signatures_and_both_libraries_carry_the_entry_points():
  cg_build.build(verbose=False)
  src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
  declared = set(re.findall(r'\b(?:int|long long)\s+(cg_\w+)\s*\(', src))
  assert 'spikes.hip' in cg_build.SOURCES
  for name in NEW:
    assert name in declared, name
    assert name in _lib.SIGNATURES, name
  for precision in ('bf16', 'f16'):
    lib = _lib.load(precision)
    for name in NEW:
      assert hasattr(lib, name), (precision, name)
  assert _lib.load().cg_abi_version() == 20
  assert '#define CG_ABI_VERSION 20' in open(HEADER).read()


def test_workspace_queries_against_their_formulas():
  lib = _lib.load()
  # 20 bytes (v, w: f64; l: i32) per stack entry, T entries per trace, traces
  # rounded up to whole waves; 1 GiB at most, in whole waves of traces
  assert lib.cg_oasis_ws_bytes(13056, 2048) == 20 * 2048 * 13056
  assert lib.cg_oasis_ws_bytes(1, 1) == 20 * 64
  assert lib.cg_oasis_ws_bytes(100, 13) == 20 * 13 * 128
  per_trace = 20 * 2048
  assert lib.cg_oasis_ws_bytes(10**6, 2048) == (2**30 // per_trace // 64 * 64) * per_trace
  assert lib.cg_oasis_ws_bytes(10**6, 2048) <= 2**30
  assert lib.cg_oasis_ws_bytes(0, 5) == -1 and lib.cg_oasis_ws_bytes(5, 0) == -1
  # one row of four partial sums per block of 2048 elements, 1024 rows at most
  assert lib.cg_spike_stats_error_ws_elems(0, 0) == 4
  assert lib.cg_spike_stats_error_ws_elems(128 * 102, 128 * 5253) == 4 * 329
  assert lib.cg_spike_stats_error_ws_elems(10**9, 5) == 4 * 1024
  assert lib.cg_spike_stats_error_ws_elems(-1, 5) == -1


def test_nothing_is_launched_for_invalid_arguments():
  """(host-side argument checks: they return before any HIP call)"""
  lib = _lib.load()
  p = ctypes.c_void_p(0x1000)
  assert lib.cg_spike_stats(p, 4, 23, 6, 0, 0, 0, p, p, None) == _lib.CG_EINVAL
  assert lib.cg_spike_stats(p, 4, 2048, 4000, 0, 0, 0, p, p, None) == _lib.CG_EINVAL
  assert lib.cg_oasis_ar1_batched(p, 1, 4, 16, 0, 1, 16, 1.0, 0.0, 0.95, 0.55,
                                  0.5, p, p, 0, 1, 16, None, None, p, 20 * 16 * 63,
                                  None) == _lib.CG_EINVAL   # < one wave of stack
  assert lib.cg_oasis_ar1_batched(p, 1, 4, 16, 0, 1, 16, 1.0, 0.0, 0.95, 0.55,
                                  0.5, None, p, 0, 1, 16, None, None, p, 1 << 20,
                                  None) == _lib.CG_EINVAL   # no power table
  assert lib.cg_spike_stats_error(p, p, 4, p, p, 4, p, None, None) == _lib.CG_EINVAL


def test_pow_table_is_libm_pow_bit_for_bit():
  libm = ctypes.CDLL(ctypes.util.find_library('m'))
  libm.pow.restype = ctypes.c_double
  libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]
  for g in (0.95, 0.5, 0.999):
    table = spike_helper.oasis_pow_table(g, 2049)
    want = np.array([libm.pow(g, float(l)) for l in range(2049)])
    assert np.array_equal(_bits(table), _bits(want)), g
  assert table[0] == 1.0 and table[1] == 0.999


def _traces():
  """name -> float32 trace: the cases of the GPU test, host-sized."""
  d = dg.make_dataset(num_neurons=16, sequence_length=2048, num_segments=2)
  rng = np.random.RandomState(3)
  t = {'dg%d' % c: d['signals'][0, :, c] for c in range(0, 16, 3)}
  t['ramp'] = np.arange(2048) * 1.0  # y[t] > g y[t-1] + s_min: no merge
  t['constant'] = np.full(400, 0.7)
  t['zeros'] = np.zeros(50)
  t['negative'] = -np.ones(50)
  for T in (1, 2, 13, 400, 2048):
    t['uniform%d' % T] = rng.uniform(0, 1, T)
    t['wide%d' % T] = rng.uniform(0, 3, T)
    t['normal%d' % T] = rng.randn(T) * 2
  return ({k: np.asarray(v, np.float32) for k, v in t.items()},
          float(d['info']['signals_min']), float(d['info']['signals_max']))


@pytest.mark.parametrize('s_min', [0.0, 0.55])
def test_flat_loop_with_the_table_equals_cg_oasis_ar1(s_min):
  """The device kernel's per-lane loop (csrc/oasis_flat.h: flat merge-or-push
  loop, register-held top pools, powers from the table, c not stored) built for
  the host: float64 bit patterns of c and s equal cg_oasis_ar1's, the trains
  equal, and the pure-python restatement agrees at its existing 1e-12 bar -- on
  traces whose result depends on the table (every merge reads it)."""
  traces, smin, smax = _traces()
  merged = 0
  for name, x in traces.items():
    for scale, offset in ((1.0, 0.0), (smax - smin, smin)):
      # (utils.denormalize on a float32 array: float32 product, float32 sum)
      y = x if scale == 1.0 else x * np.float32(scale) + np.float32(offset)
      assert y.dtype == np.float32
      c0, s0 = spike_helper.oasis_ar1(y.astype(np.float64), 0.95, s_min=s_min)
      c1, s1, sp = spike_helper.oasis_ar1_flat(x, 0.95, s_min, 0.5, scale, offset)
      assert np.array_equal(_bits(c0), _bits(c1)), (name, scale)
      assert np.array_equal(_bits(s0), _bits(s1)), (name, scale)
      assert np.array_equal(sp, np.where(s0 > 0.5, 1.0, 0.0).astype(np.float32))
      merged += int(np.sum(np.diff(c0) < 0))
      if len(x) <= 400:
        c2, s2 = spike_helper.oasis_ar1_python(y.astype(np.float64), 0.95,
                                               s_min=s_min)
        np.testing.assert_allclose(c1, c2, atol=1e-12)
        np.testing.assert_allclose(s1, s2, atol=1e-12)
  assert merged > 1000  # the decays inside merged pools: the table was used
  # the ramp never merges: full stack depth, one pool per frame
  c, _, _ = spike_helper.oasis_ar1_flat(traces['ramp'], 0.95, s_min)
  assert np.array_equal(c, traces['ramp'].astype(np.float64))


def test_flat_train_equals_deconvolve_signals():
  traces, _, _ = _traces()
  rows = np.stack([v for v in traces.values() if len(v) == 2048])
  want = spike_helper.deconvolve_signals(rows)
  got = np.stack([spike_helper.oasis_ar1_flat(r, 0.95, 0.55)[2] for r in rows])
  assert want.sum() > 0 and np.array_equal(got, want)


def test_numpy_batch_statement_equals_compute_dg_metrics(tmp_path):
  """spike_metrics.batch_statistics + error_sums + report_from_sums (what the
  device kernels are tested against) == get_data_statistics + report on a file
  written with h5_helper."""
  rng = np.random.RandomState(5)
  n, T, C = 5, 250, 7
  real = (rng.uniform(size=(n, T, C)) < 0.15).astype(np.int8)
  fake = (rng.uniform(size=(n, T, C)) < 0.10).astype(np.int8)
  fake[:, :, 2] = 0  # a silent neuron: zero variance
  files = []
  for name, spikes in (('real', real), ('fake', fake)):
    f = str(tmp_path / (name + '.h5'))
    h5_helper.write(f, {'signals': spikes.astype(np.float32), 'spikes': spikes})
    files.append(f)
  hp = SimpleNamespace(num_neurons=C, num_trials=n)
  rfr, rcov = cdm.get_data_statistics(hp, files[0])
  ffr, fcov = cdm.get_data_statistics(hp, files[1])
  want = cdm.report(rfr, ffr, rcov, fcov)
  r1, c1 = spike_metrics.batch_statistics(real)
  r2, c2 = spike_metrics.batch_statistics(fake)
  assert r1.dtype == np.float32 and c1.shape == (n, C * (C + 1) // 2)
  assert np.array_equal(r1, rfr.T) and np.array_equal(c1, rcov.T)
  assert np.array_equal(r2, ffr.T) and np.array_equal(c2, fcov.T)
  got = spike_metrics.report_from_sums(
      spike_metrics.error_sums(r1, r2, c1, c2), r1.size, c1.size)
  np.testing.assert_allclose(
      [got['spike_metrics/firing_rate_mae'], got['spike_metrics/firing_rate_rmse'],
       got['spike_metrics/covariance_mae'], got['spike_metrics/covariance_mse']],
      [want['firing_rate']['mae'], want['firing_rate']['rmse'],
       want['covariance']['mae'], want['covariance']['mse']], rtol=1e-6)
  # sums, not means: an epoch formed from two batches is the epoch
  a = spike_metrics.error_sums(r1[:2], r2[:2], c1[:2], c2[:2])
  b = spike_metrics.error_sums(r1[2:], r2[2:], c1[2:], c2[2:])
  np.testing.assert_allclose(a + b, spike_metrics.error_sums(r1, r2, c1, c2),
                             rtol=1e-12)


def test_spike_metrics_flag_parses_and_other_defaults_are_unchanged():
  p = cli.build_parser()
  d = vars(p.parse_args([]))
  # off by default: the flag is absent from a namespace that did not ask for it
  # (main.py reads getattr(hparams, 'spike_metrics', False)), which leaves the
  # namespace of a plain run the reference's flag set
  assert getattr(p.parse_args([]), 'spike_metrics', False) is False
  d.pop('spike_metrics', None)
  assert vars(p.parse_args(['--spike_metrics']))['spike_metrics'] is True
  assert d == dict(
      input_dir='dataset/tfrecords', output_dir='runs', batch_size=64,
      num_units=32, kernel_size=24, strides=2, m=2, n=2, epochs=20, dropout=0.2,
      learning_rate=0.0001, noise_dim=32, gradient_penalty=10.0, model='wavegan',
      activation='leakyrelu', batch_norm=False, layer_norm=False,
      algorithm='wgan-gp', n_critic=5, clear_output_dir=False, save_generated='',
      plot_weights=False, skip_checkpoints=False, mixed_precision=False,
      profile=False, dpi=120, verbose=1)
  m = cdm.build_parser()
  assert vars(m.parse_args([])) == dict(output_dir='runs', num_trials=5,
                                        device='cpu')
  assert m.parse_args(['--device', 'gpu']).device == 'gpu'


def test_device_entry_points_refuse_host_arrays():
  """No quiet fall-back: the device functions want device tensors."""
  with pytest.raises(ValueError):
    spike_helper.deconvolve_signals_device(np.zeros((2, 8), np.float32))
  with pytest.raises(ValueError):
    spike_metrics.batch_statistics_device(np.zeros((2, 24, 3), np.float32))
