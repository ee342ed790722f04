"""GPU tests of cg_pair_histogram (csrc/pair_hist.hip: the bin counts pandas.cut
gives the pooled upper triangles of a pair of matrices, one workgroup per pair)
against its numpy statement spike_metrics.pair_histograms -- counts, sizes,
edges (bit for bit) and status exactly -- and of compute_metrics.py --device gpu
with the histograms cut on the device against CALCIUMGAN_DEVICE_KL=0.  Every
case is one launch on valid input.  Shapes are (P, C, C)."""
import functools
import json
import os
import warnings

import numpy as np
import pytest
import torch

import compute_metrics as cm
from calciumgan_amd import _lib, nets
from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import spike_metrics
from pair_hist_cases import CASES, NUM_BINS, case, to_device
from test_hip_van_rossum import _run_dir

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _statement(name, bins=NUM_BINS):
  a, b = case(name)
  out = spike_metrics.pair_histograms(a, b, bins)
  for x in out:
    x.setflags(write=False)
  return out


def _launch(a, b, bins=NUM_BINS, with_edges=True):
  """The C entry on output buffers filled with a non-zero pattern."""
  P, C = a.shape[:2]
  counts = torch.full((P, 2, bins), -7, dtype=torch.int32, device=DEV)
  valid = torch.full((P, 2), -7, dtype=torch.int32, device=DEV)
  status = torch.full((P,), -7, dtype=torch.int32, device=DEV)
  edges = (torch.full((P, bins + 1), float('nan'), dtype=torch.float64,
                      device=DEV) if with_edges else None)
  _lib.call('cg_pair_histogram', nets._p(a), a.stride(0), a.stride(1),
            a.stride(2), nets._p(b), b.stride(0), b.stride(1), b.stride(2), P, C,
            bins, nets._p(counts), nets._p(valid), nets._p(edges),
            nets._p(status), nets._stream())
  torch.cuda.synchronize()
  return tuple(None if t is None else t.cpu().numpy()
               for t in (counts, valid, edges, status))


def _assert_equal(got, want, what):
  for name, g, w in zip(('counts', 'valid', 'edges', 'status'), got, want):
    if g is None:
      continue
    assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
    if name == 'edges':
      diff = _bits(g) != _bits(w)
    else:
      diff = g != w
    assert not diff.any(), (what, name, np.argwhere(diff)[:8])


@pytest.mark.parametrize('name', CASES)
def test_equal_to_the_statement(name):
  a, b = (to_device(x, DEV) for x in case(name))
  assert a.stride() == tuple(s // 8 for s in case(name)[0].strides)
  assert b.stride() == tuple(s // 8 for s in case(name)[1].strides)
  want = _statement(name)
  got = _launch(a, b)
  print('%s: status %s, sizes %s' % (name, got[3].tolist(), got[1].tolist()))
  _assert_equal(got, want, name)
  # a second call gives the same bits; without edges the rest is the same
  again = _launch(a, b)
  _assert_equal(again, got, name + ' (second call)')
  assert np.array_equal(_bits(again[2]), _bits(got[2]))
  _assert_equal(_launch(a, b, with_edges=False), want, name + ' (edges=NULL)')
  # the wrapper
  dev = spike_metrics.pair_histograms_device(a, b, NUM_BINS)
  assert [t.dtype for t in dev] == [torch.int32, torch.int32, torch.float64,
                                    torch.int32]
  assert all(t.is_cuda for t in dev)
  _assert_equal(tuple(t.cpu().numpy() for t in dev), want, name + ' (wrapper)')


@pytest.mark.parametrize('bins', [1, 2, 7, 256])
def test_other_bin_numbers(bins):
  a, b = (to_device(x, DEV) for x in case('c17_strided'))
  _assert_equal(_launch(a, b, bins), _statement('c17_strided', bins), bins)


def test_invalid_arguments_are_refused_and_nothing_is_written():
  a, b = (to_device(x, DEV) for x in case('c3'))
  P, C = a.shape[:2]
  counts = torch.full((P, 2, NUM_BINS), -7, dtype=torch.int32, device=DEV)
  valid = torch.full((P, 2), -7, dtype=torch.int32, device=DEV)
  status = torch.full((P,), -7, dtype=torch.int32, device=DEV)
  edges = torch.full((P, NUM_BINS + 1), -7.0, dtype=torch.float64, device=DEV)
  lib = _lib.load()

  def call(a=a, b=b, P=P, C=C, bins=NUM_BINS, counts=counts, valid=valid,
           status=status):
    return lib.cg_pair_histogram(
        nets._p(a), 9, 3, 1, nets._p(b), 9, 3, 1, P, C, bins, nets._p(counts),
        nets._p(valid), nets._p(edges), nets._p(status), nets._stream())

  E = _lib.CG_EINVAL
  for kw in (dict(a=None), dict(b=None), dict(counts=None), dict(valid=None),
             dict(status=None), dict(P=0), dict(P=-1), dict(C=1), dict(C=0),
             dict(C=4097), dict(bins=0), dict(bins=-1), dict(bins=257)):
    assert call(**kw) == E, kw
  torch.cuda.synchronize()
  for t in (counts, valid, status):
    assert bool((t == -7).all())
  assert bool((edges == -7.0).all())
  # the wrapper refuses host arrays, other dtypes, ranks and shapes
  for bad in ((case('c3')[0], case('c3')[1]), (a.float(), b.float()),
              (a[0], b[0]), (a, b[:2]), (a[:, :2], b[:, :2])):
    with pytest.raises(ValueError):
      spike_metrics.pair_histograms_device(*bad)
  with pytest.raises(ValueError):
    spike_metrics.pair_histograms_device(a, b, 0)


def _report(hp, device_kl, monkeypatch):
  monkeypatch.setenv('CALCIUMGAN_DEVICE_KL', '1' if device_kl else '0')
  with warnings.catch_warnings(), np.errstate(all='ignore'):
    warnings.simplefilter('ignore')
    report = cm.main(hp)[0]
  report.pop('elapse')
  # (NaN-aware, and what spike_metrics.json holds)
  return json.dumps(report, sort_keys=True)


@pytest.mark.parametrize('flags', [[], ['--victor_purpura']])
def test_report_equals_the_host_cut_report(tmp_path, monkeypatch, flags):
  """The run directory of test_compute_metrics_on_the_device_against_the_host_
  path: 24 trials of 6 neurons.  tests/test_pair_hist_host.py's statement says
  no pair of it is degenerate (checked on the host trains before this ran on a
  GPU), so no pair may take the host fallback."""
  d = dg.make_dataset(num_neurons=6, sequence_length=480, num_segments=24)
  _run_dir(tmp_path, d)
  args = ['--output_dir', str(tmp_path), '--num_processors', '1', '--verbose',
          '0', '--device', 'gpu', '--batch_trials', '10'] + flags
  hp = cm.build_parser().parse_args(args)
  got = _report(hp, True, monkeypatch)
  assert hp._kl_host_fallbacks == 0
  assert torch.is_tensor(hp._recorded_statistics_device['van_rossum'])
  assert not hasattr(hp, '_recorded_statistics')
  hq = cm.build_parser().parse_args(args)
  want = _report(hq, False, monkeypatch)
  assert not hasattr(hq, '_kl_host_fallbacks')
  assert not hasattr(hq, '_recorded_statistics_device')
  print(got)
  assert got == want
  keys = {'firing_rate_kl', 'correlation_kl', 'van_rossum_kl',
          'van_rossum_heatmap_min'} | ({'victor_purpura_kl'} if flags else set())
  assert set(json.loads(got)) == keys
  for key in keys - {'firing_rate_kl', 'van_rossum_heatmap_min'}:
    assert np.isfinite(json.loads(got)[key]['mean'])
  # a second epoch's call reuses the recorded side
  cached = hp._recorded_statistics_device
  assert _report(hp, True, monkeypatch) == got
  assert hp._recorded_statistics_device is cached and hp._kl_host_fallbacks == 0


def test_a_trial_without_correlations_takes_the_host_fallback(tmp_path,
                                                              monkeypatch):
  """Two trials; the recorded trains of the first are silent, so its
  correlations are all NaN: status 1, that pair alone goes through
  pairs_kl_divergence, which divides by its size 0 as it always did."""
  d = dg.make_dataset(num_neurons=6, sequence_length=480, num_segments=2)
  d['spikes'] = d['spikes'].copy()
  d['spikes'][0] = 0
  _run_dir(tmp_path, d)
  args = ['--output_dir', str(tmp_path), '--num_processors', '1', '--verbose',
          '0', '--device', 'gpu', '--victor_purpura']
  hp = cm.build_parser().parse_args(args)
  got = _report(hp, True, monkeypatch)
  assert hp._kl_host_fallbacks == 1
  want = _report(cm.build_parser().parse_args(args), False, monkeypatch)
  print(got)
  assert got == want
  assert np.isnan(json.loads(got)['correlation_kl']['mean'])
  assert np.isfinite(json.loads(got)['van_rossum_kl']['mean'])
