"""GPU tests of cg_tensor_summary (csrc/summary.hip: statistics and histogram
buckets of any number of segments of a float32 buffer in one call) against its
numpy statements (summary_helper.variable_statistics / histogram_buckets, laid
out by tensor_summary_cases.statement), and of the Python surface on top of it:
nets.TensorSummary, FlatParams.summaries and Summary.histogram.  Every case is
one call on valid input; outputs are pre-filled with a non-zero pattern and the
workspace with garbage."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tensor_summary_cases as tc
from calciumgan_amd import _lib, nets
from calciumgan_amd.gan.utils import summary_helper as sh

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
K = tc.NUM_BUCKETS
U = 2.0**-53


@pytest.fixture(autouse=True)
def _back_to_bf16():
  yield
  _lib.use('bf16')


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _launch(name, k=K, lib=None):
  """The C entry on a case -> (stats, buckets) as numpy arrays."""
  buf, offsets, lengths = tc.case(name)
  lib = lib or _lib.load()
  nseg, total = len(lengths), sum(lengths)
  data = torch.tensor(buf, device=DEV)
  off = torch.tensor(offsets, dtype=torch.int64, device=DEV)
  ln = torch.tensor(lengths, dtype=torch.int64, device=DEV)
  stats = torch.full((nseg, 8), -7.0, dtype=torch.float64, device=DEV)
  buckets = torch.full((nseg, k, 3), -7.0, dtype=torch.float64, device=DEV)
  nbytes = lib.cg_tensor_summary_ws_bytes(nseg, total, k)
  assert nbytes > 0 and nbytes % 8 == 0
  ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
  assert ws.data_ptr() % 8 == 0
  rc = lib.cg_tensor_summary(data, off, ln, nseg, total, k, stats, buckets, ws,
                             nbytes, nets._stream())
  assert rc == 0
  torch.cuda.synchronize()
  # the input is only read
  assert np.array_equal(data.cpu().numpy().view(np.int32), buf.view(np.int32))
  return stats.cpu().numpy(), buckets.cpu().numpy()


def _check(name, got, k=K, only=None):
  """Device (stats, buckets) of a case -- of its segments `only`, in that order
  -- against the statement."""
  stats, buckets = got
  want_stats, want_buckets = tc.statement(name, k)
  segs = tc.segments(name)
  if only is not None:
    want_stats, want_buckets = want_stats[only], want_buckets[only]
    segs = [segs[i] for i in only]
  assert stats.shape == want_stats.shape and buckets.shape == want_buckets.shape
  for s, seg in enumerate(segs):
    st, ws_, what = stats[s], want_stats[s], (name, s, len(seg))
    # n, nonfinite and the counts: equal
    assert st[0] == ws_[0] == len(seg) and st[7] == ws_[7], what
    assert np.array_equal(buckets[s, :, 2], want_buckets[s, :, 2]), what
    # the edges: bit for bit
    assert np.array_equal(_bits(buckets[s, :, :2]),
                          _bits(want_buckets[s, :, :2])), what
    if ws_[7] > 0:
      assert np.isnan(st[1:7]).all() and not buckets[s].any(), what
      continue
    n = float(len(seg))
    d = seg.astype(np.float64)
    # minimum and maximum: equal by value
    assert st[1] == ws_[1] == d.min() and st[2] == ws_[2] == d.max(), what
    # mean and stddev: from the returned sum and sq, bit for bit
    assert _bits(st[4]) == _bits(np.float64(st[3]) / np.float64(n)), what
    assert _bits(st[6]) == _bits(np.sqrt(np.float64(st[5]) / np.float64(n))), what
    # sum and sq: recursive summation in any order errs by at most gamma_n times
    # the sum of magnitudes, and 2 n u is above gamma_n
    assert abs(st[3] - math.fsum(d)) <= 2 * n * U * math.fsum(np.abs(d)), what
    c = d - st[4]
    c2 = c * c
    assert abs(st[5] - math.fsum(c2)) <= 2 * (n + 4) * U * math.fsum(c2), what
    if st[1] == st[2]:  # a constant segment: exact
      v = d[0]
      assert (st[3], st[4], st[5], st[6]) == (n * v, v, 0.0, 0.0), what
      assert buckets[s, 0].tolist() == [v - 0.5, v + 0.5, n], what
      assert not buckets[s, 1:].any(), what
    else:
      assert buckets[s, :, 2].sum() == n, what


@pytest.mark.parametrize('name', tc.CASES)
def test_equal_to_the_statement(name):
  got = _launch(name)
  stats = got[0]
  print('%s: %d segments, nonfinite %s' % (name, len(stats),
                                           stats[:, 7].tolist()))
  _check(name, got)
  # a second call returns the same bits
  again = _launch(name)
  assert np.array_equal(_bits(again[0]), _bits(stats))
  assert np.array_equal(_bits(again[1]), _bits(got[1]))


def test_what_the_cases_are_there_for():
  """Figures of single cases spelled out, beside the statement."""
  _, buckets = _launch('boundaries')
  assert buckets[0, :, 2].tolist() == [1.0] * 29 + [2.0]
  assert buckets[1, :, 2].tolist() == [133.0] * 29 + [266.0]
  assert buckets[2, :, 2].tolist() == [1.0] * 29 + [2.0]
  # a float32 evaluation of the index would move this many values
  _, buckets = _launch('inexact')
  for s, (pair, differing) in enumerate(tc.INEXACT):
    x = tc.inexact_widths(*pair)
    wrong = np.bincount(tc.float32_index(x), minlength=K)
    assert differing > 0 and not np.array_equal(wrong, buckets[s, :, 2])
  # a NaN and an infinity flag their own segments only
  stats, buckets = _launch('nonfinite')
  assert stats[:, 7].tolist() == [0, 1, 0, 2, 0]
  assert np.isfinite(stats[[0, 2, 4]]).all()
  assert (buckets[[0, 2, 4], :, 2].sum(axis=1) == [100, 300, 64]).all()
  # repeated and overlapping segments are segments like any other
  stats, buckets = _launch('forty')
  assert np.array_equal(_bits(stats[38]), _bits(stats[3]))
  assert np.array_equal(_bits(buckets[38]), _bits(buckets[3]))
  assert stats[39, 0] == 4200


@pytest.mark.parametrize('k', [1, 2, 7, 512])
def test_other_bucket_numbers(k):
  _check('lengths', _launch('lengths', k), k)


def test_invalid_arguments_are_refused_and_nothing_is_written():
  buf, offsets, lengths = tc.case('boundaries')
  nseg, total = len(lengths), sum(lengths)
  lib = _lib.load()
  data = torch.tensor(buf, device=DEV)
  off = torch.tensor(offsets, dtype=torch.int64, device=DEV)
  ln = torch.tensor(lengths, dtype=torch.int64, device=DEV)
  stats = torch.full((nseg, 8), -7.0, dtype=torch.float64, device=DEV)
  buckets = torch.full((nseg, 512, 3), -7.0, dtype=torch.float64, device=DEV)
  nbytes = lib.cg_tensor_summary_ws_bytes(nseg, total, K)
  ws = torch.full((nbytes + 8,), 0xA5, dtype=torch.uint8, device=DEV)

  def call(data=data, off=off, ln=ln, nseg=nseg, total=total, k=K, stats=stats,
           buckets=buckets, ws=ws, ws_bytes=nbytes):
    return lib.cg_tensor_summary(data, off, ln, nseg, total, k, stats, buckets,
                                 ws, ws_bytes, nets._stream())

  E = _lib.CG_EINVAL
  for kw in (dict(data=None), dict(off=None), dict(ln=None), dict(stats=None),
             dict(buckets=None), dict(ws=None), dict(nseg=0), dict(nseg=-1),
             dict(nseg=65536), dict(k=0), dict(k=-1), dict(k=513),
             dict(total=0), dict(total=-1), dict(ws_bytes=nbytes - 1),
             dict(ws_bytes=0), dict(ws=ws[4:]), dict(ws=ws[1:])):
    assert call(**kw) == E, kw
  torch.cuda.synchronize()
  assert bool((stats == -7.0).all()) and bool((buckets == -7.0).all())
  assert bool((ws == 0xA5).all())
  assert lib.cg_tensor_summary_ws_bytes(nseg, total, 513) == -1
  # the wrapper checks the tables it uploads: the kernel cannot
  for offsets_, lengths_, limit in (([0], [0], None), ([0], [-3], None),
                                    ([0], [2**31], None), ([-1], [4], None),
                                    ([5], [4], 8), ([0, 1], [4], None)):
    with pytest.raises(ValueError):
      nets.TensorSummary(offsets_, lengths_, DEV, K, limit=limit)
  for k in (0, 513):
    with pytest.raises(ValueError):
      nets.TensorSummary([0], [4], DEV, k)
  plan = nets.TensorSummary([0], [4], DEV, K, limit=4)
  for bad in (torch.zeros(4), torch.zeros(4, dtype=torch.float64, device=DEV),
              torch.zeros(8, device=DEV)[::2], torch.zeros(3, device=DEV)):
    with pytest.raises(ValueError):
      plan.run(bad)


def test_both_precision_builds_agree_bit_for_bit():
  got = {}
  for precision in ('bf16', 'f16'):
    lib = _lib.load(precision)
    assert lib.cg_tensor_summary and lib.cg_tensor_summary_ws_bytes
    got[precision] = _launch('forty', lib=lib)
  for a, b in zip(got['bf16'], got['f16']):
    assert np.array_equal(_bits(a), _bits(b))
  _check('forty', got['f16'])


def test_flat_params_summaries_in_one_call():
  """The small model's generator laid out by FlatParams (every tensor 4-aligned):
  names, the trainable subset, one call for all variables, one copy."""
  buf, offsets, lengths = tc.case('glorot')
  shapes = [(n,) for n in lengths[:24]]
  names = ['v{}:0'.format(i) for i in range(24)]
  p = nets.FlatParams(shapes, torch.device(DEV), frozen=[6, 7], names=names)
  assert p.names == names and tuple(p.offsets) == offsets[:24]
  assert nets.FlatParams(shapes[:2], torch.device(DEV)).names == [
      'variable_0:0', 'variable_1:0']
  p.set_weights([seg.copy() for seg in tc.segments('glorot')[:24]])
  for trainable_only, idx in ((True, [i for i in range(24) if i not in (6, 7)]),
                              (False, list(range(24)))):
    assert p.summary_indices(trainable_only) == idx
    stats, buckets = p.summaries(K, trainable_only=trainable_only)
    assert stats.is_cuda and stats.dtype == torch.float64
    assert stats.shape == (len(idx), 8) and buckets.shape == (len(idx), K, 3)
    stats, buckets = stats.cpu().numpy(), buckets.cpu().numpy()
    _check('glorot', (stats, buckets), only=idx)
    host = p.summaries_host(K, trainable_only=trainable_only)
    assert np.array_equal(_bits(host[0]), _bits(stats))
    assert np.array_equal(_bits(host[1]), _bits(buckets))
  # the tables and the workspace are kept
  plan = p._summary_plan(K, True)
  assert p._summary_plan(K, True) is plan and plan.nseg == 22
  assert p.summaries(K)[0].data_ptr() == plan.stats.data_ptr()


def test_summary_histogram_of_device_views(tmp_path):
  """A float32 device tensor goes through the kernel in place, whatever its
  offset into its storage; a strided view through a contiguous copy."""
  hp = SimpleNamespace(output_dir=str(tmp_path), verbose=0)
  summary = sh.Summary(hp)
  i = tc.LENGTHS.index(1025)
  # (the case that has this length at an odd offset)
  name = 'lengths' if i % 2 == 0 else 'lengths_aligned_first'
  buf, offsets, lengths = tc.case(name)
  data = torch.tensor(buf, device=DEV)
  view = data[offsets[i]:offsets[i] + 1025]
  assert view.storage_offset() % 4 != 0 and view.data_ptr() % 16 != 0
  square = data[offsets[i]:offsets[i] + 1024].view(32, 32).t()
  assert not square.is_contiguous()
  summary.histogram('odd_offset', view, step=4)
  summary.histogram('transposed', square, step=4, training=False)
  summary.variable_summary(view, 'var', step=5)
  hist = [json.loads(l) for l in open(os.path.join(hp.output_dir,
                                                   'histograms.jsonl'))]
  assert [(h['tag'], h['step']) for h in hist] == [('odd_offset', 4), ('var', 5)]
  seg = tc.segments(name)[i]
  want = sh.histogram_buckets(seg)
  for h in hist:
    assert np.array_equal(_bits(np.array(h['buckets'])), _bits(want))
  va = [json.loads(l) for l in open(os.path.join(hp.output_dir, 'validation',
                                                 'histograms.jsonl'))]
  assert np.array_equal(_bits(np.array(va[0]['buckets'])),
                        _bits(sh.histogram_buckets(seg[:1024])))
  sc = {r['tag']: r['value'] for r in map(json.loads, open(
      os.path.join(hp.output_dir, 'scalars.jsonl')))}
  st = sh.variable_statistics(seg)
  assert sc['var/2_min'] == st['min'] and sc['var/3_max'] == st['max']
  # (two sums of 1025 terms, each within n u sum|d| of the exact one)
  assert abs(sc['var/0_mean'] - st['mean']) <= 2 * U * (
      float(np.abs(seg.astype(np.float64)).sum()) + abs(st['mean']))
  assert sc['var/1_stddev'] == pytest.approx(st['stddev'], rel=1e-12)
  # a NaN among the values: no histogram
  with pytest.raises(ValueError):
    summary.histogram('gap', data[offsets[i] - 1:offsets[i] + 8])
