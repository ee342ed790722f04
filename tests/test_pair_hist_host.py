"""CPU tests of the device histogram KL (csrc/pair_hist.hip): the numpy statement
the kernel is tested against, spike_metrics.pair_histograms, equals pandas.cut
-- edges bit for bit, counts exactly -- on the cases of pair_hist_cases.py; its
status bits sit exactly where pandas raises or a side is empty;
compute_metrics.kl_from_counts on its counts is the float32 pairs_kl_divergence
returns; the parser is unchanged, CALCIUMGAN_DEVICE_KL is read where documented
and the C ABI carries the entry point under version 20."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest

import compute_metrics as cm
from calciumgan_amd import _lib
from calciumgan_amd import build as cg_build
from calciumgan_amd.gan.utils import spike_metrics
from pair_hist_cases import CASES, NUM_BINS, case, triangles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'calciumgan_hip.h')


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _statement(name):
  a, b = case(name)
  return spike_metrics.pair_histograms(a, b, NUM_BINS)


def _pandas(pooled):
  """(labels, edges) of pandas.cut, or the ValueError it raises."""
  try:
    cat, edges = pd.cut(pooled, bins=NUM_BINS, labels=np.arange(NUM_BINS),
                        retbins=True)
  except ValueError as e:
    return e
  return np.asarray(cat), np.asarray(edges)


def test_the_cases_cover_every_status():
  seen, pairs = set(), 0
  for name in CASES:
    status = _statement(name)[3]
    seen |= set(int(s) for s in status)
    pairs += len(status)
  assert seen == {0, 1, 2, 4}, seen
  assert pairs == 22
  assert list(_statement('degenerate')[3]) == [2, 4]
  assert list(_statement('nan_rows')[3]) == [0, 0, 1]
  assert list(_statement('one_value')[3]) == [0, 0, 0]


@pytest.mark.parametrize('name', CASES)
def test_statement_equals_pandas(name):
  a, b = case(name)
  counts, valid, edges, status = _statement(name)
  P, C = a.shape[:2]
  assert counts.shape == (P, 2, NUM_BINS) and counts.dtype == np.int32
  assert valid.shape == (P, 2) and valid.dtype == np.int32
  assert edges.shape == (P, NUM_BINS + 1) and edges.dtype == np.float64
  assert status.shape == (P,) and status.dtype == np.int32
  checked = 0
  for p in range(P):
    real, fake = triangles(a, b, p)
    ours = (cm._upper(a[p], C), cm._upper(b[p], C))
    assert np.array_equal(_bits(real), _bits(ours[0]))
    assert np.array_equal(_bits(fake), _bits(ours[1]))
    assert list(valid[p]) == [len(real), len(fake)]
    assert bool(status[p] & 1) == (len(real) == 0 or len(fake) == 0)
    pooled = np.concatenate([real, fake])
    if len(pooled) == 0:
      assert status[p] == 1
      continue
    got = _pandas(pooled)
    assert bool(status[p] & 6) == isinstance(got, ValueError), (p, got)
    if status[p] & 6:
      assert bool(status[p] & 2) == bool(np.isinf(pooled).any())
    if status[p] != 0:
      assert not counts[p].any() and not edges[p].any()
      continue
    labels, want_edges = got
    assert np.array_equal(_bits(edges[p]), _bits(want_edges)), p
    is_real = np.arange(len(pooled)) < len(real)
    for s, mask in enumerate((is_real, ~is_real)):
      want = [int(np.sum(labels[mask] == k)) for k in range(NUM_BINS)]
      assert list(counts[p, s]) == want, (p, s)
    # every value has a bin here: the counts add up to the sizes
    assert list(counts[p].sum(1)) == list(valid[p])
    checked += 1
  assert checked == int((status == 0).sum())


def test_on_edges_puts_values_on_both_sides_of_every_edge():
  """The case is what it says: every inner edge of the statement is a pooled
  value, with its two neighbours, and sits in the bin to its left."""
  a, b = case('on_edges')
  counts, _, edges, status = _statement('on_edges')
  assert not status.any()
  for p in range(2):
    pooled = np.concatenate(triangles(a, b, p))
    for k in range(1, NUM_BINS):
      e = edges[p, k]
      assert e in pooled and np.nextafter(e, np.inf) in pooled
      assert np.nextafter(e, -np.inf) in pooled
    ids = np.searchsorted(edges[p], edges[p, 1:], side='left')
    assert list(ids) == list(range(1, NUM_BINS + 1))
  # dividing instead of comparing is not the rule: it moves values there
  moved = 0
  for p in range(2):
    pooled = np.concatenate(triangles(a, b, p))
    mn, mx = pooled.min(), pooled.max()
    by_division = np.ceil((pooled - mn) / ((mx - mn) / NUM_BINS)).astype(int)
    by_edges = np.searchsorted(edges[p], pooled, side='left')
    moved += int((np.clip(by_division, 1, NUM_BINS) != by_edges).sum())
  print('values a division would put into another bin:', moved)
  assert moved > 0


def test_other_bin_numbers_and_the_one_bin_histogram():
  a, b = case('c17_strided')
  for bins in (1, 2, 7, 256):
    counts, valid, edges, status = spike_metrics.pair_histograms(a, b, bins)
    assert not status.any()
    for p in range(len(a)):
      pooled = np.concatenate(triangles(a, b, p))
      labels, want = pd.cut(pooled, bins=bins, labels=False, retbins=True)
      assert np.array_equal(_bits(edges[p]), _bits(want))
      assert list(counts[p].sum(0)) == list(np.bincount(labels, minlength=bins))


def test_arguments_of_the_statement():
  a, b = case('c3')
  for bad in ((a.astype(np.float32), b), (a[0], b[0]), (a, b[:2]),
              (a[:, :2], b[:, :2]), (a[:, :1, :1], b[:, :1, :1])):
    with pytest.raises(ValueError):
      spike_metrics.pair_histograms(*bad)
  with pytest.raises(ValueError):
    spike_metrics.pair_histograms(a, b, 0)


@pytest.mark.parametrize('name', CASES)
def test_kl_from_counts_is_the_tail_of_pairs_kl_divergence(name):
  a, b = case(name)
  counts, valid, _, status = _statement(name)
  for p in np.nonzero(status == 0)[0]:
    real, fake = triangles(a, b, p)
    want = cm.pairs_kl_divergence([(real, fake)])
    got = cm.kl_from_counts(counts[p, 0], counts[p, 1], valid[p, 0], valid[p, 1])
    assert isinstance(got, np.float32) and want.dtype == np.float32
    assert got.tobytes() == want[0].tobytes(), (p, got, want[0])
    # numpy integers as sizes do not widen the arithmetic
    assert cm.kl_from_counts(counts[p, 0], counts[p, 1], int(valid[p, 0]),
                             int(valid[p, 1])).tobytes() == got.tobytes()


def test_parser_namespace_and_the_knob(monkeypatch):
  ns = vars(cm.build_parser().parse_args([]))
  assert ns == dict(output_dir='runs', num_processors=6, all_epochs=False,
                    num_neuron_plots=6, num_trial_plots=6, plots_per_row=3,
                    dpi=120, format='pdf', verbose=1, seed=12, device='cpu',
                    batch_trials=128)
  assert cm.NUM_BINS == NUM_BINS == 30
  monkeypatch.delenv('CALCIUMGAN_DEVICE_KL', raising=False)
  assert cm.device_kl_enabled() is True
  monkeypatch.setenv('CALCIUMGAN_DEVICE_KL', '0')
  assert cm.device_kl_enabled() is False
  monkeypatch.setenv('CALCIUMGAN_DEVICE_KL', '1')
  assert cm.device_kl_enabled() is True
  assert 'CALCIUMGAN_DEVICE_KL=0' in open(os.path.join(ROOT, 'README.md')).read()


def test_header_signature_and_both_libraries_carry_the_entry_point():
  cg_build.build(verbose=False)
  src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
  declared = set(re.findall(r'\b(?:int|long long)\s+(cg_\w+)\s*\(', src))
  assert 'pair_hist.hip' in cg_build.SOURCES
  assert 'cg_pair_histogram' in declared
  assert len(_lib.SIGNATURES['cg_pair_histogram']) == 16
  for precision in ('bf16', 'f16'):
    lib = _lib.load(precision)
    assert hasattr(lib, 'cg_pair_histogram'), precision
    assert lib.cg_abi_version() == 20
  assert '#define CG_ABI_VERSION 20' in open(HEADER).read()


def test_nothing_is_launched_for_invalid_arguments():
  """(host-side argument checks: they return before any HIP call)"""
  lib = _lib.load()
  q = ctypes.c_void_p(0x1000)
  E = _lib.CG_EINVAL

  def call(a=q, b=q, P=2, C=6, bins=30, counts=q, valid=q, edges=q, status=q):
    return lib.cg_pair_histogram(a, C * C, C, 1, b, C * C, C, 1, P, C, bins,
                                 counts, valid, edges, status, None)

  assert call(a=None) == E and call(b=None) == E and call(counts=None) == E
  assert call(valid=None) == E and call(status=None) == E
  assert call(P=0) == E and call(P=-1) == E
  assert call(C=1) == E and call(C=0) == E and call(C=-5) == E
  assert call(C=4097) == E
  assert call(bins=0) == E and call(bins=-1) == E and call(bins=257) == E
  assert call(edges=None, P=0) == E
