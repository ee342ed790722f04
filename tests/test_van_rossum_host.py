"""CPU tests of the device van Rossum distances and correlations
(csrc/van_rossum.hip, cg_spike_corrcoef in csrc/spikes.hip): the C ABI carries
the entry points, invalid arguments launch nothing, and the numpy statements
the kernels are tested against -- the frame-grid recursion of the van Rossum
kernel sums and the integer form of the Pearson correlation -- equal closed
forms bit for bit and the existing host functions to stated rounding bounds."""
import ctypes
import math
import os
import re

import numpy as np

import compute_metrics as cm
from calciumgan_amd import _lib
from calciumgan_amd import build as cg_build
from calciumgan_amd.gan.utils import spike_metrics
from van_rossum_cases import (correlation_cases, dg_trial as _dg_trial,
                              gram_reference as _gram_reference,
                              random_trains as _random_trains)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'calciumgan_hip.h')
NEW = ('cg_van_rossum', 'cg_spike_corrcoef')
U = 2.0**-53


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_header_signatures_and_both_libraries_carry_the_entry_points():
  cg_build.build(verbose=False)
  src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
  declared = set(re.findall(r'\b(?:int|long long)\s+(cg_\w+)\s*\(', src))
  assert 'van_rossum.hip' in cg_build.SOURCES
  for name in NEW:
    assert name in declared, name
    assert name in _lib.SIGNATURES, name
  for precision in ('bf16', 'f16'):
    lib = _lib.load(precision)
    for name in NEW:
      assert hasattr(lib, name), (precision, name)
    assert lib.cg_abi_version() == 20
  assert '#define CG_ABI_VERSION 20' in open(HEADER).read()


def test_nothing_is_launched_for_invalid_arguments():
  """(host-side argument checks: they return before any HIP call)"""
  lib = _lib.load()
  p = ctypes.c_void_p(0x1000)
  E = _lib.CG_EINVAL

  def vr(spikes=p, B=2, T=48, C=6, decay=0.9, gram=p, dist=p):
    return lib.cg_van_rossum(spikes, B, T, C, T * C, C, 1, decay, gram, dist, None)

  assert vr(spikes=None) == E
  assert vr(gram=None, dist=None) == E
  assert vr(B=0) == E and vr(T=0) == E and vr(C=0) == E
  assert vr(B=-1) == E and vr(T=-3) == E and vr(C=-2) == E
  assert vr(decay=-1e-9) == E and vr(decay=1.0 + 1e-9) == E
  assert vr(decay=float('nan')) == E
  assert vr(C=4097) == E            # the documented limit: C <= 4096
  assert vr(T=2**24 + 1) == E       # and T <= 2^24

  def cc(spikes=p, B=2, T=48, C=6, corr=p):
    return lib.cg_spike_corrcoef(spikes, B, T, C, T * C, C, 1, corr, None)

  assert cc(spikes=None) == E and cc(corr=None) == E
  assert cc(B=0) == E and cc(T=0) == E and cc(C=0) == E
  assert cc(T=23) == E              # nb < 2
  assert cc(T=2048, C=4000) == E    # counts beyond the LDS limit


def test_gram_at_exact_decays_equals_the_closed_forms_bit_for_bit():
  for n, T in ((6, 480), (17, 13), (1, 1), (5, 40)):
    sp = _random_trains(n, T, 0.3, seed=n + T)
    counts = sp.astype(np.float64).sum(1)
    # decay 1: every pair of spikes counts 1
    S = spike_metrics.van_rossum_gram_frames(sp, 1.0)
    assert S.dtype == np.float64 and S.shape == (n, n)
    assert np.array_equal(_bits(S), _bits(np.outer(counts, counts)))
    # decay 0: only equal frames count
    S = spike_metrics.van_rossum_gram_frames(sp, 0.0)
    assert np.array_equal(_bits(S), _bits(sp.astype(np.float64) @
                                          sp.astype(np.float64).T))
  # decay 1/2 at T = 40: a direct sum of exact powers of two (>= 2^-39, sums
  # below 2^11: everything fits in 53 bits)
  sp = _random_trains(7, 40, 0.4, seed=3)
  sp[6] = 1.0
  frames = [np.nonzero(r)[0] for r in sp]
  want = np.array([[sum(2.0**-abs(int(k) - int(l)) for k in fi for l in fj)
                    for fj in frames] for fi in frames])
  S = spike_metrics.van_rossum_gram_frames(sp, 0.5)
  assert np.array_equal(_bits(S), _bits(want))


def test_distance_frames_known_answers():
  """The answers of test_van_rossum_and_victor_purpura_known_answers."""
  T = 24 * 20
  a, b, c, e = (np.zeros(T, np.float32) for _ in range(4))
  a[24] = 1
  b[24 + 12] = 1
  c[[24, 24 * 10]] = 1
  d = spike_metrics.van_rossum_distance_frames(np.stack([a, b, c, e]))
  assert d.shape == (4, 4) and np.all(np.diag(d) == 0)
  np.testing.assert_allclose(d[0, 3], 1.0, rtol=1e-12)
  np.testing.assert_allclose(d[0, 1], np.sqrt(2 * (1 - np.exp(-0.5))), rtol=1e-12)
  np.testing.assert_allclose(d[0, 2], 1.0, rtol=1e-12)
  assert np.array_equal(_bits(d), _bits(d.T))
  cross = spike_metrics.van_rossum_distance_frames(np.stack([a, b]),
                                                   np.stack([c, e]))
  assert np.array_equal(_bits(cross), _bits(d[2:, :2]))
  np.testing.assert_allclose(
      cross, spike_metrics.van_rossum_distance(np.stack([a, b]),
                                               np.stack([c, e])), rtol=1e-12)
  assert spike_metrics.van_rossum_decay(1.0) == math.exp(-1.0 / 24.0)


def test_gram_frames_against_the_kernel_matrix_statement():
  """Entrywise within 4 (n_i n_j + 2 T) 2^-53 S_ref: n_i n_j rounded
  exponentials and products on the reference side, <= 2 T recursion steps and
  additions on ours, all terms non-negative; the factor 4 is the margin."""
  worst = 0.0
  for name, sp in (('dg6', _dg_trial(6, 480)), ('dg102', _dg_trial(102, 2048)),
                   ('dense', _random_trains(6, 480, 0.5, seed=9))):
    T = sp.shape[1]
    ref = _gram_reference(sp)
    got = spike_metrics.van_rossum_gram_frames(sp, spike_metrics.van_rossum_decay())
    n = sp.sum(1).astype(np.float64)
    bound = 4 * (np.outer(n, n) + 2 * T) * U * ref
    err = np.abs(got - ref)
    assert np.all(err <= bound), (name, float(np.max(err / np.maximum(bound, 1e-300))))
    worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    assert np.array_equal(got == 0, ref == 0), name
  print('worst fraction of the bound: %.3g' % worst)


def test_correlation_exact_against_np_corrcoef():
  """NaN positions identical, finite entries within 4 nb 2^-53 absolute (np.cov
  sums nb rounded products per entry in float64; ours rounds three times), the
  diagonal exactly 1 where finite."""
  worst = 0.0
  for name, sp in correlation_cases().items():
    nb = sp.shape[1] // 12
    want = spike_metrics.correlation_coefficients(sp)
    got = spike_metrics.correlation_coefficients_exact(sp)
    assert got.dtype == np.float64 and got.shape == want.shape, name
    assert np.array_equal(np.isnan(got), np.isnan(want)), name
    fin = np.isfinite(want)
    assert fin.any(), name
    err = np.abs(got[fin] - want[fin]).max()
    assert err <= 4 * nb * U, (name, err / (nb * U))
    worst = max(worst, err / (nb * U))
    diag = np.diag(got)
    assert np.all(diag[np.isfinite(diag)] == 1.0), name
    assert np.array_equal(_bits(got), _bits(got.T)), name
  print('worst error / (nb 2^-53): %.3g' % worst)
  sp = correlation_cases()['special']
  got = spike_metrics.correlation_coefficients_exact(sp)
  assert np.isnan(got[0]).all() and np.isnan(got[1]).all() and got[2, 3] == 1.0
  # the cross block is sliced as correlation_coefficients slices it
  a, b = sp[2:4], sp[2:5]
  cross = spike_metrics.correlation_coefficients_exact(a, b)
  assert cross.shape == spike_metrics.correlation_coefficients(a, b).shape
  full = spike_metrics.correlation_coefficients_exact(np.concatenate([a, b]))
  assert np.array_equal(_bits(cross), _bits(full[len(a):, :len(b)]))


def test_compute_metrics_device_flags_parse():
  p = cm.build_parser()
  d = p.parse_args([])
  assert d.device == 'cpu' and d.batch_trials == 128
  a = p.parse_args(['--device', 'gpu', '--batch_trials', '16'])
  assert a.device == 'gpu' and a.batch_trials == 16
