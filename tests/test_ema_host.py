"""Host tests of --ema_decay: the statement in gan/algorithms/averaging.py
(decay warm-up, the three-rounding update), the header's prototype, the
refusals of cg_ema_update through the built library (they return before any
HIP call, so fake pointers do) and main.py's parser."""
import ctypes
import os
import re

import numpy as np
import pytest

import main as cli
from calciumgan_amd import _lib
from calciumgan_amd.gan.algorithms import averaging as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- decay_at ------------------------------------------------------------------
@pytest.mark.parametrize('decay', [0.1, 0.5, 0.9, 0.999, 0.9999])
def test_first_update_has_decay_one_tenth(decay):
  d = A.decay_at(decay, 0)
  assert isinstance(d, np.float64) and d == np.float64(0.1)


@pytest.mark.parametrize('decay', [0.05, 0.5, 0.9, 0.999])
def test_decay_is_monotone_and_settles_where_the_arguments_cross(decay):
  ds = [A.decay_at(decay, t) for t in range(0, 20000)]
  assert all(b >= a for a, b in zip(ds, ds[1:]))
  assert all(0.0 < d <= decay for d in ds)
  # (1 + t) / (10 + t) >= decay  <=>  t >= (10 decay - 1) / (1 - decay)
  cross = max(0, int(np.ceil((10 * decay - 1) / (1 - decay))))
  for t in range(20000):
    want = decay if (1.0 + t) / (10.0 + t) >= decay else (1.0 + t) / (10.0 + t)
    assert ds[t] == want, t
  assert all(d == decay for d in ds[cross + 1:])
  assert all(d < decay for d in ds[:max(cross - 1, 0)])


def test_one_minus_rounds_once_from_float64():
  for d in (0.1, 0.999, 0.9999, 2.0 / 11.0, 1.0 - 2.0**-30, 0.3):
    om = A.one_minus(np.float64(d))
    assert isinstance(om, np.float32)
    assert om == np.float32(np.float64(1.0) - np.float64(d))
  # rounding d to float32 first is another number: 1 - fl32(0.999) is exact in
  # float32 and is not fl32(1 - 0.999)
  assert A.one_minus(0.999) != np.float32(1.0) - np.float32(0.999)


# -- update_statement -------------------------------------------------------------
def _pairs(n=1000, seed=0):
  rng = np.random.RandomState(seed)
  e = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))).astype(np.float32)
  p = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))).astype(np.float32)
  return e, p


def test_statement_invariants():
  e, p = _pairs()
  out = A.update_statement(e, e.copy(), np.float32(0.37))
  assert out.dtype == np.float32 and out.tobytes() == e.tobytes()
  assert A.update_statement(e, p, np.float32(0.0)).tobytes() == e.tobytes()
  # om = 1 is e - fl(e - p): NOT p wherever the difference rounded
  one = A.update_statement(e, p, np.float32(1.0))
  assert one.tobytes() == (e - (e - p)).astype(np.float32).tobytes()
  assert 0 < np.count_nonzero(one != p) < e.size
  # the inputs are left alone
  e0, p0 = e.copy(), p.copy()
  A.update_statement(e, p, np.float32(0.5))
  assert e.tobytes() == e0.tobytes() and p.tobytes() == p0.tobytes()


@pytest.mark.parametrize('om', [0.001, 0.1, 0.9, 1.0])
def test_statement_is_float64_rounded_once_per_operation(om):
  e, p = _pairs(seed=1)
  om = np.float32(om)
  d = (e.astype(np.float64) - p.astype(np.float64)).astype(np.float32)
  s = (d.astype(np.float64) * np.float64(om)).astype(np.float32)
  want = (e.astype(np.float64) - s.astype(np.float64)).astype(np.float32)
  assert A.update_statement(e, p, om).tobytes() == want.tobytes()
  # a fused multiply-add would differ somewhere: the test can tell the two apart
  fused = (e.astype(np.float64) - d.astype(np.float64) * np.float64(om)).astype(
      np.float32)
  if om != np.float32(1.0):
    assert np.count_nonzero(fused != want) > 0


def test_statement_propagates_nan_and_infinities():
  inf, nan = np.float32(np.inf), np.float32(np.nan)
  e = np.array([nan, 1.0, inf, 1.0, inf, -inf, inf, 1.0], np.float32)
  p = np.array([1.0, nan, 1.0, inf, inf, inf, 1.0, -inf], np.float32)
  out = A.update_statement(e, p, np.float32(0.25))
  # d = e - p; s = d / 4; e - s
  assert np.isnan(out[0]) and np.isnan(out[1])  # a NaN on either side
  assert np.isnan(out[2])  # d = inf, s = inf, inf - inf
  assert out[3] == inf     # d = -inf, s = -inf, 1 + inf
  assert np.isnan(out[4])  # d = inf - inf
  assert np.isnan(out[5])  # d = -inf, s = -inf, -inf + inf
  assert np.isnan(out[6])  # as [2]
  assert out[7] == -inf    # d = inf, s = inf, 1 - inf
  # om = 0 does not shield from an infinity: s = inf * 0 = NaN
  z = A.update_statement(e, p, np.float32(0.0))
  assert np.isnan(z).all()


def test_statement_special_values_one_at_a_time():
  inf = np.float32(np.inf)
  f = lambda e, p, om: A.update_statement(
      np.array([e], np.float32), np.array([p], np.float32), np.float32(om))[0]
  # e finite, p = +inf: d = -inf, s = -inf, e - s = +inf
  assert f(1.0, inf, 0.25) == inf
  # e finite, p = -inf: d = +inf, s = +inf, e - s = -inf
  assert f(1.0, -inf, 0.25) == -inf
  # e = +inf, p finite: d = +inf, s = +inf, inf - inf = nan
  assert np.isnan(f(inf, 1.0, 0.25))
  # signed zeros: e = -0, p = -0: d = -0 - -0 = +0, s = +0, -0 - +0 = -0
  assert np.signbit(f(-0.0, -0.0, 0.5)) and not np.signbit(f(0.0, 0.0, 0.5))
  # denormals are kept, not flushed
  tiny = np.float32(1e-45)
  assert f(tiny, tiny, 0.5) == tiny and f(tiny, 0.0, 1.0) == 0.0
  assert f(3 * tiny, tiny, 0.5) == 2 * tiny


def test_check_decay():
  for bad in (0, 1, -0.1, 1.5, float('nan'), 0.0, 1.0):
    with pytest.raises(ValueError):
      A.check_decay(bad)
  assert A.check_decay(0.999) == 0.999
  assert A.check_decay(np.float32(0.5)) == 0.5


# -- the C ABI -----------------------------------------------------------------
def test_header_declares_cg_ema_update_at_abi_20():
  with open(_lib.HEADER) as f:
    text = f.read()
  src = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
  m = re.search(r'\bint\s+cg_ema_update\s*\(([^()]*)\)\s*;', src)
  assert m, 'no prototype of cg_ema_update'
  assert ' '.join(m.group(1).split()) == (
      'float* ema, const float* p, long long n, float om, void* stream')
  consts, _, protos = _lib.parse_header(text)
  assert consts['CG_ABI_VERSION'] == 20 and _lib.CG_ABI_VERSION == 20
  argtypes, restype = protos['cg_ema_update']
  assert restype is ctypes.c_int and len(argtypes) == 5
  assert issubclass(argtypes[0], _lib.DataPtr) and argtypes[0].ctype == 'float*'
  assert issubclass(argtypes[1], _lib.DataPtr) and argtypes[1].ctype == 'float*'
  assert argtypes[2] is ctypes.c_longlong and argtypes[3] is ctypes.c_float
  assert issubclass(argtypes[4], _lib.DataPtr) and argtypes[4].ctype == 'void*'
  for precision in ('bf16', 'f16'):
    lib = _lib.load(precision)
    assert hasattr(lib, 'cg_ema_update'), precision
    assert lib.cg_abi_version() == 20


@pytest.mark.parametrize('precision', ['bf16', 'f16'])
def test_nothing_is_launched_for_invalid_arguments(precision):
  """(host-side argument checks: they return before any HIP call)"""
  lib = _lib.load(precision)
  q = ctypes.c_void_p(0x1000)
  E = _lib.CG_EINVAL

  def call(ema=q, p=q, n=16, om=0.5):
    return lib.cg_ema_update(ema, p, n, om, None)

  assert call(ema=None) == E and call(p=None) == E
  assert call(ema=None, p=None) == E
  for n in (0, -1, -(1 << 40)):
    assert call(n=n) == E, n
  for om in (-1e-6, -1.0, 1.0 + 2.0**-23, 2.0, float('inf'), float('-inf'),
             float('nan')):
    assert call(om=om) == E, om


# -- main.py ---------------------------------------------------------------------
def test_parser_leaves_the_namespace_alone_without_the_flag():
  plain = cli.build_parser().parse_args([])
  assert not hasattr(plain, 'ema_decay')
  flagged = cli.build_parser().parse_args(['--ema_decay', '0.999'])
  assert flagged.ema_decay == 0.999
  rest = dict(vars(flagged))
  del rest['ema_decay']
  assert rest == vars(plain)
