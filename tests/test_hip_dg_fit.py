"""GPU tests of cg_dg_correlation (csrc/dg_fit.hip: the latent correlation of
every neuron pair of the dichotomised-Gaussian fit) against its numpy statement
dg_fit.gauss_correlation, and of dataset/generate_dg_data.py --device gpu
against --device cpu.  Every case is a call on valid input.

The rule, per pair (dg_fit.compare_with_statement): equal status, and lambda
and the iteration count equal bit for bit.  One excuse: the counts differ by
exactly 1 and the statement's residual at the earlier stop lies within 1e-13 of
tol (exp, sin, cos, asin or erfc of the device library rounded the other way at
the stop test); at most 1 % of a case's pairs may use it.  Whatever the excuse,
a converged pair has |f_statement(lambda)| <= tol (1 + 1e-3).  Shares observed:
profiles/dg_fit_parity.txt."""
import os
import pickle

import numpy as np
import pytest
import torch

import dg_fit_cases as cases
from calciumgan_amd import _lib, nets
from calciumgan_amd.data import dg, dg_fit

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
MAX_BLOCKS, BLOCK_PAIRS = (_lib.CONSTANTS['CG_DG_FIT_' + n]
                           for n in ('MAX_BLOCKS', 'BLOCK_PAIRS'))
POISON_F, POISON_I = -7.25, -0x01234567


def _to_device(*arrays):
  return tuple(torch.from_numpy(np.array(a)).to(DEV) for a in arrays)


def _launch(rates, gamma, cov, tol=cases.TOL, maxiters=1000, out=None):
  """The C entry on device tensors, cov of any strides; the outputs are filled
  with a pattern beforehand."""
  C = rates.shape[0]
  if out is None:
    out = (torch.full((C, C), POISON_F, dtype=torch.float64, device=DEV),
           torch.full((C, C), POISON_I, dtype=torch.int32, device=DEV),
           torch.full((C, C), POISON_I, dtype=torch.int32, device=DEV))
  _lib.call('cg_dg_correlation', rates, gamma, cov, cov.stride(0),
            cov.stride(1), C, tol, maxiters, *out, nets._stream())
  torch.cuda.synchronize()
  return tuple(t.cpu().numpy() for t in out)


def _check(system, want, what, tol=cases.TOL, maxiters=1000, cov=None):
  """Launch on `system` = (rates, gamma, cov, ...) and hold the result against
  the statement's `want` by the rule; `cov` replaces the device view of the
  covariance.  Returns the device result."""
  rates, gamma, host_cov = system[:3]
  d_rates, d_gamma, d_cov = _to_device(rates, gamma, host_cov)
  got = _launch(d_rates, d_gamma, d_cov if cov is None else cov, tol, maxiters)
  C = len(rates)
  assert got[0].dtype == np.float64 and got[1].dtype == got[2].dtype == np.int32
  np.testing.assert_array_equal(np.diag(got[0]), np.ones(C))
  assert not np.diag(got[1]).any() and not np.diag(got[2]).any()
  assert not (got[0] == POISON_F).any(), what
  assert not (got[1] == POISON_I).any() and not (got[2] == POISON_I).any(), what
  report = dg_fit.compare_with_statement(rates, gamma, host_cov, got, want, tol)
  print('{}: {} pairs, {} excused'.format(what, report['pairs'],
                                          report['excused']))
  assert not report['failures'], (what, report['failures'][:5])
  assert report['excused'] <= report['pairs'] // 100, (what, report)
  return got


def test_the_constants_are_those_the_cases_assume():
  assert MAX_BLOCKS >= 1 and BLOCK_PAIRS == 4
  assert _lib.CG_ABI_VERSION == 20


@pytest.mark.parametrize('C', [2, 3])
def test_smallest_shapes(C):
  _check(cases.random_system(C, 1), cases.statement('random_system', C, 1), C)


def test_every_status_both_signs_of_gamma_and_the_clip():
  system = cases.status_system()
  rates, gamma, _, _ = system
  assert gamma.min() < -3.7 and gamma.max() > 2.0
  assert np.isclose(rates, 1e-4).any() and (rates == 0).any()
  want = cases.statement('status_system')
  got = _check(system, want, 'statuses')
  assert sorted(np.unique(got[1])) == [0, 1, 2, 3, 4, 5]
  # the pair whose bracket closes: status 5 with the full count
  a, b = cases.CLOSING_PAIR
  assert got[1][a, b] == 5 and got[2][a, b] == 1000
  assert 0 <= dg_fit.BRACKET - got[0][a, b] < 1e-15
  for (i, j), code in cases.STATUS_PAIRS.items():
    assert got[1][i, j] == got[1][j, i] == code
  for (i, j), v in cases.NEAR_ENDS.items():    # lambda near +-0.99999
    assert abs(got[0][i, j] - v) < 1e-5 and got[1][i, j] == 0
  # status 5 through maxiters = 3
  limited = _check(system, cases.statement('status_system', maxiters=3),
                   'maxiters 3', maxiters=3)
  assert (limited[1] == 5).sum() == 2 * (28 - len(cases.STATUS_PAIRS))
  assert set(limited[2][limited[1] == 5]) == {3}


def test_more_than_one_pass_of_the_grid():
  C = 2
  while C * (C - 1) // 2 <= MAX_BLOCKS * BLOCK_PAIRS:
    C += 1
  assert C * (C - 1) // 2 - MAX_BLOCKS * BLOCK_PAIRS < C   # just past one pass
  # (tol 1e-6: a third fewer evaluations of the statement's 1024-node sums)
  system = cases.random_system(C, 2)
  want = cases.statement('random_system', C, 2, tol=1e-6)
  got = _check(system, want, 'C = {}'.format(C), tol=1e-6)
  # (at this tolerance a few pairs of two rare neurons return lambda_0 at once)
  assert (got[1] == 0).mean() > 0.9 and np.isin(got[1], (0, 2)).all()


def test_default_tolerance_on_a_few_hundred_pairs():
  system = cases.random_system(24, 3)
  want = cases.statement('random_system', 24, 3)
  got = _check(system, want, 'C = 24')
  i, j = np.tril_indices(24, -1)
  density = cases.bivariate_density(system[1][i], system[1][j], system[3][i, j])
  assert np.all(np.abs(got[0] - system[3])[i, j] <=
                2 * (cases.TOL + cases.EPS_CDF) / density)
  # the wrapper returns the same bits, as device tensors
  dev = dg_fit.gauss_correlation_device(*_to_device(*system[:3]))
  assert all(t.is_cuda for t in dev)
  for a, b in zip(dev, got):
    np.testing.assert_array_equal(a.cpu().numpy(), b)


def test_strided_and_transposed_covariance():
  system = cases.status_system()
  rates, gamma, cov, _ = system
  C = len(rates)
  want = cases.statement('status_system')
  # every other element of every third row of a larger buffer
  big = torch.full((3 * C, 2 * C), 0.5, dtype=torch.float64, device=DEV)
  big[::3, ::2] = torch.from_numpy(np.array(cov)).to(DEV)
  view = big[::3, ::2]
  assert view.stride() == (6 * C, 2)
  _check(system, want, 'strided', cov=view)
  # the transposed view of the stored transpose
  stored = torch.from_numpy(np.ascontiguousarray(np.array(cov).T)).to(DEV)
  assert stored.t().stride() == (1, C)
  _check(system, want, 'transposed', cov=stored.t())
  # only the lower triangle is read: rubbish above the diagonal changes nothing
  lower = np.tril(np.array(cov)) + np.triu(np.full((C, C), 0.123), 1)
  _check(system, want, 'lower triangle',
         cov=torch.from_numpy(lower).to(DEV))


def test_garbage_in_the_outputs_and_the_same_bits_twice():
  system = cases.random_system(24, 3)
  d = _to_device(*system[:3])
  rng = np.random.RandomState(0)
  out = (torch.from_numpy(rng.standard_normal((24, 24))).to(DEV),
         torch.from_numpy(rng.randint(-2**31, 2**31 - 1, (24, 24),
                                      dtype=np.int64).astype(np.int32)).to(DEV),
         torch.from_numpy(rng.randint(-2**31, 2**31 - 1, (24, 24),
                                      dtype=np.int64).astype(np.int32)).to(DEV))
  first = [a.copy() for a in _launch(*d, out=out)]
  second = _launch(*d, out=out)
  fresh = _launch(*d)
  for a, b, c in zip(first, second, fresh):
    np.testing.assert_array_equal(a.view(np.int64) if a.dtype == np.float64
                                  else a,
                                  b.view(np.int64) if b.dtype == np.float64
                                  else b)
    np.testing.assert_array_equal(a, c)


def test_invalid_arguments_are_refused_and_nothing_is_written():
  rates, gamma, cov = _to_device(*cases.status_system()[:3])
  C = rates.shape[0]
  out = (torch.full((C, C), POISON_F, dtype=torch.float64, device=DEV),
         torch.full((C, C), POISON_I, dtype=torch.int32, device=DEV),
         torch.full((C, C), POISON_I, dtype=torch.int32, device=DEV))
  lib = _lib.load()

  def call(rates=rates, gamma=gamma, cov=cov, C=C, tol=1e-10, maxiters=1000,
           corr=out[0], status=out[1], iterations=out[2]):
    return lib.cg_dg_correlation(rates, gamma, cov, C, 1, C, tol, maxiters,
                                 corr, status, iterations, nets._stream())

  for kw in (dict(rates=None), dict(gamma=None), dict(cov=None),
             dict(corr=None), dict(status=None), dict(iterations=None),
             dict(C=1), dict(C=0), dict(C=-3), dict(C=4097), dict(tol=0.0),
             dict(tol=-1e-10), dict(tol=float('nan')), dict(maxiters=0),
             dict(maxiters=-1)):
    assert call(**kw) == _lib.CG_EINVAL, kw
  torch.cuda.synchronize()
  assert bool((out[0] == POISON_F).all())
  assert bool((out[1] == POISON_I).all()) and bool((out[2] == POISON_I).all())
  assert call() == 0
  torch.cuda.synchronize()
  assert not bool((out[0] == POISON_F).any())
  # the wrapper refuses host arrays, other dtypes and shapes
  host = cases.status_system()
  for bad in ((host[0], host[1], host[2]),
              (rates.float(), gamma, cov), (rates, gamma[:-1], cov),
              (rates, gamma, cov[:, :-1]), (rates[:1], gamma[:1], cov[:1, :1])):
    with pytest.raises(ValueError):
      dg_fit.gauss_correlation_device(*bad)
  with pytest.raises(ValueError):
    dg_fit.gauss_correlation_device(rates, gamma, cov, tol=0.0)


def test_tool_on_the_device_writes_what_the_host_writes(tmp_path):
  import sys
  sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(
      os.path.abspath(__file__))), 'dataset'))
  import generate_dg_data as tool
  C, T = 12, 4000
  _, gamma, _, lam = cases.random_system(C, 11, spread=0.3)
  rng = np.random.RandomState(11)
  spikes = dg.sample_spikes_corr(gamma, dg_fit.corr_for_sampling(lam), T, rng)
  source = str(tmp_path / 'recording.pkl')
  with open(source, 'wb') as file:
    pickle.dump({'signals': dg.spikes_to_signals(spikes, rng), 'oasis': spikes},
                file)
  twins = {}
  for device in ('cpu', 'gpu'):
    out = str(tmp_path / (device + '.pkl'))
    tool.main(tool.build_parser().parse_args(
        ['--input', source, '--output', out, '--device', device,
         '--is_dg_data']))
    with open(out, 'rb') as file:
      twins[device] = pickle.load(file)
  cpu, gpu = twins['cpu'], twins['gpu']
  stats = dg_fit.recording_statistics(spikes)
  np.testing.assert_array_equal(gpu['covariance'], cpu['covariance'])
  np.testing.assert_array_equal(gpu['mean'], cpu['mean'])
  # (the pickles carry no iteration counts: the rule on the fits themselves)
  fits = {d: dg_fit.fit(spikes, device=d) for d in ('cpu', 'gpu')}
  for d in fits:
    np.testing.assert_array_equal(fits[d]['correlation'], twins[d]['correlation'])
  report = dg_fit.compare_with_statement(
      *stats, *((fits[d]['correlation'], fits[d]['status'],
                 fits[d]['iterations']) for d in ('gpu', 'cpu')))
  assert not report['failures'] and report['excused'] <= report['pairs'] // 100
  if np.array_equal(gpu['correlation'], cpu['correlation']):
    assert gpu['signals'].tobytes() == cpu['signals'].tobytes()
    assert gpu['oasis'].tobytes() == cpu['oasis'].tobytes()
  assert gpu['oasis'].shape == (C, T) and gpu['oasis'].mean() > 0.05
