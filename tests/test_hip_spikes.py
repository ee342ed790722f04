"""GPU tests of the on-device spike statistics (csrc/spikes.hip): batched OASIS
AR(1) deconvolution bit-identical to the host library, per-trial firing rates /
binned covariances and their ordered error sums, GAN.spike_statistics against
the host chain, main.py --spike_metrics and compute_dg_metrics.py --device gpu.
Every case is one launch on valid input.

cg_spike_stats is compared bit for bit with the exact statement of
tests/spike_stats_cases.py (integer sums, one float64 division, one rounding to
float32; tied to spike_metrics.batch_statistics in tests/test_spike_stats.py) at
the (T, C) grid of the older test and at: C = 300 (the second trip of the loops
over c += 256, P = 45 150 pairs on the capped `split` of 8, 61 200 B of LDS),
C = 240 at the 61 440 B that are the most admitted, one bin more refused by both
entries with nothing written, C = 44 / 45 and 119 / 120 on either side of a step
of `split`, channel-major storage and a slice of a wider buffer beside the
contiguous batch, and planted trains (12 spikes in every bin; 2.0, -1.0, a
subnormal and NaN as spikes; -0.0 as none).  cg_spike_stats_error is compared
exactly on planted powers of two -- a dropped, doubled or misplaced element
changes the sums -- from no element to past the 1024 x 2048 elements at which
the grid is capped and a thread strides over a ninth one, and under a derived
rounding bar on random input; its workspace is exactly the size asked for
inside a NaN buffer.  Outputs are over-allocated: their tails keep the fill.
(cg_spike_corrcoef at the same large shapes: tests/test_hip_van_rossum.py.)

Out of scope: C between 301 and the 4096 the entries admit needs T < 2400, a
regime without a path of its own; timing."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import compute_dg_metrics as cdm
import main as cli
import oracle as O
from calciumgan_amd.data import dg
from calciumgan_amd import _lib, nets
from calciumgan_amd.gan.utils import (dataset_helper, spike_helper,
                                      spike_metrics, utils)

import spike_stats_cases as SC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(autouse=True)
def _back_to_bf16():
  yield
  _lib.use('bf16')


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_deconvolution_identical(x_dev, rows_host, s_min, smin=None,
                                    smax=None):
  """x_dev: the device tensor handed to the kernel; rows_host: float32 (traces,
  T), the same traces in the kernel's trace order, BEFORE denormalisation by
  (smin, smax) = a signals_min / max pair (None: none)."""
  scale, offset = (1.0, 0.0) if smin is None else (smax - smin, smin)
  spikes, c, s = spike_helper.deconvolve_signals_device(
      x_dev, scale=scale, offset=offset, s_min=s_min, return_cs=True)
  torch.cuda.synchronize()
  y = rows_host
  if smin is not None:
    y = utils.denormalize(rows_host, x_min=smin, x_max=smax)
  assert y.dtype == np.float32
  c, s = c.cpu().numpy(), s.cpu().numpy()
  for r in range(len(y)):
    c0, s0 = spike_helper.oasis_ar1(y[r].astype(np.float64), 0.95, s_min=s_min)
    assert np.array_equal(_bits(c0), _bits(c[r])), ('c', r)
    assert np.array_equal(_bits(s0), _bits(s[r])), ('s', r)
  sp = spikes.cpu().numpy()
  if x_dev.dim() == 3:
    sp = sp.transpose(0, 2, 1).reshape(len(y), -1)
  want = np.where(s > 0.5, 1.0, 0.0).astype(np.float32)
  assert np.array_equal(sp, want)
  if s_min == 0.55:
    assert np.array_equal(sp, spike_helper.deconvolve_signals(y))
  return sp


@pytest.mark.parametrize('s_min', [0.0, 0.55])
def test_deconvolution_dg_batch_in_place_pitch_128(s_min):
  """(B, L, C) = (4, 2048, 102) DG traces inside a pitch-128 buffer (the
  generator's output layout), denormalised with the set's signals_min / max."""
  d = dg.make_dataset(num_neurons=102, sequence_length=2048, num_segments=4)
  sig = np.ascontiguousarray(d['signals'], dtype=np.float32)
  smin, smax = float(d['info']['signals_min']), float(d['info']['signals_max'])
  buf = torch.full((4, 2048, 128), 7.0, dtype=torch.float32, device=DEV)
  buf[:, :, :102] = torch.from_numpy(sig).to(DEV)
  x = buf[:, :, :102]
  assert x.stride() == (2048 * 128, 128, 1)
  rows = sig.transpose(0, 2, 1).reshape(4 * 102, 2048)
  sp = _assert_deconvolution_identical(x, rows, s_min, smin, smax)
  assert sp.sum() > 100
  # and without denormalisation
  _assert_deconvolution_identical(x, rows, s_min)


@pytest.mark.parametrize('s_min', [0.0, 0.55])
@pytest.mark.parametrize('T', [1, 2, 13, 400])
def test_deconvolution_rows_by_T(T, s_min):
  rng = np.random.RandomState(T)
  rows = np.concatenate([rng.uniform(0, 1, (40, T)), rng.uniform(0, 3, (40, T)),
                         rng.randn(20, T) * 2]).astype(np.float32)
  _assert_deconvolution_identical(torch.from_numpy(rows).to(DEV), rows, s_min)


@pytest.mark.parametrize('s_min', [0.0, 0.55])
def test_deconvolution_ramp_constant_noise(s_min):
  """A rising ramp of 2048 frames (y[t] > g y[t-1] + s_min: never merges, the
  stack reaches its full depth), a constant trace, uniform noise; denormalised
  by a real signals_min / max pair in a second pass."""
  rng = np.random.RandomState(11)
  T = 2048
  rows = np.stack([np.arange(T) * 1.0, np.arange(T) * 0.01, np.full(T, 0.7),
                   np.zeros(T), -np.ones(T)] +
                  [rng.uniform(0, 1, T) for _ in range(70)]).astype(np.float32)
  x = torch.from_numpy(rows).to(DEV)
  _assert_deconvolution_identical(x, rows, s_min)
  d = dg.make_dataset(num_neurons=4, sequence_length=64, num_segments=2)
  smin, smax = float(d['info']['signals_min']), float(d['info']['signals_max'])
  _assert_deconvolution_identical(x, rows, s_min, smin, smax)
  spikes, c, _ = spike_helper.deconvolve_signals_device(x, s_min=s_min,
                                                        return_cs=True)
  assert np.array_equal(c[0].cpu().numpy(), rows[0].astype(np.float64))


def test_deconvolution_in_groups_of_traces_matches_one_launch():
  """A workspace smaller than the batch's full-depth stack: the call walks the
  batch in groups of traces; same result."""
  from calciumgan_amd import _lib, nets
  rng = np.random.RandomState(2)
  rows = rng.uniform(0, 2, (200, 300)).astype(np.float32)
  x = torch.from_numpy(rows).to(DEV)
  want = spike_helper.deconvolve_signals_device(x)
  gpow = torch.from_numpy(spike_helper.oasis_pow_table(0.95, 301)).to(DEV)
  nbytes = 20 * 300 * 64   # one wave of traces
  ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
  out = torch.empty_like(x)
  _lib.call('cg_oasis_ar1_batched', nets._p(x), 1, 200, 300, 0, 1, 300, 1.0, 0.0,
            0.95, 0.55, 0.5, nets._p(gpow), nets._p(out), 0, 1, 300, None, None,
            nets._p(ws), nbytes, nets._stream())
  torch.cuda.synchronize()
  assert torch.equal(out, want)
  assert np.array_equal(out.cpu().numpy(), spike_helper.deconvolve_signals(rows))


_trains = SC.trains
TAIL = 64             # sentinel elements behind every output
FILL = -7.0


def _bits32(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _stats_entry(x):
  """cg_spike_stats on a (B, T, C) device tensor read in place, into outputs
  filled with NaN that are TAIL elements longer than needed, the tail -7: every
  element must be written, the tail must not.  -> numpy (rates, covs)."""
  B, T, C = x.shape
  P = C * (C + 1) // 2
  rates = torch.full((B * C + TAIL,), float('nan'), dtype=torch.float32, device=DEV)
  covs = torch.full((B * P + TAIL,), float('nan'), dtype=torch.float32, device=DEV)
  rates[B * C:] = FILL
  covs[B * P:] = FILL
  _lib.call('cg_spike_stats', nets._p(x), B, T, C, x.stride(0), x.stride(1),
            x.stride(2), nets._p(rates), nets._p(covs), nets._stream())
  torch.cuda.synchronize()
  rates, covs = rates.cpu().numpy(), covs.cpu().numpy()
  assert np.all(rates[B * C:] == FILL) and np.all(covs[B * P:] == FILL)
  assert not np.isnan(rates[:B * C]).any() and not np.isnan(covs[:B * P]).any()
  return rates[:B * C].reshape(B, C), covs[:B * P].reshape(B, P)


def _assert_cov_bits(covs, sp):
  want = SC.exact_covariance(sp)
  diff = _bits32(covs) != _bits32(want)
  print('%d of %d covariances differ from the exact statement' % (
      int(diff.sum()), diff.size))
  assert not diff.any(), np.argwhere(diff)[:8]


@pytest.mark.parametrize('C', [6, 102])
@pytest.mark.parametrize('T', [24, 250, 2048])
def test_statistics_against_spike_metrics(T, C):
  """Firing rates: the float32 the host code returns.  Covariances: the device
  divides the exact integer nb S_ij - S_i S_j once; the host's float64 np.cov
  rounds per term.  Entries whose exact value is 0 -- below half of the smallest
  non-zero magnitude 1 / (nb (nb - 1)) on the host, where np.cov may leave
  ~1e-17 of rounding -- must be exactly 0 on the device; everywhere the host
  returns 0 the device returns 0; all others agree to rtol = 1e-6."""
  B = 3
  sp = _trains(B, T, C, seed=T + C)
  rates, covs = spike_metrics.batch_statistics_device(torch.from_numpy(sp).to(DEV))
  torch.cuda.synchronize()
  rates, covs = rates.cpu().numpy(), covs.cpu().numpy()
  want_r, want_c = spike_metrics.batch_statistics(sp)
  assert rates.dtype == np.float32 and covs.dtype == np.float32
  assert np.array_equal(rates, want_r)
  nb = T // 12
  zero = np.abs(want_c) < 0.5 / (nb * (nb - 1))
  assert np.abs(want_c[zero]).max() < 1e-12          # (host rounding only)
  assert (want_c == 0).sum() >= C and np.all(covs[want_c == 0] == 0)
  assert np.all(covs[zero] == 0)
  np.testing.assert_allclose(covs[~zero], want_c[~zero], rtol=1e-6, atol=0)
  assert (~zero).sum() > 0
  # the exact statement: the same bits
  _assert_cov_bits(covs, sp)
  # a strided view gives the same bits
  buf = torch.zeros(B, T, C + 5, dtype=torch.float32, device=DEV)
  buf[:, :, :C] = torch.from_numpy(sp).to(DEV)
  r2, c2 = spike_metrics.batch_statistics_device(buf[:, :, :C])
  assert np.array_equal(r2.cpu().numpy(), rates)
  assert np.array_equal(c2.cpu().numpy(), covs)


@pytest.mark.parametrize('name', sorted(SC.SHAPES))
def test_statistics_bit_equal_to_the_exact_statement(name):
  """Rates: the float32 the host code returns for the trains `spikes != 0`.
  Covariances: the bits of the exact statement."""
  sp = SC.stats_case(name)
  T, C = SC.SHAPES[name]
  x = torch.from_numpy(sp.copy()).to(DEV)
  rates, covs = _stats_entry(x)
  want_r, _ = spike_metrics.batch_statistics(SC.binary(sp))
  assert np.array_equal(_bits32(rates), _bits32(want_r))
  _assert_cov_bits(covs, sp)
  # the wrapper's outputs hold the same bits, and so does a second call
  r2, c2 = spike_metrics.batch_statistics_device(x)
  assert np.array_equal(_bits32(r2.cpu().numpy()), _bits32(rates))
  assert np.array_equal(_bits32(c2.cpu().numpy()), _bits32(covs))
  if name == 'planted_c6_t48':
    # the {0, 1} trains the host's rule makes of the planted values: same bits
    r3, c3 = _stats_entry(torch.from_numpy(SC.binary(sp)).to(DEV))
    assert np.array_equal(_bits32(r3), _bits32(rates))
    assert np.array_equal(_bits32(c3), _bits32(covs))
    iu = np.triu_indices(C)
    assert np.all(covs[:, (iu[0] == 0) | (iu[0] == 2) | (iu[1] == 2)] == 0)


def test_statistics_same_bits_from_three_layouts():
  """(2, 250, 130) contiguous, stored channel-major (s_t = 1, s_c = T) and as a
  slice of a (2, 250, 136) buffer whose other channels hold 7.0."""
  name = 'c130_t250'
  sp = SC.stats_case(name)
  B, T, C = sp.shape
  want = _stats_entry(torch.from_numpy(sp.copy()).to(DEV))
  _assert_cov_bits(want[1], sp)
  rows = torch.from_numpy(np.ascontiguousarray(sp.transpose(0, 2, 1))).to(DEV)
  x = rows.transpose(1, 2)                             # stored (B, C, T)
  assert tuple(x.shape) == (B, T, C) and x.stride() == (C * T, 1, T)
  buf = torch.full((B, T, 136), 7.0, dtype=torch.float32, device=DEV)
  buf[:, :, :C] = torch.from_numpy(sp.copy()).to(DEV)
  y = buf[:, :, :C]
  assert y.stride() == (T * 136, 136, 1)
  for view in (x, y):
    got = _stats_entry(view)
    assert np.array_equal(_bits32(got[0]), _bits32(want[0]))
    assert np.array_equal(_bits32(got[1]), _bits32(want[1]))


@pytest.mark.parametrize('T,C', SC.REFUSED)
def test_statistics_one_bin_past_the_lds_limit_are_refused(T, C):
  """One more 500-ms bin than 60 KiB of LDS holds: CG_EINVAL, decided on the
  host, with the outputs untouched."""
  assert SC.lds_bytes(T, C) > SC.STATS_MAX_LDS >= SC.lds_bytes(T - 12, C)
  B, P = 2, C * (C + 1) // 2
  x = torch.ones(B, T, C, dtype=torch.float32, device=DEV)
  rates = torch.full((B * C,), FILL, dtype=torch.float32, device=DEV)
  covs = torch.full((B * P,), FILL, dtype=torch.float32, device=DEV)
  rc = _lib.load().cg_spike_stats(nets._p(x), B, T, C, x.stride(0), x.stride(1),
                                  x.stride(2), nets._p(rates), nets._p(covs),
                                  nets._stream())
  torch.cuda.synchronize()
  assert rc == _lib.CG_EINVAL
  assert bool((rates == FILL).all()) and bool((covs == FILL).all())
  with pytest.raises(ValueError):
    spike_metrics.batch_statistics_device(x)


def test_statistics_refuse_fewer_than_two_bins():
  with pytest.raises(ValueError):
    spike_metrics.batch_statistics_device(
        torch.zeros(2, 23, 4, dtype=torch.float32, device=DEV))


@pytest.mark.parametrize('B,C', [(3, 6), (128, 102)])
def test_error_sums_against_numpy_and_bitwise_repeatable(B, C):
  rng = np.random.RandomState(B)
  P = C * (C + 1) // 2
  ra = rng.uniform(0, 3, (B, C)).astype(np.float32)
  rb = rng.uniform(0, 3, (B, C)).astype(np.float32)
  ca = (rng.randn(B, P) * 0.3).astype(np.float32)
  cb = (rng.randn(B, P) * 0.3).astype(np.float32)
  t = [torch.from_numpy(a).to(DEV) for a in (ra, rb, ca, cb)]
  got1 = spike_metrics.error_sums_device(*t)
  got2 = spike_metrics.error_sums_device(*t)
  torch.cuda.synchronize()
  want = spike_metrics.error_sums(ra, rb, ca, cb)
  np.testing.assert_allclose(got1.cpu().numpy(), want, rtol=1e-5)
  assert np.array_equal(got1.cpu().numpy().view(np.int32),
                        got2.cpu().numpy().view(np.int32))


ERR_LEAD = 96         # NaN floats before the workspace of the error sums


def _error_entry(ra, rb, ca, cb):
  """cg_spike_stats_error on host float32 arrays (an empty side is handed over
  as null pointers), its workspace exactly cg_spike_stats_error_ws_elems floats
  inside a NaN buffer whose surroundings must stay NaN, `out` with a fifth
  element that must keep its fill; run twice, the two results the same bits.
  -> float32 (4,)."""
  n_fr, n_cov = len(ra), len(ca)
  elems = _lib.load().cg_spike_stats_error_ws_elems(n_fr, n_cov)
  assert elems == 4 * SC.err_parts(n_fr, n_cov)
  t = [torch.from_numpy(a.copy()).to(DEV) if len(a) else None
       for a in (ra, rb, ca, cb)]
  outs = []
  for _ in range(2):
    buf = torch.full((ERR_LEAD + elems + TAIL,), float('nan'), dtype=torch.float32,
                     device=DEV)
    out = torch.full((5,), FILL, dtype=torch.float32, device=DEV)
    _lib.call('cg_spike_stats_error', nets._p(t[0]), nets._p(t[1]), n_fr,
              nets._p(t[2]), nets._p(t[3]), n_cov, nets._p(out),
              nets._p(buf[ERR_LEAD:]), nets._stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:ERR_LEAD]).all()), 'floats before the workspace'
    assert bool(torch.isnan(buf[ERR_LEAD + elems:]).all()), 'floats behind it'
    assert not bool(torch.isnan(buf[ERR_LEAD:ERR_LEAD + elems]).any())
    out = out.cpu().numpy()
    assert out[4] == FILL
    outs.append(out[:4])
  assert np.array_equal(_bits32(outs[0]), _bits32(outs[1]))
  return outs[0]


@pytest.mark.parametrize('n_fr,n_cov', SC.ERROR_SIZES)
def test_error_sums_of_planted_powers_of_two_are_exact(n_fr, n_cov):
  """The two sets differ at a few indices by distinct powers of two: every
  partial sum is a float32 whatever the order, so the device's sums equal the
  float64 ones exactly."""
  ra, rb, ca, cb = SC.planted_error_inputs(n_fr, n_cov)
  got = _error_entry(ra, rb, ca, cb)
  want = spike_metrics.error_sums(ra, rb, ca, cb)
  print('device', got.tolist(), 'float64', want.tolist())
  assert np.array_equal(got.astype(np.float64), want)
  assert np.all(_bits32(got) >= 0)                     # +0.0 for an empty side


@pytest.mark.parametrize('n_fr,n_cov', SC.RANDOM_ERROR_SIZES)
def test_error_sums_of_random_input_within_the_rounding_bar(n_fr, n_cov):
  """Against the float64 sums of the float32 inputs, within SC.error_bars."""
  ra, rb, ca, cb = SC.random_error_inputs(n_fr, n_cov)
  got = _error_entry(ra, rb, ca, cb).astype(np.float64)
  want = spike_metrics.error_sums(ra, rb, ca, cb)
  bars = SC.error_bars(n_fr, n_cov, want)
  err = np.abs(got - want)
  print('worst fraction of the bar: %.3g (relative errors %s)' % (
      float((err / bars).max()), (err / want).tolist()))
  assert np.all(err <= bars), (err / bars).tolist()


def _tiny_gan(algorithm, L=256, C=16):
  from calciumgan_amd.gan.algorithms import get_algorithm
  from calciumgan_amd.gan.models import get_models
  hp = O.make_hparams(L, C, 8, m=2)
  hp.verbose = 0
  hp.algorithm = algorithm
  hp.normalize = True
  hp.signals_min, hp.signals_max = -1.3225274085998535, 4.2623491287231445
  gen, dis = get_models(hp, None)
  return hp, get_algorithm(hp, gen, dis, None)


@pytest.mark.parametrize('algorithm', ['wgan-gp', 'gan'])
def test_gan_spike_statistics_equals_the_host_chain(algorithm):
  """reverse_preprocessing -> deconvolve_signals -> spike_metrics -> report on
  the same fake batch."""
  B, L, C = 6, 256, 16
  hp, gan = _tiny_gan(algorithm, L, C)
  d = dg.make_dataset(num_neurons=C, sequence_length=L, num_segments=B)
  real = np.ascontiguousarray(d['signals'], dtype=np.float32)
  fake = gan.validate(real)[0]
  assert tuple(fake.shape) == (B, L, C)
  out = gan.spike_statistics(fake, d['spikes'])
  torch.cuda.synchronize()
  assert float(out['firing_rate_count']) == B * C
  assert float(out['covariance_count']) == B * C * (C + 1) // 2
  got = spike_metrics.report_from_sums(
      [out[k] for k in ('firing_rate_abs_sum', 'firing_rate_sq_sum',
                        'covariance_abs_sum', 'covariance_sq_sum')], B * C,
      B * C * (C + 1) // 2)
  # the host chain
  sig = utils.reverse_preprocessing(hp, fake)        # (B, L, C) float32
  assert sig.dtype == np.float32
  fake_sp = np.stack([spike_helper.deconvolve_signals(s.T).T for s in sig])
  dev_sp = spike_helper.deconvolve_signals_device(
      fake, scale=hp.signals_max - hp.signals_min, offset=hp.signals_min)
  assert np.array_equal(dev_sp.cpu().numpy(), fake_sp)
  rr, rc = spike_metrics.batch_statistics(d['spikes'])
  fr, fc = spike_metrics.batch_statistics(fake_sp)
  want = cdm.report(rr.T, fr.T, rc.T, fc.T)
  np.testing.assert_allclose(
      [got['spike_metrics/firing_rate_mae'], got['spike_metrics/firing_rate_rmse'],
       got['spike_metrics/covariance_mae'], got['spike_metrics/covariance_mse']],
      [want['firing_rate']['mae'], want['firing_rate']['rmse'],
       want['covariance']['mae'], want['covariance']['mse']], rtol=1e-5)
  # kept real-side statistics give the same sums
  kept = gan.spike_real_statistics(d['spikes'])
  again = gan.spike_statistics(fake, real_stats=kept)
  assert all(torch.equal(out[k], again[k]) for k in out)


# -- main.py / compute_dg_metrics.py (helpers as in tests/test_main_e2e.py) -----
def _dataset(tmp_path, n=70, L=256, C=16):
  d = dg.make_dataset(num_neurons=C, sequence_length=L, num_segments=n)
  info = {k: v for k, v in d['info'].items() if k != 'rates_hz'}
  path = str(tmp_path / 'ds')
  dataset_helper.write_dataset(path, d['signals'], d['spikes'], info,
                               validation_size=6)
  return path


def _args(input_dir, output_dir, *extra):
  a = cli.build_parser().parse_args([
      '--input_dir', input_dir, '--output_dir', output_dir, '--model',
      'calciumgan', '--algorithm', 'wgan-gp', '--batch_size', '8', '--num_units',
      '8', '--m', '2', '--layer_norm', '--epochs', '2', '--save_generated',
      'last', '--verbose', '0'] + list(extra))
  a.global_step = 0
  a.surrogate_ds = False
  return a


def _scalars(path):
  return [json.loads(l) for l in open(path)]


SPIKE_TAGS = ['spike_metrics/firing_rate_mae', 'spike_metrics/firing_rate_rmse',
              'spike_metrics/covariance_mae', 'spike_metrics/covariance_mse']


def test_main_spike_metrics_flag_and_compute_dg_metrics_on_the_device(tmp_path):
  ds = _dataset(tmp_path)
  out = str(tmp_path / 'run')
  cli.main(_args(ds, out, '--spike_metrics'))
  va = _scalars(os.path.join(out, 'validation', 'scalars.jsonl'))
  for epoch in (0, 1):
    tags = [r['tag'] for r in va if r['step'] == epoch]
    for tag in SPIKE_TAGS:
      assert tags.count(tag) == 1, (epoch, tag)
  assert all(np.isfinite(r['value']) for r in va)
  with_flag = {r['tag'] for r in va}
  # without the flag: exactly today's tags
  out2 = str(tmp_path / 'run_plain')
  cli.main(_args(ds, out2))
  plain = {r['tag'] for r in _scalars(os.path.join(out2, 'validation',
                                                   'scalars.jsonl'))}
  assert plain == {'loss/generator', 'loss/discriminator',
                   'loss/gradient_penalty', 'signals_metrics/min',
                   'signals_metrics/max', 'signals_metrics/mean',
                   'signals_metrics/std', 'elapse'}
  assert with_flag == plain | set(SPIKE_TAGS)
  # the last epoch's figures are compute_dg_metrics' over the 6 validated
  # samples (the saved generated set is that epoch's fake batch)
  last = {r['tag']: r['value'] for r in va if r['step'] == 1}
  cpu = cdm.main(SimpleNamespace(output_dir=out, num_trials=6, device='cpu'))
  gpu = cdm.main(SimpleNamespace(output_dir=out, num_trials=6, device='gpu'))
  for k in ('mae', 'rmse', 'mape'):
    assert gpu['firing_rate'][k] == cpu['firing_rate'][k], k
  for k in ('mae', 'mse', 'mape'):
    np.testing.assert_allclose(gpu['covariance'][k], cpu['covariance'][k],
                               rtol=1e-5)
  np.testing.assert_allclose(
      [last[t] for t in SPIKE_TAGS],
      [cpu['firing_rate']['mae'], cpu['firing_rate']['rmse'],
       cpu['covariance']['mae'], cpu['covariance']['mse']], rtol=1e-5)
