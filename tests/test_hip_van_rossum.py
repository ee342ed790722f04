"""GPU tests of cg_van_rossum (csrc/van_rossum.hip: van Rossum kernel sums and
distances on the float64 matrix pipe) and cg_spike_corrcoef (csrc/spikes.hip),
against their numpy statements in spike_metrics, and of compute_metrics.py
--device gpu against the host path.  Every case is one or two launches on valid
input.  Shapes are (B, T, C)."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import compute_metrics as cm
from calciumgan_amd import _lib, nets
from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import h5_helper, spike_metrics
import spike_stats_cases as SC
from van_rossum_cases import (correlation_cases, dg_batch, gram_reference,
                              random_trains)

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 2.0**-53
DECAY = spike_metrics.van_rossum_decay(1.0)
CHUNK = spike_metrics.VAN_ROSSUM_CHUNK


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _ulps(a, b):
  """Distance in units of the last place between non-negative float64 arrays."""
  assert np.all(a >= 0) and np.all(b >= 0)
  return np.abs(_bits(a + 0.0) - _bits(b + 0.0))


def _call(x, decay, gram=True, dist=True):
  """cg_van_rossum on a (B, T, C) device tensor read in place -> numpy (gram,
  dist), None for an output not asked for."""
  B, T, C = x.shape
  g = torch.empty(B, C, C, dtype=torch.float64, device=x.device) if gram else None
  d = torch.empty(B, C, C, dtype=torch.float64, device=x.device) if dist else None
  _lib.call('cg_van_rossum', nets._p(x), B, T, C, x.stride(0), x.stride(1),
            x.stride(2), decay, nets._p(g), nets._p(d), nets._stream())
  torch.cuda.synchronize()
  return (g.cpu().numpy() if gram else None, d.cpu().numpy() if dist else None)


def _distance_from(S):
  """sqrt(max(fl(fl(S_ii + S_jj) - 2 S_ij), 0)) of a batch of matrices."""
  d = np.einsum('bii->bi', S)
  return np.sqrt(np.maximum((d[:, :, None] + d[:, None, :]) - 2.0 * S, 0.0))


def _check_distances(S, D):
  """`dist` against the device's own `gram`: 1 ulp, symmetric bit for bit,
  diagonal exactly 0."""
  assert _ulps(D, _distance_from(S)).max() <= 1
  assert np.array_equal(_bits(D), _bits(D.transpose(0, 2, 1)))
  assert np.array_equal(_bits(S), _bits(S.transpose(0, 2, 1)))
  assert np.all(np.einsum('bii->bi', D) == 0)


def _trials(B, T, C, seed, density=0.3):
  return (np.random.RandomState(seed).uniform(size=(B, T, C)) < density
          ).astype(np.float32)


@pytest.mark.parametrize('shape', [(3, 480, 6), (2, 13, 17), (1, 1, 1),
                                   (1, 2053, 90), (1, 64, 130), (1, 96, 512)])
def test_exact_decays(shape):
  """decay 1: S = n n^T and D = |n_i - n_j|; decay 0: the coincidence counts
  and D = sqrt of an exact integer.  Every product and sum is an integer or a
  half-integer: gram is exact whatever order the matrix pipe adds in."""
  B, T, C = shape
  sp = _trials(B, T, C, seed=T + C)
  x = torch.from_numpy(sp).to(DEV)
  s64 = sp.astype(np.float64)
  n = s64.sum(1)                                    # (B, C)
  S, D = _call(x, 1.0)
  assert np.array_equal(_bits(S), _bits(n[:, :, None] * n[:, None, :]))
  assert _ulps(D, np.abs(n[:, :, None] - n[:, None, :])).max() <= 1
  _check_distances(S, D)
  S, D = _call(x, 0.0)
  co = np.einsum('bti,btj->bij', s64, s64)
  assert np.array_equal(_bits(S), _bits(co))
  d2 = n[:, :, None] + n[:, None, :] - 2.0 * co     # exact integers >= 0
  assert d2.min() >= 0 and _ulps(D, np.sqrt(d2)).max() <= 1
  _check_distances(S, D)


def test_decay_one_half_is_bit_equal_to_the_statement():
  sp = _trials(2, 40, 17, seed=8, density=0.4)
  S, D = _call(torch.from_numpy(sp).to(DEV), 0.5)
  want = np.stack([spike_metrics.van_rossum_gram_frames(t.T, 0.5) for t in sp])
  assert np.array_equal(_bits(S), _bits(want))
  _check_distances(S, D)


def _assert_gram(S, trials):
  """Entrywise within (2 T + 2) 2^-53 S_rec of van_rossum_gram_frames: M' holds
  the same bits on both sides, each side sums <= T non-negative exact products
  in some order and one addition joins them.  trials: (B, T, C) host trains."""
  T = trials.shape[1]
  worst = 0.0
  for b, t in enumerate(trials):
    rec = spike_metrics.van_rossum_gram_frames(t.T, DECAY)
    err, bound = np.abs(S[b] - rec), (2 * T + 2) * U * rec
    assert np.all(err <= bound), (b, float((err - bound).max()))
    if (bound > 0).any():
      worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
  print('worst fraction of the bound: %.3g' % worst)


def test_real_decay_dg_batch_in_a_pitch_128_buffer():
  sp = dg_batch(102, 2048, 2)
  buf = torch.full((2, 2048, 128), 7.0, dtype=torch.float32, device=DEV)
  buf[:, :, :102] = torch.from_numpy(sp).to(DEV)
  x = buf[:, :, :102]
  assert x.stride() == (2048 * 128, 128, 1)
  S, D = _call(x, DECAY)
  _assert_gram(S, sp)
  _check_distances(S, D)
  # the spikes counted are those of the 102 channels alone
  assert np.array_equal(_bits(np.einsum('bii->bi', _call(x, 1.0)[0])),
                        _bits(sp.astype(np.float64).sum(1)**2))


def test_real_decay_rows_array_through_strides():
  rows = random_trains(90, 2053, 0.1, seed=12)       # (rows, T)
  x = torch.from_numpy(rows).to(DEV).t().unsqueeze(0)
  assert x.shape == (1, 2053, 90) and x.stride()[1:] == (1, 2053)
  S, D = _call(x, DECAY)
  _assert_gram(S, rows.T[None])
  _check_distances(S, D)


@pytest.mark.parametrize('shape', [(3, 480, 6), (1, 96, 512)])
def test_real_decay_small_and_many_blocks(shape):
  sp = _trials(*shape, seed=sum(shape))
  S, D = _call(torch.from_numpy(sp).to(DEV), DECAY)
  _assert_gram(S, sp)
  _check_distances(S, D)


def test_real_decay_full_silent_and_identical_trains():
  sp = _trials(1, 100, 5, seed=2)
  sp[0, :, 0] = 1.0
  sp[0, :, 1] = 0.0
  sp[0, :, 3] = sp[0, :, 2]
  S, D = _call(torch.from_numpy(sp).to(DEV), DECAY)
  _assert_gram(S, sp)
  _check_distances(S, D)
  assert np.all(S[0, 1] == 0) and np.all(S[0, :, 1] == 0)
  assert D[0, 2, 3] == 0 and D[0, 3, 2] == 0
  assert np.array_equal(_bits(D[0, 2]), _bits(D[0, 3]))


def test_real_decay_single_spikes_at_the_ends_and_at_every_chunk_boundary():
  """One train per frame of interest: frame 0, frame T - 1 and the two frames on
  either side of every boundary between the kernel's LDS chunks."""
  T = 12 * CHUNK + 5
  frames = [0, T - 1]
  for edge in range(CHUNK, T, CHUNK):
    frames += [edge - 1, edge]
  sp = np.zeros((1, T, len(frames)), np.float32)
  sp[0, frames, np.arange(len(frames))] = 1.0
  S, D = _call(torch.from_numpy(sp).to(DEV), DECAY)
  _assert_gram(S, sp)
  _check_distances(S, D)
  assert np.all(np.diag(S[0]) == 1.0)               # S_ii = n_i = 1


def test_known_answers_and_either_output_alone():
  """The answers of test_van_rossum_and_victor_purpura_known_answers through the
  device; with gram = NULL the dist holds the same bits, with dist = NULL the
  gram does."""
  T = 24 * 20
  sp = np.zeros((1, T, 4), np.float32)
  sp[0, 24, 0] = 1
  sp[0, 24 + 12, 1] = 1
  sp[0, [24, 24 * 10], 2] = 1
  x = torch.from_numpy(sp).to(DEV)
  d = spike_metrics.van_rossum_distance_device(x)
  assert d.dtype == torch.float64 and d.is_cuda and tuple(d.shape) == (1, 4, 4)
  d = d.cpu().numpy()[0]
  np.testing.assert_allclose(d[0, 3], 1.0, rtol=1e-12)
  np.testing.assert_allclose(d[0, 1], np.sqrt(2 * (1 - np.exp(-0.5))), rtol=1e-12)
  np.testing.assert_allclose(d[0, 2], 1.0, rtol=1e-12)
  d2, g2 = spike_metrics.van_rossum_distance_device(x, return_gram=True)
  assert np.array_equal(_bits(d2.cpu().numpy()[0]), _bits(d))
  _check_distances(g2.cpu().numpy(), d2.cpu().numpy())
  # the cross block, sliced as the host slices it
  cross = spike_metrics.van_rossum_distance_frames(sp[0, :, :2].T, sp[0, :, 2:].T)
  assert _ulps(cross, d[2:, :2]).max() <= 1
  big = torch.from_numpy(_trials(2, 300, 37, seed=5)).to(DEV)
  S, D = _call(big, DECAY)
  only_d = _call(big, DECAY, gram=False)[1]
  only_s = _call(big, DECAY, dist=False)[0]
  assert np.array_equal(_bits(only_d), _bits(D))
  assert np.array_equal(_bits(only_s), _bits(S))


def test_two_calls_give_the_same_bits():
  x = torch.from_numpy(dg_batch(102, 2048, 2)).to(DEV)
  S1, D1 = _call(x, DECAY)
  S2, D2 = _call(x, DECAY)
  assert np.array_equal(_bits(S1), _bits(S2))
  assert np.array_equal(_bits(D1), _bits(D2))


@pytest.mark.parametrize('name', sorted(correlation_cases()))
def test_correlations(name):
  """NaN exactly where correlation_coefficients_exact has it, finite entries
  within 2 ulp of it (one division and one square root, on whose last-bit
  rounding on the device nothing is assumed) and within 4 nb 2^-53 of the host's
  correlation_coefficients."""
  sp = correlation_cases()[name]                     # (n, T)
  n, T = sp.shape
  buf = torch.full((1, T, 128), 7.0, dtype=torch.float32, device=DEV)
  buf[0, :, :n] = torch.from_numpy(sp.T.copy()).to(DEV)
  r = spike_metrics.correlation_coefficients_device(buf[:, :, :n])
  torch.cuda.synchronize()
  assert r.dtype == torch.float64 and tuple(r.shape) == (1, n, n)
  r = r.cpu().numpy()[0]
  want = spike_metrics.correlation_coefficients_exact(sp)
  assert np.array_equal(np.isnan(r), np.isnan(want))
  fin = np.isfinite(want)
  assert fin.any()
  assert np.abs(_bits(r[fin]) - _bits(want[fin])).max() <= 2
  host = spike_metrics.correlation_coefficients(sp)
  assert np.abs(r[fin] - host[fin]).max() <= 4 * (T // 12) * U
  assert np.array_equal(_bits(r), _bits(r.T))


CORR_TAIL = 64        # sentinel elements behind the correlation matrices


@pytest.mark.parametrize('name', SC.CORRCOEF_CASES)
def test_correlations_past_256_neurons_and_at_the_lds_limit(name):
  """cg_spike_corrcoef on the batches of the cg_spike_stats tests: C = 300 (the
  second trip of the loop over c += 256, 45 150 pairs on the capped grid of 8
  workgroups a trial, 61 200 B of LDS) and C = 240 at the 61 440 B that are the
  most admitted -- under the bars of test_correlations, trial by trial.  The
  output starts as NaN with a tail of -7 that must survive."""
  sp = SC.stats_case(name)                           # (2, T, C)
  B, T, C = sp.shape
  x = torch.from_numpy(sp.copy()).to(DEV)
  out = torch.full((B * C * C + CORR_TAIL,), float('nan'), dtype=torch.float64,
                   device=DEV)
  out[B * C * C:] = -7.0
  _lib.call('cg_spike_corrcoef', nets._p(x), B, T, C, x.stride(0), x.stride(1),
            x.stride(2), nets._p(out), nets._stream())
  torch.cuda.synchronize()
  out = out.cpu().numpy()
  assert np.all(out[B * C * C:] == -7.0)
  r = out[:B * C * C].reshape(B, C, C)
  for b in range(B):
    want = spike_metrics.correlation_coefficients_exact(sp[b].T)
    assert np.array_equal(np.isnan(r[b]), np.isnan(want))
    fin = np.isfinite(want)
    assert fin.any() and not fin.all()               # (neuron 0 is silent)
    assert np.abs(_bits(r[b][fin]) - _bits(want[fin])).max() <= 2
    host = spike_metrics.correlation_coefficients(sp[b].T)
    assert np.abs(r[b][fin] - host[fin]).max() <= 4 * (T // 12) * U
    assert np.array_equal(_bits(r[b]), _bits(r[b].T))
  again = spike_metrics.correlation_coefficients_device(x)
  assert np.array_equal(_bits(again.cpu().numpy()), _bits(r))


@pytest.mark.parametrize('T,C', SC.REFUSED)
def test_correlations_one_bin_past_the_lds_limit_are_refused(T, C):
  assert SC.lds_bytes(T, C) > SC.STATS_MAX_LDS >= SC.lds_bytes(T - 12, C)
  x = torch.ones(2, T, C, dtype=torch.float32, device=DEV)
  out = torch.full((2 * C * C,), -7.0, dtype=torch.float64, device=DEV)
  rc = _lib.load().cg_spike_corrcoef(nets._p(x), 2, T, C, x.stride(0),
                                     x.stride(1), x.stride(2), nets._p(out),
                                     nets._stream())
  torch.cuda.synchronize()
  assert rc == _lib.CG_EINVAL and bool((out == -7.0).all())
  with pytest.raises(ValueError):
    spike_metrics.correlation_coefficients_device(x)


def test_device_functions_refuse_host_arrays_and_too_few_bins():
  with pytest.raises(ValueError):
    spike_metrics.van_rossum_distance_device(np.zeros((2, 24, 3), np.float32))
  with pytest.raises(ValueError):
    spike_metrics.correlation_coefficients_device(np.zeros((2, 24, 3), np.float32))
  with pytest.raises(ValueError):
    spike_metrics.correlation_coefficients_device(
        torch.zeros(2, 23, 4, dtype=torch.float32, device=DEV))


# -- compute_metrics.py --device gpu ---------------------------------------------
def _run_dir(path, d):
  """The DG run directory of test_recorded_data_metrics_report."""
  gen_dir = path / 'generated'
  os.makedirs(gen_dir)
  val = str(gen_dir / 'validation.h5')
  sig = d['signals'] * (d['info']['signals_max'] - d['info']['signals_min']
                        ) + d['info']['signals_min']
  h5_helper.write(val, {'signals': sig.astype(np.float32),
                        'spikes': d['spikes'].astype(np.int8)})
  fake = str(gen_dir / 'epoch000_signals.h5')
  h5_helper.write(fake, {'signals': sig.astype(np.float32)})
  with open(gen_dir / 'info.pkl', 'wb') as f:
    pickle.dump({0: {'global_step': 1, 'filename': fake}}, f)
  json.dump(dict(generated_dir=str(gen_dir), validation_cache=val,
                 num_neurons=6, sequence_length=480),
            open(path / 'hparams.json', 'w'))
  return fake


def _distance_tolerance(trains):
  """Bound on |D_device - D_host| per pair of `trains` (n, T): the host's S =
  A E A^T is within 4 (n_i n_j + 2 T) 2^-53 S of the recursion statement
  (tests/test_van_rossum_host.py) and the device within (2 T + 2) 2^-53 S of it,
  so d2 = S_ii + S_jj - 2 S_ij differs by at most delta = eps (S_ii + S_jj + 2
  S_ij) plus two roundings of either side; and |sqrt(x) - sqrt(y)| <=
  min(sqrt|x - y|, |x - y| / sqrt(y)), plus the square roots' own rounding."""
  T = trains.shape[1]
  S = gram_reference(trains)
  n = trains.sum(1).astype(np.float64)
  eps = (4 * (n.max()**2 + 2 * T) + 2 * T + 2) * U
  dg_ = np.diag(S)
  total = dg_[:, None] + dg_[None, :]
  delta = eps * (total + 2 * S) + 4 * U * total
  D = np.sqrt(np.maximum(total - 2 * S, 0.0))
  with np.errstate(divide='ignore', invalid='ignore'):
    tol = np.minimum(np.sqrt(delta), np.where(D > 0, delta / D, np.inf))
  return tol + 4 * U * D


def test_compute_metrics_on_the_device_against_the_host_path(tmp_path):
  d = dg.make_dataset(num_neurons=6, sequence_length=480, num_segments=24)
  fakes, hps, reports = {}, {}, {}
  for device in ('cpu', 'gpu'):
    os.makedirs(tmp_path / device)
    fakes[device] = _run_dir(tmp_path / device, d)
    hps[device] = cm.build_parser().parse_args(
        ['--output_dir', str(tmp_path / device), '--num_processors', '1',
         '--verbose', '0', '--device', device, '--batch_trials', '10'])
    reports[device] = cm.main(hps[device])[0]
  cpu, gpu = reports['cpu'], reports['gpu']
  hc, hg = hps['cpu'], hps['gpu']
  assert set(cpu) == set(gpu)
  assert set(gpu) >= {'firing_rate_kl', 'correlation_kl', 'van_rossum_kl',
                      'van_rossum_heatmap_min'}
  # the trains written back are the host's byte for byte
  sc, sg = (h5_helper.get(fakes[k], 'spikes') for k in ('cpu', 'gpu'))
  assert sc.dtype == np.int8 and sg.dtype == np.int8 and sc.sum() > 0
  assert sc.tobytes() == sg.tobytes() and sc.shape == sg.shape
  pairs = cm.device_pairs(hg, fakes['gpu'])
  n, T = 6, 480
  # firing rates: the same bits in, the same float32 out
  for c in range(n):
    real, fake = cm.firing_rate(hc, fakes['cpu'], c, hc.num_samples)
    assert np.array_equal(real, pairs['firing_rate'][c][0])
    assert np.array_equal(fake, pairs['firing_rate'][c][1])
  assert cpu['firing_rate_kl'] == gpu['firing_rate_kl']
  assert len(pairs['correlation']) == hc.num_samples == 24
  for i in range(hc.num_samples):
    # correlations: NaNs removed alike, finite entries as in test_correlations
    for h, g in zip(cm.correlation_coefficient(hc, fakes['cpu'], i),
                    pairs['correlation'][i]):
      assert h.shape == g.shape and len(h) > 0
      assert np.abs(h - g).max() <= 4 * (T // 12) * U
    # van Rossum distances between the trial's neurons
    for f, h, g in zip((hc.validation_cache, fakes['cpu']),
                       cm.trial_van_rossum(hc, fakes['cpu'], i),
                       pairs['van_rossum'][i]):
      tol = _distance_tolerance(cm._spikes(hc, f, 'CW', trial=i))
      assert np.all(np.abs(h - g) <= tol[np.triu_indices(n, k=1)]), i
  # recorded x synthetic blocks of the chosen neurons, unsorted
  blocks = cm.neuron_van_rossum_blocks_device(hg, fakes['gpu'], hg.neurons, 45)
  assert blocks.shape == (len(hg.neurons), 24, 24)
  assert list(hc.neurons) == list(hg.neurons)
  for neuron, block in zip(hg.neurons, blocks):
    real = cm._spikes(hc, hc.validation_cache, 'NW', neuron=neuron, num_trials=45)
    fake = cm._spikes(hc, fakes['cpu'], 'NW', neuron=neuron, num_trials=45)
    want = spike_metrics.van_rossum_distance(real, fake)
    tol = _distance_tolerance(np.concatenate([real, fake]))[len(real):, :len(fake)]
    assert np.all(np.abs(block - want) <= tol)
    # the minimum of the float32 heatmap: the same tolerance plus the rounding
    # of either side to float32
    a = cpu['van_rossum_heatmap_min'][int(neuron)]
    b = gpu['van_rossum_heatmap_min'][int(neuron)]
    assert abs(a - b) <= tol.max() + 2.0**-23 * max(a, b)
  print('correlation KL cpu / gpu:', cpu['correlation_kl']['mean'],
        gpu['correlation_kl']['mean'], '; van Rossum KL cpu / gpu:',
        cpu['van_rossum_kl']['mean'], gpu['van_rossum_kl']['mean'])
  # identical spike sets: every KL is exactly zero on the device path
  h5_helper.overwrite(fakes['gpu'], 'spikes', d['spikes'].astype(np.int8))
  z = cm.main(hg)[0]
  assert z['firing_rate_kl']['mean'] == 0 and z['van_rossum_kl']['mean'] == 0
  assert z['correlation_kl']['mean'] == 0
