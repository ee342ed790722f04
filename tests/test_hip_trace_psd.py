"""GPU tests of cg_trace_psd (csrc/trace_psd.hip: per-neuron periodograms of
mean-removed, Hann-windowed calcium traces summed over trials; two neurons
packed into one complex transform, float64 sums per lane over a chunk of trials,
an ordered second launch over the chunks) on the cases of trace_psd_cases.py --
every case held to the statement wholly in float64 by the two bars of
trace_psd_cases.check_accuracy -- of its wrappers in signals_metrics, and of
compute_metrics.py --spectral_metrics on both devices.

Measured on one MI355X: profiles/trace_psd_parity.txt (the worst e1 of a case
1.5e-8 .. 2.7e-7, 0.6 .. 1.2 times that of single-precision pocketfft; 3.9
times on the pure tones at T = 2048, which pocketfft transforms to 3.9e-9) and,
for the cases of T = 128, 512, 1024 and 4096, the tones up to 8192 and the chunk
plan at its cap, profiles/fft_lengths_parity.txt (4.2e-8 .. 1.07e-7, 0.82 .. 1.04
times pocketfft's; on the tones 1.00 times up to T = 1024, 1.70 at 4096 and 10.2
at 8192, the one result held to bar (a) only)."""
import os

import numpy as np
import pytest
import torch

import compute_metrics as cm
import trace_psd_cases as PC
from calciumgan_amd import _lib
from calciumgan_amd.gan.utils import signals_metrics as sm

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 1024      # float64 elements of SENTINEL on either side of a buffer
SENTINEL = -7.0


def _view(x, layout):
  """The trials on the device in the given memory layout: a (B, T, C) view."""
  B, T, C = x.shape
  t = torch.from_numpy(np.array(x, dtype=np.float32)).to(DEV)
  if layout == 'padded':
    buf = torch.full((B, T, C + 5), float('nan'), device=DEV)
    buf[:, :, :C] = t
    view = buf[:, :, :C]
    assert view.stride() == (T * (C + 5), C + 5, 1)
    return view
  if layout == 'permuted':
    view = t.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert view.stride() == (C * T, 1, T)
    return view
  assert layout == 'contig' and t.is_contiguous()
  return t


def _guarded(n):
  buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float64,
                   device=DEV)
  return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
  return bool((buf[:GUARD] == SENTINEL).all()) and bool(
      (buf[-GUARD:] == SENTINEL).all())


def _launch(x):
  """The C entry with sentinel-filled, guarded totals and workspace; returns the
  (T / 2 + 1, C) totals on the host."""
  B, T, C = x.shape
  nbytes = _lib.load().cg_trace_psd_ws_bytes(B, T, C)
  assert nbytes == PC.plan(B, T, C)[2] * (T // 2 + 1) * C * 8
  tbuf, totals = _guarded((T // 2 + 1) * C)
  wbuf, ws = _guarded(nbytes // 8)
  _lib.call('cg_trace_psd', x, B, T, C, x.stride(0), x.stride(1), x.stride(2),
            totals, ws, _lib.stream())
  torch.cuda.synchronize()
  assert _guards_intact(tbuf) and _guards_intact(wbuf)
  # every partial element and every total is written
  assert not bool((ws == SENTINEL).any()) and not bool((totals == SENTINEL).any())
  return totals.view(T // 2 + 1, C).cpu().numpy()


def _totals(x_host, layout='contig'):
  return _launch(_view(x_host, layout))


@pytest.mark.parametrize('name', PC.CASES)
def test_against_the_float64_statement(name):
  x_host, layout = PC.case(name)
  x = _view(x_host, layout)
  got = _launch(x)
  assert np.isfinite(got).all() and (got >= 0).all()
  PC.check_accuracy(got, name)
  # two calls give the same bits, and so does the wrapper
  assert _launch(x).tobytes() == got.tobytes()
  dev = sm.trace_power_spectrum_device(x)
  assert dev.is_cuda and dev.dtype == torch.float64 and dev.is_contiguous()
  assert dev.cpu().numpy().tobytes() == got.tobytes()
  # the bars hold against the float64 reference; the module's statement (float32
  # y, float64 transform) is closer still
  PC.check_accuracy(sm.trace_power_spectrum(x_host), name, what='numpy')


@pytest.mark.parametrize('name', ['t128_c33_normal', 't512_c5_dg',
                                  't1024_c17_normal', 't4096_c5_normal'])
def test_the_f16_library_holds_the_same_kernel(name):
  """The kernel of the other precision build, at the lengths the case table
  gained: under both bars, and the bf16 build's bits."""
  x = _view(*PC.case(name))
  want = _launch(x)
  _lib.use('f16')
  try:
    got = _launch(x)
  finally:
    _lib.use('bf16')
  PC.check_accuracy(got, name, what='f16')
  assert got.tobytes() == want.tobytes()


def test_the_case_table_reaches_every_path():
  shapes = {n: PC.case(n)[0].shape for n in PC.CASES}
  assert PC.plan(*shapes['t64_c3_three_chunks'])[1:] == (4, 3)
  groups, _, chunks = PC.plan(*shapes['t32_c32769_grid_stride'])
  assert groups * chunks > PC.MAX_GRID
  assert shapes['t32_c33_normal'][2] == 2 * PC.group(32) + 1
  assert PC.group(8192) == 1 and PC.group(2048) == 4
  # every accepted length, so every geometry, each with a ragged last group
  assert {s[1] for s in shapes.values()} == {32 << i for i in range(9)}
  assert {PC.group(s[1]) for s in shapes.values()} == {16, 8, 4, 2, 1}
  for T in (32, 128, 1024, 2048, 4096, 8192):   # 2 G + 1 neurons
    assert any(s[1] == T and s[2] == 2 * PC.group(T) + 1
               for s in shapes.values()), T
  assert shapes['t512_c5_dg'][1:] == (512, 5)
  assert shapes['t4096_c1_dg'][2] == 1
  # both walks of the items under the grid cap, and the grid-stride one
  items = {n: PC.items(n) for n in PC.CASES}
  assert items['t1024_c128_renumbered'] == 8
  assert any(i % 8 for i in items.values())
  assert any(i % 8 == 0 and i < PC.MAX_GRID for i in items.values())
  # the chunk plan at its cap and past it, each with a last chunk of one trial
  assert PC.plan(*shapes['t32_c3_64_chunks']) == (1, 4, PC.MAX_CHUNKS)
  assert shapes['t32_c3_64_chunks'][0] == 63 * 4 + 1
  assert PC.plan(*shapes['t32_c3_chunks_of_5']) == (1, 5, 61)
  assert shapes['t32_c3_chunks_of_5'][0] == 60 * 5 + 1
  # bar (b) is left out only where the case table's docstring says why
  assert {n for n, w in PC.BAR_A_ONLY.items() if 'device' in w} == {
      't8192_tones'}


@pytest.mark.parametrize('T', [32, 64, 128, 512, 1024, 2048, 4096, 8192])
def test_tones_sit_at_their_own_bins(T):
  """Neuron 0 holds bins 1 and T / 2 - 1, its partner T / 4 + 1 and T / 2: each
  has its tones' power at its own bins and none at the partner's, the isolated
  bin T / 4 + 1 holds T^2 / 16 and its neighbours T^2 / 64, and every bin is
  the float64 statement's to 1e-5 of the neuron's peak."""
  name = 't%d_tones' % T
  got, P64 = _totals(PC.case(name)[0]), PC.reference(name)
  for c in range(2):
    assert np.abs(got[:, c] - P64[:, c]).max() <= 1e-5 * P64[:, c].max()
    for (_, n), k in PC.tone_bins(T).items():
      if n == c:
        assert got[k, c] >= 0.9 * T * T / 16.0, (c, k)
  # (bins no tone of the neuron is beside)
  assert got[1, 1] <= 1e-9 * T * T
  k = T // 4 + 1
  assert abs(got[k, 1] - T * T / 16.0) <= 1e-5 * T * T / 16.0
  for side in (k - 1, k + 1):
    assert abs(got[side, 1] - T * T / 64.0) <= 1e-5 * T * T / 16.0
  assert got[k, 0] <= 1e-9 * T * T


def test_a_constant_trace_gives_exact_zeros_beside_a_live_partner():
  x = np.array(PC.case('t256_c5_normal')[0])
  x[:, :, 2] = 3.25          # partner: neuron 3
  x[:, :, 4] = -1e30         # the odd leftover, pairs with zeros
  got = _totals(x)
  assert not got[:, 2].any() and not got[:, 4].any()
  assert got[:, [0, 1, 3]].all()
  assert not sm.trace_power_spectrum(x)[:, [2, 4]].any()
  PC.check_accuracy(got, 't256_c5_normal', x=x)


@pytest.mark.parametrize('name', ['t64_c3_three_chunks', 't2048_c9_dg',
                                  't1024_c17_normal'])
def test_a_nan_and_an_inf_stay_in_their_own_neuron(name):
  """Neuron 1 (partner: neuron 0) has a NaN in one trial and an Inf in another:
  it is all NaN, every neuron of another pair keeps its bits, and its partner
  holds the bits it has when those two trials of neuron 1 are constant (zeros
  are transformed in their place)."""
  clean = np.array(PC.case(name)[0])
  B, T, C = clean.shape
  dirty = clean.copy()
  dirty[0, 5, 1] = np.nan
  dirty[B - 1, T - 1, 1] = -np.inf
  blank = clean.copy()
  blank[0, :, 1] = 0.0
  blank[B - 1, :, 1] = 0.0
  got, base, ref = _totals(dirty), _totals(clean), _totals(blank)
  assert np.isnan(got[:, 1]).all()
  others = [c for c in range(C) if c not in (0, 1)]
  assert np.isfinite(got[:, [0] + others]).all()
  assert got[:, others].tobytes() == base[:, others].tobytes()
  assert got[:, 0].tobytes() == ref[:, 0].tobytes()
  PC.check_accuracy(np.delete(got, 1, axis=1), name, x=np.delete(clean, 1, axis=2))
  want = sm.trace_power_spectrum(dirty)
  assert np.isnan(want[:, 1]).all() and np.isfinite(np.delete(want, 1, 1)).all()


def test_a_nan_does_not_reach_the_next_item_of_its_workgroup():
  """1025 items on 1024 workgroups: workgroup 0 takes item 0 (neurons 0 .. 31)
  and then item 1024 (neuron 32768), and clears its bad[] flags in between.  A
  NaN in neuron 0 makes neuron 0 all NaN and nothing else: neuron 32768 -- the
  same flag slot of the same workgroup, one item later -- and every neuron of
  another pair keep the bits of the run without the NaN.  Neuron 1, packed
  into one transform with neuron 0, holds the bits it has beside a zero trace
  (zeros are transformed in the NaN trace's place), as in the test above."""
  name = 't32_c32769_grid_stride'
  clean = np.array(PC.case(name)[0])
  B, T, C = clean.shape
  groups, _, chunks = PC.plan(B, T, C)
  assert (B, chunks, groups) == (1, 1, PC.MAX_GRID + 1)
  last = C - 1
  assert last // (2 * PC.group(T)) == PC.MAX_GRID   # item 1024: workgroup 0 again
  dirty = clean.copy()
  dirty[0, 7, 0] = np.nan
  blank = clean.copy()
  blank[0, :, 0] = 0.0
  got, base, ref = _totals(dirty), _totals(clean), _totals(blank)
  assert np.isnan(got[:, 0]).all()
  assert np.isfinite(got[:, last]).all()
  assert np.isfinite(got[:, 1:]).all() and np.isfinite(base).all()
  assert got[:, 2:].tobytes() == base[:, 2:].tobytes()
  assert got[:, 1].tobytes() == ref[:, 1].tobytes()


def test_totals_in_groups_equal_the_single_call():
  x_host = PC.case('t64_c3_three_chunks')[0]
  B, T, C = x_host.shape
  x = _view(x_host, 'contig')
  one, n = sm.spectral_totals_device(x)
  assert n == B and one.dtype == torch.float64 and one.is_cuda
  assert torch.equal(one, sm.trace_power_spectrum_device(x))
  for group_bytes in (2 * T * C * 4, 1):   # five groups of two trials; of one
    part, n = sm.spectral_totals_device(x, group_bytes=group_bytes)
    assert n == B
    a, b = part.cpu().numpy(), one.cpu().numpy()
    assert (np.abs(a - b) <= 1e-12 * b).all()
  PC.check_accuracy(one.cpu().numpy(), 't64_c3_three_chunks')


def test_other_lengths_take_the_host_statement():
  x = PC._normal(2, 96, 3, 5)
  got = sm.trace_power_spectrum_device(torch.from_numpy(x).to(DEV))
  assert got.is_cuda and got.dtype == torch.float64
  assert got.cpu().numpy().tobytes() == sm.trace_power_spectrum(x).tobytes()
  t = torch.from_numpy(x).to(DEV)
  for bad in (x, torch.from_numpy(x), t.double(), t[0]):
    with pytest.raises(ValueError):
      sm.trace_power_spectrum_device(bad)


def test_refused_arguments_return_einval_and_write_nothing():
  lib = _lib.load()
  x = torch.zeros((2, 16384, 3), device=DEV)
  totals = torch.full((8193 * 3,), SENTINEL, dtype=torch.float64, device=DEV)
  ws = torch.full((8193 * 3,), SENTINEL, dtype=torch.float64, device=DEV)

  def call(x=x, totals=totals, ws=ws, B=2, T=64, C=3):
    return lib.cg_trace_psd(x, B, T, C, T * 3, 3, 1, totals, ws, _lib.stream())

  for kw in (dict(T=96), dict(T=16384), dict(T=16), dict(B=0), dict(C=0),
             dict(B=-2), dict(x=None), dict(totals=None), dict(ws=None)):
    assert call(**kw) == _lib.CG_EINVAL, kw
  unaligned = torch.zeros(64 * 3 * 40 + 8, dtype=torch.uint8, device=DEV)[4:]
  assert call(ws=unaligned.data_ptr()) == _lib.CG_EINVAL
  for shape in ((0, 64, 3), (2, 96, 3), (2, 16384, 3), (2, 64, 0)):
    assert lib.cg_trace_psd_ws_bytes(*shape) == -1
  torch.cuda.synchronize()
  assert bool((totals == SENTINEL).all()) and bool((ws == SENTINEL).all())
  assert call() == 0
  torch.cuda.synchronize()
  assert not bool((totals[:33 * 3] == SENTINEL).any())
  assert bool((totals[33 * 3:] == SENTINEL).all())


DB_FIGURES = ('log_spectral_distance_db', 'log_spectral_rmse_db',
              'total_power_ratio_db')


def _flat_db(scores):
  """Every dB figure of a spectral dict as one vector."""
  return np.array([scores[k] for k in DB_FIGURES] + scores['band_power_ratio_db']
                  + scores['stride_peak_db']['recorded']
                  + scores['stride_peak_db']['generated'], dtype=np.float64)


def test_compute_metrics_spectral_flag_on_both_devices(tmp_path):
  """The dB figures of the two devices' dicts within 4 x the distance between
  the float64 statement's and the single-precision statement's figures: the
  largest |gpu - cpu| over the figures against the largest |single - cpu|, the
  worst-against-worst form of trace_psd_cases.check_accuracy.  (Figure by
  figure the comparison is one of two signed means of rounding residuals of the
  same size: |g| <= 4 |s| for independent zero-mean g and s of equal spread
  holds with probability 1 - (2 / pi) atan(1 / 4) = 0.84, for all 17 figures at
  once with probability 0.06, whatever the kernel does.  Every figure's two
  distances are printed.)"""
  T = 512
  reports = {}
  for device in ('cpu', 'gpu'):
    os.makedirs(tmp_path / device)
    _, sig, gen = PC.run_dir(tmp_path / device, T=T)
    hp = cm.build_parser().parse_args(
        ['--output_dir', str(tmp_path / device), '--num_processors', '1',
         '--verbose', '0', '--device', device, '--batch_trials', '5',
         '--spectral_metrics'])
    reports[device] = cm.main(hp)[0]
  cpu, gpu = reports['cpu']['spectral'], reports['gpu']['spectral']
  print('spectral cpu:', cpu)
  print('spectral gpu:', gpu)
  assert set(reports['cpu']) == set(reports['gpu'])
  assert set(cpu) == set(gpu)
  assert cpu['num_trials'] == gpu['num_trials'] == [12, 12]
  assert cpu['bins_excluded'] == gpu['bins_excluded'] == 0
  n = len(sig)
  single = sm.spectral_scores(
      (sm.trace_power_spectrum(sig, single_precision=True), n),
      (sm.trace_power_spectrum(gen, single_precision=True), n), T)
  assert cpu == sm.spectral_scores(sm.spectral_totals(sig),
                                   sm.spectral_totals(gen), T)
  a, b, s = _flat_db(cpu), _flat_db(gpu), _flat_db(single)
  assert np.isfinite(a).all() and np.isfinite(b).all()
  print('|gpu - cpu| dB', np.abs(b - a), '|single - cpu| dB', np.abs(s - a))
  assert np.abs(b - a).max() <= 4 * np.abs(s - a).max()
  for x, y in zip(cpu['spectral_centroid_hz'], gpu['spectral_centroid_hz']):
    assert abs(x - y) <= 1e-5 * x
  # the artefact the generated file carries shows at the Nyquist bin
  assert (gpu['stride_peak_db']['generated'][0] >
          gpu['stride_peak_db']['recorded'][0] + 6)
  # without the flag the device report has no such key
  plain = cm.build_parser().parse_args(
      ['--output_dir', str(tmp_path / 'gpu'), '--num_processors', '1',
       '--verbose', '0', '--device', 'gpu', '--batch_trials', '5'])
  assert not hasattr(plain, 'spectral_metrics')
  assert 'spectral' not in cm.main(plain)[0]
