"""Host tests of the trace power spectrum (gan/utils/signals_metrics.py: the numpy
statement cg_trace_psd is tested against, and spectral_scores), of the C
header's new prototypes, and of compute_metrics.py --spectral_metrics on the
host path.  No GPU.

The tone identity: a unit cosine at bin k0 (2 <= k0 <= T / 2 - 2) under the
periodic Hann window has |X|^2 = T^2 / 16 at k0, T^2 / 64 at k0 +- 1 and nothing
elsewhere.  Wholly in float64 (trace_psd_cases.float64_totals of a float64
cosine) that holds to 1e-12 relative and 1e-24 T^2 elsewhere.  The statement
itself rounds the cosine, x - m and the product to float32: with u = 2^-24 every
y_t is within 3 u |y_t| of the exact one, so every X_k is within 3 u T of its
exact value -- 9 u^2 T^2 = 3.2e-14 T^2 where the exact bin is empty (measured:
5e-17 T^2), 25 u relative at the peak (|X| = T / 4) and 50 u beside it."""
import json
import os
import re

import numpy as np
import pytest

import compute_metrics as cm
import trace_psd_cases as PC
from calciumgan_amd import _lib
from calciumgan_amd.gan.utils import signals_metrics as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
PLAIN_KEYS = {'firing_rate_kl', 'correlation_kl', 'van_rossum_kl',
              'van_rossum_heatmap_min', 'elapse'}


def _tone(T, k0, dtype):
  return np.cos(2 * np.pi * k0 * np.arange(T) / T).astype(dtype)[None, :, None]


@pytest.mark.parametrize('T', [32, 2048])
def test_the_tone_identity(T):
  for k0 in (2, T // 4 + 1, T // 2 - 2):
    rest = np.ones(T // 2 + 1, bool)
    rest[k0 - 1:k0 + 2] = False
    exact = PC.float64_totals(_tone(T, k0, np.float64))[:, 0]
    assert abs(exact[k0] - T * T / 16.0) <= 1e-12 * T * T / 16.0
    for side in (k0 - 1, k0 + 1):
      assert abs(exact[side] - T * T / 64.0) <= 1e-12 * T * T / 64.0
    assert exact[rest].max() < 1e-24 * T * T
    P = sm.trace_power_spectrum(_tone(T, k0, np.float32))[:, 0]
    print(T, k0, P[k0] * 16 / T ** 2 - 1, P[k0 - 1] * 64 / T ** 2 - 1,
          P[rest].max() / T ** 2)
    assert abs(P[k0] - T * T / 16.0) <= 25 * U * T * T / 16.0
    for side in (k0 - 1, k0 + 1):
      assert abs(P[side] - T * T / 64.0) <= 50 * U * T * T / 64.0
    assert P[rest].max() <= 9 * U * U * T * T


def test_hann_window():
  for T in (32, 480, 2048):
    w = sm.hann_window(T)
    assert w.dtype == np.float32 and w.shape == (T,)
    assert w[0] == 0 and w[T // 2] == 1 and w[T // 4] == 0.5
    assert np.array_equal(w[1:], w[1:][::-1])
    want = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(T) / T)
    assert np.abs(w - want).max() <= U
    # sum of squares: 3 T / 8, the normalisation of spectral_scores
    assert abs((w.astype(np.float64) ** 2).sum() - 3 * T / 8) <= 1e-6 * T


def test_parseval_on_the_two_sided_sum():
  x = PC.case('t256_c5_normal')[0]
  T = x.shape[1]
  P = sm.trace_power_spectrum(x)
  two_sided = P[0] + 2 * P[1:T // 2].sum(axis=0) + P[T // 2]
  y = sm._windowed(x, sm.hann_window(T)).astype(np.float64)
  energy = T * (y * y).sum(axis=(0, 1))
  assert (np.abs(two_sided - energy) <= 1e-12 * energy).all()
  # white noise of variance 1: S ~ 1
  S = P / (x.shape[0] * 3 * T / 8)
  assert 0.7 < S[1:].mean() < 1.3


def test_a_constant_trace_gives_exactly_zero_totals():
  x = np.array(PC.case('t256_c5_normal')[0])
  x[:, :, 1] = 3.25
  x[:, :, 3] = -1e30
  for single in (False, True):
    P = sm.trace_power_spectrum(x, single_precision=single)
    assert not P[:, [1, 3]].any() and P[:, [0, 2, 4]].all()
  assert not PC.float64_totals(x)[:, [1, 3]].any()


def test_a_nan_gives_nan_in_that_column_only():
  clean = np.array(PC.case('t64_c3_three_chunks')[0])
  dirty = clean.copy()
  dirty[0, 5, 1] = np.nan
  dirty[8, 63, 1] = np.inf
  for single in (False, True):
    P = sm.trace_power_spectrum(dirty, single_precision=single)
    want = sm.trace_power_spectrum(clean, single_precision=single)
    assert np.isnan(P[:, 1]).all()
    assert P[:, [0, 2]].tobytes() == want[:, [0, 2]].tobytes()
  totals, n = sm.spectral_totals(dirty)
  assert n == 9 and np.isnan(totals[:, 1]).all()
  # the scores leave that neuron out
  s = sm.spectral_scores((totals, n), sm.spectral_totals(clean), 64)
  assert np.isfinite(s['log_spectral_distance_db'])
  assert s['log_spectral_distance_db'] == 0 and s['bins_excluded'] == 0


def test_single_precision_is_the_yardstick_not_the_statement():
  for name in ('t32_c1_dg', 't256_c5_normal', 't2048_c9_dg'):
    x = PC.case(name)[0]
    e64 = PC.e1(sm.trace_power_spectrum(x), PC.reference(name))
    e32 = PC.single_precision_e1(name)
    print(name, e64.max(), e32.max(), PC.derived_bound(x).min())
    assert 0 < e32.max() < 1e-6 and e64.max() < 1e-6
    PC.check_accuracy(sm.trace_power_spectrum(x), name, what='numpy')
    PC.check_accuracy(sm.trace_power_spectrum(x, single_precision=True), name,
                      what='single')


def test_the_case_table_reaches_every_path():
  shapes = {n: PC.case(n)[0].shape for n in PC.CASES}
  assert PC.plan(*shapes['t64_c3_three_chunks']) == (1, 4, 3)
  groups, _, chunks = PC.plan(*shapes['t32_c32769_grid_stride'])
  assert groups * chunks > PC.MAX_GRID
  assert PC.plan(128, 2048, 102) == (13, 4, 32)
  # every accepted length: every G, and for each a ragged last group (2 G + 1
  # neurons: a second group of one neuron whose partner is absent)
  Ts = {s[1] for s in shapes.values()}
  assert Ts == {32, 64, 128, 256, 512, 1024, 2048, 4096, 8192}
  assert {PC.group(T) for T in Ts} == {16, 8, 4, 2, 1}
  for G in (16, 8, 4, 2, 1):
    assert any(PC.group(s[1]) == G and s[2] == 2 * G + 1
               for s in shapes.values()), G
  for T in (128, 512, 1024, 4096):
    assert any(s[1] == T and s[2] % (2 * PC.group(T)) for s in shapes.values()), T
    assert 't%d_tones' % T in shapes
  assert shapes['t4096_c1_dg'][1:] == (4096, 1)
  # the walk of the items: renumbered when the grid (the item count, below the
  # cap) is a multiple of 8, as they come otherwise, grid-stride past the cap
  items = {n: PC.items(n) for n in PC.CASES}
  assert items['t1024_c128_renumbered'] == 8
  assert any(i % 8 == 0 and i < PC.MAX_GRID for i in items.values())
  assert any(i % 8 and i < PC.MAX_GRID for i in items.values())
  # the chunk plan at its cap of 64 chunks and past it (chunks of 5), each with
  # a last chunk of one trial
  assert PC.plan(*shapes['t32_c3_64_chunks']) == (1, 4, 64)
  assert shapes['t32_c3_64_chunks'][0] - 63 * 4 == 1
  assert PC.plan(*shapes['t32_c3_chunks_of_5']) == (1, 5, 61)
  assert shapes['t32_c3_chunks_of_5'][0] - 60 * 5 == 1
  assert PC.MAX_CHUNKS == 64
  src = open(os.path.join(ROOT, 'calciumgan_amd', 'csrc', 'trace_psd.hip')).read()
  for text in ('kPsdMaxGrid = %d;' % PC.MAX_GRID, 'kPsdMaxChunks = %d;' %
               PC.MAX_CHUNKS, 'kPsdMinChunk = %d;' % PC.MIN_CHUNK,
               'kPsdTargetItems = %d;' % PC.TARGET_ITEMS):
    assert text in src, text
  # bar (b) is left out only where trace_psd_cases' docstring says why: of the
  # device's totals on the tones at 8192, of the numpy statement's at 512 and
  # 1024
  assert PC.BAR_A_ONLY == {'t512_tones': {'numpy'}, 't1024_tones': {'numpy'},
                           't8192_tones': {'device'}}


def test_the_statement_on_every_tones_case():
  """The module's numpy statement (float32 y, float64 transform) under bar (a)
  on every tones case, and under bar (b) wherever the table holds it to both."""
  for name in PC.CASES:
    if name.endswith('_tones'):
      PC.check_accuracy(sm.trace_power_spectrum(PC.case(name)[0]), name,
                        what='numpy')


# -- spectral_scores -----------------------------------------------------------
DB = 20 * np.log10(2.0)


def _dg_totals(T=256, C=5, B=6, seed=3):
  x = PC._dg(B, T, C, seed)
  return x, sm.spectral_totals(x)


def test_identical_sides_score_zero():
  _, t = _dg_totals()
  s = sm.spectral_scores(t, t, 256)
  assert s['log_spectral_distance_db'] == 0 and s['log_spectral_rmse_db'] == 0
  assert s['bins_excluded'] == 0 and s['total_power_ratio_db'] == 0
  assert s['band_power_ratio_db'] == [0, 0, 0, 0]
  assert s['stride_peak_db']['recorded'] == s['stride_peak_db']['generated']
  assert len(s['stride_peak_db']['recorded']) == 5   # 256 / 32 = 8
  assert s['spectral_centroid_hz'][0] == s['spectral_centroid_hz'][1]
  assert 0 < s['spectral_centroid_hz'][0] < 12.0
  assert s['num_trials'] == [6, 6] and s['frame_rate'] == 24.0
  json.dumps(s)
  # a shorter trace has fewer periods to look at: T / h >= 8
  x = PC._dg(3, 64, 2, 4)
  t64 = sm.spectral_totals(x)
  assert len(sm.spectral_scores(t64, t64, 64)['stride_peak_db']['recorded']) == 3


def test_one_side_scaled_by_two():
  x, t = _dg_totals()
  t2 = sm.spectral_totals(x * np.float32(2))
  s = sm.spectral_scores(t, t2, 256)
  assert abs(s['total_power_ratio_db'] - DB) <= 1e-12
  assert all(abs(b - DB) <= 1e-12 for b in s['band_power_ratio_db'])
  assert abs(s['log_spectral_distance_db'] - DB) <= 1e-12
  assert abs(s['log_spectral_rmse_db'] - DB) <= 1e-12
  assert s['bins_excluded'] == 0
  # the peaks are ratios within a side, the centroid a ratio too
  for a, b in zip(s['stride_peak_db']['recorded'],
                  s['stride_peak_db']['generated']):
    assert abs(a - b) <= 1e-12
  back = sm.spectral_scores(t2, t, 256)
  assert abs(back['total_power_ratio_db'] + DB) <= 1e-12
  # the number of trials is divided out
  half = sm.spectral_totals(np.concatenate([x, x]))
  assert abs(sm.spectral_scores(t, half, 256)['total_power_ratio_db']) <= 1e-12


def test_an_alternating_offset_raises_the_nyquist_peak():
  """0.01 on every even frame of DG traces at T = 2048: the figure for
  transposed-convolution artefacts rises by more than 6 dB at h = 2 (measured:
  about +10 dB against about -3 dB)."""
  x = PC._dg(8, 2048, 4, 9)
  y = x.copy()
  y[:, 0::2] += np.float32(0.01)
  s = sm.spectral_scores(sm.spectral_totals(x), sm.spectral_totals(y), 2048)
  rec, gen = s['stride_peak_db']['recorded'], s['stride_peak_db']['generated']
  print('stride_peak_db', rec, gen)
  assert len(rec) == len(gen) == 5
  assert gen[0] > rec[0] + 6
  assert all(abs(a - b) < 1 for a, b in zip(rec[1:], gen[1:]))
  assert s['bins_excluded'] == 0


def test_scores_refuse_mismatched_totals_and_leave_dead_neurons_out():
  _, t = _dg_totals()
  with pytest.raises(ValueError):
    sm.spectral_scores(t, t, 128)
  with pytest.raises(ValueError):
    sm.spectral_scores(t, (t[0][:, :3], 6), 256)
  with pytest.raises(ValueError):
    sm.spectral_scores(t, (t[0], 0), 256)
  dead = (np.zeros_like(t[0]), 6)
  s = sm.spectral_scores(t, dead, 256)
  assert np.isnan(s['log_spectral_distance_db'])
  assert np.isnan(s['total_power_ratio_db']) and s['bins_excluded'] == 0
  one_dead = t[0].copy()
  one_dead[:, 2] = 0
  s = sm.spectral_scores(t, (one_dead, 6), 256)
  assert s['log_spectral_distance_db'] == 0
  # a bin 1e-13 of the neuron's mean level is left out and counted
  low = t[0].copy()
  low[7, 1] = 1e-13 * low[1:, 1].mean()
  s = sm.spectral_scores(t, (low, 6), 256)
  assert s['bins_excluded'] == 1 and s['log_spectral_distance_db'] == 0


# -- the C header ----------------------------------------------------------------
def test_the_header_holds_the_two_prototypes_and_abi_20():
  assert _lib.CG_ABI_VERSION == 20
  text = re.sub(r'\s+', ' ', open(_lib.HEADER).read())
  assert ('long long cg_trace_psd_ws_bytes(int B, int T, int C);') in text
  assert ('int cg_trace_psd(const float* x, int B, int T, int C, long long s_b, '
          'long long s_t, long long s_c, double* totals, void* ws, void* '
          'stream);') in text
  argtypes = _lib.SIGNATURES['cg_trace_psd']
  assert len(argtypes) == 10 and len(_lib.SIGNATURES['cg_trace_psd_ws_bytes']) == 3
  assert argtypes[0].ctype == 'float*' and argtypes[7].ctype == 'double*'
  assert argtypes[8].ctype == 'void*'


# -- compute_metrics.py ------------------------------------------------------------
def test_compute_metrics_spectral_flag_on_the_host(tmp_path):
  T = 512
  fake, sig, gen = PC.run_dir(tmp_path, T=T)
  args = ['--output_dir', str(tmp_path), '--num_processors', '1', '--verbose',
          '0', '--device', 'cpu']
  plain = cm.build_parser().parse_args(args)
  assert not hasattr(plain, 'spectral_metrics')
  assert set(cm.main(plain)[0]) == PLAIN_KEYS
  hp = cm.build_parser().parse_args(args + ['--spectral_metrics'])
  assert hp.spectral_metrics is True
  report = cm.main(hp)[0]
  assert set(report) == PLAIN_KEYS | {'spectral'}
  s = report['spectral']
  assert s == sm.spectral_scores(sm.spectral_totals(sig), sm.spectral_totals(gen),
                                 T)
  assert s['num_trials'] == [12, 12] and s['bins_excluded'] == 0
  assert np.isfinite(s['log_spectral_distance_db'])
  assert s['stride_peak_db']['generated'][0] > s['stride_peak_db']['recorded'][0]
  on_disk = json.load(open(tmp_path / 'spike_metrics.json'))
  assert on_disk['0']['spectral'] == s
  # the recorded side's totals are kept on hparams for the next epoch
  assert hp._recorded_spectral_totals[1] == T
  assert hp._recorded_spectral_totals[0][1] == 12
  # a generated file of another length is refused, as --temporal_metrics does
  hp2 = cm.build_parser().parse_args(args + ['--spectral_metrics'])
  hp2.validation_cache = hp.validation_cache

  def totals(hparams, filename):
    T_file = 256 if filename == fake else T
    return (np.ones((T_file // 2 + 1, 6)), 12), T_file

  with pytest.raises(ValueError, match='256 frames'):
    cm.spectral_report(hp2, fake, totals)
