"""Host tests of the interval figures (gan/utils/spike_metrics.py: the numpy
statement cg_spike_intervals is tested against, and interval_scores), of the C
entry points' argument checks in both precision builds, and of
compute_metrics.py --interval_metrics on the host path.  No GPU.  Counts are
compared as integers, reports as dicts."""
import json
import math

import numpy as np
import pytest

import compute_metrics as cm
import interval_cases as IC
from calciumgan_amd import _lib
from calciumgan_amd.gan.utils import spike_metrics as sm

PLAIN_KEYS = {'firing_rate_kl', 'correlation_kl', 'van_rossum_kl',
              'van_rossum_heatmap_min', 'elapse'}


# -- the statement -----------------------------------------------------------------
def _statement_is_the_loop(sp, max_isi):
  got = sm.interval_counts(sp, max_isi)
  N, T, C = np.asarray(sp).shape
  assert [x.dtype for x in got] == [np.int64] * 3
  assert [x.shape for x in got] == [(C, max_isi + 1), (C, 6), (N, C)]
  for g, w in zip(got, IC.train_loop(sp, max_isi)):
    assert np.array_equal(g, w)
  IC.identities(sp, got)
  return got


@pytest.mark.parametrize('max_isi', IC.MAX_ISIS)
@pytest.mark.parametrize('case', IC.TRAINS, ids=lambda s: 'x'.join(map(str, s)))
def test_statement_equals_the_loop_over_single_trains(case, max_isi):
  _statement_is_the_loop(IC.trains(*case), max_isi)


@pytest.mark.parametrize('max_isi', IC.MAX_ISIS)
def test_statement_on_full_empty_and_two_spike_trials(max_isi):
  T, C = 70, 3
  sp = np.zeros((4, T, C), np.float32)
  sp[0] = 1.0                     # all ones
  sp[2, 0] = sp[2, T - 1] = 1.0   # frames 0 and T - 1 only; 1 and 3 all zeros
  hist, moments, counts = _statement_is_the_loop(sp, max_isi)
  assert counts.tolist() == [[T] * C, [0] * C, [2] * C, [0] * C]
  # T - 1 intervals of one frame, and the one of T - 1 frames
  at = min(T - 1, max_isi + 1) - 1
  want = np.zeros(max_isi + 1, np.int64)
  want[0] += T - 1
  want[at] += 1
  assert (hist == want).all()
  assert moments[0].tolist() == [T + 2, T, 2 * (T - 1),
                                 (T - 1) + (T - 1) ** 2, T - 2, T - 2]
  # intervals never run from one trial into the next: trial by trial
  parts = [sm.interval_counts(sp[n:n + 1], max_isi) for n in range(4)]
  assert np.array_equal(hist, sum(p[0] for p in parts))
  assert np.array_equal(moments, sum(p[1] for p in parts))


def test_statement_nan_minus_zero_and_refused_arguments():
  sp = np.zeros((1, 24, 3), np.float32)
  sp[0, 1, 0] = np.nan
  sp[0, 5, 0] = 2.0
  sp[0, 2, 1] = -0.0
  sp[0, 13, 1] = -3.5
  hist, moments, counts = _statement_is_the_loop(sp, 24)
  assert counts.tolist() == [[2, 1, 0]]
  assert moments[:, :3].tolist() == [[2, 1, 4], [1, 0, 0], [0, 0, 0]]
  assert hist[0, 3] == 1 and hist.sum() == 1
  for bad in (0, -1, 4096):
    with pytest.raises(ValueError):
      sm.interval_counts(sp, bad)
  with pytest.raises(ValueError):
    sm.interval_counts(np.ones((11, 3), np.float32))


# -- what the figures see ---------------------------------------------------------
def _scores(ref, floor, generated):
  ref = IC.side(ref)
  out = (sm.interval_scores(ref, IC.side(floor)),
         sm.interval_scores(ref, IC.side(generated)))
  print('floor    ', out[0])
  print('generator', out[1])
  json.dumps(out)
  return out


def test_regular_trains_against_bernoulli_trains_of_the_same_rate():
  """60 trials x 2048 frames x 8 neurons a side (interval_cases).  The truth:
  gamma-renewal trains of shape 4 (CV 0.5 in theory, 0.494 once discretised;
  Fano 0.267 against the 0.25 of long trials); `floor` a second draw of it,
  `generator` Bernoulli trains of the same rate (CV sqrt(1 - p) = 0.987, Fano
  0.967).  Measured here with these seeds: cv_mae floor 0.0086, generator
  0.494; fano_mae 0.043 against 0.700; isi_js_bits 0.015 against 0.167; the
  mean intervals 0.65 frames apart."""
  floor, gen = _scores(IC.gamma_trains(1), IC.gamma_trains(2),
                       IC.bernoulli_trains(3))
  assert gen['isi_mean_mae'] < 1.5           # the same rate
  assert floor['cv_mae'] < 0.1
  assert gen['cv_mae'] > 0.3
  assert abs(gen['cv_mean'][0] - 0.5) < 0.03
  assert abs(gen['cv_mean'][1] - math.sqrt(1 - 1 / 39.5)) < 0.03
  assert floor['fano_mean'][0] < 0.35 and gen['fano_mean'][1] > 0.8
  assert gen['fano_mae'] > 3 * floor['fano_mae']


def test_alternating_intervals_against_the_same_intervals_shuffled():
  """The truth: short (5 .. 14) and long (60 .. 99 frames) intervals in turn;
  `generator` the same intervals of every train in a random order, so the same
  rate, histogram and CV.  Measured here with these seeds:
  serial_correlation_mae floor 0.0015, generator 0.879 (means -0.900 against
  -0.021); cv_mae 0.0005 against 0.0012 (CV 0.821 on every side); isi_js_bits
  0.0064 against 0.0064."""
  floor, gen = _scores(IC.alternating_trains(1), IC.alternating_trains(2),
                       IC.alternating_trains(3, shuffled=True))
  assert floor['serial_correlation_mae'] < 0.1
  assert gen['serial_correlation_mae'] > 0.5
  assert gen['cv_mae'] < 0.05
  assert gen['isi_js_bits'] < 2 * floor['isi_js_bits']


def test_a_gain_per_trial_against_trains_without_one():
  """The truth: Bernoulli trains; `generator` the same with a log-normal gain
  (sigma 0.5, mean 1) per trial shared by its neurons.  Measured here with these
  seeds: fano_mae floor 0.117, generator 14.7 (Fano 0.98 against 15.7);
  count_correlation_mae 0.163 against 0.937."""
  floor, gen = _scores(IC.bernoulli_trains(1), IC.bernoulli_trains(2),
                       IC.bernoulli_trains(3, gain_sigma=0.5))
  assert gen['fano_mae'] >= 3 * floor['fano_mae']
  assert gen['count_correlation_mae'] >= 3 * floor['count_correlation_mae']


# -- the scores -------------------------------------------------------------------
def test_scores_of_a_side_against_itself():
  a = IC.side(IC.gamma_trains(5, shape=(12, 600, 6)))
  s = sm.interval_scores(a, a)
  for key in ('isi_js_bits', 'isi_js_bits_pooled', 'isi_mean_mae', 'cv_mae',
              'serial_correlation_mae', 'fano_mae', 'count_correlation_mae'):
    assert s[key] == 0.0, key
  for key in ('cv_correlation', 'fano_correlation',
              'count_correlation_correlation'):
    assert s[key] == 1.0, key
  for key in ('cv_mean', 'serial_correlation_mean', 'adjacent_fraction',
              'overflow_fraction', 'fano_mean', 'silent_trains', 'num_trials',
              'num_intervals'):
    assert s[key][0] == s[key][1], key
  assert s['num_trials'] == [12, 12] and s['max_isi'] == 240
  assert s['num_intervals'][0] == int(a[1][:, 1].sum()) > 0
  # the definitions, neuron 0
  hist, m, counts = a
  mu = m[0, 2] / m[0, 1]
  var = m[0, 3] / m[0, 1] - mu * mu
  side = sm._interval_side(a)
  assert side['cv'][0] == math.sqrt(var) / mu
  assert side['rho'][0] == (m[0, 5] / m[0, 4] - mu * mu) / var
  assert side['fano'][0] == np.var(counts[:, 0], ddof=1) / np.mean(counts[:, 0])
  assert abs(side['r'][0, 1] - np.corrcoef(counts[:, 0], counts[:, 1])[0, 1]
             ) < 1e-12


def test_scores_nan_rules_and_mismatched_sides():
  # neuron 0 silent, 1: one spike a trial (no interval), 2: two spikes (one
  # interval, no pair), 3: three spikes at equal intervals (sigma^2 = 0), 4 and
  # 5: irregular, counts varying across trials
  sp = np.zeros((4, 100, 6), np.uint8)
  sp[:, 10, 1] = 1
  sp[:, [10, 30], 2] = 1
  sp[:, [10, 30, 50], 3] = 1
  sp[:, [1, 3, 9, 30], 4] = 1
  sp[:, [2, 7, 8, 50, 90], 5] = 1
  sp[0, 95, 4] = sp[1, 96, 5] = sp[2, 97, 5] = 1
  a = IC.side(sp)
  s = sm.interval_scores(a, a)
  side = sm._interval_side(a)
  assert np.isnan(side['mu'][:2]).all() and side['mu'][2] == 20.0
  assert side['cv'][2] == 0.0 and side['cv'][3] == 0.0
  assert np.isnan(side['rho'][:4]).all() and not np.isnan(side['rho'][4:]).any()
  assert np.isnan(side['fano'][0]) and side['fano'][1] == 0.0
  assert s['silent_trains'] == [1 / 6, 1 / 6]
  assert s['adjacent_fraction'][0] == 4 / int(a[1][:, 1].sum())
  assert s['cv_mae'] == 0.0 and s['serial_correlation_mae'] == 0.0
  # one pair of neurons varies: a mean absolute error, no correlation
  assert s['count_correlation_mae'] == 0.0
  assert math.isnan(s['count_correlation_correlation'])
  # nothing but silent neurons, or single spikes: every interval figure is NaN
  for quiet in (sp[:, :, :1], sp[:, :, :2]):
    q = IC.side(quiet)
    s0 = sm.interval_scores(q, q)
    for key in ('isi_js_bits', 'isi_js_bits_pooled', 'isi_mean_mae', 'cv_mae',
                'cv_correlation', 'serial_correlation_mae', 'fano_correlation',
                'count_correlation_mae', 'count_correlation_correlation'):
      assert math.isnan(s0[key]), key
    for key in ('cv_mean', 'serial_correlation_mean', 'adjacent_fraction',
                'overflow_fraction'):
      assert all(math.isnan(v) for v in s0[key]), key
    assert s0['num_intervals'] == [0, 0]
  assert math.isnan(sm.interval_scores(IC.side(sp[:, :, :1]),
                                       IC.side(sp[:, :, :1]))['fano_mae'])
  # one interval a neuron: a mean but no CV
  s2 = sm.interval_scores(IC.side(sp[:1, :, 2:3].repeat(2, 0)),
                          IC.side(sp[:2, :, 2:3]))
  assert s2['isi_mean_mae'] == 0.0 and s2['cv_mae'] == 0.0
  one = np.zeros((2, 100, 1), np.uint8)
  one[0, [10, 30], 0] = 1
  s1 = sm.interval_scores(IC.side(one), IC.side(one))
  assert s1['isi_mean_mae'] == 0.0 and math.isnan(s1['cv_mae'])
  # mismatched sides
  with pytest.raises(ValueError):
    sm.interval_scores(a, IC.side(sp[:, :, :5]))          # another C
  with pytest.raises(ValueError):
    sm.interval_scores(a, IC.side(sp, max_isi=24))        # another max_isi
  with pytest.raises(ValueError):
    sm.interval_scores(a, IC.side(sp[:1]))                # one trial


# -- the C entry points --------------------------------------------------------------
def test_the_header_holds_the_prototypes_and_abi_20():
  assert _lib.CG_ABI_VERSION == 20
  c = _lib.CONSTANTS
  assert c['CG_INTERVAL_MAX_C'] == sm.INTERVAL_MAX_NEURONS == 4096
  assert c['CG_INTERVAL_MAX_ISI'] == sm.INTERVAL_MAX_ISI == 4095
  assert len(_lib.SIGNATURES['cg_spike_intervals_ws_bytes']) == 4
  argtypes = _lib.SIGNATURES['cg_spike_intervals']
  assert len(argtypes) == 11
  assert [argtypes[i].ctype for i in (0, 6, 7, 8, 9)] == [
      'void*', 'int*', 'long long*', 'int*', 'void*']
  from calciumgan_amd import build
  assert 'spike_intervals.hip' in build.SOURCES


@pytest.mark.parametrize('precision', ['bf16', 'f16'])
def test_refused_arguments_return_einval_before_anything_touches_hip(precision):
  """The checks come before the first HIP call, so they run without a device:
  the pointers are never followed."""
  lib = _lib.load(precision)
  assert lib.cg_abi_version() == 20
  P = 1 << 20   # a 16-byte aligned address nobody reads

  def count(w=P, C=102, trials=10, wpt=64, stride=None, max_isi=240,
            hist=P + 64, moments=P + 128, counts=P + 256, ws=P + 512):
    return lib.cg_spike_intervals(
        w, C, trials, wpt, trials * wpt if stride is None else stride, max_isi,
        hist, moments, counts, ws, None)

  ws = lib.cg_spike_intervals_ws_bytes
  shapes = (dict(C=0), dict(C=-1), dict(C=4097), dict(trials=0),
            dict(trials=-3), dict(wpt=0), dict(wpt=-1), dict(max_isi=0),
            dict(max_isi=4096), dict(max_isi=-1),
            dict(trials=1 << 13, wpt=1 << 13),        # 2^26 words
            dict(trials=1 << 26, wpt=1), dict(trials=1, wpt=1 << 26),
            dict(trials=1 << 20, wpt=1 << 20))        # past 2^31
  for kw in shapes:
    shape = dict(C=102, trials=10, wpt=64, max_isi=240)
    shape.update(kw)
    assert ws(shape['C'], shape['trials'], shape['wpt'],
              shape['max_isi']) == -1, kw
    assert count(stride=1 << 45, **kw) == _lib.CG_EINVAL, kw
  for kw in (dict(w=None), dict(ws=None), dict(hist=None), dict(moments=None),
             dict(counts=None), dict(w=P + 8), dict(ws=P + 520),
             dict(hist=P + 66), dict(counts=P + 257), dict(moments=P + 132),
             dict(stride=639), dict(stride=0), dict(stride=-640)):
    assert count(**kw) == _lib.CG_EINVAL, kw
  # admitted shapes: at least 16 bytes; one split where there is one trial, the
  # partial histograms and moments of every split otherwise
  assert ws(1, 1, 1, 1) == ws(4096, 1, 1, 4095) == ws(102, 1, 64, 240) == 16
  for C, trials, wpt, max_isi in ((102, 500, 64, 240), (512, 500, 256, 240),
                                  (1, (1 << 26) - 1, 1, 4095),
                                  (4096, 1, (1 << 26) - 1, 1), IC.SPLIT_CASE +
                                  (240,)):
    assert ws(C, trials, wpt, max_isi) >= 16, (C, trials, wpt, max_isi)
  C, trials, wpt = IC.SPLIT_CASE
  assert ws(C, trials, wpt, 240) > ws(C, 1, wpt, 240)
  # 64 splits of 63 trials: 241 int32 and 6 int64 a neuron and split
  assert ws(C, trials, wpt, 240) == 64 * 3 * (241 * 4 + 6 * 8)


# -- compute_metrics.py ------------------------------------------------------------
def _args(path, *more):
  return ['--output_dir', str(path), '--num_processors', '1', '--verbose', '0',
          '--device', 'cpu'] + list(more)


def test_compute_metrics_interval_flag_on_the_host(tmp_path, capsys):
  fake, real_spikes, fake_spikes = IC.run_dir(tmp_path)
  plain = cm.build_parser().parse_args(_args(tmp_path))
  for name in ('interval_metrics', 'max_isi'):
    assert not hasattr(plain, name)
  before = cm.main(plain)[0]
  assert set(before) == PLAIN_KEYS
  assert 'intervals' not in json.load(open(tmp_path / 'spike_metrics.json'))['0']
  hp = cm.build_parser().parse_args(_args(tmp_path, '--interval_metrics'))
  assert hp.interval_metrics is True
  report = cm.main(hp)[0]
  assert set(report) == PLAIN_KEYS | {'intervals'}

  def rest(r):
    return json.dumps({k: v for k, v in r.items()
                       if k not in ('intervals', 'elapse')}, sort_keys=True)

  assert rest(report) == rest(before)
  s = report['intervals']
  assert set(s) == {'generated', 'floor', 'max_isi'}
  assert s['max_isi'] == 240
  assert IC.same(s, IC.expected_report(real_spikes, fake_spikes))
  assert s['floor']['num_trials'] == s['generated']['num_trials'] == [12, 12]
  assert s['floor']['num_intervals'][0] > 1000
  assert not IC.same(s['generated'], s['floor'])
  assert IC.same(json.load(open(tmp_path / 'spike_metrics.json'))['0']['intervals'],
                 s)
  # the recorded side is kept on hparams for the next epoch
  ref, floor, frames = hp._recorded_intervals
  assert ref[2].shape == (12, 7) and frames == 480
  assert IC.same(floor, s['floor'])
  # --max_isi is honoured
  hp2 = cm.build_parser().parse_args(
      _args(tmp_path, '--interval_metrics', '--max_isi', '5'))
  s2 = cm.main(hp2)[0]['intervals']
  assert IC.same(s2, IC.expected_report(real_spikes, fake_spikes, max_isi=5))
  assert s2['max_isi'] == s2['floor']['max_isi'] == 5
  assert s2['floor']['overflow_fraction'][0] > s['floor']['overflow_fraction'][0]
  # verbose: three figures beside their floor
  hp3 = cm.build_parser().parse_args(_args(tmp_path, '--interval_metrics'))
  hp3.verbose = 1
  capsys.readouterr()
  cm.main(hp3)
  out = capsys.readouterr().out
  for key in ('cv_mae', 'isi_js_bits', 'fano_mae'):
    assert 'interval {:<12}  gen | floor: {:.06f} | {:.06f}'.format(
        key, s['generated'][key], s['floor'][key]) in out
  # a generated file of another length is refused, as the other reports do
  hp._recorded_intervals = (ref, floor, 256)
  with pytest.raises(ValueError, match='480 frames'):
    cm.interval_report(hp, fake, cm.interval_sets_host)
  with pytest.raises(ValueError):
    cm.main(cm.build_parser().parse_args(
        _args(tmp_path, '--interval_metrics', '--max_isi', '4096')))


def test_compute_metrics_takes_few_neurons_and_refuses_one_trial_a_side(tmp_path):
  # two neurons, which cg_binary_words would refuse (the rest of the report
  # needs a pair of neurons; the interval figures take one)
  fake, real_spikes, fake_spikes = IC.run_dir(tmp_path / 'a', trials=6, C=2)
  hp = cm.build_parser().parse_args(_args(tmp_path / 'a', '--interval_metrics'))
  s = cm.main(hp)[0]['intervals']
  assert s['floor']['num_trials'] == [3, 3]
  assert IC.same(s, IC.expected_report(real_spikes, fake_spikes))
  one = cm.interval_sets_host(hp, real_spikes[:, :, :1])
  assert one[0].shape == (1, 241) and one[2].shape == (6, 1)
  assert sm.interval_scores(one, one)['isi_js_bits'] == 0.0
  IC.run_dir(tmp_path / 'b', trials=3, C=2)
  with pytest.raises(ValueError, match='two trials'):
    cm.main(cm.build_parser().parse_args(
        _args(tmp_path / 'b', '--interval_metrics')))
