"""Host tests of the nearest-stretch figures (gan/utils/signals_metrics.py: the
numpy statement cg_nearest_stretch is tested against, its expanded form and
novelty_scores), of the C header's new prototypes and the entry's argument
checks (they come before anything touches HIP), and of compute_metrics.py
--novelty_metrics on the host path.  No GPU.

The expanded form is held to the direct form by nearest_stretch_cases.check: the
derived bar 4 K 2^-53 (|q_n|^2 + W_j), and equal bits on integer data."""
import json
import os
import re

import numpy as np
import pytest

import compute_metrics as cm
import nearest_stretch_cases as NC
from calciumgan_amd import _lib
from calciumgan_amd.gan.utils import signals_metrics as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_KEYS = {'firing_rate_kl', 'correlation_kl', 'van_rossum_kl',
              'van_rossum_heatmap_min', 'elapse'}
NOVELTY_KEYS = {'nearest_rms', 'nearest_rms_ratio', 'copied_fraction',
                'below_recorded_median', 'distinct_stretches', 'step', 'offsets',
                'num_trials', 'undefined'}


@pytest.mark.parametrize('name', NC.CASES)
def test_the_expanded_form_against_the_direct_form(name):
  c = NC.case(name)
  nearest, index, d2 = sm.nearest_stretch(
      c['Q'], c['R'], c['step'], c['exclude'], c['exclude_len'],
      return_profile=True, expanded=True)
  assert nearest.dtype == np.float64 and index.dtype == np.int64
  assert d2.dtype == np.float64 and d2.shape == (len(c['Q']), NC.plan(
      *NC.shape(name))['S'])
  worst = NC.check(d2, nearest, index, name, what='expanded')
  print(name, 'err / bar', worst)
  # without the profile: the same bits
  again = sm.nearest_stretch(c['Q'], c['R'], c['step'], c['exclude'],
                             c['exclude_len'], expanded=True)
  assert again[0].tobytes() == nearest.tobytes()
  assert again[1].tobytes() == index.tobytes()
  # the statement holds itself
  ref = NC.reference(name)
  assert NC.check(ref['d2'], ref['nearest'], ref['index'], name) == 0.0


def test_the_statement_by_hand():
  R = np.arange(24, dtype=np.float32).reshape(8, 3)
  Q = np.stack([R[2:5], R[3:6] + np.float32(1)])
  nearest, index, d2 = sm.nearest_stretch(Q, R, step=2, return_profile=True)
  # offsets 0, 2, 4 (the stretch at row 5 is the last full one: on no grid row)
  assert d2.shape == (2, 3)
  # rows differ by 3 per row of shift: 9 elements of (3 shift)^2
  assert d2[0].tolist() == [9 * 36.0, 0.0, 9 * 36.0]
  assert d2[1].tolist() == [9 * 100.0, 9 * 16.0, 9 * 4.0]
  assert nearest.tolist() == [0.0, 36.0] and index.tolist() == [1, 2]
  # every full stretch counts, the last one included
  assert sm.nearest_stretch(Q, R, step=1)[1].tolist() == [2, 3]
  assert sm.stretch_offsets(8, 3, 1) == 6 and sm.stretch_offsets(8, 3, 2) == 3
  assert sm.stretch_offsets(8, 8, 5) == 1
  # exclusion: |s_j - exclude| < exclude_len, a negative start row for none
  n, i = sm.nearest_stretch(Q, R, step=2, exclude=[2, -1], exclude_len=1)
  assert n.tolist() == [9 * 36.0, 36.0] and i.tolist() == [0, 2]
  n, i = sm.nearest_stretch(Q, R, step=2, exclude=[2, 4], exclude_len=3)
  assert np.isnan(n[0]) and i.tolist() == [-1, 0] and n[1] == 900.0
  n, i = sm.nearest_stretch(Q, R, step=2, exclude=[2, 4], exclude_len=0)
  assert n.tolist() == [0.0, 36.0] and i.tolist() == [1, 2]
  for bad in (dict(step=0), dict(exclude_len=-1), dict(exclude=[1])):
    with pytest.raises(ValueError):
      sm.nearest_stretch(Q, R, **bad)
  with pytest.raises(ValueError):
    sm.nearest_stretch(Q, R[:2])
  with pytest.raises(ValueError):
    sm.nearest_stretch(Q, R[:, :2])


@pytest.mark.parametrize('expanded', [False, True])
def test_non_finite_samples_spoil_only_their_own_entries(expanded):
  name = 'n17_s64_k15_step2'
  c = NC.case(name)
  L, step = c['Q'].shape[1], c['step']
  clean = sm.nearest_stretch(c['Q'], c['R'], step, return_profile=True,
                             expanded=expanded)
  Q, R = np.array(c['Q']), np.array(c['R'])
  Q[3, 2, 1] = np.nan
  Q[9, 0, 0] = -np.inf
  R[40, 2] = np.nan
  R[101, 0] = np.inf
  nearest, index, d2 = sm.nearest_stretch(Q, R, step, return_profile=True,
                                          expanded=expanded)
  s = np.arange(d2.shape[1]) * step
  covered = ((s <= 40) & (40 < s + L)) | ((s <= 101) & (101 < s + L))
  spoiled = np.zeros(d2.shape, bool)
  spoiled[[3, 9]] = True
  spoiled[:, covered] = True
  assert 0 < covered.sum() < 8
  assert np.isnan(d2[spoiled]).all()
  assert d2[~spoiled].tobytes() == clean[2][~spoiled].tobytes()
  assert np.isnan(nearest[[3, 9]]).all() and (index[[3, 9]] == -1).all()
  rest = [n for n in range(len(Q)) if n not in (3, 9)]
  want = np.where(spoiled, np.inf, clean[2])[rest]
  assert (index[rest] == want.argmin(axis=1)).all()
  assert nearest[rest].tobytes() == want.min(axis=1).tobytes()


def test_the_case_table_reaches_every_path():
  plans = {n: NC.plan(*NC.shape(n)) for n in NC.CASES}
  shapes = {n: NC.shape(n) for n in NC.CASES}
  assert {s[0] for s in shapes.values()} >= {1, 16, 17, 33, 130}
  assert {p['S'] for p in plans.values()} >= {1, 63, 64, 65, 257, 1025}
  assert {s[1] * s[2] for s in shapes.values()} >= {15, 16, 17, 64 * 102, 52224}
  assert {s[4] for s in shapes.values()} == {1, 2, 3, 4}
  # a T_raw - L the step does not divide, at every step above 1
  for step in (2, 3, 4):
    assert any(s[4] == step and (s[3] - s[1]) % step for s in shapes.values())
  assert plans['n130_s257_k15_step2']['tiles_n'] == 2
  assert plans['n3_s1025_k15']['segments'] == 2
  assert plans['n1_s1_k15']['splits'] == 1 and plans['n1_s1_k15']['steps'] == 1
  big = plans['n17_s257_l512_c102_step2']
  assert big['splits'] == 16 and big['split_steps'] == 204 and big['staged']
  two = plans['n17_s71_l256_c130_step2_two_chunks']
  assert (two['split_steps'], two['chunk_steps']) == (130, 128)
  six = plans['n4_s70_l8_c97_step3_chunks_of_6']
  assert six['staged'] and six['chunk_steps'] == 6 and six['splits'] == 1
  assert six['steps'] == 49
  for name in ('n4_s70_l8_c73_step4_unstaged', 'exact_unstaged',
               'n17_s47_l64_c102_step3_unstaged', 'padded_both_unstaged'):
    assert not plans[name]['staged'], name
  # a split count between the ends, and the report's shape
  assert NC.plan(1, 64, 48, 200, 1)['splits'] == 3
  cfg2 = NC.plan(128, 2048, 102, 20432, 2)
  assert (cfg2['S'], cfg2['tiles_s'], cfg2['splits']) == (9193, 144, 7)
  assert cfg2['staged'] and cfg2['chunk_steps'] == 348
  layouts = {(NC.case(n)['q_layout'], NC.case(n)['r_layout']) for n in NC.CASES}
  assert layouts >= {('contig', 'contig'), ('padded', 'contig'),
                     ('permuted', 'contig'), ('contig', 'padded'),
                     ('contig', 'permuted'), ('permuted', 'permuted'),
                     ('padded', 'padded')}
  src = open(os.path.join(ROOT, 'calciumgan_amd', 'csrc',
                          'nearest_stretch.hip')).read()
  for text in ('kNsTileN = %d;' % NC.TILE_N, 'kNsTileS = %d;' % NC.TILE_S,
               'kNsGroup = %d;' % NC.GROUP, 'kNsLdsFloats = %d;' % NC.LDS_FLOATS,
               'kNsMinChunk = %d;' % NC.MIN_CHUNK,
               'kNsMaxChunk = %d;' % NC.MAX_CHUNK,
               'kNsMaxSplits = %d;' % NC.MAX_SPLITS,
               'kNsMinSplitSteps = %d;' % NC.MIN_SPLIT_STEPS,
               'kNsUnits = %d;' % NC.UNITS, 'kNsSegment = %d;' % NC.SEGMENT):
    assert text in src, text


def test_exact_cases_hit_what_they_are_for():
  c, ref = NC.case('exact_periodic'), NC.reference('exact_periodic')
  # period 6 rows = 3 offsets: the lowest of the offsets at distance 0
  assert ref['nearest'].tolist() == [0.0] * 6
  for n in range(6):
    zeros = np.flatnonzero(ref['d2'][n] == 0)
    assert len(zeros) >= 9 and ref['index'][n] == zeros[0]
    assert ref['index'][n] == (c['starts'][n] % 6) // 2
  c = NC.case('exact_cut_from_recording')
  ref = NC.reference('exact_cut_from_recording')
  assert ref['nearest'][:4].tolist() == [0.0] * 4
  assert ref['index'][:4].tolist() == [v // 3 for v in c['starts'][:4]]
  assert (ref['nearest'][4:] > 0).all()
  ref = NC.reference('exclude_bands_at_both_ends')
  assert (ref['nearest'][:3] > 0).all()
  assert ref['nearest'][3:5].tolist() == [0.0, 0.0]
  assert ref['index'][3:5].tolist() == [0, 26]
  ref = NC.reference('exclude_leaves_one')
  assert ref['index'].tolist() == [26, 0, -1, -1, 26, -1]
  ref = NC.reference('exclude_leaves_none')
  assert ref['index'].tolist()[:3] == [-1, -1, -1]
  assert ref['index'][3] == 0 and ref['index'][4] == -1
  assert np.isnan(ref['nearest'][[0, 1, 2, 4, 5]]).all()
  ref = NC.reference('exclude_len_zero')
  assert ref['nearest'].tolist() == [0.0] * 6
  assert ref['index'].tolist() == [0, 26, 10, 0, 26, 13]


# -- novelty_scores --------------------------------------------------------------
def test_novelty_scores_by_hand():
  L, C = 4, 5
  k = L * C
  rec = (np.array([4.0, 9.0, 16.0, 25.0]) * k, np.array([3, 1, 0, 2]))
  gen = (np.array([1.0, 36.0, 12.25, 4.0, 9.0]) * k, np.array([7, 7, 2, 7, 0]))
  s = sm.novelty_scores(rec, gen, L, C, step=2, offsets=11)
  assert set(s) == NOVELTY_KEYS
  assert s['nearest_rms'] == {'recorded': [2.0, 3.5, 5.0],
                              'generated': [1.0, 3.0, 6.0]}
  assert s['nearest_rms_ratio'] == 3.0 / 3.5
  assert s['copied_fraction'] == 1 / 5         # below 2: the 1 only
  assert s['below_recorded_median'] == 3 / 5   # below 3.5: 1, 2, 3
  assert s['distinct_stretches'] == 3 / 5
  assert (s['step'], s['offsets']) == (2, 11)
  assert s['num_trials'] == [4, 5] and s['undefined'] == [0, 0]
  json.dumps(s)
  # a collapse onto one stretch
  one = (gen[0], np.full(5, 4))
  assert sm.novelty_scores(rec, one, L, C, 2)['distinct_stretches'] == 1 / 5
  assert sm.novelty_scores(rec, one, L, C, 2)['offsets'] is None
  # NaNs are left out and counted
  gen_nan = (np.array([1.0, np.nan, 12.25, np.nan, 9.0]) * k,
             np.array([7, -1, 2, -1, 0]))
  rec_nan = (np.array([4.0, np.nan, 16.0, 25.0]) * k, np.array([3, -1, 0, 2]))
  s = sm.novelty_scores(rec_nan, gen_nan, L, C, 2)
  assert s['nearest_rms'] == {'recorded': [2.0, 4.0, 5.0],
                              'generated': [1.0, 3.0, 3.5]}
  assert s['num_trials'] == [4, 5] and s['undefined'] == [1, 2]
  assert s['copied_fraction'] == 1 / 3 and s['distinct_stretches'] == 1.0
  assert s['below_recorded_median'] == 3 / 3
  # an empty side
  none = (np.array([np.nan, np.nan]), np.array([-1, -1]))
  for s in (sm.novelty_scores(none, gen, L, C, 2),
            sm.novelty_scores((np.zeros(0), np.zeros(0, int)), gen, L, C, 2)):
    assert np.isnan(s['nearest_rms']['recorded']).all()
    assert s['nearest_rms']['generated'] == [1.0, 3.0, 6.0]
    assert np.isnan([s['nearest_rms_ratio'], s['copied_fraction'],
                     s['below_recorded_median']]).all()
    assert s['distinct_stretches'] == 3 / 5
  s = sm.novelty_scores(rec, none, L, C, 2)
  assert np.isnan(s['nearest_rms']['generated']).all()
  assert np.isnan([s['nearest_rms_ratio'], s['copied_fraction'],
                   s['distinct_stretches']]).all()
  assert s['undefined'] == [0, 2]
  with pytest.raises(ValueError):
    sm.novelty_scores(rec, (gen[0], gen[1][:3]), L, C, 2)


def test_recorded_starts_lie_on_the_grid_and_span_it():
  v = sm.recorded_starts(319, 12, 2)
  assert v[0] == 0 and v[-1] == 2 * 318 and (v % 2 == 0).all()
  assert (np.diff(v) > 0).all()
  assert v.tolist() == [2 * ((i * 318) // 11) for i in range(12)]
  assert sm.recorded_starts(5, 1, 3).tolist() == [0]
  assert sm.recorded_starts(1, 4, 3).tolist() == [0, 0, 0, 0]


# -- the C header and the entry's argument checks ----------------------------------
def test_the_header_holds_the_two_prototypes_and_abi_20():
  assert _lib.CG_ABI_VERSION == 20
  text = re.sub(r'\s+', ' ', open(_lib.HEADER).read())
  assert ('long long cg_nearest_stretch_ws_bytes(int N, int L, int C, long long '
          'T_raw, int step);') in text
  assert ('int cg_nearest_stretch(const float* q, int N, int L, int C, long long '
          'q_sn, long long q_st, long long q_sc, const float* raw, long long '
          'T_raw, long long r_st, long long r_sc, int step, const int* exclude, '
          'int exclude_len, double* d2, double* nearest, int* index, void* ws, '
          'void* stream);') in text
  argtypes = _lib.SIGNATURES['cg_nearest_stretch']
  assert len(argtypes) == 19
  assert len(_lib.SIGNATURES['cg_nearest_stretch_ws_bytes']) == 5
  assert argtypes[0].ctype == 'float*' and argtypes[12].ctype == 'int*'
  assert argtypes[14].ctype == 'double*' and argtypes[17].ctype == 'void*'
  from calciumgan_amd import build
  assert 'nearest_stretch.hip' in build.SOURCES


def test_refused_arguments_return_einval_before_anything_touches_hip():
  """The checks come before the first HIP call, so they run without a device:
  the pointers are never followed."""
  lib = _lib.load()
  for shape, want in (((128, 2048, 102, 20432, 2),
                       8 * NC.ws_doubles(128, 2048, 102, 20432, 2)),
                      ((1, 5, 3, 5, 1), 8 * NC.ws_doubles(1, 5, 3, 5, 1))):
    assert lib.cg_nearest_stretch_ws_bytes(*shape) == want
  for name in NC.CASES:
    assert lib.cg_nearest_stretch_ws_bytes(*NC.shape(name)) == 8 * NC.ws_doubles(
        *NC.shape(name)), name
  refused = [(0, 5, 3, 50, 1), (2, 0, 3, 50, 1), (2, 5, 0, 50, 1),
             (2, 5, 3, 50, 0), (2, 5, 3, 4, 1), (65536, 5, 3, 50, 1),
             (2, 1 << 20, 1025, 1 << 21, 1), (2, 5, 3, (1 << 31) - 64, 1),
             (2, 5, 1 << 20, (1 << 20) + 1, 1), (2, 5, 3, 50, (1 << 20) + 1),
             (-1, 5, 3, 50, 1)]
  for shape in refused:
    assert lib.cg_nearest_stretch_ws_bytes(*shape) == -1, shape

  def call(q=64, raw=128, nearest=192, index=256, ws=320, shape=(2, 5, 3, 50, 1),
           exclude_len=0):
    N, L, C, T_raw, step = shape
    return lib.cg_nearest_stretch(q, N, L, C, L * C, C, 1, raw, T_raw, C, 1,
                                  step, None, exclude_len, None, nearest, index,
                                  ws, None)

  for kw in (dict(q=None), dict(raw=None), dict(nearest=None), dict(index=None),
             dict(ws=None), dict(ws=324), dict(exclude_len=-1)):
    assert call(**kw) == _lib.CG_EINVAL, kw
  for shape in refused:
    assert call(shape=shape) == _lib.CG_EINVAL, shape


# -- compute_metrics.py ------------------------------------------------------------
def _args(path, *more):
  return ['--output_dir', str(path), '--num_processors', '1', '--verbose', '0',
          '--device', 'cpu'] + list(more)


def test_compute_metrics_novelty_flag_on_the_host(tmp_path):
  os.makedirs(tmp_path / 'copies')
  fake, rec, gen = NC.run_dir(tmp_path / 'copies', kind='copies')
  raw, L, C = rec['raw'], 256, 24
  plain = cm.build_parser().parse_args(_args(tmp_path / 'copies'))
  assert not hasattr(plain, 'novelty_metrics')
  assert not hasattr(plain, 'novelty_step')
  report = cm.main(plain)[0]
  assert set(report) == PLAIN_KEYS
  hp = cm.build_parser().parse_args(
      _args(tmp_path / 'copies', '--novelty_metrics'))
  assert hp.novelty_metrics is True and not hasattr(hp, 'novelty_step')
  with_flag = cm.main(hp)[0]
  assert set(with_flag) == PLAIN_KEYS | {'novelty'}
  for key in PLAIN_KEYS - {'elapse'}:   # what was there is unchanged
    assert with_flag[key] == report[key], key
  s = with_flag['novelty']
  assert set(s) == NOVELTY_KEYS
  # the dataset's stride is the step; every full stretch is an offset
  S = (1500 - L) // 2 + 1
  assert (s['step'], s['offsets']) == (2, S)
  assert s['num_trials'] == [12, 12] and s['undefined'] == [0, 0]
  starts = sm.recorded_starts(S, 12, 2)
  want = sm.novelty_scores(
      sm.nearest_stretch(np.stack([raw[v:v + L] for v in starts]), raw, 2,
                         starts, L, expanded=True),
      sm.nearest_stretch(gen, raw, 2, expanded=True), L, C, 2, offsets=S)
  assert s == want
  # noisy copies: every one closer than any stretch of the recording comes to
  # the rest of it, about the noise's 0.01 away
  assert s['copied_fraction'] == 1.0 and s['below_recorded_median'] == 1.0
  assert 0.005 < s['nearest_rms']['generated'][1] < 0.02
  assert s['nearest_rms']['recorded'][0] > 0.05
  on_disk = json.load(open(tmp_path / 'copies' / 'spike_metrics.json'))
  assert on_disk['0']['novelty'] == s
  # the recorded side is kept on hparams for the next epoch
  assert hp._recorded_novelty[0].shape == (12,)
  # --novelty_step is honoured
  hp4 = cm.build_parser().parse_args(
      _args(tmp_path / 'copies', '--novelty_metrics', '--novelty_step', '4'))
  s4 = cm.main(hp4)[0]['novelty']
  assert (s4['step'], s4['offsets']) == (4, (1500 - L) // 4 + 1)
  assert s4['copied_fraction'] == 1.0
  assert s4['nearest_rms']['recorded'] != s['nearest_rms']['recorded']
  # a generated file of another length is refused
  hp5 = cm.build_parser().parse_args(
      _args(tmp_path / 'copies', '--novelty_metrics'))
  cm.utils.load_hparams(hp5)
  hp5.num_samples = 12
  short = str(tmp_path / 'short.h5')
  cm.h5_helper.write(short, {'signals': gen[:, :128]})
  with pytest.raises(ValueError, match='128 frames'):
    cm.novelty_report(hp5, short, cm.novelty_nearest_host)


def test_a_recording_of_another_seed_is_not_a_copy(tmp_path):
  fake, rec, gen = NC.run_dir(tmp_path, kind='other')
  hp = cm.build_parser().parse_args(_args(tmp_path, '--novelty_metrics'))
  s = cm.main(hp)[0]['novelty']
  print(s)
  assert s['copied_fraction'] == 0.0
  assert s['nearest_rms']['generated'][0] > s['nearest_rms']['recorded'][0]
  assert s['num_trials'] == [12, 12] and s['undefined'] == [0, 0]


def test_a_run_that_was_not_trained_on_a_recording_is_refused(tmp_path):
  import trace_psd_cases as PC
  PC.run_dir(tmp_path, T=256)         # hparams.json without an input_dir
  hp = cm.build_parser().parse_args(_args(tmp_path, '--novelty_metrics'))
  with pytest.raises(ValueError, match='recording directory'):
    cm.main(hp)
  # an input_dir that holds a dataset of windows
  hparams = json.load(open(tmp_path / 'hparams.json'))
  os.makedirs(tmp_path / 'windows')
  with open(tmp_path / 'windows' / 'info.pkl', 'wb') as f:
    import pickle
    pickle.dump(dict(sequence_length=256, stride=2), f)
  hparams['input_dir'] = str(tmp_path / 'windows')
  json.dump(hparams, open(tmp_path / 'hparams.json', 'w'))
  hp = cm.build_parser().parse_args(_args(tmp_path, '--novelty_metrics'))
  with pytest.raises(ValueError, match='recording directory'):
    cm.main(hp)
  # without the flag the same run reports as before
  plain = cm.build_parser().parse_args(_args(tmp_path))
  assert set(cm.main(plain)[0]) == PLAIN_KEYS
