"""Host tests of the population-state figures (gan/utils/spike_metrics.py: the
numpy statements cg_population_states and cg_state_neighbours are tested
against, and state_scores), of the C entry points' argument checks in both
precision builds, and of compute_metrics.py --state_metrics on the host path.
No GPU.  Every comparison is of integers or of dicts."""
import json
import os

import numpy as np
import pytest

import compute_metrics as cm
import state_neighbour_cases as SC
from calciumgan_amd import _lib
from calciumgan_amd.gan.utils import spike_metrics as sm

PLAIN_KEYS = {'firing_rate_kl', 'correlation_kl', 'van_rossum_kl',
              'van_rossum_heatmap_min', 'elapse'}


# -- population_states ---------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 12, 3), (2, 50, 17), (3, 300, 102)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_population_states_are_bin_counts_rearranged(shape):
  B, T, C = shape
  sp = (np.random.RandomState(T).uniform(size=shape) < 0.4).astype(np.float32)
  x = sm.population_states(sp)
  nb = T // 12
  assert x.dtype == np.int32 and x.shape == (B * nb, C)
  # bin_counts takes (..., neurons, T): (B, C, nb) -> rows n nb + b
  want = sm.bin_counts(sp.transpose(0, 2, 1)).transpose(0, 2, 1).reshape(B * nb, C)
  assert np.array_equal(x, want)
  # a trailing partial bin is dropped
  if T % 12:
    assert np.array_equal(x, sm.population_states(sp[:, :nb * 12]))
  # other bins; anything non-zero is a spike
  assert np.array_equal(sm.population_states(sp, 1), (sp != 0).reshape(B * T, C))
  assert np.array_equal(sm.population_states(sp * np.float32(-2.5), 5),
                        sm.population_states(sp, 5))
  if T <= sm.STATE_MAX_BIN:
    assert sm.population_states(sp, T).shape == (B, C)


def test_population_states_refuse_what_holds_no_bin():
  sp = np.ones((2, 11, 3), np.float32)
  with pytest.raises(ValueError):
    sm.population_states(sp)            # T < bin
  for bin in (0, -1, 128):
    with pytest.raises(ValueError):
      sm.population_states(np.ones((2, 200, 3), np.float32), bin)
  with pytest.raises(ValueError):
    sm.population_states(np.ones((11, 3), np.float32))
  assert sm.population_states(np.ones((1, 127, 2), np.float32), 127).tolist() == [
      [127, 127]]


# -- state_neighbours -----------------------------------------------------------
def _same(got, want):
  assert np.array_equal(got[0], want[0])
  if want[1] is None:
    assert got[1] is None
  else:
    assert np.array_equal(got[1], want[1])


@pytest.mark.parametrize('sizes', [(1, 1), (5, 9), (9, 5), (20, 3)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_neighbours_equal_the_double_loop(sizes):
  Sa, Sb = sizes
  for C, density in ((1, 0.5), (4, 0.1), (7, 0.5)):
    a = SC.with_duplicates(SC.states(Sa, C, density, 1))
    b = SC.with_duplicates(SC.states(Sb, C, density, 2))
    b[0] = a[-1]                       # an exact match across the sets
    for k in (1, 5, 8):                # 5 and 8 exceed Sb = 3: the 2^31 - 1 tail
      for kind in (None, 'zero', 'huge', 'mixed'):
        rad = None if kind is None else SC.radii(Sb, kind, C)
        got = sm.state_neighbours(a, b, k, radius_b=rad)
        _same(got, SC.double_loop(a, b, k, radius_b=rad))
        assert got[0].dtype == np.int32
        # the chunked walk does not show
        _same(sm.state_neighbours(a, b, k, radius_b=rad, chunk=4), got)
        if Sb < k:
          assert (got[0][:, Sb:] == SC.NONE).all()
          assert (got[0][:, :Sb] < SC.NONE).all()
        if kind == 'huge':
          assert (got[1] == Sb).all()
        if kind == 'zero':
          assert np.array_equal(got[1], (a[:, None] == b[None]).all(-1).sum(1))


@pytest.mark.parametrize('S', [1, 2, 6, 11])
def test_self_exclusion_is_by_index(S):
  x = SC.with_duplicates(SC.states(S, 5, 0.5, 3), seed=S)
  for k in (1, 5, 8):
    for kind in (None, 'zero', 'huge'):
      rad = None if kind is None else SC.radii(S, kind, 5)
      got = sm.state_neighbours(x, x, k, exclude_self=True, radius_b=rad)
      _same(got, SC.double_loop(x, x, k, exclude_self=True, radius_b=rad))
      _same(sm.state_neighbours(x, x, k, exclude_self=True, radius_b=rad,
                                chunk=4), got)
      assert (got[0][:, min(S - 1, k):] == SC.NONE).all()
      if kind == 'huge':
        assert (got[1] == S - 1).all()
  # a twin at another index gives 0; a state alone in its value does not
  x = np.array([[1, 2, 3], [4, 4, 4], [1, 2, 3]])
  knn, within = sm.state_neighbours(x, x, 2, exclude_self=True,
                                    radius_b=np.zeros(3, np.int32))
  assert knn.tolist() == [[0, 14], [14, 14], [0, 14]]
  assert within.tolist() == [1, 0, 1]
  with pytest.raises(ValueError):
    sm.state_neighbours(x, x[:2], 1, exclude_self=True)
  for k in (0, 9):
    with pytest.raises(ValueError):
      sm.state_neighbours(x, x, k)


# -- state_scores -----------------------------------------------------------------
def test_a_set_against_itself_scores_one():
  x = SC.states(60, 9, 0.3, 4)
  s = sm.state_scores(x, x, 5)
  assert (s['precision'], s['recall'], s['coverage']) == (1.0, 1.0, 1.0)
  assert s['exact_match'] == [1.0, 1.0]
  assert s['nearest_distance'] == [0.0, 0.0]
  assert s['radius_median'][0] == s['radius_median'][1] > 0
  assert s['num_states'] == [60, 60]
  json.dumps(s)
  # the caller's radii are the ones the function would form
  assert s == sm.state_scores(x, x, 5, rad_ref=sm.state_radii(x, 5))
  # both sets need more than k states
  for ref, other in ((x[:5], x), (x, x[:5])):
    with pytest.raises(ValueError):
      sm.state_scores(ref, other, 5)
  assert sm.state_scores(x[:6], x[:6], 5)['precision'] == 1.0


def test_disjoint_sets_far_apart_score_zero():
  x = SC.states(40, 9, 0.3, 5)
  far = x + 100
  s = sm.state_scores(x, far, 3)
  assert (s['precision'], s['recall'], s['coverage']) == (0.0, 0.0, 0.0)
  assert s['exact_match'] == [0.0, 0.0]
  assert s['nearest_distance'][0] > 100 and s['nearest_distance'][1] > 100
  assert s['radius_median'][0] == s['radius_median'][1]


def test_a_clipped_gain_lowers_recall_below_its_floor():
  """100 trials of 480 frames of 102 neurons with a gain shared per bin, 4000
  states a side, k = 5.  Measured here with these seeds: floor precision 0.804,
  recall 0.794, coverage 0.982; with the high-gain bins clipped away recall
  0.614 (precision 0.793, coverage 0.881)."""
  ref = sm.population_states(SC.gain_trials(1))
  floor = sm.state_scores(ref, sm.population_states(SC.gain_trials(2)), 5)
  clipped = sm.state_scores(
      ref, sm.population_states(SC.gain_trials(3, clip=True)), 5)
  print('floor  ', floor)
  print('clipped', clipped)
  assert floor['num_states'] == clipped['num_states'] == [4000, 4000]
  assert clipped['recall'] <= floor['recall'] - 0.05
  assert clipped['coverage'] < floor['coverage']
  # what is produced is still something the data contains
  assert clipped['precision'] > floor['precision'] - 0.05
  # two draws of one model do not score 1
  assert 0.5 < floor['precision'] < 0.95 and 0.5 < floor['recall'] < 0.95


# -- the C entry points --------------------------------------------------------------
def test_the_header_holds_the_prototypes_and_abi_20():
  assert _lib.CG_ABI_VERSION == 20
  c = _lib.CONSTANTS
  assert (c['CG_STATE_K_STEP'], c['CG_STATE_MAX_K'], c['CG_STATE_MAX_BIN'],
          c['CG_STATE_NONE'], c['CG_STATE_EXACT_SUM']) == (
              sm.STATE_K_STEP, sm.STATE_MAX_K, sm.STATE_MAX_BIN, sm.STATE_NONE,
              sm.STATE_EXACT_SUM) == (32, 8, 127, 2**31 - 1, 1 << 24)
  assert c['CG_STATE_MAX_C'] == sm.STATE_MAX_NEURONS == 4096
  assert len(_lib.SIGNATURES['cg_population_states']) == 10
  assert len(_lib.SIGNATURES['cg_state_neighbours_ws_bytes']) == 5
  argtypes = _lib.SIGNATURES['cg_state_neighbours']
  assert len(argtypes) == 13
  assert argtypes[0].ctype == 'void*' and argtypes[8].ctype == 'int*'
  src = open(os.path.join(os.path.dirname(_lib.HEADER), '..', 'calciumgan_amd',
                          'build.py')).read()
  assert "'state_neighbours.hip'" in src


@pytest.mark.parametrize('precision', ['bf16', 'f16'])
def test_refused_arguments_return_einval_before_anything_touches_hip(precision):
  """The checks come before the first HIP call, so they run without a device:
  the pointers are never followed."""
  lib = _lib.load(precision)
  assert lib.cg_abi_version() == 20
  P = 1 << 20   # a 16-byte aligned address nobody reads

  def ws(Sa=40, Sb=2500, C=102, bin=12, k=5):
    return lib.cg_state_neighbours_ws_bytes(Sa, Sb, C, bin, k)

  def query(a=P, Sa=40, b=P + 4096, Sb=2500, C=102, bin=12, k=5, excl=0,
            rad=P + 64, knn=P + 128, within=P + 256, w=P + 512):
    return lib.cg_state_neighbours(a, Sa, b, Sb, C, bin, k, excl, rad, knn,
                                   within, w, None)

  def states(x=P, B=2, T=50, C=17, bin=12, out=P + 64):
    return lib.cg_population_states(x, B, T, C, T * C, C, 1, bin, out, None)

  # the plan: one workgroup per 128 states of A; B split while that leaves
  # fewer than 1024 workgroups, over at most 64 and at most its 64-state tiles
  assert ws(700, 40) == 4 * (700 + 40)
  assert ws(40, 2500) == 4 * (40 + 2500 + 40 * 40 * 6)
  assert ws(85000, 85000) == 4 * (170000 + 2 * 85000 * 6)
  assert ws(1 << 24, 1 << 24, 4096, 64, 8) == 4 * (1 << 25)
  shapes = [dict(Sa=0), dict(Sb=0), dict(C=0), dict(Sa=-1), dict(Sb=-5),
            dict(Sa=(1 << 24) + 1), dict(Sb=(1 << 24) + 1), dict(C=4097),
            dict(bin=0), dict(bin=128), dict(bin=-3), dict(k=0), dict(k=9),
            dict(k=-1), dict(C=4096, bin=65), dict(C=1041, bin=127),
            dict(C=2048, bin=91)]
  for kw in shapes:
    assert ws(**kw) == -1, kw
    assert query(**kw) == _lib.CG_EINVAL, kw
  for kw in (dict(C=4096, bin=64), dict(C=1040, bin=127), dict(C=2048, bin=90)):
    assert ws(**kw) > 0, kw
  for kw in (dict(a=None), dict(b=None), dict(w=None), dict(a=P + 8),
             dict(b=P + 4), dict(w=P + 520), dict(rad=P + 66), dict(knn=P + 130),
             dict(within=P + 257), dict(knn=None, within=None, rad=None),
             dict(within=None), dict(rad=None), dict(excl=1),
             dict(excl=1, b=P, Sb=41), dict(excl=1, b=P + 16, Sb=40)):
    assert query(**kw) == _lib.CG_EINVAL, kw
  for kw in (dict(x=None), dict(out=None), dict(out=P + 8), dict(B=0),
             dict(T=0), dict(C=0), dict(bin=0), dict(bin=128), dict(T=11),
             dict(C=4097), dict(C=4096, bin=65, T=130),
             dict(B=1 << 20, T=12 * 17)):
    assert states(**kw) == _lib.CG_EINVAL, kw


# -- compute_metrics.py ------------------------------------------------------------
def _args(path, *more):
  return ['--output_dir', str(path), '--num_processors', '1', '--verbose', '0',
          '--device', 'cpu'] + list(more)


def test_compute_metrics_state_flag_on_the_host(tmp_path, capsys):
  fake, real_spikes, fake_spikes = SC.run_dir(tmp_path)
  plain = cm.build_parser().parse_args(_args(tmp_path))
  for name in ('state_metrics', 'state_k', 'state_bin'):
    assert not hasattr(plain, name)
  before = cm.main(plain)[0]
  assert set(before) == PLAIN_KEYS
  assert 'states' not in json.load(open(tmp_path / 'spike_metrics.json'))['0']
  hp = cm.build_parser().parse_args(_args(tmp_path, '--state_metrics'))
  assert hp.state_metrics is True
  report = cm.main(hp)[0]
  assert set(report) == PLAIN_KEYS | {'states'}
  assert {k: v for k, v in report.items() if k not in ('states', 'elapse')} == {
      k: v for k, v in before.items() if k != 'elapse'}
  s = report['states']
  assert set(s) == {'generated', 'floor', 'k', 'bin_frames'}
  assert (s['k'], s['bin_frames']) == (5, 12)
  assert s == SC.expected_report(real_spikes, fake_spikes)
  assert s['floor']['num_states'] == s['generated']['num_states'] == [480, 480]
  assert json.load(open(tmp_path / 'spike_metrics.json'))['0']['states'] == s
  # the recorded side is kept on hparams for the next epoch
  ref, rad_ref, floor, frames = hp._recorded_states
  assert len(ref) == 480 and rad_ref.shape == (480,) and frames == 480
  assert floor == s['floor']
  # --state_k and --state_bin are honoured
  hp2 = cm.build_parser().parse_args(
      _args(tmp_path, '--state_metrics', '--state_k', '3', '--state_bin', '24'))
  s2 = cm.main(hp2)[0]['states']
  assert s2 == SC.expected_report(real_spikes, fake_spikes, k=3, bin=24)
  assert s2['floor']['num_states'] == [240, 240]
  # verbose: the three figures beside their floor
  hp3 = cm.build_parser().parse_args(_args(tmp_path, '--state_metrics'))
  hp3.verbose = 1
  capsys.readouterr()
  cm.main(hp3)
  out = capsys.readouterr().out
  for name in ('precision', 'recall', 'coverage'):
    assert 'state {:<9}  gen | floor: {:.04f} | {:.04f}'.format(
        name, s['generated'][name], s['floor'][name]) in out
  # a generated file of another length is refused, as the other reports do
  hp._recorded_states = (ref, rad_ref, floor, 256)
  with pytest.raises(ValueError, match='480 frames'):
    cm.state_report(hp, fake, cm.state_sets_host, sm.state_neighbours)
