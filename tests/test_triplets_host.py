"""Host tests of the third-order figures (gan/utils/spike_metrics.py: the numpy
statements cg_binary_words and cg_triplet_counts are tested against, and
triplet_scores), of the C entry points' argument checks in both precision
builds, and of compute_metrics.py --triplet_metrics on the host path.  No GPU.
Counts are compared as integers, reports as dicts."""
import itertools
import json
import math

import numpy as np
import pytest

import compute_metrics as cm
import triplet_cases as TC
from calciumgan_amd import _lib
from calciumgan_amd.gan.utils import spike_metrics as sm

PLAIN_KEYS = {'firing_rate_kl', 'correlation_kl', 'van_rossum_kl',
              'van_rossum_heatmap_min', 'elapse'}


# -- the statements --------------------------------------------------------------
@pytest.mark.parametrize('case', TC.TRAINS, ids=lambda s: 'x'.join(map(str, s)))
def test_binary_states_are_any_spike_in_the_bin(case):
  B, T, C, bin, density = case
  sp = TC.trains(B, T, C, density)
  x = sm.binary_states(sp, bin)
  nb = T // bin
  assert x.dtype == np.uint8 and x.shape == (B * nb, C)
  for n, b, c in itertools.product(range(B), range(min(nb, 3)), range(min(C, 4))):
    assert x[n * nb + b, c] == int(sp[n, b * bin:(b + 1) * bin, c].any())
  # a trailing partial bin is dropped, whatever it holds
  more = np.concatenate([sp[:, :nb * bin], np.ones((B, bin - 1, C), np.float32)],
                        axis=1)
  assert np.array_equal(sm.binary_states(more, bin), x)
  # anything non-zero is a spike; the counts past one do not show
  assert np.array_equal(sm.binary_states(sp * np.float32(-2.5), bin), x)
  if bin <= sm.STATE_MAX_BIN:
    assert np.array_equal(x, sm.population_states(sp, bin) > 0)


def test_binary_states_nan_minus_zero_and_what_holds_no_bin():
  sp = np.zeros((1, 24, 3), np.float32)
  sp[0, 1, 0] = np.nan
  sp[0, 2, 1] = -0.0
  sp[0, 13, 2] = -3.5
  assert sm.binary_states(sp).tolist() == [[1, 0, 0], [0, 0, 1]]
  with pytest.raises(ValueError):
    sm.binary_states(np.ones((2, 11, 3), np.float32))       # T < bin
  for bin in (0, -1):
    with pytest.raises(ValueError):
      sm.binary_states(np.ones((2, 20, 3), np.float32), bin)
  with pytest.raises(ValueError):
    sm.binary_states(np.ones((11, 3), np.float32))


@pytest.mark.parametrize('C', [3, 4, 5, 6])
def test_counts_equal_the_triple_loop(C):
  for S, density in ((1, 0.5), (7, 0.5), (200, 0.3), (200, 1.0), (50, 0.0)):
    x = (np.random.RandomState(S + C).uniform(size=(S, C)) < density).astype(
        np.uint8)
    got = sm.triplet_counts(x)
    want = TC.triple_loop(x)
    for g, w in zip(got, want):
      assert g.dtype == np.int64 and np.array_equal(g, w)
    singles, pairs, triplets = got
    assert pairs.shape == (C, C) and np.array_equal(pairs, pairs.T)
    assert np.array_equal(np.diagonal(pairs), singles)
    assert triplets.shape == (math.comb(C, 3),)
    # the chunked walk does not show
    for g, w in zip(sm.triplet_counts(x, chunk=3), got):
      assert np.array_equal(g, w)
  for bad in (np.ones((5, 2)), np.ones((0, 4)), np.ones((4,))):
    with pytest.raises(ValueError):
      sm.triplet_counts(bad)


@pytest.mark.parametrize('C', [3, 4, 7, 17, 33])
def test_triplet_index_is_combinations(C):
  idx = sm.triplet_index(C)
  assert idx.dtype == np.int32
  assert idx.tolist() == [list(t) for t in
                          itertools.combinations(range(C), 3)]
  with pytest.raises(ValueError):
    sm.triplet_index(2)


def test_counts_at_the_ranks_of_triplet_index():
  x = (np.random.RandomState(1).uniform(size=(300, 19)) < 0.4).astype(np.int64)
  triplets = sm.triplet_counts(x)[2]
  i, j, k = sm.triplet_index(19).T
  assert np.array_equal(triplets, (x[:, i] * x[:, j] * x[:, k]).sum(0))


@pytest.mark.parametrize('nb', [1, 3, 31, 32, 33, 64, 65, 170])
def test_packing_round_trip(nb):
  N, C = 3, 5
  x = (np.random.RandomState(nb).uniform(size=(N * nb, C)) < 0.5).astype(np.uint8)
  w = sm.pack_state_words(x, nb)
  wpt = -(-nb // 32)
  assert w.dtype == np.uint32 and w.shape == (C, N * wpt)
  assert np.array_equal(sm.unpack_state_words(w, nb), x)
  # bit b % 32 of word b // 32 of trial n; the tail bits are zero
  for n, b, c in ((0, 0, 0), (1, nb - 1, 2), (2, nb // 2, 4)):
    assert (int(w[c, n * wpt + b // 32]) >> (b % 32)) & 1 == x[n * nb + b, c]
  tail = wpt * 32 - nb
  if tail:
    assert not (w.reshape(C, N, wpt)[:, :, -1] >> np.uint32(32 - tail)).any()
  # the popcounts are the singles
  ones = np.array([[bin(int(v)).count('1') for v in row] for row in w]).sum(1)
  assert np.array_equal(ones, sm.triplet_counts(x)[0])
  with pytest.raises(ValueError):
    sm.pack_state_words(x, N * nb + 1)      # no whole trials


# -- the scores -------------------------------------------------------------------
def test_kappa_of_the_xor_trios():
  """s_k = s_i XOR s_j at p = 1/2: every pair independent, kappa = -1/8.  40 000
  states; the bound is five times the delta-method deviation of kappa-hat with
  its terms taken as fully correlated: 0.5 sd(p_ab) on each of the three pairs
  and 0.25 sd(p_c) on each of the three singles (p_ijk is exactly 0 in a
  trio)."""
  S = 40000
  x = TC.xor_states(11, S)
  cov, p3, kappa = sm._triplet_moments(TC.side(x))
  idx = sm.triplet_index(TC.XOR_NEURONS).tolist()
  sd = 3 * 0.5 * math.sqrt(0.25 * 0.75 / S) + 3 * 0.25 * math.sqrt(0.25 / S)
  tol = 5 * sd
  print('tolerance', tol)
  assert tol < 0.125 / 4
  for t in range(TC.XOR_TRIOS):
    r = idx.index([3 * t, 3 * t + 1, 3 * t + 2])
    print('trio', t, 'kappa', kappa[r])
    assert p3[r] == 0.0
    assert abs(kappa[r] + 0.125) < tol
  # pairwise independent: no pair of the 24 neurons has a covariance (the same
  # bound: sd(p_ab) and 0.5 sd(p) on either single, at the fair coins' worst)
  assert np.abs(cov).max() < 5 * (math.sqrt(0.25 * 0.75 / S) +
                                  2 * 0.5 * math.sqrt(0.25 / S))
  # the independent neurons have none of the third order either
  r = idx.index([12, 13, 14])
  assert abs(kappa[r]) < tol


def test_the_pair_figure_is_blind_where_the_cumulant_is_not():
  """24 neurons, 4000 states a side (triplet_cases.xor_states).  `floor` is a
  second draw of the true model, `generator` the model with every s_k a coin of
  its own.  Measured here with these seeds: pair-covariance MAE floor 0.00280,
  generator 0.00297 (1.06 x the floor); cumulant correlation floor 0.963,
  generator -0.003; cumulant MAE floor 0.00112, generator 0.00139; over the top
  1 % of triplets (21) the correlation is 0.995 against -0.146 and the MAE
  0.0040 against 0.0273."""
  ref_states = TC.xor_states(1)
  # the inputs: rates and pair covariances of the broken model are the true ones
  for seed, broken in ((2, False), (3, True)):
    x = TC.xor_states(seed, broken=broken).astype(np.float64)
    assert np.abs(x[:, :12].mean(0) - 0.5).max() < 0.04
    assert np.abs(x[:, 12:].mean(0) - 0.1).max() < 0.03
    c = np.cov(x.T)
    assert np.abs(c - np.diag(np.diagonal(c))).max() < 0.03
  ref = TC.side(ref_states)
  floor = sm.triplet_scores(ref, TC.side(TC.xor_states(2)))
  gen = sm.triplet_scores(ref, TC.side(TC.xor_states(3, broken=True)))
  print('floor    ', floor)
  print('generator', gen)
  assert floor['num_states'] == gen['num_states'] == [4000, 4000]
  assert floor['num_triplets'] == gen['num_triplets'] == 2024
  assert gen['pair_covariance_mae'] <= 1.25 * floor['pair_covariance_mae']
  assert gen['triplet_cumulant_correlation'] < 0.2
  assert floor['triplet_cumulant_correlation'] > 0.9
  assert floor['triplet_cumulant_top_correlation'] > 0.9
  assert gen['triplet_cumulant_top_correlation'] < 0.2
  json.dumps(floor)


def test_scores_of_a_side_against_itself_and_their_nan_rules():
  x = TC.xor_states(5, 500)
  s = sm.triplet_scores(TC.side(x), TC.side(x))
  assert s['pair_covariance_mae'] == s['triplet_probability_mae'] == 0.0
  assert s['triplet_cumulant_mae'] == s['triplet_cumulant_top_mae'] == 0.0
  assert s['pair_covariance_correlation'] == 1.0
  assert s['triplet_cumulant_correlation'] == 1.0
  assert s['triplet_cumulant_top_correlation'] == 1.0
  assert s['triplet_cumulant_mean_abs'][0] == s['triplet_cumulant_mean_abs'][1] > 0
  assert 0 < s['triplets_observed'][0] == s['triplets_observed'][1] <= 1
  assert s['num_triplets'] == 2024 and s['num_states'] == [500, 500]
  # the top set: max(2, ceil(Tr / 100)) triplets of largest |kappa_ref|, the
  # lower rank first on ties
  _, _, kappa = sm._triplet_moments(TC.side(x))
  top = sorted(range(2024), key=lambda r: (-abs(kappa[r]), r))[:21]
  other = TC.side(TC.xor_states(6, 500))
  ko = sm._triplet_moments(other)[2]
  got = sm.triplet_scores(TC.side(x), other)
  assert got['triplet_cumulant_top_mae'] == float(
      np.mean(np.abs(kappa[top] - ko[top])))
  # one triplet: every correlation over triplets and the top figures are NaN
  three = sm.triplet_scores(TC.side(x[:, :3]), TC.side(x[:, 3:6]))
  assert three['num_triplets'] == 1
  for key in ('triplet_cumulant_correlation', 'triplet_cumulant_top_correlation',
              'triplet_cumulant_top_mae'):
    assert math.isnan(three[key])
  assert not math.isnan(three['triplet_cumulant_mae'])
  assert not math.isnan(three['pair_covariance_correlation'])
  # four neurons, four triplets: the top set is two of them
  four = sm.triplet_scores(TC.side(x[:, :4]), TC.side(x[:, 3:7]))
  assert four['num_triplets'] == 4
  assert not math.isnan(four['triplet_cumulant_top_mae'])
  # no variance on a side: silent neurons
  silent = TC.side(np.zeros((10, 4), np.uint8))
  s0 = sm.triplet_scores(silent, TC.side(x[:, :4]))
  assert math.isnan(s0['triplet_cumulant_correlation'])
  assert math.isnan(s0['pair_covariance_correlation'])
  assert s0['triplets_observed'][0] == 0.0
  with pytest.raises(ValueError):
    sm.triplet_scores(TC.side(x[:, :4]), TC.side(x[:, :5]))


# -- the C entry points --------------------------------------------------------------
def test_the_header_holds_the_prototypes_and_abi_20():
  assert _lib.CG_ABI_VERSION == 20
  c = _lib.CONSTANTS
  assert c['CG_TRIPLET_MAX_C'] == sm.TRIPLET_MAX_NEURONS == 512
  assert c['CG_TRIPLET_MAX_WORDS'] == sm.TRIPLET_MAX_WORDS == 2**26 - 1
  assert len(_lib.SIGNATURES['cg_binary_words']) == 11
  assert len(_lib.SIGNATURES['cg_triplet_counts_ws_bytes']) == 2
  argtypes = _lib.SIGNATURES['cg_triplet_counts']
  assert len(argtypes) == 9
  assert argtypes[0].ctype == 'void*' and argtypes[4].ctype == 'int*'
  from calciumgan_amd import build
  assert 'triplets.hip' in build.SOURCES


@pytest.mark.parametrize('precision', ['bf16', 'f16'])
def test_refused_arguments_return_einval_before_anything_touches_hip(precision):
  """The checks come before the first HIP call, so they run without a device:
  the pointers are never followed."""
  lib = _lib.load(precision)
  assert lib.cg_abi_version() == 20
  P = 1 << 20   # a 16-byte aligned address nobody reads
  MAXW = 2**26 - 1

  def pack(x=P, B=2, T=50, C=17, bin=12, out=P + 4096, stride=None):
    wpt = -(-(T // bin) // 32) if 0 < bin <= T else 1
    return lib.cg_binary_words(x, B, T, C, T * C, C, 1, bin, out,
                               B * wpt if stride is None else stride, None)

  def count(w=P, C=102, W=100, stride=None, singles=P + 64, pairs=P + 128,
            triplets=P + 256, ws=P + 512):
    return lib.cg_triplet_counts(w, C, W, W if stride is None else stride,
                                 singles, pairs, triplets, ws, None)

  for kw in (dict(x=None), dict(out=None), dict(out=P + 8), dict(out=P + 4),
             dict(B=0), dict(B=-1), dict(T=0), dict(bin=0), dict(bin=-2),
             dict(T=11), dict(C=2), dict(C=0), dict(C=513), dict(stride=1),
             dict(stride=-5),
             # 2^21 trials of 33 bins: 2 words a trial, 2^22 words fit; of 1025
             # bins: 33 a trial, 33 2^21 > 2^26 - 1
             dict(B=1 << 21, T=1025, bin=1)):
    assert pack(**kw) == _lib.CG_EINVAL, kw
  # the plan: 16^3 int32 a tile triple and split; 84 triples at C = 102, split
  # while that leaves fewer than 2048 workgroups, over at most 64 and at most
  # the 64-word chunks
  ws = lib.cg_triplet_counts_ws_bytes
  assert ws(102, 1) == ws(3, 64) == 16          # one split: nothing staged
  assert ws(5, 5000) == 40 * 1 * 4096 * 4       # 79 chunks, two a split
  assert ws(102, 2668) == 21 * 84 * 4096 * 4    # 42 chunks, 25 wanted
  assert ws(512, 11000) == 16                   # 5984 triples: no split
  assert ws(512, MAXW) == 16 and ws(3, MAXW) == 64 * 4096 * 4
  for C, W in ((2, 10), (513, 10), (0, 10), (-1, 10), (102, 0), (102, -1),
               (102, MAXW + 1)):
    assert ws(C, W) == -1, (C, W)
    assert count(C=C, W=W, stride=MAXW + 1) == _lib.CG_EINVAL, (C, W)
  for kw in (dict(w=None), dict(ws=None), dict(singles=None), dict(pairs=None),
             dict(triplets=None), dict(w=P + 8), dict(ws=P + 520),
             dict(singles=P + 66), dict(pairs=P + 129), dict(triplets=P + 258),
             dict(stride=99), dict(stride=0), dict(stride=-100)):
    assert count(**kw) == _lib.CG_EINVAL, kw


# -- compute_metrics.py ------------------------------------------------------------
def _args(path, *more):
  return ['--output_dir', str(path), '--num_processors', '1', '--verbose', '0',
          '--device', 'cpu'] + list(more)


def test_compute_metrics_triplet_flag_on_the_host(tmp_path, capsys):
  fake, real_spikes, fake_spikes = TC.run_dir(tmp_path)
  plain = cm.build_parser().parse_args(_args(tmp_path))
  for name in ('triplet_metrics', 'triplet_bin'):
    assert not hasattr(plain, name)
  before = cm.main(plain)[0]
  assert set(before) == PLAIN_KEYS
  assert 'triplets' not in json.load(open(tmp_path / 'spike_metrics.json'))['0']
  hp = cm.build_parser().parse_args(_args(tmp_path, '--triplet_metrics'))
  assert hp.triplet_metrics is True
  report = cm.main(hp)[0]
  assert set(report) == PLAIN_KEYS | {'triplets'}

  def rest(r):
    return json.dumps({k: v for k, v in r.items()
                       if k not in ('triplets', 'elapse')}, sort_keys=True)

  assert rest(report) == rest(before)
  s = report['triplets']
  assert set(s) == {'generated', 'floor', 'bin_frames'}
  assert s['bin_frames'] == 12
  assert TC.same(s, TC.expected_report(real_spikes, fake_spikes))
  assert s['floor']['num_states'] == s['generated']['num_states'] == [480, 480]
  assert s['floor']['num_triplets'] == 35
  assert s['floor']['triplets_observed'][0] > 0.9
  assert not TC.same(s['generated'], s['floor'])
  assert TC.same(json.load(open(tmp_path / 'spike_metrics.json'))['0']['triplets'], s)
  # the recorded side is kept on hparams for the next epoch
  ref, floor, frames = hp._recorded_triplets
  assert ref[3] == 480 and frames == 480 and TC.same(floor, s['floor'])
  # --triplet_bin is honoured
  hp2 = cm.build_parser().parse_args(
      _args(tmp_path, '--triplet_metrics', '--triplet_bin', '5'))
  s2 = cm.main(hp2)[0]['triplets']
  assert TC.same(s2, TC.expected_report(real_spikes, fake_spikes, bin=5))
  assert s2['floor']['num_states'] == [12 * 96, 12 * 96]
  # verbose: the two figures beside their floor
  hp3 = cm.build_parser().parse_args(_args(tmp_path, '--triplet_metrics'))
  hp3.verbose = 1
  capsys.readouterr()
  cm.main(hp3)
  out = capsys.readouterr().out
  for name in ('correlation', 'mae'):
    key = 'triplet_cumulant_' + name
    assert 'triplet cumulant {:<11}  gen | floor: {:.06f} | {:.06f}'.format(
        name, s['generated'][key], s['floor'][key]) in out
  # a generated file of another length is refused, as the other reports do
  hp._recorded_triplets = (ref, floor, 256)
  with pytest.raises(ValueError, match='480 frames'):
    cm.triplet_report(hp, fake, cm.triplet_sets_host)
  # a bin longer than the trials
  with pytest.raises(ValueError, match='no bin'):
    cm.main(cm.build_parser().parse_args(
        _args(tmp_path, '--triplet_metrics', '--triplet_bin', '481')))


def test_compute_metrics_refuses_fewer_than_three_neurons(tmp_path):
  TC.run_dir(tmp_path, trials=6, C=2)
  with pytest.raises(ValueError, match='three neurons'):
    cm.main(cm.build_parser().parse_args(_args(tmp_path, '--triplet_metrics')))
