"""CPU tests of the device Victor-Purpura distances (csrc/victor_purpura.hip):
the numpy statement the kernel is tested against -- the dynamic programme on the
frame grid, all pairs of a trial in one sweep over the anti-diagonals -- equals
closed forms bit for bit and the existing pair loop to a stated rounding bound;
the C ABI carries the two entry points, invalid arguments launch nothing, and
compute_metrics.py --victor_purpura adds exactly one key to the report."""
import ctypes
import json
import os
import pickle
import re

import numpy as np

import compute_metrics as cm
from calciumgan_amd import _lib
from calciumgan_amd import build as cg_build
from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import h5_helper, spike_metrics
from van_rossum_cases import dg_trial
from victor_purpura_cases import (GRID_CASES, QS, ROW_SLOTS, counts_difference,
                                  crafted_trial, double_loop_pair, first_set,
                                  grid_case, pair_count, second_set,
                                  unmatched_spikes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'calciumgan_hip.h')
NEW = ('cg_victor_purpura', 'cg_victor_purpura_ws_bytes')
U = 2.0**-53
vp = spike_metrics.victor_purpura_distance_frames


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_statement_against_the_pair_loop_in_seconds():
  """Per element within 3 (n_i + n_j) 2^-53 D_ij of victor_purpura_distance:
  one rounded product, one rounded time difference and one rounded sum per step
  of a path of at most n_i + n_j steps."""
  worst = 0.0
  for name, sp in (('first', first_set()), ('second', second_set())):
    n = sp.sum(1).astype(np.float64)
    for q in QS:
      want = spike_metrics.victor_purpura_distance(sp, q=q)
      got = vp(sp, q=q)
      assert got.dtype == np.float64 and got.shape == want.shape
      bound = 3 * (n[:, None] + n[None, :]) * U * want
      err = np.abs(got - want)
      ok = bound > 0
      frac = float((err[ok] / bound[ok]).max())
      print('%s q=%g: largest relative difference %.3g, worst fraction of the '
            'bound %.3g' % (name, q, float((err[ok] / want[ok]).max()), frac))
      assert np.all(err <= bound), (name, q, frac)
      worst = max(worst, frac)
  assert worst <= 1.0


def test_closed_forms_hold_exactly():
  for sp in (first_set(), second_set(), crafted_trial()):
    assert np.array_equal(vp(sp, q=0.0), counts_difference(sp))
    assert spike_metrics.victor_purpura_cost(48.0) == 2.0
    for q in (48.0, 1000.0):
      assert np.array_equal(vp(sp, q=q), unmatched_spikes(sp))


def test_symmetry_diagonal_triangle_inequality_and_cross_block():
  for sp in (first_set(), second_set()):
    for q in QS:
      d = vp(sp, q=q)
      assert np.array_equal(_bits(d), _bits(d.T))
      assert np.all(np.diag(d) == 0) and np.all(d >= 0)
      # d_ij <= d_ik + d_kj for every k
      through = (d[:, :, None] + d.T[None, :, :]).min(axis=1)
      assert np.all(d <= through + 1e-12)
  sp = first_set()
  assert vp(sp)[2, 3] == 0 and vp(sp)[0, 1] == 96    # identical; silent vs full
  full = vp(sp)
  a, b = sp[:3], sp[3:]
  cross = vp(a, b)
  assert cross.shape == spike_metrics.victor_purpura_distance(a, b).shape
  assert np.array_equal(_bits(cross), _bits(full[len(a):, :len(b)]))


def test_known_answers():
  """The four of test_van_rossum_and_victor_purpura_known_answers, to 1 ulp."""
  T = 24 * 20
  a, b, c, e, far = (np.zeros(T, np.float32) for _ in range(5))
  a[24] = 1
  b[24 + 12] = 1
  c[[24, 24 * 10]] = 1
  far[24 * 15] = 1
  d = vp(np.stack([a, b, c, e]))
  for got, want in ((d[0, 1], 0.5), (d[0, 3], 1.0), (d[0, 2], 1.0),
                    (vp(np.stack([a, far]))[0, 1], 2.0)):
    assert abs(got - want) <= np.spacing(want)
  # one train alone, and silent trains alone
  assert np.array_equal(vp(a[None]), np.zeros((1, 1)))
  assert np.array_equal(vp(np.zeros((3, 5), np.float32)), np.zeros((3, 3)))


def test_statement_runs_a_whole_trial_at_the_flagship_shape():
  sp = dg_trial(102, 2048)
  d = vp(sp)
  assert d.shape == (102, 102) and np.array_equal(_bits(d), _bits(d.T))
  n = sp.sum(1).astype(np.float64)
  # between |n_i - n_j| (shifts free) and n_i + n_j - 2 |f_i & f_j| (no shifts)
  assert np.all(d >= counts_difference(sp)) and np.all(d <= unmatched_spikes(sp))
  few = np.argsort(n)[:4]
  want = spike_metrics.victor_purpura_distance(sp[few])
  got = d[np.ix_(few, few)]
  assert np.all(np.abs(got - want) <= 3 * (n[few][:, None] + n[few][None, :]) *
                U * want)


def test_grid_cases_are_what_their_names_say():
  shapes = {n: grid_case(n).shape for n in GRID_CASES}
  assert shapes == {'reuse_3x96x102': (3, 96, 102), 'reuse_40x48x27': (40, 48, 27),
                    'long_1x2048x6': (1, 2048, 6),
                    't16384_1x16384x3': (1, 16384, 3),
                    'dg_2x2048x102': (2, 2048, 102),
                    'decode_1x4x4096': (1, 4, 4096)}
  for name in GRID_CASES:
    sp = grid_case(name)
    assert sp.dtype == np.float32 and set(np.unique(sp)) <= {0.0, 1.0}
  sp = grid_case('reuse_3x96x102')
  assert pair_count(sp) == 15453 and pair_count(sp) - ROW_SLOTS == 7261
  n = sp.sum(1)
  assert np.all((n == 0).sum(1) >= 1) and np.all((n == 96).sum(1) >= 1)
  # most pairs need two to six strips of 16 columns of the shorter train
  I, J = np.triu_indices(102, k=1)
  strips = (np.minimum(n[:, I], n[:, J]) + 15) // 16
  assert ((strips >= 2) & (strips <= 6)).mean() > 0.5
  sp = grid_case('reuse_40x48x27')
  assert pair_count(sp) == 14040 > ROW_SLOTS and (27 * 26 // 2) % 4 != 0
  assert pair_count(grid_case('dg_2x2048x102')) == 10302 > ROW_SLOTS
  assert pair_count(grid_case('decode_1x4x4096')) == 8386560
  sp = grid_case('t16384_1x16384x3')[0]
  assert sp[0, 0] == 1 and sp[16383, 0] == 1 and sp[16383, 2] == 1
  assert sp[255, 1] == 1 and sp[256, 1] == 1 and sp[256, 2] == 1
  assert np.all(np.abs(sp.mean(0) - 0.02) < 0.005)


# (case, trial, i, j): a handful of pairs per case for the plain double loop --
# silent / full / ordinary trains, the last pair of a trial, and the longest
# pair of the long-train case (2048 against 1024 spikes, 2 M cells)
LOOP_PAIRS = (
    ('reuse_3x96x102', 0, 0, 1), ('reuse_3x96x102', 0, 1, 2),
    ('reuse_3x96x102', 1, 37, 90), ('reuse_3x96x102', 2, 100, 101),
    ('reuse_40x48x27', 0, 0, 1), ('reuse_40x48x27', 23, 12, 26),
    ('reuse_40x48x27', 39, 25, 26),
    ('long_1x2048x6', 0, 0, 1), ('long_1x2048x6', 0, 1, 3),
    ('long_1x2048x6', 0, 3, 4), ('long_1x2048x6', 0, 0, 5),
    ('t16384_1x16384x3', 0, 0, 1), ('t16384_1x16384x3', 0, 1, 2),
    ('dg_2x2048x102', 0, 3, 77), ('dg_2x2048x102', 1, 100, 101),
    ('decode_1x4x4096', 0, 0, 4095), ('decode_1x4x4096', 0, 2047, 2048),
)


def test_statement_against_the_plain_double_loop_on_the_grid_cases():
  """Bit for bit: the double loop performs the statement's operations."""
  qf = spike_metrics.victor_purpura_cost(1.0)
  for name, b, i, j in LOOP_PAIRS:
    trial = grid_case(name)[b].T                       # (C, T)
    got = vp(trial[[i, j]])
    want = double_loop_pair(trial[i], trial[j], qf)
    assert _bits(got[0, 1]) == _bits(want) and _bits(got[1, 0]) == _bits(want), (
        name, b, i, j, got[0, 1], want)
  # the whole trial gives the pair what the two trains alone give it
  trial = grid_case('reuse_3x96x102')[1].T
  assert _bits(vp(trial)[37, 90]) == _bits(
      double_loop_pair(trial[37], trial[90], qf))
  # and the longest pair is worth running: its distance is no count difference
  long_ = grid_case('long_1x2048x6')[0].T
  assert vp(long_[:2])[0, 1] == 1024.0
  assert vp(long_[[1, 2]])[0, 1] > abs(long_[1].sum() - long_[2].sum())


def test_closed_forms_on_a_slice_of_the_decode_case():
  sp = grid_case('decode_1x4x4096')[0].T[:64]         # (64, 4)
  assert np.array_equal(_bits(vp(sp, q=0.0)), _bits(counts_difference(sp)))
  want = unmatched_spikes(sp)
  assert np.array_equal(want, np.rint(want))
  assert np.array_equal(_bits(vp(sp, q=1000.0)), _bits(want))
  # the whole case: the forms hold small integers only
  full = grid_case('decode_1x4x4096')[0].T
  for form in (counts_difference(full), unmatched_spikes(full)):
    assert form.shape == (4096, 4096) and np.array_equal(form, np.rint(form))
    assert form.min() == 0 and form.max() <= 8


def test_header_signatures_and_both_libraries_carry_the_entry_points():
  cg_build.build(verbose=False)
  src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
  declared = set(re.findall(r'\b(?:int|long long)\s+(cg_\w+)\s*\(', src))
  assert 'victor_purpura.hip' in cg_build.SOURCES
  for name in NEW:
    assert name in declared, name
    assert name in _lib.SIGNATURES, name
  for precision in ('bf16', 'f16'):
    lib = _lib.load(precision)
    for name in NEW:
      assert hasattr(lib, name), (precision, name)
    assert lib.cg_abi_version() == 20
  assert '#define CG_ABI_VERSION 20' in open(HEADER).read()


def test_nothing_is_launched_for_invalid_arguments():
  """(host-side argument checks: they return before any HIP call)"""
  lib = _lib.load()
  p = ctypes.c_void_p(0x1000)
  E = _lib.CG_EINVAL
  need = lib.cg_victor_purpura_ws_bytes

  def call(spikes=p, B=2, T=48, C=6, qf=1.0 / 24, dist=p, ws=p, ws_bytes=None):
    if ws_bytes is None:
      ws_bytes = max(need(B, T, C), 0)
    return lib.cg_victor_purpura(spikes, B, T, C, T * C, C, 1, qf, dist, ws,
                                 ws_bytes, None)

  assert call(spikes=None) == E and call(dist=None) == E and call(ws=None) == E
  assert call(B=0) == E and call(T=0) == E and call(C=0) == E
  assert call(B=-1) == E and call(T=-3) == E and call(C=-2) == E
  assert call(qf=-1e-9) == E and call(qf=float('nan')) == E
  assert call(ws_bytes=need(2, 48, 6) - 1) == E and call(ws_bytes=0) == E
  assert call(ws=ctypes.c_void_p(0x1004)) == E      # 8-byte alignment
  # the documented limits: B <= 65536, T <= 16384, C <= 4096
  big = 1 << 62
  assert call(B=65537, ws_bytes=big) == E
  assert call(T=16385, ws_bytes=big) == E
  assert call(C=4097, ws_bytes=big) == E


def test_workspace_size():
  need = _lib.load().cg_victor_purpura_ws_bytes
  for shape in ((0, 48, 6), (2, 0, 6), (2, 48, 0), (-1, 48, 6), (65537, 48, 6),
                (2, 16385, 6), (2, 48, 4097)):
    assert need(*shape) == -1, shape
  # at least the limits the interface promises
  assert need(1, 4096, 512) > 0 and need(65536, 16384, 4096) > 0
  base = (4, 96, 7)
  for axis in range(3):
    sizes = []
    for step in range(6):
      shape = list(base)
      shape[axis] += step
      sizes.append(need(*shape))
    assert all(a < b for a, b in zip(sizes, sizes[1:])), (axis, sizes)
  # frames (uint16, pitch T) and counts of every train, and at least one
  # boundary column of T + 1 float64
  B, T, C = 128, 2048, 102
  assert need(B, T, C) >= B * C * (2 * T + 4) + 8 * (T + 1)
  assert need(1, 1, 1) > 0


def test_compute_metrics_flags_parse():
  p = cm.build_parser()
  d = p.parse_args([])
  assert not hasattr(d, 'victor_purpura') and not hasattr(d, 'vp_q')
  a = p.parse_args(['--victor_purpura', '--vp_q', '2'])
  assert a.victor_purpura is True and a.vp_q == 2.0
  assert p.parse_args(['--victor_purpura']).victor_purpura is True


def test_report_gains_one_key_with_the_flag(tmp_path):
  """The run directory of test_recorded_data_metrics_report."""
  d = dg.make_dataset(num_neurons=6, sequence_length=480, num_segments=24)
  gen_dir = tmp_path / 'generated'
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
            open(tmp_path / 'hparams.json', 'w'))
  base = ['--output_dir', str(tmp_path), '--num_processors', '1', '--verbose', '0']
  today = {'firing_rate_kl', 'correlation_kl', 'van_rossum_heatmap_min',
           'van_rossum_kl', 'elapse'}
  plain = cm.main(cm.build_parser().parse_args(base))[0]
  assert set(plain) == today
  written = json.load(open(tmp_path / 'spike_metrics.json'))
  assert set(written['0']) == today
  hp = cm.build_parser().parse_args(base + ['--victor_purpura'])
  r = cm.main(hp)[0]
  assert set(r) == today | {'victor_purpura_kl'}
  assert set(r['victor_purpura_kl']) == {'mean'}
  assert np.isfinite(r['victor_purpura_kl']['mean'])
  for key in today - {'elapse'}:
    assert r[key] == plain[key], key
  written = json.load(open(tmp_path / 'spike_metrics.json'))
  assert written['0']['victor_purpura_kl'] == r['victor_purpura_kl']
  # the samples behind the figure are the statement's upper triangles
  real, synth = cm.trial_victor_purpura(hp, fake, 3)
  want = vp(cm._spikes(hp, fake, 'CW', trial=3))
  assert np.array_equal(_bits(synth), _bits(want[np.triu_indices(6, k=1)]))
  assert real.shape == synth.shape == (15,)
  # another cost per second gives another sample
  hq = cm.build_parser().parse_args(base + ['--victor_purpura', '--vp_q', '12'])
  cm.main(hq)
  assert np.array_equal(
      _bits(cm.trial_victor_purpura(hq, fake, 3)[1]),
      _bits(vp(cm._spikes(hq, fake, 'CW', trial=3), q=12.0)[np.triu_indices(6, k=1)]))
  # identical spike sets score exactly 0
  h5_helper.overwrite(fake, 'spikes', d['spikes'].astype(np.int8))
  z = cm.main(hp)[0]
  assert z['victor_purpura_kl']['mean'] == 0 and z['van_rossum_kl']['mean'] == 0
