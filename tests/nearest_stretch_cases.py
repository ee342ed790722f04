"""The shared case table of the nearest-stretch tests
(tests/test_nearest_stretch_host.py, tests/test_hip_nearest_stretch.py): seeded
queries (N, L, C) and recordings (T_raw, C) as read-only float32 numpy arrays
with the memory layouts the device test gives them, the statement
(signals_metrics.nearest_stretch, direct difference form) computed once per
case, and `check`, the bar every result is held to.

The bar is derived, not tuned.  Recursive float64 summation of K exact terms
errs by at most K 2^-53 sum |terms| (any order of the additions).  The expanded
form's terms are q^2, r^2 and 2 q r with sum |2 q r| <= |q|^2 + W, so it is
within 2 K 2^-53 (|q_n|^2 + W_j) of the exact value; the direct form's terms are
(q - r)^2 <= 2 (q^2 + r^2), the same figure.  Hence
  |d2 - d2_stmt| <= 4 K 2^-53 (|q_n|^2 + W_j) =: bar[n][j]
for the device as well as for the numpy expanded form.  With i the result's
index and s the statement's:
  -bar[n][i] <= nearest - nearest_stmt <= bar[n][s]
    (nearest <= d2[n][s] <= stmt + bar[n][s];
     nearest = d2[n][i] >= d2_stmt[n][i] - bar[n][i] >= stmt - bar[n][i])
  d2_stmt[n][i] <= nearest_stmt + min(bar[n][i], bar[n][s])
and the result is held to itself: index admitted, nearest the bits of d2 at it,
and no admitted lower d2 -- or an equal one at a lower offset -- in its own
profile.  On `exact` cases (small integer samples: every product and sum is
exact in float64) d2, nearest and index equal the statement bit for bit.

Shapes are the smallest at which each mechanism of csrc/nearest_stretch.hip can
break; `plan` mirrors its ns_plan.  A workgroup owns 128 queries (32 per wave,
two row tiles of 16) x 64 offsets x one split of K; K is walked in steps of 16,
in chunks of at most 512 steps or what 18432 floats of LDS leave beside the
63 step C floats of the tile's span; the finish pass owns segments of 1024
offsets.  So: N = 1, 16, 17 (a second row tile), 33 (a second wave), 130 (a
second query tile); S = 1, 63, 64, 65, 257 and 1025 (a second segment); K = 15,
16 and 17 (the tail of a step), one split and sixteen, a split of two chunks
(130 steps at a chunk of 128), step C = 291 (the last staged span, chunks of 6
steps) and 292 and 306 (the recording read from global memory); steps 1, 2, 3
and 4 with a T_raw - L the step does not divide; contiguous, row-padded and
permuted layouts of both operands, and query rows at odd 4-byte offsets (K = 15
contiguous) for the 16-byte loads."""
import functools
import json
import os
import pickle

import numpy as np

from calciumgan_amd.data import dg, recording
from calciumgan_amd.gan.utils import h5_helper, signals_metrics

U = 2.0 ** -53
TILE_N, TILE_S, GROUP = 128, 64, 16   # csrc/nearest_stretch.hip: kNsTileN, ...
LDS_FLOATS = 18432                    # kNsLdsFloats
MIN_CHUNK, MAX_CHUNK = 4, 512         # kNsMinChunk, kNsMaxChunk
MAX_SPLITS, MIN_SPLIT_STEPS = 16, 64  # kNsMaxSplits, kNsMinSplitSteps
UNITS = 256                           # kNsUnits
SEGMENT = 1024                        # kNsSegment


def offsets(T_raw, L, step):
  return (T_raw - L) // step + 1


def plan(N, L, C, T_raw, step):
  """csrc/nearest_stretch.hip: ns_plan, as a dict."""
  S = offsets(T_raw, L, step)
  tiles_s, tiles_n = (S - 1) // TILE_S + 1, (N - 1) // TILE_N + 1
  steps = (L * C - 1) // GROUP + 1
  span = (TILE_S - 1) * step * C
  staged = span + MIN_CHUNK * GROUP <= LDS_FLOATS
  chunk = min(MAX_CHUNK, (LDS_FLOATS - span) // GROUP) if staged else MAX_CHUNK
  most = min((steps - 1) // MIN_SPLIT_STEPS + 1, MAX_SPLITS)
  tiles = tiles_s * tiles_n
  cost = {s: ((tiles * s - 1) // UNITS + 1) / s for s in range(1, most + 1)}
  splits = next(s for s in range(1, most + 1)
                if cost[s] <= 1.03 * min(cost.values()))
  split_steps = (steps - 1) // splits + 1
  splits = (steps - 1) // split_steps + 1
  return dict(S=S, S_pad=tiles_s * TILE_S, tiles_s=tiles_s, tiles_n=tiles_n,
              steps=steps, staged=staged, splits=splits,
              split_steps=split_steps, chunk_steps=min(chunk, split_steps),
              segments=(S - 1) // SEGMENT + 1)


def ws_doubles(N, L, C, T_raw, step):
  """The workspace of cg_nearest_stretch in float64 elements: ns_layout."""
  p = plan(N, L, C, T_raw, step)
  return (N + T_raw + p['S'] + N * p['segments'] + (N * p['segments'] + 1) // 2
          + p['splits'] * N * p['S_pad'])


def _normal(shape, seed):
  return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def _integers(shape, seed):
  return np.random.RandomState(seed).randint(-4, 5, size=shape).astype(
      np.float32)


def _cut(R, L, starts):
  return np.stack([R[v:v + L] for v in starts])


def _random_case(N, L, C, T_raw, step, seed, exact=False, **kw):
  """N queries: stretches of the recording at any row plus noise (so the
  minimum is somewhere meaningful), or independent integers when exact."""
  def build():
    rng = np.random.RandomState(seed + 1)
    if exact:
      R = _integers((T_raw, C), seed)
      Q = _integers((N, L, C), seed + 2)
    else:
      R = _normal((T_raw, C), seed)
      starts = rng.randint(0, T_raw - L + 1, size=N)
      Q = _cut(R, L, starts) + np.float32(0.5) * _normal((N, L, C), seed + 2)
    return dict(Q=Q.astype(np.float32), R=R, step=step, exact=exact, **kw)
  return build


def _periodic():
  """A recording of period 6 rows under step 2: every query cut from it is at
  distance 0 from a third of the offsets, and the lowest wins."""
  def build():
    L, C, T_raw, step = 7, 3, 61, 2
    R = np.tile(_integers((6, C), 31), (11, 1))[:T_raw]
    starts = [0, 4, 8, 14, 54, 26]
    return dict(Q=_cut(R, L, starts), R=R, step=step, exact=True, starts=starts)
  return build


def _cut_from_recording():
  """Integer recording, queries cut on the offset grid (distance 0 exactly at
  their start) and one row off it."""
  def build():
    L, C, T_raw, step = 9, 4, 300, 3
    R = _integers((T_raw, C), 41)
    starts = [0, 3, 150, 291, 151, 290]
    return dict(Q=_cut(R, L, starts), R=R, step=step, exact=True, starts=starts)
  return build


def _excluded(exclude, exclude_len, seed=51):
  """Integer recording of 27 offsets at step 2 (rows 0 .. 52), 6 queries cut
  from it on the grid."""
  def build():
    L, C, T_raw, step = 5, 3, 58, 2
    R = _integers((T_raw, C), seed)
    starts = [0, 52, 20, 0, 52, 26]
    assert offsets(T_raw, L, step) == 27
    return dict(Q=_cut(R, L, starts), R=R, step=step, exact=True,
                exclude=np.array(exclude, np.int32), exclude_len=exclude_len,
                starts=starts)
  return build


# name -> builder of dict(Q, R, step, exact[, exclude, exclude_len, q_layout,
# r_layout]); layouts: 'contig', 'padded' (a row pitch > C), 'permuted' (the
# time axis innermost in memory)
_TABLE = {
    # N and S edges at K = 15 (one step with a tail; one split, one chunk)
    'n1_s1_k15': _random_case(1, 5, 3, 5, 1, 1),
    'n16_s63_k15': _random_case(16, 5, 3, 67, 1, 2),
    'n17_s64_k15_step2': _random_case(17, 5, 3, 132, 2, 3),
    'n33_s65_k15_step3': _random_case(33, 5, 3, 199, 3, 4),
    'n130_s257_k15_step2': _random_case(130, 5, 3, 518, 2, 5),
    'n3_s1025_k15': _random_case(3, 5, 3, 1029, 1, 6),
    'n5_s70_c1_k16': _random_case(5, 16, 1, 85, 1, 7),
    'n5_s70_c1_k17_step2': _random_case(5, 17, 1, 156, 2, 8),
    # the report's row width
    'n17_s71_l64_c102_step2': _random_case(17, 64, 102, 205, 2, 9),
    'n17_s47_l64_c102_step3_unstaged': _random_case(17, 64, 102, 204, 3, 10),
    'n17_s257_l512_c102_step2': _random_case(17, 512, 102, 1024, 2, 11),
    # a split of two chunks: 130 steps at a chunk of 128
    'n17_s71_l256_c130_step2_two_chunks': _random_case(17, 256, 130, 397, 2, 12),
    # the last staged span and the first unstaged one
    'n4_s70_l8_c97_step3_chunks_of_6': _random_case(4, 8, 97, 216, 3, 13),
    'n4_s70_l8_c73_step4_unstaged': _random_case(4, 8, 73, 286, 4, 14),
    # layouts
    'padded_q': _random_case(17, 6, 5, 80, 2, 15, q_layout='padded'),
    'permuted_q': _random_case(17, 6, 5, 80, 2, 16, q_layout='permuted'),
    'padded_r': _random_case(17, 6, 5, 80, 2, 17, r_layout='padded'),
    'permuted_r': _random_case(17, 6, 5, 80, 2, 18, r_layout='permuted'),
    'permuted_both_l64_c102': _random_case(
        18, 64, 102, 205, 2, 19, q_layout='permuted', r_layout='permuted'),
    'padded_both_unstaged': _random_case(
        4, 8, 73, 286, 4, 20, q_layout='padded', r_layout='padded'),
    # exact data
    'exact_n17_s65_k15': _random_case(17, 5, 3, 133, 2, 21, exact=True),
    'exact_l64_c102_step2': _random_case(18, 64, 102, 205, 2, 22, exact=True),
    'exact_l512_c102_step2': _random_case(3, 512, 102, 1024, 2, 23, exact=True),
    'exact_unstaged': _random_case(4, 8, 73, 286, 4, 24, exact=True),
    'exact_permuted_r': _random_case(5, 6, 5, 80, 2, 25, exact=True,
                                     r_layout='permuted'),
    'exact_periodic': _periodic(),
    'exact_cut_from_recording': _cut_from_recording(),
    # exclusion: bands at row 0 and at the last offset, -1 mixed in; a band
    # that leaves one offset; one that leaves none; exclude_len = 0
    'exclude_bands_at_both_ends': _excluded([0, 52, 20, -1, -1, 26], 5),
    'exclude_leaves_one': _excluded([0, 52, 20, 1, -1, 26], 52),
    'exclude_leaves_none': _excluded([26, 52, 20, -1, 0, 25], 53),
    'exclude_len_zero': _excluded([0, 52, 20, -1, -1, 26], 0),
}
CASES = tuple(_TABLE)


@functools.lru_cache(maxsize=None)
def case(name):
  """dict(Q (N, L, C), R (T_raw, C), step, exact, exclude, exclude_len,
  q_layout, r_layout[, starts]) of a case; the arrays read-only."""
  c = dict(exclude=None, exclude_len=0, q_layout='contig', r_layout='contig')
  c.update(_TABLE[name]())
  for key in ('Q', 'R', 'exclude'):
    if c[key] is not None:
      c[key] = np.ascontiguousarray(c[key])
      c[key].setflags(write=False)
  return c


def shape(name):
  """(N, L, C, T_raw, step) of a case."""
  c = case(name)
  return c['Q'].shape + (c['R'].shape[0], c['step'])


def statement(c):
  """dict(nearest, index, d2, bar) of a case dict: the direct form and
  bar[n][j] = 4 K 2^-53 (|q_n|^2 + W_j)."""
  nearest, index, d2 = signals_metrics.nearest_stretch(
      c['Q'], c['R'], c['step'], c['exclude'], c['exclude_len'],
      return_profile=True)
  N, L, C = c['Q'].shape
  q64, r64 = c['Q'].astype(np.float64), c['R'].astype(np.float64)
  with np.errstate(invalid='ignore', over='ignore'):
    q2 = (q64 * q64).sum(axis=(1, 2))
    rows = (r64 * r64).sum(axis=1)
    w = np.array([rows[j * c['step']:j * c['step'] + L].sum()
                  for j in range(d2.shape[1])])
    bar = 4.0 * L * C * U * (q2[:, None] + w[None, :])
  for a in (nearest, index, d2, bar):
    a.setflags(write=False)
  return dict(nearest=nearest, index=index, d2=d2, bar=bar)


@functools.lru_cache(maxsize=None)
def reference(name):
  return statement(case(name))


def admitted(c, S):
  """bool (N, S): the offsets exclusion leaves query n."""
  N = c['Q'].shape[0]
  ok = np.ones((N, S), bool)
  if c['exclude'] is not None:
    s = np.arange(S, dtype=np.int64) * c['step']
    ex = c['exclude'].astype(np.int64)
    ok &= ~((ex[:, None] >= 0) &
            (np.abs(s[None, :] - ex[:, None]) < c['exclude_len']))
  return ok


def check(d2, nearest, index, name, ref=None, what='device'):
  """Holds a result to the statement (the module docstring); d2 may be None.
  `name` is a case name or a case dict (then `ref` is its `statement`).
  Returns the largest err / bar seen (0 where everything is exact)."""
  c = case(name) if isinstance(name, str) else name
  ref = reference(name) if ref is None else ref
  N, L, C = c['Q'].shape
  S = ref['d2'].shape[1]
  nearest = np.asarray(nearest, dtype=np.float64)
  index = np.asarray(index).astype(np.int64)
  assert nearest.shape == (N,) and index.shape == (N,)
  ok = admitted(c, S)
  worst = 0.0
  defined = ref['index'] >= 0
  assert ((index >= 0) == defined).all(), (what, index, ref['index'])
  assert np.isnan(nearest[~defined]).all() and (index[~defined] == -1).all()
  assert np.isfinite(nearest[defined]).all()
  assert ((index[defined] >= 0) & (index[defined] < S)).all()
  rows = np.flatnonzero(defined)
  i_d, i_s = index[rows], ref['index'][rows]
  assert ok[rows, i_d].all(), 'an excluded offset was chosen'
  if d2 is not None:
    d2 = np.asarray(d2, dtype=np.float64)
    assert d2.shape == (N, S)
    finite = np.isfinite(ref['d2'])
    assert (np.isfinite(d2) == finite).all() and np.isnan(d2[~finite]).all()
    assert (d2[finite] >= 0).all()
    # the result against its own profile: the least admitted value, lowest offset
    cand = np.where(ok & finite, d2, np.inf)
    assert (cand.argmin(axis=1)[rows] == i_d).all(), what
    assert nearest[rows].tobytes() == d2[rows, i_d].tobytes(), what
  if c['exact']:
    assert nearest.tobytes() == ref['nearest'].tobytes(), what
    assert (index == ref['index']).all(), what
    if d2 is not None:
      assert d2.tobytes() == ref['d2'].tobytes(), what
    return 0.0
  bar = ref['bar']
  if d2 is not None:
    err = np.abs(d2 - ref['d2'])[finite]
    ratio = err / bar[finite]
    worst = float(ratio.max()) if ratio.size else 0.0
    assert (err <= bar[finite]).all(), (what, worst)
  diff = nearest[rows] - ref['nearest'][rows]
  assert (diff >= -bar[rows, i_d]).all() and (diff <= bar[rows, i_s]).all(), what
  if rows.size:
    worst = max(worst, float(np.max(np.where(
        diff < 0, -diff / bar[rows, i_d], diff / bar[rows, i_s]))))
  slack = np.minimum(bar[rows, i_d], bar[rows, i_s])
  assert (ref['d2'][rows, i_d] <= ref['nearest'][rows] + slack).all(), what
  return worst


def run_dir(path, C=24, T_raw=1500, L=256, stride=2, trials=12, kind='copies',
            seed=21):
  """A run directory trained on a DG recording directory (`path`/dataset): the
  validation cache, hparams.json with input_dir, and one generated file of
  `trials` trials -- 'copies': stretches of the recording at multiples of four
  rows plus N(0, 0.01) noise; 'other': stretches of a recording of another seed.  (Trials
  of 256 frames: the report's KL figures need spikes in every trial.  24
  neurons: two DG recordings differ in every neuron's rate, and over 24 of them
  every stretch of the other one lies farther from this recording -- 0.529 ..
  0.586 per sample -- than any of its own stretches does from the rest of it,
  0.486 .. 0.516; with 6 neurons the two ranges overlap.)
  Returns (generated file, recording dict, generated signals)."""
  signals, spikes, _ = dg.make_recording(C, T_raw, seed=seed)
  rec = recording.build(signals, spikes, L, stride=stride, normalize=True,
                        validation_size=trials, seed=seed)
  input_dir = str(path / 'dataset')
  recording.write(input_dir, rec)
  raw = rec['raw']
  rng = np.random.RandomState(seed + 1)
  starts = 4 * rng.randint(0, (T_raw - L) // 4 + 1, size=trials)
  if kind == 'copies':
    gen = _cut(raw, L, starts) + np.float32(0.01) * _normal((trials, L, C),
                                                            seed + 2)
  else:
    other = dg.make_recording(C, T_raw, seed=seed + 100)[0]
    gen = _cut(np.ascontiguousarray(other.T), L, starts)
  gen = np.ascontiguousarray(gen, dtype=np.float32)
  gen_dir = path / 'generated'
  os.makedirs(gen_dir)
  val = str(gen_dir / 'validation.h5')
  vstarts = np.sort(rec['validation_starts'])
  h5_helper.write(val, {
      'signals': _cut(raw, L, vstarts),
      'spikes': _cut(rec['spikes'], L, vstarts).astype(np.int8)})
  fake = str(gen_dir / 'epoch000_signals.h5')
  h5_helper.write(fake, {'signals': gen})
  with open(gen_dir / 'info.pkl', 'wb') as f:
    pickle.dump({0: {'global_step': 1, 'filename': fake}}, f)
  with open(path / 'hparams.json', 'w') as f:
    json.dump(dict(generated_dir=str(gen_dir), validation_cache=val,
                   input_dir=input_dir, num_neurons=C, sequence_length=L), f)
  return fake, rec, gen
