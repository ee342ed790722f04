"""Float64 statements of the convolution weight gradient (cg_wgrad /
cg_wgrad_batched, calciumgan_amd/csrc/wgrad.hip) and of the operand packer
(cg_pack_weights / cg_pack_batched, swconv.hip), written from the comments of
include/calciumgan_hip.h, the error bar of the f32 K' contraction, and the data
recipes the parity tests of tests/test_hip_wgrad.py run them on.

Everything here is numpy float64 on the host.  tests/test_wgrad_ref.py ties each
statement to an independent one (float64 autograd of the oracle's convolutions
with its PhaseShuffle, hip_utils.numpy_pack) and checks on the CPU that the
recipes can tell a wrong kernel from a right one."""
from collections import namedtuple

import numpy as np

import pointwise_ref as R


# ---------------------------------------------------------------------------
# geometry of one launch
# ---------------------------------------------------------------------------
# shifts: tuple of ints (one per segment of seg samples) or None
Geom = namedtuple('Geom', 'nB Lu taps Cx Cg shifts seg')


def geom(nB, Lu, taps, Cx, Cg, shifts=None, seg=1):
  if shifts is not None:
    shifts = tuple(int(s) for s in shifts)
    assert len(shifts) == -(-nB // seg)
  return Geom(nB, Lu, taps, Cx, Cg, shifts, seg)


def stride_of(G):
  """(stride, Lx, off): taps 1 is the per-timestep Dense (stride 1), every other
  tap count the stride-2 'same' convolution over a long side of 2 Lu rows (left
  pad (taps - 2) // 2)."""
  if G.taps == 1:
    return 1, G.Lu, 0
  return 2, 2 * G.Lu, -((G.taps - 2) // 2)


def rows_of(G):
  return G.nB * G.Lu


# ---------------------------------------------------------------------------
# statements
# ---------------------------------------------------------------------------
def shuffle_src(t, s, w):
  """Source row of PhaseShuffle's reflect gather: out[t] = x[shuffle_src(t, s, w)]
  (|s| < w): s > 0 reads t + s, mirrored at w - 1; s <= 0 reads |t + s|."""
  t = np.asarray(t, np.int64)
  if s > 0:
    u = t + s
    return np.where(u < w, u, 2 * (w - 1) - u)
  return np.abs(t + s)


def shuffled(x, shifts, seg_size):
  """xs[b] = x[b][shuffle_src(., shifts[b // seg_size])], x (nB, Lx, C)."""
  x = np.asarray(x, np.float64)
  if shifts is None:
    return x
  out = np.empty_like(x)
  t = np.arange(x.shape[1])
  for b in range(x.shape[0]):
    out[b] = x[b, shuffle_src(t, int(shifts[b // seg_size]), x.shape[1])]
  return out


def _contract(X, G):
  """sum over the rows of X (n, cx) x G (n, cg) with IEEE semantics for
  non-finite values (an explicit loop nest: no library shortcut for zeros)."""
  if np.isfinite(X).all() and np.isfinite(G).all():
    return X.T @ G
  with np.errstate(invalid='ignore', over='ignore'):
    return np.einsum('nc,nd->cd', X, G)


def wgrad(x, g, taps, stride, off, shifts=None, seg_size=1, keep=None):
  """dw[tap][cx][cg] = sum_{b,u} xs[b, stride*u + off + tap, cx] * g[b, u, cg], x
  (nB, Lx, cx), g (nB, Lu, cg).  Rows outside [0, Lx) do not take part (selected
  away: a NaN in g meets no zero there).  keep: boolean (nB * Lu,) -- the (b, u)
  rows that take part (the mutants of tests/test_wgrad_ref.py)."""
  xs = shuffled(x, shifts, seg_size)
  g = np.asarray(g, np.float64)
  nB, Lx, cx = xs.shape
  Lu, cg = g.shape[1], g.shape[2]
  dw = np.zeros((taps, cx, cg))
  u = np.arange(Lu)
  kept = np.ones((nB, Lu), bool) if keep is None else np.asarray(keep).reshape(nB, Lu)
  for tap in range(taps):
    r = stride * u + off + tap
    ok = (r >= 0) & (r < Lx)
    sel = kept & ok[None, :]
    X = np.where(ok[None, :, None], xs[:, np.clip(r, 0, Lx - 1), :], 0.0)
    dw[tap] = _contract(X[sel], g[sel])
  return dw


def dbias(g, bias_rows):
  """sum of g over its first bias_rows (b, u) rows."""
  g = np.asarray(g, np.float64)
  with np.errstate(invalid='ignore'):
    return g.reshape(-1, g.shape[-1])[:bias_rows].sum(axis=0)


def flush(v, f16=True):
  """Subnormals of the activation type -> zero of the same sign."""
  v = np.asarray(v, np.float64)
  mn = 2.0**-14 if f16 else 2.0**-126
  return np.where(np.abs(v) < mn, np.copysign(0.0, v), v)


def wgrad_of(G, x, g, keep=None):
  stride, Lx, off = stride_of(G)
  return wgrad(x, g, G.taps, stride, off, G.shifts, G.seg, keep)


# ---------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------
def joins(G):
  """An upper count of the partial sums a launch joins, whatever its form: a K'
  split, an atomic, a flex slot or a ring stage set owns at least one tile of
  64 (b, u) rows (1-tap form: 256 rows, times its 8 waves)."""
  M = rows_of(G)
  return 8 * -(-M // 256) if G.taps == 1 else -(-M // 64)


def _gamma(k):
  u = 2.0**-23
  return k * u / (1 - k * u)


def acc_bound(G, x, g, P=None, start=0.0):
  """Error bar of dw as an f32 contraction over K' = nB Lu products joined from P
  partial sums onto `start` (the value the output held when the call ADDS):

      gamma(K' + P) (sum_{b,u} |xs g| + |start|),  gamma(k) = k u / (1 - k u), u = 2^-23.

  The operands are values of the activation type, so every product is exact in
  f32 (8 x 8 or 11 x 11 significand bits).  A sum of K' terms in ANY order is a
  tree of K' - 1 additions; splitting it into P partial sums that start from zero
  and are then added (to each other, or one by one onto `start`) adds at most P
  more.  Every addition rounds its result by at most one ulp <= u |result| (a
  truncating adder included), and every intermediate result is bounded by the
  sum of the magnitudes: the standard bound gamma(additions) x sum of magnitudes.
  Terms the statement selects away (padding rows, the rows of a ragged tile) are
  exact zeros in the kernel and add nothing.  Derived, not measured."""
  P = joins(G) if P is None else P
  mag = wgrad_of(G, np.abs(x), np.abs(g))
  return _gamma(rows_of(G) + P) * (mag + abs(start))


def dbias_bound(G, g, bias_rows, P=None, start=0.0):
  """The same bar for the column sums of g: bias_rows terms, P joins."""
  P = joins(G) if P is None else P
  return _gamma(bias_rows + P) * (dbias(np.abs(g), bias_rows) + abs(start))


# ---------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------
class PackDesc(object):
  """The fields of cg_pack_desc that define the layout (strides in elements of
  the flat f32 source)."""

  def __init__(self, taps, C_real, N_real, Cx, CK=32, tap0=0, tap_step=1, s_tap=None,
               s_c=None, s_n=1, parity_major=0, narrow_last=0):
    self.taps, self.C_real, self.N_real, self.Cx, self.CK = taps, C_real, N_real, Cx, CK
    self.tap0, self.tap_step = tap0, tap_step
    self.s_c = N_real if s_c is None else s_c
    self.s_n = s_n
    self.s_tap = C_real * N_real if s_tap is None else s_tap
    self.parity_major, self.narrow_last = parity_major, narrow_last


def packed_elems(N, taps, Cx, CK):
  """cg_packed_elems: whole 128-column tiles, Cx / CK chunks of ceil16(taps CK / 8)
  groups of 8 channels; -1 for a geometry the header excludes."""
  if CK < 32 or CK % 8 or Cx % CK or taps < 1 or N < 1:
    return -1
  Fp = -(-(taps * (CK // 8)) // 16) * 16
  return -(-N // 128) * 128 * (Cx // CK) * Fp * 8


def pack_admissible(d):
  """Header: C_real <= Cx; parity_major for even taps only; narrow_last needs
  parity_major, CK == 32, even taps <= 32, Cx - 32 < C_real <= Cx - 24 and a last
  chunk that exists next to a full one (Cx >= 64) and has room for the 32 narrow
  groups (ceil16(4 taps) >= 32: taps >= 6)."""
  if packed_elems(d.N_real, d.taps, d.Cx, d.CK) < 0 or d.C_real > d.Cx:
    return False
  if d.narrow_last:
    return bool(d.parity_major and d.CK == 32 and d.taps <= 32 and d.taps % 2 == 0 and
                d.taps >= 6 and d.Cx >= 64 and d.Cx - 32 < d.C_real <= d.Cx - 24)
  return True


def logical(src, d):
  """Wl[tap][c][n] = src[(tap0 + tap * tap_step) * s_tap + c * s_c + n * s_n]."""
  src = np.asarray(src, np.float64).ravel()
  t = (d.tap0 + np.arange(d.taps) * d.tap_step)[:, None, None] * d.s_tap
  c = np.arange(d.C_real)[None, :, None] * d.s_c
  n = np.arange(d.N_real)[None, None, :] * d.s_n
  return src[t + c + n]


def pack(src, d, f16):
  """The packed operand of `d` as float64 values of the activation type, flat,
  packed_elems long: [column n][chunk cc][position f][8 channels], +0 wherever no
  Wl element lands.  Position f = p * (CK / 8) + q holds channels cc CK + 8 q .. + 7
  of packed tap p; packed tap p is tap p, or with parity_major the even taps in
  order and then the odd ones.  narrow_last: in the LAST chunk, position f < 32 is
  packed tap (f >> 4) * (taps / 2) + (f & 15) (slots f & 15 >= taps / 2 stay zero)
  and holds that chunk's first 8 channels."""
  assert pack_admissible(d)
  Wl = R.round_act(logical(src, d), f16)
  c8, nch = d.CK // 8, d.Cx // d.CK
  Fp = -(-(d.taps * c8) // 16) * 16
  Npad = -(-d.N_real // 128) * 128
  out = np.zeros((Npad, nch, Fp, 8))
  half = d.taps // 2
  for p in range(d.taps):
    tap = p if not d.parity_major else (2 * p if p < half else 2 * (p - half) + 1)
    for c in range(d.C_real):
      cc, r = divmod(c, d.CK)
      q, e = divmod(r, 8)
      if d.narrow_last and cc == nch - 1:
        assert q == 0
        f = (p // half) * 16 + p % half
      else:
        f = p * c8 + q
      out[:d.N_real, cc, f, e] = Wl[tap, c, :]
  return out.ravel()


# ---------------------------------------------------------------------------
# data recipes (numpy only: the CPU tests check them, the GPU tests run them)
# ---------------------------------------------------------------------------
def seed_of(G):
  return (1000 + 7 * G.nB + 13 * G.Lu + 31 * G.taps + 3 * G.Cx + 5 * G.Cg +
          (sum(abs(s) for s in G.shifts) if G.shifts else 0))


def real_recipe(G, f16):
  """x, g = randn rounded to the activation type (|values| in ~[2^-6, 4]: no fp16
  product comes near its subnormals -- they are exact in f32 anyway), every
  sample starting with +-0 where there are 8 channels or more."""
  rng = np.random.RandomState(seed_of(G))
  _, Lx, _ = stride_of(G)
  x = R.round_act(rng.randn(G.nB, Lx, G.Cx), f16)
  g = R.round_act(rng.randn(G.nB, G.Lu, G.Cg), f16)
  if G.Cx >= 8:
    x[:, 0, :2] = [0.0, -0.0]
  if G.Cg >= 8:
    g[:, 0, :2] = [-0.0, 0.0]
  return x, g


def exact_unit(f16):
  """(unit of x, smallest power of g): a product is a multiple of their product."""
  return (2.0**-10, 2.0**-2) if f16 else (2.0**-7, 2.0**-3)


def exact_recipe(G, f16):
  """x = +-(2^(s-1) + j) 2^-(s-1), j uniform in [0, 2^(s-1)): every one of the s = 8
  (bf16) / 11 (fp16) significand bits varies at the one exponent [1, 2); g in {0,
  +-1, +-2^-k} (k <= 3 / 2).  Products are multiples of 2^-10 / 2^-12 below 2; g is
  zero often enough that sum |x g| stays below 2^10 (checked by test_wgrad_ref):
  every partial sum in every order is exact in f32, so a correct kernel matches
  bit for bit, and a kernel that drops any operand bit does not."""
  rng = np.random.RandomState(seed_of(G) + 1)
  _, Lx, _ = stride_of(G)
  s = 11 if f16 else 8
  h = 2**(s - 1)
  x = (h + rng.randint(0, h, (G.nB, Lx, G.Cx))) / float(h)
  x *= rng.choice([-1.0, 1.0], x.shape)
  kmax = 2 if f16 else 3
  mag = 2.0**-rng.randint(0, kmax + 1, (G.nB, G.Lu, G.Cg))
  # E|x g| = 1.5 x ~0.6 per live term: keep the expected sum near 2^8
  live = min(0.75, 2.0**8 / (0.9 * rows_of(G)))
  g = mag * rng.choice([-1.0, 1.0], mag.shape) * (rng.rand(*mag.shape) < live)
  return x, g


def subnormal_recipe(G, which):
  """fp16 only.  which = 'x': x = +-j 2^-24, j in [1, 1023] (every fp16 subnormal),
  g = +-2^k, k in [8, 12]; which = 'g': the roles swapped.  All sums are exact in f32
  (multiples of 2^-16 below 2^-2 rows); the statement keeps the subnormals."""
  rng = np.random.RandomState(seed_of(G) + 2)
  _, Lx, _ = stride_of(G)
  def sub(shape):
    return rng.randint(1, 1024, shape) * 2.0**-24 * rng.choice([-1.0, 1.0], shape)
  def pw(shape):
    return 2.0**rng.randint(8, 13, shape) * rng.choice([-1.0, 1.0], shape)
  xs, gs = (G.nB, Lx, G.Cx), (G.nB, G.Lu, G.Cg)
  return (sub(xs), pw(gs)) if which == 'x' else (pw(xs), sub(gs))


def unread_rows(s, w):
  """Rows of a sample no shuffled row reads under shift s: the first s (s > 0) or
  the last |s| (s < 0), less what the mirrored branch reaches back to (2 |s| >= w)."""
  return sorted(set(range(w)) - set(shuffle_src(np.arange(w), s, w).tolist()))


def reflected_rows(s, w):
  """Shuffled rows t that come from the mirrored branch."""
  t = np.arange(w)
  return [int(v) for v in (t[t + s >= w] if s > 0 else t[t + s < 0])]


# ---------------------------------------------------------------------------
# the shapes the GPU tests run on rounded reals (tests/test_wgrad_ref.py checks
# each of them against the mutants); every other GPU shape runs the exact recipe
# ---------------------------------------------------------------------------
MIXED5 = (-1, 0, 2, 1, -2)


def instantiation_geoms(taps):
  """Three geometries per tap count: Lu = 8 (eight samples per 64-row tile, nB Lu
  = 72: the second tile is ragged), Lu = 64 (one sample per tile) and Lu = 128
  (128-row tiles, or 64-row ones when forced)."""
  return [geom(9, 8, taps, 33, 40, MIXED5, 2),
          geom(3, 64, taps, 33, 40, (1, -2, 0), 1),
          geom(2, 128, taps, 8, 65, (-3, 2), 1)]


TAPS = list(range(2, 25, 2))  # every kernel size geometry.validate_hparams admits
CHANNELS = [(1, 8, 1, 8), (8, 16, 40, 48), (33, 40, 65, 72), (102, 128, 130, 136),
            (102, 128, 1, 8), (1, 8, 130, 136)]  # Cx_real, Cx, Cg_real, Cg
# (Cx_real, Cg_real) -> gmode of plan_wgrad's XCD grouping (gx = ceil(Cx / 32) cx
# blocks, gy = ceil(Cg / 64) cg blocks): 2 when gx gy divides 32; else 0 when gx
# does (the cx blocks of a cg block share g), else 1 when gy does, else 3
GROUPING = [(102, 130, 0), (70, 65, 1), (33, 65, 2), (70, 130, 3)]
DENSE = [geom(300, 1, 1, 33, 40), geom(2, 256, 1, 33, 40), geom(1, 512, 1, 8, 65),
         geom(9, 32, 1, 33, 40)]
# (no shuffle: at 1152 rows one reflected row no longer moves an output by 20 bars)
JOIN = geom(18, 64, 8, 33, 40)
BIAS_RING = geom(4, 64, 24, 8, 65, (2, -1), 2)
BIAS_NSEG = geom(9, 8, 8, 8, 65, MIXED5, 2)
BATCH = [geom(4, 64, 24, 33, 40, (1, -2), 2), geom(2, 128, 24, 8, 65, (-1, 3), 1),
         geom(4, 64, 24, 40, 33, (0, 2), 2)]


# shapes that run the exact recipe only: more than 64 shift segments (the ring
# is refused; 4160 rows: a single reflected row is below 20 bars), and the
# largest shifts at the smallest long sides and on the ring
SEGS65 = geom(65, 64, 24, 8, 40, tuple(((i * 7) % 5) - 2 for i in range(65)), 1)
SHIFT_EDGES = [geom(5, 8, 8, 8, 40, (15, -15, 0, 1, -1), 1),
               geom(70, 2, 8, 8, 40, (3, -3, 1, -1, 0, 2, -2), 10),
               geom(3, 8, 12, 33, 40, (-2,), 8),
               geom(4, 64, 24, 8, 40, (127, -127, 63, -64), 1)]
EXACT_ONLY = [SEGS65] + SHIFT_EDGES


def pitch_of(c):
  """A channel pitch above the real count (a multiple of 8)."""
  return (c // 8 + 1) * 8


def channel_geom(cx, cg):
  """(a single x channel: one reflected row is one number, which may be small --
  those shapes run without a shuffle)"""
  return geom(4, 64, 8, cx, cg, (2, -1) if cx >= 8 else None, 2)


def real_geoms():
  out = []
  for taps in TAPS:
    out += instantiation_geoms(taps)
  out += [channel_geom(cx, cg) for cx, _, cg, _ in CHANNELS]
  out += [geom(4, 64, 8, cx, cg, (2, -1), 2) for cx, cg, _ in GROUPING]
  out += DENSE + [JOIN, BIAS_RING, BIAS_NSEG] + BATCH
  seen, uniq = set(), []
  for G in out:
    if G not in seen:
      seen.add(G)
      uniq.append(G)
  return uniq


def gmode_of(Cx_real, Cg_real, nB, Lx, Cx, M, Cg):
  """plan_wgrad's choice restated (bytes re-read per grouping; see GROUPING)."""
  gx, gy = -(-Cx_real // 32), -(-Cg_real // 64)
  fits = lambda n: 1 <= n <= 32 and 32 % n == 0
  xb, gb = float(nB * Lx * Cx), float(M * Cg)
  mode, best = 3, xb * gy + gb * gx
  if fits(gx) and xb * gy + gb < best:
    mode, best = 0, xb * gy + gb
  if fits(gy) and xb + gb * gx < best:
    mode, best = 1, xb + gb * gx
  if fits(gx * gy):
    mode = 2
  return mode
