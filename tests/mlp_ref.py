"""Float64 statements of the MLP entry points of the C ABI
(calciumgan_amd/csrc/mlp.hip), written from the comments of
include/calciumgan_hip.h, a restatement of cg_mlp_dense_wgrad's launch plan,
the per-element error bars of an f32 evaluation, and the data recipes the
parity tests of tests/test_hip_mlp_parity.py run them on.

Everything here is numpy on the host.  Every statement takes `dt`: float64 is
the statement, float32 the same numpy code as a stand-in for "some f32
evaluation" (tests/test_mlp_ref.py keeps it inside the bars and, under the exact
recipe, bit-equal to float64).  Inputs are float32 arrays; float scalars of the
ABI are taken at their f32 value (pointwise_ref.f32); the keep mask is
mlp.dropout_keep_mask.

Bars.  U = 2^-24.  A rounding of + * / sqrt moves a result by at most U times
its magnitude (half a spacing), or by 2^-150 in the subnormals; a sum of n terms
in ANY order by n U sum |terms| (pointwise_ref.sum_bound).  No bar is a measured
number.

Zeros.  Equality under the exact recipe is equality of VALUES of the float32
results (a non-zero float32 has one bit pattern).  The sign of a zero is stated
only where the header states it: dropped elements are +0, a cancelled segment
pair is +0, a kept negative under alpha = 0 is -0."""
import numpy as np

import pointwise_ref as R
from calciumgan_amd.gan.models import mlp

U = R.U32
TINY = 2.0**-149  # the subnormal spacing of f32: the floor of one rounding

FWD_ACT, FWD_TANGENT, FWD_SIGMOID = mlp.FWD_ACT, mlp.FWD_TANGENT, mlp.FWD_SIGMOID
BWD_MASK, BWD_SIGMOID, BWD_NONE = mlp.BWD_MASK, mlp.BWD_SIGMOID, mlp.BWD_NONE

F32_MAX = float(np.finfo(np.float32).max)


def _a(x, dt=np.float64):
  return np.asarray(x, dtype=dt)


def scale_of(p):
  """float32(1 / (1 - p)) as a python float; 1 for p == 0."""
  return float(mlp.dropout_scale(p))


def keep_mask(seed, stream, rows, N, p):
  return mlp.dropout_keep_mask(seed, stream, rows * N, p).reshape(rows, N)


# ---------------------------------------------------------------------------
# statements
# ---------------------------------------------------------------------------
def act(z, alpha, dt=np.float64):
  """act(z) = max(z, alpha z); a NaN operand of the max is ignored (fmax)."""
  with np.errstate(invalid='ignore'):
    return np.fmax(z, dt(R.f32(alpha)) * z)


def slope_mask(h, alpha, p, dt=np.float64):
  """m(h) = s * keep * act' read back from a stored h: h > 0: s, h < 0: s alpha,
  h == 0 (either sign): 0 -- the element counts as dropped.  NaN: 0 as well
  (neither comparison holds)."""
  h = _a(h, dt)
  s = dt(scale_of(p))
  with np.errstate(invalid='ignore'):
    return np.where(h > 0, s, np.where(h < 0, s * dt(R.f32(alpha)), dt(0)))


def preact(x, W, b=None, dt=np.float64):
  with np.errstate(invalid='ignore', over='ignore'):
    z = _a(x, dt) @ _a(W, dt)
    if b is not None:
      z = z + _a(b, dt)[None, :]
  return z


def dense_fwd(x, W, b, mode, alpha=0.0, p=0.0, keep=None, h_mask=None,
              dt=np.float64):
  """cg_mlp_dense_fwd.  x (rows, Cin) -- the caller strips the pitch --, W (Cin,
  Cout), b (Cout,) or None, keep (rows, Cout) bool for p > 0.
    ACT:     h = drop(act(x W + b)): kept elements times s, the others +0
    TANGENT: h = m(h_mask) * (x W)
    SIGMOID: h = 1 / (1 + exp(-(x W + b)))"""
  if mode == FWD_TANGENT:
    with np.errstate(invalid='ignore'):
      return slope_mask(h_mask, alpha, p, dt) * preact(x, W, None, dt)
  z = preact(x, W, b, dt)
  if mode == FWD_SIGMOID:
    with np.errstate(over='ignore'):
      return dt(1) / (dt(1) + np.exp(-z))
  assert mode == FWD_ACT
  h = act(z, alpha, dt)
  if p > 0:
    with np.errstate(invalid='ignore', over='ignore'):
      h = np.where(keep, h * dt(scale_of(p)), dt(0))
  return h


def dense_dgrad(dh, h, W, mode, alpha=0.0, p=0.0, dt=np.float64):
  """cg_mlp_dense_dgrad: (dz, dx).  dz = dh m(h) / dh h (1 - h) / dh; dx = dz
  W^T, W (Cin, Cout)."""
  dh = _a(dh, dt)
  with np.errstate(invalid='ignore', over='ignore'):
    if mode == BWD_MASK:
      dz = dh * slope_mask(h, alpha, p, dt)
    elif mode == BWD_SIGMOID:
      y = _a(h, dt)
      dz = dh * (y * (dt(1) - y))
    else:
      assert mode == BWD_NONE
      dz = dh
    return dz, dz @ _a(W, dt).T


def segments(rows, seg_rows):
  """[(start, end)] of the up to three segments: [0, seg), [seg, 2 seg), [2 seg,
  rows); the last one that holds rows ends at `rows`."""
  nseg = 1 if rows <= seg_rows else (2 if rows <= 2 * seg_rows else 3)
  return [(k * seg_rows, rows if k == nseg - 1 else (k + 1) * seg_rows)
          for k in range(nseg)]


def wgrad_x(x, tail, tail_row0):
  """The rows the weight gradient multiplies: x, rows >= tail_row0 from tail."""
  x = np.array(x, copy=True)
  if tail is not None and tail_row0 < x.shape[0]:
    x[tail_row0:] = np.asarray(tail)[:x.shape[0] - tail_row0]
  return x


def dense_wgrad(x, tail, tail_row0, dz, seg_rows, coef, bias_rows,
                dt=np.float64, row_seg=None):
  """cg_mlp_dense_wgrad: (dW, db, parts).  dW = sum_k c_k S_k, S_k = sum of
  x[r]^T dz[r] over the rows of segment k, every product c_k S_k and every sum of
  them rounded on its own in `dt`; db likewise over the rows < bias_rows.
  parts = [(c_k, S_k, T_k)] (T_k the bias sums) for the bars.  row_seg
  overrides the segment of every row (for planting a fault)."""
  xe = _a(wgrad_x(x, tail, tail_row0), dt)
  dz = _a(dz, dt)
  rows = xe.shape[0]
  segs = segments(rows, seg_rows)
  if row_seg is None:
    row_seg = np.minimum(np.arange(rows) // seg_rows, 2)
  parts, dW, db = [], None, None
  with np.errstate(invalid='ignore', over='ignore'):
    for k in range(len(segs)):
      c = dt(R.f32(coef[k]))
      rk = np.flatnonzero(row_seg == k)
      S = xe[rk].T @ dz[rk]
      T = dz[rk[rk < bias_rows]].sum(axis=0, dtype=dt)
      parts.append((c, S, T))
      dW = c * S if dW is None else dW + c * S
      db = c * T if db is None else db + c * T
  return dW, db, parts


def interp(real, fake, alpha, dt=np.float64):
  """cg_mlp_interp: out (3, B, n) = [real | fake | a_b real + (1 - a_b) fake]."""
  r, f = _a(real, dt), _a(fake, dt)
  a = _a(alpha, dt)[:, None]
  return np.stack([r, f, a * r + (dt(1) - a) * f])


def gp_loss(g, d_out, penalty, dt=np.float64):
  """cg_mlp_gp_loss: dict(norm, gp, coef, v, loss) from g (B, n), d_out (3B,).
  v is stated from the STORED coef (v[b] = coef[b] g[b]): callers that compare
  bits pass the float32 coef through `v_of`."""
  g, d = _a(g, dt), _a(d_out, dt)
  B = g.shape[0]
  lam = dt(R.f32(penalty))
  with np.errstate(invalid='ignore', divide='ignore'):
    norm = np.sqrt((g * g).sum(axis=1, dtype=dt))
    dd = norm - dt(1)
    gp = (dd * dd).sum(dtype=dt) / dt(B)
    coef = lam * dt(2) * dd / (dt(B) * norm)
    mr, mf = d[:B].sum(dtype=dt) / dt(B), d[B:2 * B].sum(dtype=dt) / dt(B)
    loss = np.array([-mr + mf + lam * gp, -mf], dtype=dt)
  return dict(norm=norm, gp=np.array([gp], dtype=dt), coef=coef,
              v=v_of(coef, g, dt), loss=loss)


def v_of(coef, g, dt=np.float64):
  with np.errstate(invalid='ignore'):
    return _a(coef, dt)[:, None] * _a(g, dt)


# ---------------------------------------------------------------------------
# the launch plan of cg_mlp_dense_wgrad
# ---------------------------------------------------------------------------
def wgrad_chunk_rows(rows):
  """At most 64 chunks over `rows`, each a multiple of the 16-row staging pass
  and at least 64 rows."""
  return -(-max(-(-rows // 64), 64) // 16) * 16


def wgrad_plan(rows, seg_rows, Cin=1, Cout=1):
  """dict(chunk_rows, nseg, cps, chunks, slice, used, bound).  Every segment is
  cut into cps chunks of chunk_rows rows (cps from the LONGEST segment); chunk c
  of segment k owns slot k cps + c of ws, a slice of Cin Cout + Cout floats,
  and stores it even when it holds no rows (zeros).  chunks = [(slot, k, r0,
  r1)], r0 == r1 for an empty one.  used = nseg cps slice floats are written,
  bound = 3 ceil(rows / chunk_rows) slice is cg_mlp_wgrad_ws_elems."""
  cr = wgrad_chunk_rows(rows)
  segs = segments(rows, seg_rows)
  cps = -(-max(e - s for s, e in segs) // cr)
  chunks = []
  for k, (s, e) in enumerate(segs):
    for c in range(cps):
      r0 = min(s + c * cr, e)
      chunks.append((k * cps + c, k, r0, min(r0 + cr, e)))
  sl = Cin * Cout + Cout
  return dict(chunk_rows=cr, nseg=len(segs), cps=cps, chunks=chunks, slice=sl,
              used=len(segs) * cps * sl, bound=3 * -(-rows // cr) * sl)


# ---------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------
def _abs(x):
  return np.abs(_a(x))


def dense_sum_bar(a, B, bias, c):
  """(K + c) U (|a| |B| + |bias|) + c 2^-149: K products added in any order and c
  roundings of the epilogue."""
  with np.errstate(invalid='ignore'):
    s = _abs(a) @ _abs(B)
    if bias is not None:
      s = s + _abs(bias)[None, :]
  return (np.shape(a)[1] + c) * U * s + c * TINY


def fwd_bar(x, W, b, mode, alpha=0.0, p=0.0, keep=None, h_mask=None):
  """Bar of an f32 dense_fwd.
    ACT: the sum, the bias, alpha z and the dropout scale: c = 3; act is
      Lipschitz with max(1, |alpha|) and the result is scaled by s.  Dropped
      elements: 0 (they are exactly +0).
    TANGENT: the sum, s alpha and the product with m: c = 2, times |m|.
    SIGMOID: z with c = 1, then `sigmoid_bar`."""
  if mode == FWD_TANGENT:
    return np.abs(slope_mask(h_mask, alpha, p)) * dense_sum_bar(x, W, None, 2)
  if mode == FWD_SIGMOID:
    return sigmoid_bar(preact(x, W, b), dense_sum_bar(x, W, b, 1))
  e = scale_of(p) * max(1.0, abs(R.f32(alpha))) * dense_sum_bar(x, W, b, 3)
  return np.where(keep, e, 0.0) if p > 0 else e


def sigmoid_bar(z, ez):
  """1 / (1 + expf(-z)) in f32 on an argument that is off by at most ez: e =
  expf(-z) carries e (exp(ez) - 1) and R.LIBM_SPACINGS spacings; d = 1 + e and
  the quotient half a spacing each, carried by the derivative 1 / d^2.  Where
  e can exceed the largest f32 the naive form gives 1 / inf = 0: the bar is the
  value itself."""
  z = _a(z)
  with np.errstate(over='ignore', invalid='ignore'):
    e = np.exp(-z)
    d = 1.0 + e
    s = 1.0 / d
    de = e * np.expm1(ez) + R.LIBM_SPACINGS * R.ulp_f32(np.minimum(e, F32_MAX))
    dd = de + 0.5 * R.ulp_f32(np.minimum(d, F32_MAX))
    bar = dd / d**2 + 0.5 * R.ulp_f32(s)
    over = e + de >= F32_MAX
  return np.where(over, np.maximum(s, TINY), bar)


def dgrad_bars(dh, h, W, mode, alpha=0.0, p=0.0):
  """(bar dz, bar dx).  dz: s alpha and the product (MASK: 2 roundings), 1 - y
  and two products (SIGMOID: 3), none (NONE: the same bits).  dx: Cout products
  of the ROUNDED dz added in any order."""
  dz, _ = dense_dgrad(dh, h, W, mode, alpha, p)
  c = {BWD_MASK: 2, BWD_SIGMOID: 3, BWD_NONE: 0}[mode]
  ez = c * (U * np.abs(dz) + TINY)
  return ez, dense_sum_bar(dz, _a(W).T, None, c)


def wgrad_bars(x, tail, tail_row0, dz, seg_rows, coef, bias_rows):
  """(bar dW, bar db).  Segment k: chains of at most chunk_rows rows (never more
  than the segment holds), one rounding per chunk sum (cps), one for the
  product with c_k, and one per segment addition (nseg), all on |c_k| A_k, A_k =
  sum_r |x[r]|^T |dz[r]| over the segment."""
  xe = _abs(wgrad_x(x, tail, tail_row0))
  ad = _abs(dz)
  rows = xe.shape[0]
  plan = wgrad_plan(rows, seg_rows)
  eW = eb = 0.0
  for k, (s, e) in enumerate(segments(rows, seg_rows)):
    n = min(e - s, plan['chunk_rows']) + plan['cps'] + 1 + plan['nseg']
    c = abs(R.f32(coef[k]))
    eW = eW + n * U * c * (xe[s:e].T @ ad[s:e]) + TINY
    eb = eb + n * U * c * ad[s:min(e, max(bias_rows, s))].sum(axis=0) + TINY
  return eW, eb


def interp_bar(real, fake, alpha):
  """a r + (1 - a) f: 1 - a, two products and the sum (fused or not): at most
  three roundings on |a r| + |(1 - a) f|.  The copies are the same bits."""
  a = _abs(alpha)[:, None]
  mag = a * _abs(real) + np.abs(1.0 - _a(alpha)[:, None]) * _abs(fake)
  return 3 * U * mag + 3 * TINY


def gp_loss_bars(g, d_out, penalty):
  """Bars of an f32 gp_loss, operation by operation:
    norm: n squares added in a chain (n U ss), carried through the root by 1 /
      (2 norm), and the root's half spacing;
    d = norm - 1: E_d = E_norm + U |d|;
    gp: d^2 (2 |d| E_d + E_d^2 + U d^2), their sum in any order, 1 / B and the
      product (2 U gp);
    coef = lam 2 d / (B norm): E_d and E_norm through the quotient, and lam 2 d,
      B norm, the quotient: 3 U |coef|;
    v = coef g: measured from the STORED coef: U |v|;
    loss[0] = -mr + mf + lam gp: the two sums over B (sum_bound / B), 1 / B,
      three products and two additions on the magnitudes that meet (6 U), and
      lam E_gp;  loss[1] = -mf: its sum, 1 / B and the product (2 U)."""
  g, d = _a(g), _a(d_out)
  B, n = g.shape
  lam = abs(R.f32(penalty))
  ss = (g * g).sum(axis=1)
  norm = np.sqrt(ss)
  safe = np.where(norm > 0, norm, 1.0)
  e_norm = n * U * ss / (2 * safe) + U * norm + TINY
  dd = norm - 1.0
  e_d = e_norm + U * np.abs(dd)
  e2 = 2 * np.abs(dd) * e_d + e_d * e_d + U * dd * dd
  gp = (dd * dd).mean()
  e_gp = (e2.sum() + R.sum_bound(dd * dd)) / B + 2 * U * gp + TINY
  K = 2.0 * lam / B
  coef = K * np.abs(dd) / safe
  e_coef = K * e_d / safe + K * np.abs(dd) * e_norm / safe**2 + 3 * U * coef + TINY
  mr, mf = d[:B].mean(), d[B:2 * B].mean()
  sr, sf = R.sum_bound(d[:B]) / B, R.sum_bound(d[B:2 * B]) / B
  e_loss = np.array([sr + sf + lam * e_gp + 6 * U * (abs(mr) + abs(mf) + lam * gp),
                     sf + 2 * U * abs(mf)]) + TINY
  return dict(norm=e_norm, gp=np.array([e_gp]), coef=e_coef, loss=e_loss,
              v_from_coef=lambda v: U * np.abs(v) + TINY)


def used(got, want, bar):
  """The largest fraction of its bar any finite element uses (0 where the bar
  is 0 and the values agree, inf where they do not)."""
  got, want, bar = np.broadcast_arrays(_a(got), _a(want), _a(bar))
  fin = np.isfinite(want) & np.isfinite(bar)
  if not fin.any():
    return 0.0
  err = np.abs(got[fin] - want[fin])
  b = bar[fin]
  with np.errstate(divide='ignore', invalid='ignore'):
    f = np.where(err == 0, 0.0, np.where(b > 0, err / np.where(b > 0, b, 1), np.inf))
  f = np.where(np.isnan(f), np.inf, f)  # a non-finite result where a finite one is due
  return float(f.max())


def same_values(got, want):
  """got (float32) equals the float64 statement, which must itself be a float32
  (the exact recipe's promise)."""
  want = _a(want)
  w32 = want.astype(np.float32)
  assert np.array_equal(w32.astype(np.float64), want), 'statement is no float32'
  return np.array_equal(np.asarray(got, np.float32), w32)


def same_classes(got, want):
  """NaN where the statement has NaN, the same infinity where it has one, and
  finite where it is finite."""
  got, want = _a(got), _a(want)
  inf = np.isinf(want)
  return (np.array_equal(np.isnan(got), np.isnan(want)) and
          np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]))


# ---------------------------------------------------------------------------
# recipes
# ---------------------------------------------------------------------------
def _f32(a):
  return np.ascontiguousarray(a, dtype=np.float32)


def _ints(rng, *shape):
  """Non-zero integers in [-4, 4]."""
  return _f32(rng.randint(1, 5, shape) * rng.choice([-1, 1], shape))


def real_dense(seed, rows, K, N):
  """x, W (scaled by 1 / sqrt(K)), b, dh: rounded normals."""
  rng = np.random.RandomState(seed)
  f = lambda *s: _f32(rng.standard_normal(s))
  return dict(x=f(rows, K), W=_f32(f(K, N) / np.sqrt(K)), b=f(N), dh=f(rows, N),
              t=f(rows, K))


def exact_dense(seed, rows, K, N):
  """Integer operands: every partial sum of x W + b is an integer below 16 K + 4
  <= 2^20 + 4 in any order; alpha = 0.25 and the scales 2 and 4 keep 24 bits."""
  rng = np.random.RandomState(seed)
  return dict(x=_ints(rng, rows, K), W=_ints(rng, K, N), b=_ints(rng, N),
              dh=_ints(rng, rows, N), t=_ints(rng, rows, K))


EXACT_ALPHA = 0.25
EXACT_P = (0.5, 0.75)


def planted_h(seed, keep, exact):
  """A stored h with known signs: positive, negative (kept) or +0 (dropped)."""
  rng = np.random.RandomState(seed)
  mag = (rng.randint(1, 5, keep.shape) if exact else
         np.abs(rng.standard_normal(keep.shape)) + 0.01)
  sign = rng.choice([-1.0, 1.0], keep.shape)
  return _f32(np.where(keep, sign * mag, 0.0))


def planted_y(seed, rows, N, exact):
  """A stored sigmoid output: from {0.25, 0.5, 0.75} / uniform in (0, 1)."""
  rng = np.random.RandomState(seed)
  if exact:
    return _f32(rng.choice([0.25, 0.5, 0.75], (rows, N)))
  return _f32(rng.uniform(0.01, 0.99, (rows, N)))


def wgrad_data(seed, rows, Cin, Cout, ntail, exact):
  """x, dz, tail (ntail rows, or None)."""
  rng = np.random.RandomState(seed)
  f = ((lambda *s: _ints(rng, *s)) if exact else
       (lambda *s: _f32(rng.standard_normal(s))))
  return dict(x=f(rows, Cin), dz=f(rows, Cout),
              tail=f(ntail, Cin) if ntail else None)


def exact_coef(B=128):
  """Powers of two (-1 / B, 1 / B, 1)."""
  return (-1.0 / B, 1.0 / B, 1.0)


EXACT_PENALTY = 8.0


def gp_data(seed, B, n, exact):
  """g (B, n), d_out (3B,).  exact: rows of integer norm 1, 2, 4 and (n >= 2) 5
  -- (3, 4, 0, ...) --, the non-zero entries at random places and signs, and
  integer d_out: with B a power of two and penalty 8 every result but coef and
  v of the norm-5 rows is a float32 exactly, and those are single roundings."""
  rng = np.random.RandomState(seed)
  if not exact:
    return dict(g=_f32(rng.standard_normal((B, n)) * 0.4 / np.sqrt(max(n, 1) / 12.0)),
                d_out=_f32(rng.standard_normal(3 * B)))
  g = np.zeros((B, n), np.float32)
  kinds = [(1,), (2,), (4,)] + ([(3, 4)] if n >= 2 else [])
  for b in range(B):
    vals = kinds[b % len(kinds)]
    pos = rng.choice(n, len(vals), replace=False)
    g[b, pos] = np.array(vals) * rng.choice([-1, 1], len(vals))
  return dict(g=g, d_out=_ints(rng, 3 * B))


def interp_data(seed, B, n, exact):
  """real, fake, alpha; exact: integers and alpha from {0, 0.25, 0.5, 1}."""
  rng = np.random.RandomState(seed)
  if exact:
    return dict(real=_ints(rng, B, n), fake=_ints(rng, B, n),
                alpha=_f32(rng.choice([0.0, 0.25, 0.5, 1.0], B)))
  return dict(real=_f32(rng.uniform(0, 1, (B, n))), fake=_f32(rng.uniform(0, 1, (B, n))),
              alpha=_f32(rng.uniform(0, 1, B)))


# the special recipe's planted places (rows >= 33, K >= 16, N >= 16)
SP = dict(inf_row=1, inf_k=7, nan_row=16, nan_k=9, zero_row=32, sub_row=4,
          zero_col=2, hi_col=5, lo_col=6, sub_col=7)
SUB = 2.0**-140


def special_dense(seed, rows, K, N):
  """real_dense plus: x[inf_row][inf_k] = +inf, x[nan_row][nan_k] = NaN, row
  zero_row of x all zero, column zero_col of W all zero, b[hi_col] = +100 and
  b[lo_col] = -100 (|x W| stays below 11 there: W's two columns are scaled so),
  row sub_row of x zero but for the subnormal 2^-140 in column 0, b[sub_col] =
  0 (so h[sub_row][sub_col] is a subnormal product), and subnormals in x[3][0],
  W[0][4].  dh gets the same inf / NaN / zero rows (in its own columns)."""
  assert rows > SP['zero_row'] and K >= 16 and N >= 16
  d = real_dense(seed, rows, K, N)
  x, W, b, dh = d['x'], d['W'], d['b'], d['dh']
  W[:, SP['zero_col']] = 0
  for c in (SP['hi_col'], SP['lo_col']):  # |x W| <= 8 in the two columns
    W[:, c] /= np.float32(2.0**np.ceil(np.log2(max(1.0, np.abs(x @ W[:, c]).max() / 8))))
  b[SP['hi_col']], b[SP['lo_col']], b[SP['sub_col']] = 100.0, -100.0, 0.0
  x[3, 0] = -SUB
  W[0, 4] = 2.0**-130
  x[SP['zero_row']] = 0
  x[SP['sub_row']] = 0
  x[SP['sub_row'], 0] = SUB
  x[SP['inf_row'], SP['inf_k']] = np.inf
  x[SP['nan_row'], SP['nan_k']] = np.nan
  dh[SP['zero_row']] = 0
  dh[SP['inf_row'], SP['inf_k']] = np.inf
  dh[SP['nan_row'], SP['nan_k']] = np.nan
  dh[3, 0] = -SUB
  return d


# ---------------------------------------------------------------------------
# cases (shared by the host and the GPU tests)
# ---------------------------------------------------------------------------
# (rows, K, N) of a layer: the row block is 32, the K panel 32, the column tile
# 64; every extent at 1, at the edge and one past it, each met with each other
DENSE_SMALL = [(1, 1, 1), (1, 33, 64), (32, 32, 65), (33, 1, 65), (33, 33, 1),
               (32, 33, 64), (33, 32, 64), (33, 33, 65), (32, 1, 1), (1, 32, 65)]
# width 1024 (CG_MLP_MAX_WIDTH) on the narrow side
DENSE_WIDE = [(2, 1030, 1024)]
# the head (K flat: a chain of 65536, 2048 panels) and the generator's first
# Dense (N flat: 1024 column tiles).  The input gradient of the same layers
# sees them transposed: 1024 column tiles of dx / a chain of 65536.
DENSE_FLAT = [(3, 65536, 1), (3, 5, 65536)]
SPECIAL_SHAPE = (33, 33, 65)

_C = (-2.0**-7, 2.0**-7, 1.0)


def _wg(id, rows, Cin, Cout, seg, tail=True, bias_rows=None, coef=_C, **kw):
  ntail = max(rows - 2 * seg, 0) if tail else 0
  return dict(id=id, rows=rows, Cin=Cin, Cout=Cout, seg=seg, ntail=ntail,
              bias_rows=min(2 * seg, rows) if bias_rows is None else bias_rows,
              coef=coef, **kw)


# the dW tile is 64 x 64, the staging pass 16 rows; chunk_rows is 64 up to 4096
# rows and 80 at 4097
WGRAD_CASES = [
    _wg('1x1', 50, 1, 1, 16),
    _wg('64x65', 50, 64, 65, 16),
    _wg('65x64', 50, 65, 64, 16, bias_rows=50),
    _wg('1x64-bias0', 50, 1, 64, 16, bias_rows=0),
    _wg('65x1-bias-in-pass', 50, 65, 1, 16, bias_rows=21),
    _wg('one-segment', 33, 5, 7, 33, tail=False, coef=(0.5, 0.0, 0.0)),
    _wg('two-segments', 40, 5, 7, 25, tail=False),
    _wg('head-65536x1', 24, 65536, 1, 8, coef=(-0.125, 0.125, 1.0)),
    _wg('flat-5x65536', 24, 5, 65536, 8, coef=(-0.125, 0.125, 1.0)),
    # 4097 = 1366 + 1366 + 1365: a segment's last chunk has 6 rows, no boundary
    # is a multiple of 16 or 80
    _wg('4097-seg1366', 4097, 3, 5, 1366),
    _wg('4097-seg1366-bias-in-pass', 4097, 3, 5, 1366, bias_rows=1373),
    # a third segment of 97 rows against cps = 25: 23 empty chunks store zeros
    _wg('4097-short-third', 4097, 3, 5, 2000, bias_rows=4097),
    # a third segment of 2097 rows against seg_rows = 1000: it sets cps
    _wg('4097-long-third', 4097, 3, 5, 1000, bias_rows=0),
    # x at a pitch, its replaced rows NaN (the GPU test; the host sees x dense)
    _wg('tail-and-pitch', 50, 65, 3, 16, pitch=70),
    _wg('no-db', 50, 5, 7, 16, no_db=True),
    # segments 0 and 1 hold the same rows: c0 S0 + c1 S1 is exactly +0
    _wg('cancel', 50, 5, 7, 16, cancel=True),
    _wg('cancel-head', 24, 65536, 1, 8, coef=(-0.125, 0.125, 1.0), cancel=True),
]


def wgrad_case(case, exact):
  """(data, keyword arguments of dense_wgrad / wgrad_bars) of a case."""
  rows, seg = case['rows'], case['seg']
  d = wgrad_data(100 + rows + case['Cin'] + case['Cout'], rows, case['Cin'],
                 case['Cout'], case['ntail'], exact)
  if case.get('cancel'):
    d['x'][seg:2 * seg] = d['x'][:seg]
    d['dz'][seg:2 * seg] = d['dz'][:seg]
  return d, dict(tail_row0=rows - case['ntail'], dz=d['dz'], seg_rows=seg,
                 coef=case['coef'], bias_rows=case['bias_rows'])


# ---------------------------------------------------------------------------
# planted faults (host tests: the bars / bit equality must reject each)
# ---------------------------------------------------------------------------
def fault_dropped_k(x, W):
  """The last K-term is not added."""
  x, W = np.array(x), np.array(W)
  x[:, -1] = 0
  return x, W


def fault_bias_column(b, j):
  b = np.array(b)
  b[j] = 0
  return b


def rejected(faulty, want, bar=None):
  """Some element of `faulty` lies outside its bar (bar None: differs at all)."""
  faulty, want = _a(faulty), _a(want)
  if bar is None:
    return bool((faulty != want).any())
  fin = np.isfinite(want)
  return bool((np.abs(faulty - want)[fin] > np.broadcast_to(bar, want.shape)[fin]).any())
