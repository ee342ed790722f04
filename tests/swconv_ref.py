"""Float64 statement of the sliding-window convolution (cg_swconv:
calciumgan_amd/csrc/swconv.hip, swconv_swp.hip) and of cg_unshuffle_fixup,
written from the comments of cg_conv_desc in include/calciumgan_hip.h, the error
bars of an f32 MFMA contraction carried through each epilogue, and the data
recipes and geometries the parity tests of tests/test_hip_swconv.py run.

Everything here is numpy float64 on the host.  tests/test_swconv_ref.py ties the
statement to float64 autograd of the oracle's layers and checks on the CPU that
the recipes can tell a wrong kernel from a right one.

One point the header leaves open is settled from the code and stated here (and
now in the header): `rowsumsq` adds the squares of the f32 epilogue result after
the channel-padding select and BEFORE it is rounded to the activation type."""
from collections import namedtuple

import numpy as np

import dense_ref as D
import pointwise_ref as R
import wgrad_ref as W

EPI_NONE, EPI_LRELU, EPI_MASK, EPI_SIGMOID, EPI_LN = 0, 1, 2, 3, 4
U = 2.0**-23  # one f32 ulp, relative (the convention of wgrad_ref.acc_bound)

# What gfx950's matrix cores do with subnormal OPERANDS of the activation type on
# cg_swconv's staging paths (False: kept, as the statement says).  The GPU test
# test_hip_swconv.py::test_subnormal_operands confirms or flips it.
FLUSH_SUBNORMAL_OPERANDS = False


# ---------------------------------------------------------------------------
# geometry of one launch
# ---------------------------------------------------------------------------
# Cr real channels of x in a pitch of Cx; shifts: tuple (one per seg samples) or None
Geom = namedtuple(
    'Geom', 'nB Lx Cr Cx taps stride off Lu N Ly y_stride y_off nphase off_step '
    'yoff_step shifts seg')


def _shifts(shifts, nB, seg):
  if shifts is None:
    return None
  shifts = tuple(int(s) for s in shifts)
  assert len(shifts) == -(-nB // seg)
  return shifts


def pitch32(c):
  return -(-c // 32) * 32


def pitch8(c):
  return -(-c // 8) * 8


def down(nB, Lu, taps, Cr, N, shifts=None, seg=1):
  """The stride-2 'same' convolution over a long side of 2 Lu rows (left pad (taps
  - 2) // 2): Conv1D forward, Conv1DTranspose input gradient."""
  return Geom(nB, 2 * Lu, Cr, pitch32(Cr), taps, 2, -((taps - 2) // 2), Lu, N, Lu, 1, 0,
              1, 0, 0, _shifts(shifts, nB, seg), seg)


def up(nB, Lu, k, Cr, N, shifts=None, seg=1, swap_rows=False):
  """The two stride-1 phases of a k-tap stride-2 transposed convolution (k / 2
  taps each): output rows 2 u + z.  swap_rows: the phases' rows the other way
  round (odd y_off, yoff_phase_step -1) -- not a convolution, a launch."""
  pl = (k - 2) // 2
  offs = []
  for p in (0, 1):
    kk0 = (p + pl) & 1
    offs.append((p + pl - kk0) // 2 - (k // 2 - 1))
  return Geom(nB, Lu, Cr, pitch32(Cr), k // 2, 1, offs[0], Lu, N, 2 * Lu, 2,
              1 if swap_rows else 0, 2, offs[1] - offs[0], -1 if swap_rows else 1,
              _shifts(shifts, nB, seg), seg)


def dense(nB, Lu, Cr, N):
  """The 1-tap launch: a Dense on the last axis."""
  return Geom(nB, Lu, Cr, pitch32(Cr), 1, 1, 0, Lu, N, Lu, 1, 0, 1, 0, 0, None, 1)


def K_of(G):
  return G.taps * G.Cx


def gid(G):
  """Short pytest id of a geometry."""
  s = 's{}t{}-{}x{}-c{}of{}-n{}'.format(G.stride, G.taps, G.nB, G.Lu, G.Cr, G.Cx, G.N)
  if G.nphase == 2:
    s += '-ph2' + ('swap' if G.y_off else '')
  if G.shifts is not None:
    s += '-sh' + '.'.join(str(v) for v in G.shifts[:4]) + 'seg{}'.format(G.seg)
  return s


# ---------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------
def _mm(X, Wt):
  """(b, u, c) x (c, n) with IEEE semantics for non-finite values."""
  if np.isfinite(X).all() and np.isfinite(Wt).all():
    return X @ Wt
  with np.errstate(invalid='ignore', over='ignore'):
    return np.einsum('buc,cn->bun', X, Wt)


def linear(G, x, Wl, bias=None, off_delta=0, plain_reflected=False):
  """lin[z][b, u, n] = bias[n] + sum_{tap, c} xs[b, stride u + off_z + tap, c] Wl[z][tap][c][n],
  x (nB, Lx, Cr), Wl (nphase, taps, Cr, N).  Rows of xs outside [0, Lx) do not take
  part (selected away: an inf in a weight meets no zero there).  off_delta,
  plain_reflected (reflected rows of the shuffle read their own row): mutants."""
  x = np.asarray(x, np.float64)
  xs = W.shuffled(x, G.shifts, G.seg)
  if plain_reflected and G.shifts is not None:
    for b in range(G.nB):
      t = W.reflected_rows(G.shifts[b // G.seg], G.Lx)
      xs[b, t] = x[b, t]
  Wl = np.asarray(Wl, np.float64)
  u = np.arange(G.Lu)
  lin = np.zeros((G.nphase, G.nB, G.Lu, G.N))
  for z in range(G.nphase):
    for tap in range(G.taps):
      r = G.stride * u + G.off + z * G.off_step + off_delta + tap
      ok = (r >= 0) & (r < G.Lx)
      if not ok.any():
        continue
      with np.errstate(invalid='ignore'):
        lin[z][:, ok] += _mm(xs[:, r[ok], :], Wl[z, tap])
    if bias is not None:
      lin[z] += np.asarray(bias, np.float64)
  return lin


def rows_of(G, z):
  """Output rows of phase z: y_stride u + y_off + z yoff_phase_step."""
  return G.y_stride * np.arange(G.Lu) + G.y_off + z * G.yoff_step


def place(G, lin, fill=0.0):
  """(nphase, nB, Lu, N) -> (nB, Ly, N) in the geometry of y, and the (Ly,) mask of
  the rows the launch addresses (every other row of y is left untouched)."""
  out = np.full((G.nB, G.Ly, G.N), fill, np.float64)
  own = np.zeros(G.Ly, bool)
  for z in range(G.nphase):
    t = rows_of(G, z)
    out[:, t] = lin[z]
    own[t] = True
  return out, own


def lrelu(v, alpha):
  with np.errstate(invalid='ignore'):
    return np.maximum(v, alpha * v)


def mask_factor(mask_src, alpha, ge=False):
  """mask_src > 0 ? 1 : alpha -- -0, NaN and negative values give alpha.  ge: the
  mutant that takes >= 0."""
  m = np.asarray(mask_src, np.float64)
  with np.errstate(invalid='ignore'):
    return np.where((m >= 0) if ge else (m > 0), 1.0, alpha)


def epilogue(v, epi, alpha, mask_src=None, row_scale=None, ge=False):
  """epi(v * row_scale[b]) for the pointwise epilogues, v in the geometry of y."""
  if row_scale is not None:
    with np.errstate(invalid='ignore'):
      v = v * np.asarray(row_scale, np.float64)[:, None, None]
  if epi == EPI_NONE:
    return v
  if epi == EPI_LRELU:
    return lrelu(v, alpha)
  if epi == EPI_MASK:
    with np.errstate(invalid='ignore'):
      return v * mask_factor(mask_src, alpha, ge)
  assert epi == EPI_SIGMOID
  return D.sigmoid(v)


def swconv(G, x, Wl, bias=None, epi=EPI_NONE, alpha=0.3, mask_src=None, row_scale=None,
           **mut):
  """The header's formula: (y, own) with y (nB, Ly, N) float64 BEFORE the store's
  rounding and own (Ly,) the rows the launch addresses.  Channels [N, Cy) of an
  addressed row are +0; the callers compare them separately."""
  ge = mut.pop('ge', False)
  bias_after = mut.pop('bias_after', False)
  lin = linear(G, x, Wl, None if bias_after else bias, **mut)
  v, own = place(G, lin)
  y = epilogue(v, epi, alpha, mask_src, row_scale, ge)
  if bias_after and bias is not None:
    y = y + np.asarray(bias, np.float64)
  return y, own


def layernorm(pre, gamma, beta, eps, alpha, f16):
  """CG_EPI_LN_LRELU: y = the pre-activation rounded to the activation type; the
  statistics are those of the ROUNDED values over the N real channels (biased
  variance); ln_h = lrelu((y - mean) rstd gamma + beta).  Returns y, h, mean, rstd."""
  y = R.round_act(pre, f16)
  with np.errstate(invalid='ignore'):
    mean = y.mean(axis=-1)
    var = ((y - mean[..., None])**2).mean(axis=-1)
    rstd = 1.0 / np.sqrt(var + eps)
    t = (y - mean[..., None]) * rstd[..., None] * gamma + beta
  return y, lrelu(t, alpha), mean, rstd


def out_shift_rows(s, Ly):
  """Where output row t of a sample with out_shift s is stored: (direct t -> row r of
  y, reflected t -> row j of side).  r = shuffle_src(t, s, Ly) on the direct branch."""
  t = np.arange(Ly)
  if s > 0:
    side = t >= Ly - s
    return t[~side], t[~side] + s, t[side], t[side] - (Ly - s)
  side = t < -s
  return t[~side], t[~side] + s, t[side], t[side]


def swconv_out_shifts(G, x, Wl, out_shifts, out_seg, side_rows, f16, bias=None,
                      epi=EPI_NONE, alpha=0.3, mask_src=None):
  """cg_conv_desc.out_shifts (every row of y addressed: y_stride 1 or two phases).
  Direct rows land at r = shuffle_src(t); bias as usual; MASK reads mask_src at row r
  and masks the value ROUNDED to the activation type (the unfused form stores this
  gradient before masking); reflected rows go unmasked to side[b][j].  Returns (y,
  y_own (nB, Ly), side, side_own (nB, side_rows)), float64 before the store."""
  v, own = place(G, linear(G, x, Wl, bias))
  assert own.all() and epi in (EPI_NONE, EPI_MASK)
  y = np.zeros_like(v)
  y_own = np.zeros((G.nB, G.Ly), bool)
  side = np.zeros((G.nB, side_rows, G.N))
  side_own = np.zeros((G.nB, side_rows), bool)
  for b in range(G.nB):
    td, r, ts, j = out_shift_rows(int(out_shifts[b // out_seg]), G.Ly)
    val = v[b, td]
    if epi == EPI_MASK:
      with np.errstate(invalid='ignore'):
        val = R.round_act(val, f16) * mask_factor(mask_src[b, r], alpha)
    y[b, r], y_own[b, r] = val, True
    side[b, j], side_own[b, j] = v[b, ts], True
  return y, y_own, side, side_own


def unshuffle_fixup(side, h, delta, shifts, seg, alpha):
  """cg_unshuffle_fixup: per sample with shift s, delta[b, r] = 0 for the |s| rows no
  output row maps to ([0, s) for s > 0, [w - |s|, w) for s < 0), and delta[b, r] +=
  side[b, j] (h[b, r] > 0 ? 1 : alpha) for the |s| reflected rows (s > 0: r = w - 2 - j;
  s < 0: r = |s| - j).  Float64 before the store."""
  out = np.array(delta, np.float64)
  w = out.shape[1]
  for b in range(out.shape[0]):
    s = int(shifts[b // seg])
    n = abs(s)
    for j in range(n):
      r = w - 2 - j if s > 0 else n - j
      out[b, r] = out[b, r] + side[b, j] * mask_factor(h[b, r], alpha)
    if s > 0:
      out[b, :n] = 0.0
    elif s < 0:
      out[b, w - n:] = 0.0
  return out


def rowsumsq(y, own):
  """rowsumsq[b] = sum over the addressed rows and the N real channels of the f32
  epilogue result squared (before the store's rounding; the padding adds zeros)."""
  return (np.asarray(y, np.float64)[:, own]**2).sum(axis=(1, 2))


# ---------------------------------------------------------------------------
# bars (derived, never measured)
# ---------------------------------------------------------------------------
def acc_bound(G, x, Wl, bias=None, ksplit=1):
  """Error bar of bias + the f32 MFMA contraction, in the geometry of y:

      gamma(K + P) (sum |xs| |Wl| + |bias|),  gamma(k) = k u / (1 - k u), u = 2^-23,

  K = taps Cx terms, P = the extra additions: ksplit - 1 joins and 1 for the bias.
  Operands are values of the activation type, so every product is exact in f32; a
  sum of K terms in any order is K - 1 additions, each rounding its result by at
  most one ulp (a truncating adder included), every intermediate bounded by the sum
  of magnitudes (wgrad_ref.acc_bound has the same argument)."""
  P = (ksplit - 1) + (1 if bias is not None else 0)
  mag = linear(G, np.abs(x), np.abs(Wl), None if bias is None else np.abs(bias))
  return W._gamma(K_of(G) + P) * place(G, mag)[0]


def epilogue_bound(acc_err, v, y, epi, row_scale=None):
  """acc_err carried through an f32 epilogue, v = bias + sum (float64), y = the
  statement's result.  row_scale: one product, |rs| acc_err + u |v rs|.  LRELU / MASK:
  Lipschitz constant <= 1 and one product with the f32 slope, + u |y|.  SIGMOID:
  dense_ref.sigmoid_bar (its slope 1/4 times the bar of its argument plus the
  project's bar of the fast-exponential form, for |t| <= dense_ref.T_MAX)."""
  e = np.array(acc_err, np.float64)
  if row_scale is not None:
    rs = np.abs(np.asarray(row_scale, np.float64))[:, None, None]
    e = e * rs + U * np.abs(v) * rs
  if epi in (EPI_LRELU, EPI_MASK):
    e = e + U * np.abs(y)
  elif epi == EPI_SIGMOID:
    e = D.sigmoid_bar(e, y)
  return e


def rounded_spread(pre, err, f16):
  """How far the kernel's rounded pre-activation may lie from round_act(pre) when
  its f32 value is within err of pre: rounding is monotone, so it lies between the
  roundings of pre -+ err -- zero unless pre is within err of a rounding boundary."""
  r = R.round_act(pre, f16)
  return np.maximum(R.round_act(pre + err, f16) - r, r - R.round_act(pre - err, f16))


def layernorm_bounds(pre, err, gamma, beta, eps, alpha, f16):
  """Bars (h, mean, rstd) of the fused LayerNorm as the kernels evaluate it in f32:
  s1 = sum v, s2 = sum v^2 over the N rounded pre-activations (any order, two waves),
  mean = s1 / N, var = max(s2 / N - mean^2, 0), rstd = rsqrt(var + eps), h = lrelu((v -
  mean) rstd gamma + beta).  Two parts, with d_i = rounded_spread, a_i = v_i - mean and
  U24 = 2^-24 per rounding.
  (1) The kernel's rounded values v + delta, |delta_i| <= d_i, have other EXACT statistics:
    mean moves by at most sum d / N;
    var(v + delta) - var(v) = (2 / N) sum a_i delta_i + var(delta): at most (2 / N) sum |a_i| d_i +
    sum d_i^2 / N  (the common shift of v and mean cancels: |a|, not |v|, multiplies d).
  (2) The f32 evaluation of the E[v^2] - mean^2 form on those values (w = |v| + d):
    mean: U24 sum w  (sum_bound / N) + 2 U24 |mean|            (1 / N, the product)
    q = s2 / N: U24 sum w^2 + 2 U24 q
    var = q - mean^2: e_q + 2 |mean| e_mean + e_mean^2 + U24 mean^2 + U24 |var|
      -- with q = var + mean^2 this is ~ (N + 4) U24 (var + mean^2): relative to var, the
      amplification (1 + mean^2 / var) of the cancellation, explicit in the mean^2 terms.
  Then s = var + eps: e_var + U24 s;  rstd: its change over [s - e_s, s] plus 2 ulp of the
  hardware reciprocal square root (4 U24 rstd);  a: d + e_mean + U24 |a|;  p = a rstd: e_a
  rstd + |a| e_rstd + e_a e_rstd + U24 |p|;  t = p gamma + beta: e_p |gamma| + U24 |p gamma| +
  U24 |t|;  lrelu: Lipschitz <= 1, + U24 |t|."""
  U24 = R.U32
  y, h, mean, rstd = layernorm(pre, gamma, beta, eps, alpha, f16)
  N = y.shape[-1]
  d = rounded_spread(pre, err, f16)
  a = y - mean[..., None]
  w = np.abs(y) + d
  q = (w * w).mean(axis=-1)
  var = (a * a).mean(axis=-1)
  f_mean = U24 * w.sum(axis=-1) + 2 * U24 * (np.abs(mean) + d.mean(axis=-1))
  e_mean = d.mean(axis=-1) + f_mean
  f_q = U24 * (w * w).sum(axis=-1) + 2 * U24 * q
  m_hi = np.abs(mean) + d.mean(axis=-1)
  flip = (2 * np.abs(a) * d + d * d).mean(axis=-1)
  e_var = (flip + f_q + 2 * m_hi * f_mean + f_mean**2 + U24 * m_hi**2 +
           U24 * (var + flip))
  s = var + eps
  e_s = e_var + U24 * (s + e_var)
  assert (e_s < s).all(), 'the variance bar reaches var + eps: no bar on rstd'
  e_rstd = (1.0 / np.sqrt(s - e_s) - 1.0 / np.sqrt(s)) + 4 * U24 * (rstd + 1.0 / np.sqrt(s - e_s))
  e_a = d + e_mean[..., None] + U24 * np.abs(a)
  p = a * rstd[..., None]
  e_p = (e_a * rstd[..., None] + np.abs(a) * e_rstd[..., None] + e_a * e_rstd[..., None] +
         U24 * np.abs(p))
  t = p * gamma + beta
  e_h = e_p * np.abs(gamma) + U24 * np.abs(p * gamma) + 2 * U24 * np.abs(t)
  return e_h, e_mean, e_rstd


def rowsumsq_bound(y, err, own):
  """sum 2 |v| err(v) + err^2 over a sample's outputs, plus sum_bound(v^2) for the
  f32 sum of the squares in any order (workgroup shares, atomics or slots)."""
  y = np.asarray(y, np.float64)
  y, err = y[:, own], np.broadcast_to(np.asarray(err, np.float64), y.shape)[:, own]
  return ((2 * np.abs(y) * err + err * err).sum(axis=(1, 2)) +
          R.sum_bound((y * y).reshape(y.shape[0], -1), axis=1))


# ---------------------------------------------------------------------------
# an f32 emulation (sequential over K; tests/test_swconv_ref.py holds it against
# the bars -- no kernel involved)
# ---------------------------------------------------------------------------
def linear_f32(G, x, Wl, bias=None):
  xs = W.shuffled(x, G.shifts, G.seg).astype(np.float32)
  Wl = np.asarray(Wl, np.float32)
  u = np.arange(G.Lu)
  lin = np.zeros((G.nphase, G.nB, G.Lu, G.N), np.float32)
  for z in range(G.nphase):
    for tap in range(G.taps):
      r = G.stride * u + G.off + z * G.off_step + tap
      ok = (r >= 0) & (r < G.Lx)
      for c in range(G.Cr):
        lin[z][:, ok] += xs[:, r[ok], c, None] * Wl[z, tap, c][None, None, :]
    if bias is not None:
      lin[z] += np.asarray(bias, np.float32)
  return lin


# ---------------------------------------------------------------------------
# data recipes (numpy only: the CPU tests check them, the GPU tests run them)
# ---------------------------------------------------------------------------
def seed_of(G):
  return (2000 + 7 * G.nB + 13 * G.Lu + 31 * G.taps + 3 * G.Cr + 5 * G.N + 17 * G.stride +
          G.nphase + (sum(abs(s) for s in G.shifts) if G.shifts else 0))


def wshape(G):
  return (G.nphase, G.taps, G.Cr, G.N)


def real_recipe(G, f16, sigmoid=False):
  """x = round_act(randn), Wl = round_act(randn / sqrt(taps Cr)) (pre-activations of
  unit scale; halved until they lie within dense_ref.T_MAX where a sigmoid
  follows), bias = f32(0.5 randn).  Every sample starts with +-0."""
  rng = np.random.RandomState(seed_of(G))
  x = R.round_act(rng.randn(G.nB, G.Lx, G.Cr), f16)
  x[:, 0, :2] = [0.0, -0.0]
  Wl = rng.randn(*wshape(G)) / np.sqrt(G.taps * G.Cr)
  bias = (0.5 * rng.randn(G.N)).astype(np.float32).astype(np.float64)
  Wl = R.round_act(Wl, f16)
  while sigmoid and np.abs(linear(G, x, Wl, bias)).max() > D.T_MAX:
    Wl = Wl / 2
  return x, Wl, bias


def exact_recipe(G, f16):
  """x = +-(2^(s-1) + j) 2^-(s-1), j uniform in [0, 2^(s-1)): every one of the s = 8
  (bf16) / 11 (fp16) significand bits in use at the one exponent [1, 2); Wl in {0, +-1,
  +-1/2, +-1/4}, zero often enough that sum |x Wl| stays below 2^6 (bf16) / 2^9 (fp16);
  bias a multiple of 1/4.  Every product is a multiple of 2^-9 / 2^-12 and every
  partial sum in every order is exact in f32 (at most 2^15 / 2^21 units), so a
  correct kernel matches bit for bit -- while most sums carry more bits than the
  activation type keeps.  Planted at sample 0, phase 0, output row Lu / 2, through
  the first tap whose source row exists (h = 2^(s-1)):
    column 0: 1 x 1 + (h + 2) / h x 1/4 -- an exact tie whose even neighbour is below;
    column 1: (h + 1) / h x 1 + (h + 2) / h x 1/4 -- an exact tie whose even neighbour is above;
    columns 2 / 3: 2^15 x (+-1) twice = +-2^16: beyond +-65504 in fp16 (+-inf), exact in
    bf16.  Channels 4 and 5 (the 2^15) meet no other weight.
  Returns x, Wl, bias, plants = {'ties': [(b, row, n, value)], 'over': [(b, row, n, sign)]}."""
  assert G.Cr >= 6 and G.N >= 4
  rng = np.random.RandomState(seed_of(G) + 1)
  s = 11 if f16 else 8
  h = 2**(s - 1)
  x = (h + rng.randint(0, h, (G.nB, G.Lx, G.Cr))) / float(h)
  x *= rng.choice([-1.0, 1.0], x.shape)
  cap = 2.0**9 if f16 else 2.0**6
  live = min(0.75, cap / (2.0 * 0.9 * G.taps * G.Cr))  # E|x Wl| ~ 1.5 x 0.6 per live term
  mag = 2.0**-rng.randint(0, 3, wshape(G))
  Wl = mag * rng.choice([-1.0, 1.0], mag.shape) * (rng.rand(*mag.shape) < live)
  bias = rng.randint(-8, 9, G.N) / 4.0
  bias[:4] = 0.0
  u0 = G.Lu // 2
  tap = max(0, -(G.stride * u0 + G.off))
  assert tap < G.taps
  src = int(W.shuffle_src(G.stride * u0 + G.off + tap, G.shifts[0] if G.shifts else 0, G.Lx))
  Wl[0, :, :, :4] = 0.0
  Wl[:, :, 4:6, :] = 0.0
  x[0, src, :6] = [1.0, (h + 2.0) / h, (h + 1.0) / h, (h + 2.0) / h, 2.0**15, 2.0**15]
  Wl[0, tap, 0, 0], Wl[0, tap, 1, 0] = 1.0, 0.25
  Wl[0, tap, 2, 1], Wl[0, tap, 3, 1] = 1.0, 0.25
  Wl[0, tap, 4:6, 2], Wl[0, tap, 4:6, 3] = 1.0, -1.0
  row = G.y_stride * u0 + G.y_off
  plants = {'ties': [(0, row, 0, 1.0 + (h + 2.0) / (4 * h)),
                     (0, row, 1, (h + 1.0) / h + (h + 2.0) / (4 * h))],
            'over': [(0, row, 2, 1.0), (0, row, 3, -1.0)]}
  return x, Wl, bias, plants


def subnormal_recipe(G, f16):
  """x = +-j times the smallest subnormal, j in [1, 2^(s-1)) (fp16: 2^-24 .. 2^-14;
  bf16: 2^-133 .. 2^-126), against Wl = +-2^10 on one tap and channel per output
  column (one product per output: nothing to round), no bias.  The statement
  keeps the subnormals; FLUSH_SUBNORMAL_OPERANDS says what the GPU run saw."""
  rng = np.random.RandomState(seed_of(G) + 2)
  s = 11 if f16 else 8
  tiny = R.act_limits(f16)[0]
  x = rng.randint(1, 2**(s - 1), (G.nB, G.Lx, G.Cr)) * tiny
  x *= rng.choice([-1.0, 1.0], x.shape)
  Wl = np.zeros(wshape(G))
  for z in range(G.nphase):
    for n in range(G.N):
      Wl[z, rng.randint(G.taps), rng.randint(G.Cr), n] = 2.0**10 * rng.choice([-1.0, 1.0])
  return x, Wl


def flush(v, f16):
  return D.flush(v, f16)


# ---------------------------------------------------------------------------
# named geometries (shared by the CPU and the GPU tests)
# ---------------------------------------------------------------------------
MIXED3 = (1, -2, 0)
# software-pipelined tiles: exactly 24 taps at stride 2 / 12 per phase at stride 1,
# CK = 32, S >= 16 mt, nseg <= 8: Lu = 64 with nB = 3 (a ragged last tile that holds
# several samples on the 128-row tiles and up), and Lu = tile rows
SWP_DOWN = down(3, 64, 24, 32, 40, MIXED3, 1)
SWP_DOWN_NARROW = down(3, 64, 24, 38, 40, MIXED3, 1)
SWP_UP = up(3, 64, 24, 32, 40)
SWP_UP_LN = up(3, 64, 24, 32, 102)
# classic tiles
CLASSIC_DOWN = [down(3, 64, 24, 32, 40, MIXED3, 1),      # one chunk
                down(5, 16, 8, 96, 102, (1, -1, 0), 2),   # three chunks, several samples per tile
                down(3, 4, 2, 32, 6, (3, -3, 0), 1),      # Lu = 4, shifts +-(Lx / 2 - 1)
                down(3, 64, 24, 38, 130, MIXED3, 1)]      # narrow last chunk, a second column tile
CLASSIC_UP = [up(3, 64, 24, 32, 40), up(5, 16, 8, 64, 102), up(3, 4, 8, 32, 6),
              up(3, 64, 24, 32, 64, swap_rows=True)]
DENSE = [dense(3, 64, 38, 102), dense(5, 16, 96, 130), dense(3, 4, 32, 6)]
# a 40-channel chunk (CK = 40: c8 = 5, the non-uniform K walk of the MFMA-16 tiles)
NON_UNI = Geom(3, 128, 40, 40, 8, 2, -3, 64, 40, 64, 1, 0, 1, 0, 0, MIXED3, 1)
# LN: N = 102 and N = 128, rows of one tile and two tiles, several samples per tile
LN_GEOMS = [up(3, 64, 24, 32, 102), up(2, 128, 24, 32, 128), up(5, 16, 8, 64, 102)]
NON_UNI_UP = up(3, 64, 8, 40, 40)._replace(Cx=40)
# split-K: four / two / four channel chunks
SPLIT_CLASSIC = down(3, 64, 8, 128, 40, MIXED3, 1)
SPLIT_SWP2 = down(3, 64, 24, 64, 40, MIXED3, 1)
SPLIT_SWP4 = down(3, 64, 24, 128, 40, MIXED3, 1)
# Lu = the tile's rows and twice that (one sample per tile, no ragged tile), by tile rows
FULL_TILE = {r: up(2, r, 24, 32, 40) for r in (64, 128, 256, 512)}
TWO_TILES = {r: up(2, 2 * r, 8, 32, 40) for r in (64, 128, 256)}
# N = 102 in a pitch of 104: the epilogue cases and the penalty norm (128-row tiles)
EPI_GEOM = down(3, 64, 24, 32, 102, MIXED3, 1)
SSQ_GEOMS = {Lu: up(2, Lu, 24, 32, 102) for Lu in (128, 256)}
# shifts of +-(Lx - 1), mixed signs within a launch, a segment larger than the batch
# (exact recipe only)
SHIFT_GEOMS = [down(5, 8, 8, 32, 40, (15, -15, 0, 1, -1), 1),
               down(5, 16, 8, 32, 40, (3,), 8),
               down(3, 64, 24, 32, 40, (127, -127, 0), 1)]
# the non-finite source rows: N = 38 in a pitch of 40 (two padding columns whose zero
# weights meet the NaN rows), with and without shifts, one and two channel chunks
SPECIAL_GEOMS = {(shifted, split): down(3, 64, 24, 64 if split else 32, 38,
                                        MIXED3 if shifted else (0, 0, 0), 1)
                 for shifted in (0, 1) for split in (0, 1)}
# the classic tiles' further shapes: 1 / 2 / 8 taps, Lu = 4 and 16, Cx = 64 / 96, N = 6 /
# 64 / 102 / 130, the two phases' rows the other way round
CLASSIC_MORE = DENSE + CLASSIC_DOWN[1:3] + CLASSIC_UP[1:]
# every admitted kernel size next to 24, 8 and 2 (all of them on the classic tiles:
# the software-pipelined ones take 12 taps per pass only).  With CK = 32 a chunk is
# walked in ceil16(4 taps) K groups: taps = 6, 10, 14, 18, 22 at stride 2 and k / 2 = 2, 3,
# 5, 6, 7, 9, 10, 11 per phase end in padded groups (the tap clamped, the operand zero);
# the narrow last chunk clamps to half_taps - 1 = 2 .. 10; k = 6, 10, 14, 18, 22 give both
# phases one window offset (off_step 0) and start phase 0 on an even tap
TAP_SWEEP = (4, 6, 10, 12, 14, 16, 18, 20, 22)
K_DOWN = {k: down(3, 64, k, 32, 40, MIXED3, 1) for k in TAP_SWEEP}
K_DOWN_NARROW = {k: down(3, 64, k, 38, 40, MIXED3, 1) for k in TAP_SWEEP if k >= 6}
K_UP = {k: up(3, 64, k, 32, 40) for k in TAP_SWEEP}
K_UP_LN = {k: up(3, 64, k, 32, 102) for k in (6, 22)}
# three chunks, several samples per tile, segments of two: the padded groups of a
# middle chunk
K_DOWN_MULTI = {k: down(5, 16, k, 96, 102, (1, -1, 0), 2) for k in TAP_SWEEP}
# out_shifts + fix-up and the shift edges away from 24 taps: an odd half_taps and a
# multiple of 4
FIXUP_K = (6, 12)
SHIFT_GEOMS_K = [down(5, 8, 6, 32, 40, (15, -15, 0, 1, -1), 1),
                 down(3, 64, 12, 32, 40, (127, -127, 0), 1)]


def sweep_geoms():
  return (list(K_DOWN.values()) + list(K_DOWN_NARROW.values()) + list(K_UP.values()) +
          list(K_UP_LN.values()) + list(K_DOWN_MULTI.values()))


# shapes where one dropped K-step is below 20 bars too often (K = 24 x 128)
# ... and the three-chunk sweep geometries from K = 14 x 96 on (16 x 96 holds under the
# linear epilogue of sweep_epi)
K_MULTI_EXACT_ONLY = [K_DOWN_MULTI[k] for k in (14, 18, 20, 22)]
EXACT_ONLY = [SPLIT_SWP4] + K_MULTI_EXACT_ONLY


def sweep_epi(G):
  """The epilogue the dispatch sweep runs a geometry with: LeakyReLU + bias, except
  where K = taps Cx reaches 24 x 64 -- there one dropped K-step moves a NEGATIVE output
  (slope 0.3) by less than 20 bars too often, and the sweep stores the linear result.
  (tests/test_swconv_ref.py checks the mutants under this choice.)"""
  return EPI_NONE if K_of(G) >= 24 * 64 else EPI_LRELU


def real_geoms():
  out = ([SWP_DOWN, SWP_DOWN_NARROW, SWP_UP, SWP_UP_LN, NON_UNI] + CLASSIC_DOWN +
         CLASSIC_UP + DENSE + LN_GEOMS + [NON_UNI_UP, SPLIT_CLASSIC, SPLIT_SWP2, EPI_GEOM] + list(SPECIAL_GEOMS.values()) +
         list(FULL_TILE.values()) + list(TWO_TILES.values()) + list(SSQ_GEOMS.values()) +
         sweep_geoms())
  seen, uniq = set(), []
  for G in out:
    if G not in seen and G not in EXACT_ONLY:
      seen.add(G)
      uniq.append(G)
  return uniq
