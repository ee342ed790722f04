"""Float64 statements of the normalisation family of the C ABI
(calciumgan_amd/csrc/pointwise.hip): cg_ln_lrelu_fwd / cg_ln_lrelu_bwd,
cg_bn_stats / cg_bn_apply / cg_bn_bwd and cg_unshuffle_mask, written from the
comments of include/calciumgan_hip.h, with the error bars of an f32 evaluation
of each formula.

Everything here is numpy float64 on the host.  Every statement takes values
already rounded to the type the kernel reads (activations: round_act; f32
parameters and statistics: f32 values) and returns the expected outputs BEFORE
the store's rounding plus their bars.  tests/test_norm_ref.py ties each
statement to float64 autograd and caps every bar; tests/test_hip_norm.py runs
the kernels against them.

Bars.  U = 2^-24 is one f32 rounding, relative.  A bar is counted from the
operations of the formula: k U |x| for a value that went through k roundings,
pointwise_ref.sum_bound (n U sum |terms|: n terms added in ANY order, one
rounding of each term included) for a sum, and wherever terms cancel the bar
multiplies U by the SUM OF THE MAGNITUDES that met, never by the small result.
A fused multiply-add has fewer roundings than the separate operations counted
here, so the bars hold whichever the compiler chose.  The hardware reciprocal
square root is taken as 2 ulp (4 U), as swconv_ref.layernorm_bounds does.  An
f32 result below the smallest normal number is rounded at 2^-149 or flushed to
zero, not rounded relatively: every f32 output's bar carries FLOOR = 2^-126 per
term that may have been (the planted subnormals make such terms; a stored
activation needs none: its own ulp is the larger in fp16, and in bf16 the
subnormal products round to the same neighbours).  No bar is a measured number."""
import numpy as np

import pointwise_ref as R
import swconv_ref as S
import wgrad_ref as W

U = R.U32
RSQ = 4 * U  # the hardware reciprocal square root: 2 ulp
FLOOR = 2.0**-126  # the smallest normal f32: what a flushed subnormal result loses at most


def _f64(*a):
  return [np.asarray(x, np.float64) for x in a]


def mask_factor(h, alpha):
  """h > 0 ? 1 : alpha -- +0, -0, negative values and NaN give alpha."""
  with np.errstate(invalid='ignore'):
    return np.where(np.asarray(h, np.float64) > 0, 1.0, alpha)


# ---------------------------------------------------------------------------
# LayerNorm + LeakyReLU
# ---------------------------------------------------------------------------
def ln_fwd(y, gamma, beta, eps, alpha, f16):
  """cg_ln_lrelu_fwd on y (rows, C) of the activation type: (h, mean, rstd) with
  mean / biased variance over the C real channels, rstd = 1 / sqrt(var + eps), h =
  lrelu((y - mean) rstd gamma + beta), lrelu(t) = t > 0 ? t : alpha t
  (swconv_ref.layernorm: y is representable, so its rounding is the identity),
  and the bars (e_h, e_mean, e_rstd) of the standalone kernels' TWO-PASS f32
  evaluation, a_i = y_i - mean:
    mean = (sum y) (1 / C): sum_bound(y) / C + 2 U |mean|        (1 / C, the product)
    d_i = y_i - mean_f: the exact shift delta = mean_f - mean, |delta| <= e_mean, and
      one rounding.  sum_i a_i = 0, so sum (a_i - delta)^2 = sum a_i^2 + C delta^2: the
      shift adds delta^2 to the variance and nothing of first order
    var = (sum d_i^2) (1 / C): e_mean^2 + (C + 4) U (var + e_mean^2)
      -- two roundings through the square of d, sum_bound's C U for the squares and
      their sum, 1 / C and the product; no mean^2 term: the two-pass form does not
      cancel, which is what makes this bar no looser than the one-pass bar of
      swconv_ref.layernorm_bounds
    s = var + eps: e_var + U s;  rstd: its change over [s - e_s, s] + 4 U rstd
    a = y - mean: e_mean + U |a|;  p = a rstd: e_a rstd + |a| e_rstd + e_a e_rstd + U |p|
    t = p gamma + beta: e_p |gamma| + U |p gamma| + U |t|;  lrelu: Lipschitz <= 1, + U |t|."""
  y, gamma, beta = _f64(y, gamma, beta)
  _, h, mean, rstd = S.layernorm(y, gamma, beta, eps, alpha, f16)
  C = y.shape[-1]
  a = y - mean[..., None]
  var = (a * a).mean(axis=-1)
  e_mean = R.sum_bound(y, axis=-1) / C + 2 * U * np.abs(mean) + FLOOR
  e_var = e_mean**2 + (C + 4) * U * (var + e_mean**2)
  s = var + eps
  e_s = e_var + U * (s + e_var)
  assert (e_s < s).all(), 'the variance bar reaches var + eps: no bar on rstd'
  lo = 1.0 / np.sqrt(s - e_s)
  e_rstd = (lo - rstd) + RSQ * lo
  e_a = e_mean[..., None] + U * np.abs(a)
  p = a * rstd[..., None]
  e_p = (e_a * rstd[..., None] + np.abs(a) * e_rstd[..., None] +
         e_a * e_rstd[..., None] + U * np.abs(p))
  t = p * gamma + beta
  e_h = e_p * np.abs(gamma) + U * np.abs(p * gamma) + 2 * U * np.abs(t)
  return dict(h=h, mean=mean, rstd=rstd, e_h=e_h, e_mean=e_mean, e_rstd=e_rstd)


def ln_bwd(dh, h, y, mean, rstd, gamma, alpha):
  """cg_ln_lrelu_bwd.  mean / rstd (rows,) are the f32 values the kernel is handed:
  GIVEN inputs, never recomputed.  With mask = h > 0 ? 1 : alpha (+-0 and NaN take
  alpha), do = dh mask, xhat = (y - mean) rstd, dyh = do gamma and mean_c the mean over
  the C real channels:
    dy = rstd (dyh - mean_c(dyh) - xhat mean_c(dyh xhat))
    dgamma = sum_rows do xhat,  dbeta = sum_rows do
  (dbias, the column sum of the STORED dy, is dbias() below: it takes the kernel's
  own output).  Bars, operation by operation:
    do: one product, U |do|;  xhat: a difference of exact inputs and a product, 2 U |xhat|;
    dyh: 2 U |dyh|
    dbeta: sum_bound(do) over the rows (its one rounding per term is do's product)
    dgamma: terms do xhat carry 3 U before their own rounding: 3 U sum |do xhat| + sum_bound
    s1 = mean_c(dyh): (U sum_c |dyh| + sum_bound_c(dyh)) / C + 2 U |s1|   (1 / C, the product)
    s2 = mean_c(dyh xhat): (4 U sum_c |dyh xhat| + sum_bound_c(dyh xhat)) / C + 2 U |s2|
    I = dyh - s1 - xhat s2 is where terms cancel; every piece enters by its magnitude:
      dyh 2 U |dyh|;  s1 e_s1;  xhat s2: |xhat| e_s2 + 3 U |xhat s2|;  the first difference
      U (|dyh| + |s1|), the second U (|dyh| + |s1| + |xhat s2|):
      e_I = 4 U |dyh| + 2 U |s1| + 4 U |xhat s2| + e_s1 + |xhat| e_s2
    dy = rstd I: |rstd| e_I + U |dy|."""
  dh, h, y, mean, rstd, gamma = _f64(dh, h, y, mean, rstd, gamma)
  rows, C = y.shape
  m, r = mean[:, None], rstd[:, None]
  do = dh * mask_factor(h, alpha)
  xh = (y - m) * r
  dyh = do * gamma
  px = dyh * xh
  s1 = dyh.mean(axis=1, keepdims=True)
  s2 = px.mean(axis=1, keepdims=True)
  I = dyh - s1 - xh * s2
  dy = r * I
  tg = do * xh
  e_s1 = ((U * np.abs(dyh).sum(axis=1) + R.sum_bound(dyh, axis=1)) / C)[:, None] + 2 * U * np.abs(s1)
  e_s2 = ((4 * U * np.abs(px).sum(axis=1) + R.sum_bound(px, axis=1)) / C)[:, None] + 2 * U * np.abs(s2)
  e_I = (4 * U * np.abs(dyh) + 2 * U * np.abs(s1) + 4 * U * np.abs(xh * s2) + e_s1 +
         np.abs(xh) * e_s2)
  e_dy = np.abs(r) * e_I + U * np.abs(dy)
  return dict(dy=dy, dgamma=tg.sum(axis=0), dbeta=do.sum(axis=0), e_dy=e_dy,
              e_dgamma=3 * U * np.abs(tg).sum(axis=0) + R.sum_bound(tg, axis=0) + rows * FLOOR,
              e_dbeta=R.sum_bound(do, axis=0) + rows * FLOOR)


def dbias(dy_stored):
  """(dbias, bar): the column sums of the STORED dy (values of the activation type,
  exact in f32: nothing but the sum rounds) -- sum_bound over the rows."""
  d = np.asarray(dy_stored, np.float64)
  return d.sum(axis=0), R.sum_bound(d, axis=0) + d.shape[0] * FLOOR


# ---------------------------------------------------------------------------
# BatchNormalization
# ---------------------------------------------------------------------------
def bn_rows_per_block(rows):
  """Rows per block of the BatchNorm column sums below the kMaxParts / workspace
  caps (rows <= 8M): 256, doubled up to 4096 while there are >= 512 blocks of twice
  the size.  bn_stats' bars follow the kernel's block structure through this."""
  rpb = 256
  while rpb < 4096 and rows // (rpb * 2) >= 512:
    rpb *= 2
  return rpb


def bn_row_lanes(Cp):
  """Row lanes of a block of the BatchNorm column sums: 256 threads over Cp / 8 channel
  groups."""
  return 256 // (Cp // 8)


def lane_sum_bound(terms, rlanes):
  """sum_bound for the column sum of n rows INSIDE ONE BLOCK of the BatchNorm kernels,
  whose order is fixed by the launch: row lane l adds rows l, l + rlanes, ... one after the
  other (m = ceil(n / rlanes) terms, m - 1 additions), then the rlanes partial sums are
  added one after the other (rlanes - 1 additions).  A term passes through at most m +
  rlanes - 2 additions, each rounding a partial sum that sum |terms| bounds, and was
  itself rounded once: (m + rlanes - 1) U sum |terms| -- sum_bound with the count of the
  terms replaced by the roundings one term can meet, never more than sum_bound (n terms
  in any order).  rlanes None: any order."""
  t = np.abs(np.asarray(terms, np.float64))
  n = t.shape[0]
  k = n if rlanes is None else min(n, -(-n // rlanes) + rlanes - 1)
  return k * U * t.sum(axis=0)


def bn_stats(y, momentum, mm=None, mv=None, rpb=None, rlanes=None):
  """cg_bn_stats on y (rows, C): mean = column mean, var = mean((y - mean)^2) (biased),
  and with the moving pair moving' = moving momentum + batch (1 - momentum).

  Bars, following the kernel's form: blocks b of n_b <= rpb rows sum d = y - K_b and d^2
  around their own first row K_b (S1_b, S2_b); the finish combines (count, mean, M2):
    mean = sum_b (S1_b + n_b K_b) / R
    var = sum_b [(S2_b - S1_b^2 / n_b) + n_b (K_b + S1_b / n_b - mean)^2] / R,   R = rows.
    d: one rounding (in the sum's bar);  e_S1_b = lane_sum_bound(d_b);  e_S2_b = 2 U S2_b +
      lane_sum_bound(d_b^2)  (rlanes = bn_row_lanes(Cp); None: sum_bound, any order)
    block sum S1_b + n_b K_b (n_b K_b exact: 13 + 11 bits) and the sum over the P blocks:
      e_sum = sum_b e_S1_b + sum_bound_b(|S1_b| + n_b |K_b|)  -- magnitudes, not the sum
    mean: e_sum / R + 2 U |mean|                                  (1 / R, the product)
    q_b = S1_b / n_b: e_S1_b / n_b + U |q_b|
    r_b = S1_b^2 / n_b: (2 |S1_b| e_S1_b + e_S1_b^2) / n_b + 2 U r_b
    M2_b = S2_b - r_b CANCELS: the operands' bars stay as they are, absolute, beside a small
      result: e_S2_b + e_r_b, and the difference's own rounding U M2_b
    dd_b = (K_b + q_b) - mean CANCELS: K_b + q_b rounds at its own magnitude, U (|K_b| + |q_b|), and
      that stays beside the small dd_b: e_q_b + U (|K_b| + |q_b|) + U |dd_b|.  The error delta of
      the f32 mean (|delta| <= e_mean) is one shift common to all blocks, and sum_b n_b (mean_b -
      mean) = 0: sum_b n_b (mean_b - mean - delta)^2 = sum_b n_b (mean_b - mean)^2 + R delta^2 -- it adds
      delta^2 to the variance and nothing of first order (as in ln_fwd)
    n_b dd_b^2: n_b (2 |dd_b| e_dd_b + e_dd_b^2) + 2 U n_b dd_b^2
    term_b = M2_b + n_b dd_b^2 (both >= 0): the above + U term_b; the P terms: sum_bound_b
    var = max(T / R, 0): e_T / R + e_mean^2 + 2 U var
    moving' = moving momentum + batch (1 - momentum): U |moving momentum| + (1 - momentum)
      e_batch + 2 U |batch (1 - momentum)| + U (|moving momentum| + |batch (1 - momentum)|)."""
  y = np.asarray(y, np.float64)
  rows, C = y.shape
  rpb = rpb or bn_rows_per_block(rows)
  mean = y.mean(axis=0)
  var = ((y - mean)**2).mean(axis=0)
  starts = range(0, rows, rpb)
  P = len(starts)
  e_sum_in, mag_sum, blocks = np.zeros(C), np.zeros(C), []
  for r0 in starts:
    blk = y[r0:r0 + rpb]
    n, K = blk.shape[0], blk[0]
    d = blk - K
    S1, S2 = d.sum(axis=0), (d * d).sum(axis=0)
    e_S1 = lane_sum_bound(d, rlanes)
    e_S2 = 2 * U * S2 + lane_sum_bound(d * d, rlanes)
    e_sum_in += e_S1
    mag_sum += np.abs(S1) + n * np.abs(K)
    blocks.append((n, K, S1, S2, e_S1, e_S2))
  e_mean = (e_sum_in + P * U * mag_sum) / rows + 2 * U * np.abs(mean) + 2 * FLOOR
  e_T_in, mag_T = np.zeros(C), np.zeros(C)
  for n, K, S1, S2, e_S1, e_S2 in blocks:
    q = S1 / n
    e_q = e_S1 / n + U * np.abs(q)
    r = S1 * S1 / n
    e_r = (2 * np.abs(S1) * e_S1 + e_S1**2) / n + 2 * U * r
    M2 = np.maximum(S2 - r, 0.0)
    e_M2 = e_S2 + e_r + U * M2
    dd = K + q - mean
    e_dd = e_q + U * (np.abs(K) + np.abs(q)) + U * np.abs(dd)
    e_nd = n * (2 * np.abs(dd) * e_dd + e_dd**2) + 2 * U * n * dd * dd
    mag = M2 + n * dd * dd
    e_T_in += e_M2 + e_nd + U * mag
    mag_T += mag
  e_var = (e_T_in + P * U * mag_T) / rows + e_mean**2 + 2 * U * var + 2 * FLOOR
  out = dict(mean=mean, var=var, e_mean=e_mean, e_var=e_var)
  if mm is not None:
    mm, mv = _f64(mm, mv)
    for k, old, new, e_new in (('mm', mm, mean, e_mean), ('mv', mv, var, e_var)):
      a, b = old * momentum, new * (1.0 - momentum)
      out[k] = a + b
      out['e_' + k] = (U * np.abs(a) + (1.0 - momentum) * e_new + 2 * U * np.abs(b) +
                       U * (np.abs(a) + np.abs(b)) + 2 * FLOOR)
  return out


def bn_apply(y, mean, var, gamma, beta, eps, alpha):
  """cg_bn_apply: out = f((y - mean) rsqrt(var + eps) gamma + beta), f(t) = max(t, alpha t)
  (alpha = 1: the identity); mean / var (C,) are the f32 values handed in.  Bar of the
  f32 evaluation: a = y - mean one rounding; rs = rsqrt(var + eps): the sum's rounding
  halves through the root, plus the hardware's 4 U: 5 U rs; p = a rs: 7 U |p|; p gamma: 8 U
  |p gamma|; + beta: U |t|; alpha t: U |t|  ->  8 U |p gamma| + 2 U |t|."""
  y, mean, var, gamma, beta = _f64(y, mean, var, gamma, beta)
  pg = (y - mean) / np.sqrt(var + eps) * gamma
  t = pg + beta
  return np.maximum(t, alpha * t), 8 * U * np.abs(pg) + 2 * U * np.abs(t)


def bn_bwd(dout, h, y, mean, var, gamma, eps, alpha, act, dgamma=None, dbeta=None):
  """cg_bn_bwd: do = dout (act ? (h > 0 ? 1 : alpha) : 1), rs = rsqrt(var + eps), xhat = (y -
  mean) rs; dbeta = sum_rows do, dgamma = sum_rows do xhat; dy = gamma rs (do - dbeta / R -
  xhat dgamma / R), R = rows.  mean / var are the f32 values handed in.  dgamma / dbeta given
  (the kernel's own stored sums): dy is evaluated with THEM, as the kernel's third launch
  does, and their bars do not enter e_dy.  Bars:
    rs: 5 U rs (bn_apply);  do: U |do|;  xhat: difference, rs, product: 7 U |xhat|
    dbeta: sum_bound(do);  dgamma: 8 U sum |do xhat| + sum_bound(do xhat)
    A = dbeta (1 / R): 2 U |A|;  B = xhat dgamma (1 / R): 7 + 3 = 10 U |B|
    I = do - A - B CANCELS: U |do| + 2 U |A| + 10 U |B| + U (|do| + |A|) + U (|do| + |A| + |B|)
      = 3 U |do| + 4 U |A| + 11 U |B|, and from the sums' own bars (pure chain only)
      e_dbeta / R + |xhat| e_dgamma / R
    G = gamma rs: 6 U |G|;  dy = G I: |G| e_I + 7 U |dy|."""
  dout, y, mean, var, gamma = _f64(dout, y, mean, var, gamma)
  rows = y.shape[0]
  do = dout * mask_factor(h, alpha) if act else dout
  rs = 1.0 / np.sqrt(var + eps)
  xh = (y - mean) * rs
  tg = do * xh
  dg_ref, db_ref = tg.sum(axis=0), do.sum(axis=0)
  e_dg = 8 * U * np.abs(tg).sum(axis=0) + R.sum_bound(tg, axis=0) + rows * FLOOR
  e_db = R.sum_bound(do, axis=0) + rows * FLOOR
  given = dgamma is not None
  dg, db = (_f64(dgamma, dbeta) if given else (dg_ref, db_ref))
  A, B = db / rows, xh * dg / rows
  I = do - A - B
  G = gamma * rs
  dy = G * I
  e_I = 3 * U * np.abs(do) + 4 * U * np.abs(A) + 11 * U * np.abs(B)
  if not given:
    e_I = e_I + e_db / rows + np.abs(xh) * e_dg / rows
  return dict(dy=dy, dgamma=dg_ref, dbeta=db_ref, e_dy=np.abs(G) * e_I + 7 * U * np.abs(dy),
              e_dgamma=e_dg, e_dbeta=e_db)


# ---------------------------------------------------------------------------
# phase unshuffle + LeakyReLU mask
# ---------------------------------------------------------------------------
def unshuffle_mask(e, h, shifts, seg, alpha):
  """cg_unshuffle_mask on e, h (nB, w, C): delta[b, r] = (h[b, r] > 0 ? 1 : alpha) sum_{t:
  shuffle_src(t, s_b, w) = r} e[b, t], s_b = shifts[b / seg] (None: 0).  A row has 0, 1 or 2
  sources.  Returns (delta, exact): the float64 value (exact: two activation values and
  a 24-bit factor fit 53 bits) and where the kernel's f32 evaluation -- the sum, then
  the product -- rounds nothing, so that the store's is the only rounding and the
  result must match round_act(delta) bit for bit; elsewhere up to two f32 roundings
  come first: one activation ulp + 2 U |delta|."""
  e, h = _f64(e, h)
  nB, w, _ = e.shape
  acc = np.zeros_like(e)
  t = np.arange(w)
  for b in range(nB):
    s = 0 if shifts is None else int(shifts[b // seg])
    np.add.at(acc[b], W.shuffle_src(t, s, w), e[b])
  delta = acc * mask_factor(h, alpha)
  fits = lambda v: v.astype(np.float32).astype(np.float64) == v
  with np.errstate(over='ignore'):
    exact = fits(acc) & fits(delta)
  return delta, exact


# ---------------------------------------------------------------------------
# data recipes (numpy only: the CPU tests cap their bars, the GPU tests run them)
# ---------------------------------------------------------------------------
def big_value(f16):
  """The large planted value: fp16's largest finite one (its square, 2^32, is nothing
  to f32); for bf16 2^60 -- the kernels square differences and add up to 2^19 of them,
  and 2^120 2^19 is finite in f32 where the square of bf16's largest value is not."""
  return 65504.0 if f16 else 2.0**60


def plant(row, f16):
  """+0, -0, the smallest subnormal of either sign at the start of a row (as far as
  it reaches)."""
  tiny = R.act_limits(f16)[0]
  vals = [0.0, -0.0, tiny, -tiny][:row.shape[-1]]
  row[..., :len(vals)] = vals


def ln_recipe(seed, rows, C, f16, big=True):
  """y = round_act(2 randn + 0.5) (the old LayerNorm test's scale), gamma = f32(rand +
  0.5), beta = f32(0.1 randn) (never 0: a constant row gives h = lrelu(beta)), dh =
  round_act(randn).  Row 0 starts with the planted zeros and subnormals (dh too); row 1
  is constant (variance exactly 0); row 2 holds big_value (forward only)."""
  rng = np.random.RandomState(seed)
  y = R.round_act(rng.randn(rows, C) * 2 + 0.5, f16)
  dh = R.round_act(rng.randn(rows, C), f16)
  gamma = (rng.rand(C) + 0.5).astype(np.float32).astype(np.float64)
  beta = (0.1 * rng.randn(C)).astype(np.float32).astype(np.float64)
  plant(y[0], f16)
  plant(dh[0, ::-1], f16)
  if rows > 1:
    y[1] = 0.75
  if rows > 2 and big:
    y[2, C // 2] = -big_value(f16)
  return y, gamma, beta, dh


def plant_mask_zeros(h, dh):
  """Zeros of both signs in h where the mask is decided: every row's channels 0 / 1
  (as far as they exist) become +0 / -0, under a dh of magnitude >= 1 there."""
  h[:, 0] = 0.0
  dh[:, 0] = np.where(np.abs(dh[:, 0]) < 1, 1.5, dh[:, 0])
  if h.shape[1] > 1:
    h[:, 1] = -0.0
    dh[:, 1] = np.where(np.abs(dh[:, 1]) < 1, -1.25, dh[:, 1])


def bn_recipe(seed, rows, C, f16):
  """y = round_act(1.5 randn + 0.3) (the old BatchNorm test's scale), gamma = f32(uniform(0.5,
  1.5)), beta = f32(0.2 randn), dout = round_act(randn).  Row 0 starts with the planted
  zeros and subnormals; column C - 1 is constant (variance exactly 0: rstd = 1 / sqrt(eps));
  the last row holds big_value in column 1 (C > 2)."""
  rng = np.random.RandomState(seed)
  y = R.round_act(rng.randn(rows, C) * 1.5 + 0.3, f16)
  dout = R.round_act(rng.randn(rows, C), f16)
  gamma = rng.uniform(0.5, 1.5, C).astype(np.float32).astype(np.float64)
  beta = (0.2 * rng.randn(C)).astype(np.float32).astype(np.float64)
  plant(y[0], f16)
  plant(dout[0, ::-1], f16)
  y[:, C - 1] = 0.75
  if C > 2:
    y[rows - 1, 1] = big_value(f16)
  return y, gamma, beta, dout


def off_centre_recipe(seed, rows, C, centre, spread, f16):
  """The old off-centre statistics test: channels whose |mean| / std is 50 .. 100."""
  rng = np.random.RandomState(seed)
  offs = centre * (1.0 + 0.1 * rng.rand(C))
  return R.round_act(rng.randn(rows, C) * spread + offs, f16)


def tie_values(f16):
  """(a, b) of the activation type whose sum lies exactly halfway between two
  neighbours: a = 1 + 2^-(p-1) (1 plus one ulp; p = 8 / 11 significand bits), b = 1.  a + b =
  2 + 2^-(p-1), and the ulp at 2 is 2^-(p-2): a tie between 2 (even) and 2 + 2^-(p-2)."""
  p = 11 if f16 else 8
  return 1.0 + 2.0**-(p - 1), 1.0


def unshuffle_recipe(seed, nB, w, C, seg, f16):
  """e = round_act(randn) (reals: the sums of the rows with two sources round), h =
  round_act(randn) with +0 / -0 in channels 0 / 1 of every row.  Shifts, one per seg
  samples: 0, 1, -1, w - 1, -(w - 1) first, then random values in between.  Exact ties:
  channel 2 of e holds one of tie_values per row at random, under h = 1 (mask 1), so
  about half of the rows with two sources sum to an exact tie of the activation type
  (the others to 2 or 2 + 2^-(p-2), both representable).  Returns e, h, shifts."""
  rng = np.random.RandomState(seed)
  e = R.round_act(rng.randn(nB, w, C), f16)
  h = R.round_act(rng.randn(nB, w, C), f16)
  h[:, :, 0] = 0.0
  h[:, :, 1] = -0.0
  nseg = -(-nB // seg)
  first = [0, 1, -1, w - 1, -(w - 1)]
  shifts = np.array([first[i] if i < len(first) else rng.randint(-(w - 1), w)
                     for i in range(nseg)], np.int32)
  a, b = tie_values(f16)
  e[:, :, 2] = np.where(rng.rand(nB, w) < 0.5, a, b)
  h[:, :, 2] = 1.0
  return e, h, shifts
