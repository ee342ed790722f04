"""Float64 statements of the pointwise / reduction entry points of the C ABI
(calciumgan_amd/csrc/pointwise.hip), written from the comments of
include/calciumgan_hip.h, and the rounding / error-bar helpers the parity tests
of tests/test_hip_pointwise.py state their bars with.

Everything here is numpy float64 on the host.  tests/test_pointwise_ref.py ties
each statement to an independent one (torch autograd in float64, the oracle of
oracle/calciumgan_oracle.py), so a wrong reference cannot make a wrong kernel
pass."""
import numpy as np
import torch

U32 = 2.0**-24  # unit roundoff of f32: one rounding changes x by at most U32 |x|


# ---------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------
def act_dtype(f16):
  return torch.float16 if f16 else torch.bfloat16


def round_act(x, f16):
  """x (any real array) -> the activation type (fp16 / bf16) -> float64, through
  torch's CPU conversion of f32: round to nearest even, subnormals kept,
  overflow to +-inf; independent of the kernels."""
  t = torch.tensor(np.asarray(x), dtype=torch.float32)
  return t.to(act_dtype(f16)).double().numpy()


def ulp_act(x, f16):
  """One ulp of bf16 (8 significant bits, subnormals from 2^-126) / fp16 (11,
  subnormals from 2^-14) at |x|, float64."""
  a = np.abs(np.asarray(x, np.float64))
  e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
  if f16:
    return np.where(a > 0, 2.0**np.maximum(e - 10, -24), 2.0**-24)
  return np.where(a > 0, 2.0**np.maximum(e - 7, -133), 2.0**-133)


def ulp_f32(x):
  """One ulp of f32 (24 significant bits, subnormals from 2^-126) at |x|."""
  a = np.abs(np.asarray(x, np.float64))
  e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
  return np.where(a > 0, 2.0**np.maximum(e - 23, -149), 2.0**-149)


def sum_bound(terms, axis=None):
  """Worst-case error of an f32 sum of n terms added in ANY order, each term
  itself the result of at most one rounding: n * 2^-24 * sum |terms|."""
  t = np.abs(np.asarray(terms, np.float64))
  n = t.size if axis is None else t.shape[axis]
  return n * U32 * t.sum(axis=axis)


def act_limits(f16):
  """(smallest subnormal, largest finite) of the activation type."""
  return (2.0**-24, 65504.0) if f16 else (2.0**-133, float.fromhex('0x1.fep127'))


def f32(x):
  """The f32 value of a host scalar (what a `float` argument of the C ABI
  carries), as a python float."""
  return float(np.float32(x))


# ---------------------------------------------------------------------------
# WGAN-GP pieces
# ---------------------------------------------------------------------------
def interp(real, fake, alpha):
  """x^ = alpha * real + (1 - alpha) * fake, alpha per sample (B,)."""
  a = np.asarray(alpha, np.float64).reshape(-1, *([1] * (np.ndim(real) - 1)))
  return a * np.asarray(real, np.float64) + (1 - a) * np.asarray(fake, np.float64)


def rownorm(g):
  """norm[b] = ||g[b]||_2, g (B, n)."""
  g = np.asarray(g, np.float64)
  return np.sqrt((g * g).sum(axis=1))


def gp_finalize(norm, scale, squared=0, coef_mul=1.0):
  """(norm, gp, coef): gp = mean((norm - 1)^2), coef[b] = scale * 2 * (norm_b -
  1) / (B * norm_b) * coef_mul; squared: `norm` holds sums of squares."""
  nv = np.asarray(norm, np.float64)
  if squared:
    nv = np.sqrt(nv)
  B = nv.shape[0]
  d = nv - 1.0
  return nv, (d * d).mean(), scale * 2.0 * d / (B * nv) * coef_mul


def critic_loss(d_out, gp, penalty, B):
  """[-mean(d_out[0:B]) + mean(d_out[B:2B]) + penalty * gp, -mean(d_out[B:2B])]"""
  d = np.asarray(d_out, np.float64)
  mr, mf = d[:B].mean(), d[B:2 * B].mean()
  return np.array([-mr + mf + penalty * gp, -mf])


def neg_mean(d_out, B):
  return -np.asarray(d_out, np.float64)[:B].mean()


def scale_rows(g, coef):
  return np.asarray(coef, np.float64)[:, None] * np.asarray(g, np.float64)


def step_outputs(gen_loss, loss, gp, metrics, n):
  """[gen_loss, mean_k loss[k][0], mean_k gp[k], metrics x 4]; n = 0: zeros."""
  loss = np.asarray(loss, np.float64).reshape(-1, 2)
  gp = np.asarray(gp, np.float64)
  m1 = loss[:n, 0].mean() if n > 0 else 0.0
  m2 = gp[:n].mean() if n > 0 else 0.0
  return np.array([float(gen_loss), m1, m2] + [float(x) for x in metrics[:4]])


# ---------------------------------------------------------------------------
# elementwise backward pieces, column sums
# ---------------------------------------------------------------------------
def lrelu_grad(h, alpha):
  """lrelu'(h): 1 where h > 0, alpha elsewhere (h = +-0 included)."""
  return np.where(np.asarray(h, np.float64) > 0, 1.0, alpha)


def lrelu_bwd(dh, h, alpha):
  return np.asarray(dh, np.float64) * lrelu_grad(h, alpha)


def sigmoid_bwd(dfake, s):
  s = np.asarray(s, np.float64)
  return np.asarray(dfake, np.float64) * s * (1 - s)


def lrelu_mix_parts(ha, hb, mix, alpha):
  """The two products of cg_lrelu_mix's sum: mix * act^-1(h_a), (1 - mix) *
  act^-1(h_b); act^-1(h) = h for h > 0, h / alpha elsewhere."""
  inv = lambda h: np.where(h > 0, h, h / alpha)
  m = np.asarray(mix, np.float64)[:, None]
  return (m * inv(np.asarray(ha, np.float64)),
          (1 - m) * inv(np.asarray(hb, np.float64)))


def lrelu_mix(ha, hb, mix, alpha):
  pa, pb = lrelu_mix_parts(ha, hb, mix, alpha)
  y = pa + pb
  return np.maximum(y, alpha * y)


def colsum(x):
  return np.asarray(x, np.float64).sum(axis=0)


# ---------------------------------------------------------------------------
# discriminator head
# ---------------------------------------------------------------------------
def dense1_terms(h, wq):
  """The products h[b][t][c] * act(w[t*C+c]) of the logit, (nB, Lt, C)."""
  return np.asarray(h, np.float64) * np.asarray(wq, np.float64)[None]


def dense1_fwd(h, wq, bias):
  return dense1_terms(h, wq).sum(axis=(1, 2)) + float(bias)


def dense1_bwd(h, wq, coef, seg, alpha):
  """delta[b][t][c] = coef[b / seg] * act(w[t*C+c]) * lrelu'(h[b][t][c])"""
  c = np.repeat(np.asarray(coef, np.float64), seg)[:np.shape(h)[0]]
  return c[:, None, None] * np.asarray(wq, np.float64)[None] * lrelu_grad(h, alpha)


def dense1_wgrad_terms(x, coef, seg):
  c = np.repeat(np.asarray(coef, np.float64), seg)[:np.shape(x)[0]]
  return c[:, None, None] * np.asarray(x, np.float64)


# ---------------------------------------------------------------------------
# BCE head of the vanilla GAN step (cg_dense1_bce)
# ---------------------------------------------------------------------------
def sigmoid64(x):
  """s(x) with the sign split: e^-|x| never overflows, and for x < 0 the result
  e / (1 + e) keeps its relative accuracy down to the smallest float64."""
  x = np.asarray(x, np.float64)
  e = np.exp(-np.abs(x))
  return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_logits(x, y):
  """Keras BCE from logits, max(x, 0) - x y + log1p(exp(-|x|)), for y in {0, 1}:
  max(x, 0) - x y is exact (0, x or -x), so nothing cancels at any |x|."""
  x = np.asarray(x, np.float64)
  return np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))


def bce_from_logits(x, B, S_d=1.0, S_g=1.0):
  """Everything cg_dense1_bce derives from the 2B logits x = [fake | real]:
    t0, t1 (2B,): BCE(0, x), BCE(1, x);   td = [t0 fake | t1 real], tg = t1 fake
    loss = [mean_fake t1, mean_real t1 + mean_fake t0]
    coef_d = S_d (s(x) - y) / B (y = 0 fake, 1 real; s(x) - 1 as -s(-x): exact),
    coef_g = S_g (s(x) - 1) / B on the fake segment."""
  x = np.asarray(x, np.float64)
  assert x.shape == (2 * B,)
  t0, t1 = bce_logits(x, 0.0), bce_logits(x, 1.0)
  sd = np.r_[sigmoid64(x[:B]), -sigmoid64(-x[B:])]
  return dict(t0=t0, t1=t1, td=np.r_[t0[:B], t1[B:]], tg=t1[:B],
              loss=np.array([t1[:B].mean(), t1[B:].mean() + t0[:B].mean()]),
              coef_d=S_d * sd / B, coef_g=-S_g * sigmoid64(-x[:B]) / B)


def bce_head(hq, wq, bias, B, alpha, S_d=1.0, S_g=1.0):
  """The float64 statement of cg_dense1_bce (include/calciumgan_hip.h).  hq (2B,
  Lt, Cp) activations [fake | real], wq (Lt, C) the weights as the kernel
  multiplies them (round_act(w)), C <= Cp.  bce_from_logits of x = bias + <h, wq>
  plus `x` and the unrounded seeds delta_d (2B, Lt, Cp), delta_g (B, Lt, Cp) =
  coef * wq * lrelu'(h), channels [C, Cp) zero."""
  hq, wq = np.asarray(hq, np.float64), np.asarray(wq, np.float64)
  C, Cp = wq.shape[1], hq.shape[2]
  x = dense1_fwd(hq[:, :, :C], wq, bias)
  r = bce_from_logits(x, B, S_d, S_g)
  r['x'] = x
  g = np.zeros(hq.shape)
  g[:, :, :C] = wq[None] * lrelu_grad(hq[:, :, :C], alpha)
  r['delta_d'] = r['coef_d'][:, None, None] * g
  r['delta_g'] = r['coef_g'][:, None, None] * g[:B]
  return r


def bce_planted_logits(f16):
  """Logits where one guard of the head's arithmetic matters, each on one segment
  at one sign: exponent overflow from 88.8 on, the cancellation of s(x) - 1 and
  the loss of log(1 + e) from 17 on; expf(-|x|) is subnormal from 87.4 on and
  zero at 104; the largest finite value of the activation type."""
  big = act_limits(f16)[1]
  v = [2.0**-10, 1.0, 20.0, 40.0, 88.0, 89.0, 104.0, big]
  return np.array([0.0, -0.0] + [s * a for a in v for s in (1.0, -1.0)])


# expf and log1pf: spacings charged per call.  An allowance taken from
# documentation memory (the HIP math API's accuracy table lists single-digit ulp
# maxima for both), NOT read off the kernel; tests/test_pointwise_ref.py shows
# that the naive forms miss the bars by far more than any such allowance.
LIBM_SPACINGS = 2.0


def _sigmoid_bar(x):
  """(s, E) of sigmoid_stable(x) in f32, spacings carried to the result by the
  derivative: e = expf(-|x|) LIBM sp(e); d = 1 + e half a spacing; the quotient
  (1 / d for x >= 0, e / d below) half a spacing -- LIBM + 1 spacings, each at
  its own magnitude (2^-149 in the subnormals)."""
  x = np.asarray(x, np.float64)
  e = np.exp(-np.abs(x))
  d = 1.0 + e
  de = LIBM_SPACINGS * ulp_f32(e)
  dd = de + 0.5 * ulp_f32(d)
  s = np.where(x >= 0, 1.0 / d, e / d)
  ds = np.where(x >= 0, dd / d**2, de / d + e * dd / d**2) + 0.5 * ulp_f32(s)
  return s, ds


def _coef_bar(s, ds, B, S):
  """S s / B as (s * (1 / B)) * S: 1 / B and two products, half a spacing each
  (1.5 spacings on top of the sigmoid's); the first product's rounding is
  multiplied by S (it matters where s / B is subnormal)."""
  q = s / B
  dq = ds / B + U32 * q + 0.5 * ulp_f32(q)
  return S * dq + 0.5 * ulp_f32(S * q)


def _term_bar(x, y):
  """BCE(y, x) in f32: max(x, 0) - x y is exact; e = expf(-|x|) LIBM sp(e), l =
  log1pf(e) LIBM sp(l) (+ e's error, derivative 1 / (1 + e)), the final sum half
  a spacing: 2 LIBM + 0.5 spacings."""
  x = np.asarray(x, np.float64)
  e = np.exp(-np.abs(x))
  de = LIBM_SPACINGS * ulp_f32(e)
  dl = de / (1.0 + e) + LIBM_SPACINGS * ulp_f32(np.log1p(e))
  return dl + 0.5 * ulp_f32(bce_logits(x, y))


def bce_bars(x, B, S_d=1.0, S_g=1.0):
  """Error bars of an f32 evaluation of bce_from_logits on the SAME logits, in
  f32 spacings counted from the operations (a rounding of + * / is half a
  spacing, expf / log1pf LIBM_SPACINGS):
    t0, t1, td, tg: _term_bar;  coef_d, coef_g: _sigmoid_bar then _coef_bar;
    loss (ordered form): each segment's sum of B terms -- the terms' own bars and
      sum_bound -- over B, the quotient's half spacing (x 2 segments and the
      final sum's half spacing for loss[1]);
    loss_atomic: every term times 1 / B first (1 / B, the product: 1.5
      spacings of t / B), then one sum of B (loss[0]) / 2B (loss[1]) terms in
      any order."""
  x = np.asarray(x, np.float64)
  r = bce_from_logits(x, B, S_d, S_g)
  e_t0, e_t1 = _term_bar(x, 0.0), _term_bar(x, 1.0)
  e_td, e_tg = np.r_[e_t0[:B], e_t1[B:]], e_t1[:B]
  sf, dsf = _sigmoid_bar(x[:B])     # fake: s(x)
  sn, dsn = _sigmoid_bar(-x)        # s(-x): real coef_d, every coef_g
  e_cd = np.r_[_coef_bar(sf, dsf, B, S_d), _coef_bar(sn[B:], dsn[B:], B, S_d)]
  e_cg = _coef_bar(sn[:B], dsn[:B], B, S_g)

  def mean_bar(t, et):
    return (et.sum() + sum_bound(t)) / B + 0.5 * ulp_f32(t.mean())

  td, tg = r['td'], r['tg']
  e_loss = np.array([mean_bar(tg, e_tg),
                     mean_bar(td[B:], e_td[B:]) + mean_bar(td[:B], e_td[:B]) +
                     0.5 * ulp_f32(r['loss'][1])])

  def atomic_bar(t, et):
    v = t / B
    return (et / B + U32 * v + 0.5 * ulp_f32(v)).sum() + sum_bound(v)

  return dict(t0=e_t0, t1=e_t1, td=e_td, tg=e_tg, coef_d=e_cd, coef_g=e_cg,
              loss=e_loss,
              loss_atomic=np.array([atomic_bar(tg, e_tg), atomic_bar(td, e_td)]))


# ---------------------------------------------------------------------------
# dynamic loss scale (cg_loss_scale_update)
# ---------------------------------------------------------------------------
def loss_scale_update(ls, interval):
  """The state machine of the header on four f32 [S, good, t, flag], in f32
  arithmetic: flag != 0 (finite gradients): t += 1, and the `interval`-th
  consecutive one doubles S (unless 2 S overflows: S stays) and restarts the
  count; flag == 0: S = max(S / 2, 1), the count restarts, t stays.  The flag is
  1 afterwards."""
  f = np.float32
  S, good, t, flag = (f(v) for v in ls)
  if flag != 0:
    t = f(t + f(1))
    if f(good + f(1)) >= f(interval):
      with np.errstate(over='ignore'):
        s2 = f(S * f(2))
      S = s2 if np.isfinite(s2) else S
      good = f(0)
    else:
      good = f(good + f(1))
  else:
    S, good = f(max(f(S * f(0.5)), f(1))), f(0)
  return np.array([S, good, t, f(1)], np.float32)


# ---------------------------------------------------------------------------
# Keras Adam
# ---------------------------------------------------------------------------
def adam_lr_t(lr, b1, b2, t):
  return lr * np.sqrt(1.0 - b2**t) / (1.0 - b1**t)


def adam(p, g, m, v, lr_t, b1, b2, eps, grad_scale=1.0):
  """(p, m, v) after g = grad * grad_scale; m = b1 m + (1 - b1) g; v = b2 v +
  (1 - b2) g^2; p -= lr_t m / (sqrt(v) + eps)."""
  p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
  g = g * grad_scale
  m = b1 * m + (1 - b1) * g
  v = b2 * v + (1 - b2) * g * g
  return p - lr_t * m / (np.sqrt(v) + eps), m, v


def adam_bars(p, g, m, v, lr_t, b1, b2, eps, grad_scale=1.0, lr_t_rel=0.0,
              g_roundings=1):
  """Error bars (p, m, v) of an f32 evaluation of adam(), operation by
  operation (U = 2^-24 per rounding, relative to the magnitudes that enter):
    g: g_roundings (the product with grad_scale);
    m: + (1 - b1), two products, one sum -> (g_roundings + 4) U (|b1 m| + |(1 - b1) g|);
    v: + g * g, (1 - b2), two products, one sum -> (2 g_roundings + 5) U v_new (all >= 0);
    den = sqrt(v) + eps: the error of v through the root, + 2 U den (root, sum);
    u = lr_t m / den: errors of m, den and lr_t (lr_t_rel, relative) + 2 U |u|;
    p - u: + U (|p| + |u|)."""
  p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
  gs = np.abs(g * grad_scale)
  m1 = b1 * m + (1 - b1) * g * grad_scale
  v1 = b2 * v + (1 - b2) * gs * gs
  em = (g_roundings + 4) * U32 * (np.abs(b1 * m) + (1 - b1) * gs)
  ev = (2 * g_roundings + 5) * U32 * v1
  root = np.sqrt(v1)
  den = root + eps
  eden = np.where(v1 > 0, ev / (2 * np.where(v1 > 0, root, 1.0)), 0.0) + 2 * U32 * den
  u = np.abs(lr_t * m1 / den)
  eu = np.abs(lr_t) * (em / den + np.abs(m1) * eden / den**2) + (2 * U32 + lr_t_rel) * u
  return eu + U32 * (np.abs(p) + u), em, ev


# ---------------------------------------------------------------------------
# signal metrics
# ---------------------------------------------------------------------------
def signal_stats(x, smin, smax):
  """Per-row (min, max, mean, population std) over the channels of the
  denormalised x (rows, C): (4, rows)."""
  t = np.asarray(x, np.float64) * (smax - smin) + smin
  return np.stack([t.min(axis=1), t.max(axis=1), t.mean(axis=1), t.std(axis=1)])


def signal_metrics(real, fake, smin, smax):
  """Means over rows of the squared differences of signal_stats: (4,)."""
  d = signal_stats(real, smin, smax) - signal_stats(fake, smin, smax)
  return (d * d).mean(axis=1)


def signal_stats_bars(x, smin, smax):
  """Error bars (4, rows) of an f32 evaluation of signal_stats, U = 2^-24:
    t = x * scale + smin: two roundings, E_t = 2 U max_c(|x scale| + |smin|);
    min / max: E_t;
    mean = sum_c t / C: E_t + sum_bound(t) / C + 2 U |mean| (1 / C and the product);
    std = sqrt(sum_c (t - mean)^2 / C): every difference is off by at most E_t +
      E_mean + U |d|, which moves the root mean square by at most E_t + E_mean +
      U std; the C squares and their sum, 1 / C, the product and the root add
      (C / 2 + 5) U std."""
  x = np.asarray(x, np.float64)
  C = x.shape[1]
  scale = smax - smin
  t = x * scale + smin
  et = 2 * U32 * (np.abs(x * scale) + abs(smin)).max(axis=1)
  emean = et + sum_bound(t, axis=1) / C + 2 * U32 * np.abs(t.mean(axis=1))
  estd = et + emean + (C / 2 + 5) * U32 * t.std(axis=1)
  return np.stack([et, et, emean, estd])


def signal_metrics_bars(real, fake, smin, smax):
  """Error bars (4,) of the means over rows of squared differences D = q_real -
  q_fake: E_D = E_q(real) + E_q(fake) + U |D|; D^2 moves by 2 |D| E_D + E_D^2 + U
  D^2; the sum over rows by sum_bound; 1 / rows and the product by 2 U."""
  d = signal_stats(real, smin, smax) - signal_stats(fake, smin, smax)
  ed = (signal_stats_bars(real, smin, smax) + signal_stats_bars(fake, smin, smax) +
        U32 * np.abs(d))
  rows = d.shape[1]
  e2 = 2 * np.abs(d) * ed + ed * ed + U32 * d * d
  return ((e2.sum(axis=1) + sum_bound(d * d, axis=1)) / rows +
          2 * U32 * (d * d).mean(axis=1))


# ---------------------------------------------------------------------------
# bars of the penalty's scalar chain
# ---------------------------------------------------------------------------
def gp_bars(nv, scale, coef_mul, e_nv):
  """Error bars (gp, coef) of an f32 evaluation of gp_finalize on norms nv that
  are themselves off by at most e_nv (array), U = 2^-24:
    d = nv - 1: E_d = e_nv + U |d|;
    d^2: 2 |d| E_d + E_d^2 + U d^2; their sum: sum_bound; / B: U gp;
    coef = K d / nv, K = 2 scale coef_mul / B: |K| E_d / nv + |K d| e_nv / nv^2,
      and 5 roundings (scale * 2 * d, B * nv, the quotient, * coef_mul)."""
  nv = np.asarray(nv, np.float64)
  B = nv.shape[0]
  d = nv - 1.0
  ed = e_nv + U32 * np.abs(d)
  e2 = 2 * np.abs(d) * ed + ed * ed + U32 * d * d
  gp = (d * d).mean()
  egp = (e2.sum() + sum_bound(d * d)) / B + U32 * gp
  K = abs(2.0 * scale * coef_mul / B)
  coef = K * np.abs(d) / nv
  ecoef = K * ed / nv + K * np.abs(d) * e_nv / nv**2 + 5 * U32 * coef
  return egp, ecoef


def critic_loss_bars(d_out, gp, e_gp, penalty, B):
  """Error bars of critic_loss: the two sums (sum_bound), the two quotients, the
  product with the penalty and two additions -- 5 roundings on the magnitudes
  that meet, and the penalty's own error."""
  d = np.asarray(d_out, np.float64)
  sr, sf = sum_bound(d[:B]) / B, sum_bound(d[B:2 * B]) / B
  mag = abs(d[:B].mean()) + abs(d[B:2 * B].mean()) + abs(penalty * gp)
  return np.array([sr + sf + abs(penalty) * e_gp + 5 * U32 * mag,
                   sf + U32 * abs(d[B:2 * B].mean())])
