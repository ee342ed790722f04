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
