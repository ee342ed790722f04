"""CPU oracle of the MLP model (reference gan/models/mlp.py:15-77) under WGAN-GP
(gan/algorithms/wgan_gp.py:12-95) for the tests of `--model mlp`: torch with
autograd, `create_graph=True` for the penalty.  Noise, alpha and the dropout
keep masks are passed in; the computation runs in `dtype` (float64 for the
reference values, float32 for the rounding yardstick of the comparisons).

Weights are Keras-order lists [W0, b0, ..., W4, b4], W (in, out).  Masks: per
dropout layer a bool / 0-1 array shaped like that layer's output; None = no
dropout (training=False).

`hand_critic_grads` is the schedule the device runs, written without autograd:
input-gradient chain, v = lambda dgp/dg, tangent chain, weight gradients over
[h_real | h_fake | tangent] x [delta_real | delta_fake | delta_x^].
"""
import numpy as np
import torch

import oracle as O


def _act(z, alpha):
  return torch.where(z > 0, z, alpha * z)


def _t(x, dtype):
  return torch.as_tensor(np.asarray(x)).to(dtype)


def _masks(masks, dtype):
  return None if masks is None else [_t(m, dtype) for m in masks]


def generator_forward(w, z, L, alpha, masks, scale, normalize):
  """z (n, noise) -> (n, L, C).  masks: 3 arrays (n, L, U / 2U / 3U) or None."""
  n, nd = z.shape
  h = _act(z @ w[0] + w[1], alpha).reshape(n, L, nd)
  for l in range(1, 4):
    h = _act(h @ w[2 * l] + w[2 * l + 1], alpha)
    if masks is not None:
      h = h * masks[l - 1] * scale
  y = h @ w[8] + w[9]
  return torch.sigmoid(y) if normalize else y


def discriminator_forward(w, x, alpha, masks, scale):
  """x (n, L, C) -> (n, 1).  masks: 4 arrays (n, L, 4U / 3U / 2U / U) or None."""
  h = x
  for l in range(4):
    h = _act(h @ w[2 * l] + w[2 * l + 1], alpha)
    if masks is not None:
      h = h * masks[l] * scale
  return h.reshape(h.shape[0], -1) @ w[8] + w[9]


def _seg(masks, i, B):
  return None if masks is None else [m[i * B:(i + 1) * B] for m in masks]


def critic_step(gen_w, dis_w, real, r, hp, dtype=torch.float64, grads=True):
  """One critic update's losses and gradients.  r: dict(z=, alpha= (B,),
  masks_g= 3 arrays or None, masks_d= 4 arrays over the 3B samples [real | fake
  | x^] or None).  Returns dict(loss, gen_loss, gp, fake, grads)."""
  alpha, scale = hp.alpha, _scale(hp, r.get('masks_d'))
  gw = [_t(v, dtype) for v in gen_w]
  dw = [_t(v, dtype).requires_grad_(grads) for v in dis_w]
  real = _t(real, dtype)
  B, L, _ = real.shape
  mg, md = _masks(r.get('masks_g'), dtype), _masks(r.get('masks_d'), dtype)
  fake = generator_forward(gw, _t(r['z'], dtype), L, alpha, mg,
                           _scale(hp, mg), hp.normalize).detach()
  a = _t(r['alpha'], dtype).reshape(B, 1, 1)
  inter = (a * real + (1 - a) * fake).requires_grad_(True)
  real_out = discriminator_forward(dw, real, alpha, _seg(md, 0, B), scale)
  fake_out = discriminator_forward(dw, fake, alpha, _seg(md, 1, B), scale)
  inter_out = discriminator_forward(dw, inter, alpha, _seg(md, 2, B), scale)
  g, = torch.autograd.grad(inter_out.sum(), inter, create_graph=grads)
  norm = g.reshape(B, -1).norm(dim=1)
  gp = ((norm - 1.0)**2).mean()
  loss = -real_out.mean() + fake_out.mean() + hp.gradient_penalty * gp
  out = dict(loss=loss.detach(), gen_loss=(-fake_out.mean()).detach(),
             gp=gp.detach(), fake=fake, g=g.detach())
  if grads:
    out['grads'] = [v.detach() for v in torch.autograd.grad(loss, dw)]
  return out


def generator_step(gen_w, dis_w, r, hp, L, dtype=torch.float64):
  """The generator update's loss and gradients.  r: dict(z=, masks_g=,
  masks_d= 4 arrays over the B fake samples)."""
  alpha = hp.alpha
  gw = [_t(v, dtype).requires_grad_(True) for v in gen_w]
  dw = [_t(v, dtype) for v in dis_w]
  mg, md = _masks(r.get('masks_g'), dtype), _masks(r.get('masks_d'), dtype)
  fake = generator_forward(gw, _t(r['z'], dtype), L, alpha, mg, _scale(hp, mg),
                           hp.normalize)
  loss = -discriminator_forward(dw, fake, alpha, md, _scale(hp, md)).mean()
  return dict(loss=loss.detach(), fake=fake.detach(),
              grads=[v.detach() for v in torch.autograd.grad(loss, gw)])


def _scale(hp, masks):
  """float32(1 / (1 - p)) as the kernels apply it; 1 without masks."""
  return 1.0 if masks is None else float(np.float32(1.0 / (1.0 - hp.dropout)))


def hand_critic_grads(dis_w, real, fake, alpha_b, masks_d, hp):
  """The device's schedule in float64 without autograd.  Returns (loss, gp,
  grads) of -E[D(real)] + E[D(fake)] + lambda gp with respect to dis_w."""
  f64 = torch.float64
  w = [_t(v, f64) for v in dis_w]
  real, fake = _t(real, f64), _t(fake, f64)
  B, L, C = real.shape
  a = _t(alpha_b, f64).reshape(B, 1, 1)
  x0 = torch.cat([real, fake, a * real + (1 - a) * fake]).reshape(3 * B * L, C)
  s = _scale(hp, masks_d)
  al = hp.alpha
  # forward over 3B, storing the inputs and m = s * keep * act'
  xs, ms = [x0], []
  h = x0
  for l in range(4):
    z = h @ w[2 * l] + w[2 * l + 1]
    keep = (torch.ones_like(z) if masks_d is None else
            _t(masks_d[l], f64).reshape(z.shape))
    ms.append(s * keep * torch.where(z > 0, torch.ones_like(z),
                                     al * torch.ones_like(z)))
    h = s * keep * _act(z, al)
    xs.append(h)
  flat = h.reshape(3 * B, -1)
  d_out = flat @ w[8] + w[9]
  # input-gradient chain from seeds of 1
  dz = [None] * 5
  dz[4] = torch.ones(3 * B, 1, dtype=f64)
  dh = (dz[4] @ w[8].T).reshape(3 * B * L, -1)
  for l in range(3, -1, -1):
    dz[l] = dh * ms[l]
    dh = dz[l] @ w[2 * l].T
  n = L * C
  g = dh[2 * B * L:].reshape(B, n)
  norm = g.norm(dim=1)
  gp = ((norm - 1)**2).mean()
  lam = hp.gradient_penalty
  v = (lam * 2 * (norm - 1) / (B * norm)).reshape(B, 1) * g
  # tangent chain over the x^ segment
  tang = [v.reshape(B * L, C)]
  for l in range(4):
    tang.append(ms[l][2 * B * L:] * (tang[-1] @ w[2 * l]))
  coef = torch.tensor([-1.0 / B, 1.0 / B, 1.0], dtype=f64)
  grads = []
  for l in range(5):
    per = 1 if l == 4 else L
    x = (flat if l == 4 else xs[l]).clone()
    t = tang[l].reshape(B, -1) if l == 4 else tang[l]
    x[2 * B * per:] = t
    c = coef.repeat_interleave(B * per).reshape(-1, 1)
    d = dz[l] * c
    grads.append(x.T @ d)
    grads.append(d[:2 * B * per].sum(0))
  loss = -d_out[:B].mean() + d_out[B:2 * B].mean() + lam * gp
  return loss, gp, grads


class OracleMLPGAN(object):
  """Stateful float64 / float32 oracle of the MLP WGAN-GP step: weights and
  Keras-Adam moments of both models."""

  def __init__(self, hp, gen_weights, dis_weights, dtype=torch.float64):
    self.hp, self.dtype = hp, dtype
    t = lambda ws: [_t(w, dtype).clone() for w in ws]
    self.gen, self.dis = t(gen_weights), t(dis_weights)
    self.gen_m = [torch.zeros_like(w) for w in self.gen]
    self.gen_v = [torch.zeros_like(w) for w in self.gen]
    self.dis_m = [torch.zeros_like(w) for w in self.dis]
    self.dis_v = [torch.zeros_like(w) for w in self.dis]
    self.gen_steps = self.dis_steps = 0

  def critic_update(self, real, r):
    res = critic_step(self.gen, self.dis, real, r, self.hp, self.dtype)
    self.dis_steps += 1
    for p, g, m, v in zip(self.dis, res['grads'], self.dis_m, self.dis_v):
      O.keras_adam(p, g, m, v, self.dis_steps, self.hp.learning_rate)
    return res

  def generator_update(self, real, r):
    L = np.asarray(real).shape[1]
    res = generator_step(self.gen, self.dis, r, self.hp, L, self.dtype)
    self.gen_steps += 1
    for p, g, m, v in zip(self.gen, res['grads'], self.gen_m, self.gen_v):
      O.keras_adam(p, g, m, v, self.gen_steps, self.hp.learning_rate)
    return res

  def train(self, real, rand):
    """rand: dict(critic=[r, ...], gen=r).  Returns (gen_loss, dis_loss, gp) and
    keeps every update's record in self.last."""
    cs = [self.critic_update(real, r) for r in rand['critic']]
    gs = self.generator_update(real, rand['gen'])
    self.last = dict(critic=cs, gen=gs)
    return (float(gs['loss']), float(np.mean([float(c['loss']) for c in cs])),
            float(np.mean([float(c['gp']) for c in cs])))

  def validate(self, real, r):
    """(fake, gen_loss, dis_loss, gp): training=False, no masks, no update."""
    r = dict(z=r['z'], alpha=r['alpha'])
    res = critic_step(self.gen, self.dis, real, r, self.hp, self.dtype,
                      grads=False)
    return (res['fake'], float(res['gen_loss']), float(res['loss']),
            float(res['gp']))


# -- the bar of the float64 comparisons ----------------------------------------
def rel_distance(a, ref):
  """Relative 2-norm distance of a from ref (float64); the plain norm of a where
  ref is all zero."""
  a = np.asarray(a, dtype=np.float64).reshape(-1)
  ref = np.asarray(ref, dtype=np.float64).reshape(-1)
  n = np.linalg.norm(ref)
  return float(np.linalg.norm(a - ref) / n) if n > 0 else float(np.linalg.norm(a))


def check_parity(name, dev, ref64, ref32, report=None):
  """The device result must lie within 4 x the distance of the SAME oracle code
  run in float32 on the CPU from its float64 result; where that distance is
  below 1e-7 the bar is 1e-6.  Prints (and appends to `report`) the figures
  before it asserts."""
  d32 = rel_distance(ref32, ref64)
  ddev = rel_distance(dev, ref64)
  bar = 4.0 * d32 if d32 >= 1e-7 else 1e-6
  line = 'PARITY {:<28} f32 {:.3e}  device {:.3e}  ratio {:.2f}  bar {:.3e}'.format(
      name, d32, ddev, ddev / d32 if d32 > 0 else float('nan'), bar)
  print(line)
  if report is not None:
    report.append((name, d32, ddev))
  assert np.all(np.isfinite(np.asarray(dev, dtype=np.float64))), name
  assert ddev <= bar, line
