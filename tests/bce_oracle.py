"""CPU reference of the vanilla GAN step (reference gan/algorithms/gan.py:43-90)
for the tests of calciumgan_amd's `--algorithm gan`: the oracle's generator /
discriminator forwards, Keras Adam, signal metrics and dynamic loss scale,
composed with torch's binary_cross_entropy_with_logits and autograd.

Modes: 'f32' (plain), 'bf16' (stored activations, weight operands and their
gradients rounded like the bf16 kernels: oracle.bf16_round) and 'f16' (the
mixed_float16 storage points: oracle.f16_round).  Stateful like
oracle.OracleGAN: it holds both models' weights and Adam moments."""
import numpy as np
import torch
import torch.nn.functional as F

import oracle as O


def draw_randomness(hp, batch_size, seed):
  """The draws of one GAN.train call: z (B, noise_dim), then the PhaseShuffle
  draws of the two discriminator calls, shifts_real[4] and shifts_fake[4]."""
  rng = np.random.RandomState(seed)
  z = rng.standard_normal((batch_size, hp.noise_dim)).astype(np.float32)
  sh = lambda: rng.randint(-hp.m, hp.m + 1, size=O.NUM_CONVS - 1).astype(np.int32)
  return dict(z=z, shifts_real=sh(), shifts_fake=sh())


def bce_seed(x, y):
  """d BCE(y, x) / dx per sample (the seed of a backward chain before the 1/B
  of the mean): s(x) - y."""
  return torch.sigmoid(x) - y


def bce_losses(real_out, fake_out):
  """(gen_loss, dis_loss): Keras BinaryCrossentropy(from_logits=True), means
  over the batch (gan.py:43-56)."""
  ones, zeros = torch.ones_like(fake_out), torch.zeros_like(fake_out)
  gen = F.binary_cross_entropy_with_logits(fake_out, ones)
  dis = (F.binary_cross_entropy_with_logits(real_out, torch.ones_like(real_out)) +
         F.binary_cross_entropy_with_logits(fake_out, zeros))
  return gen, dis


def _ident(x):
  return x


def _rounding(mode):
  return {'f32': _ident, 'bf16': O.bf16_round, 'f16': O.f16_round}[mode]


def step_grads(hp, gen_weights, dis_weights, real, r, mode='f32',
               training=True, dtype=torch.float32):
  """Losses and both models' gradients of one step from the SAME forward, with
  the weights before either update (gan.py:72-85).  dtype: of the weights,
  the batch and z inside the computation (float64 for the CPU tests' exact
  identities)."""
  q = _rounding(mode)
  gen = [torch.as_tensor(w).detach().to(dtype).clone().requires_grad_(True)
         for w in gen_weights]
  dis = [torch.as_tensor(w).detach().to(dtype).clone().requires_grad_(True)
         for w in dis_weights]
  real = torch.as_tensor(real).to(dtype)
  bn_updates = {}
  z = torch.as_tensor(np.asarray(r['z'])).to(dtype)
  fake = O.generator_forward(gen, z, hp, q, q, training=training,
                             bn_updates=bn_updates)
  real_out = O.discriminator_forward(dis, real, list(r['shifts_real']), hp, q, q)
  fake_out = O.discriminator_forward(dis, fake, list(r['shifts_fake']), hp, q, q)
  gen_loss, dis_loss = bce_losses(real_out, fake_out)
  d_grads = torch.autograd.grad(dis_loss, dis, retain_graph=True,
                                allow_unused=True)
  g_grads = torch.autograd.grad(gen_loss, gen, allow_unused=True)
  fix = lambda gs, ws: [torch.zeros_like(w) if g is None else g.detach()
                        for g, w in zip(gs, ws)]
  return dict(gen_loss=gen_loss.detach(), dis_loss=dis_loss.detach(),
              d_grads=fix(d_grads, dis), g_grads=fix(g_grads, gen),
              fake=fake.detach(), real_out=real_out.detach(),
              fake_out=fake_out.detach(),
              bn_updates={k: v.detach() for k, v in bn_updates.items()})


class OracleBCEGAN(object):
  """Stateful oracle of GAN (weights + Keras-Adam state + optional dynamic
  loss scales, one per optimizer)."""

  def __init__(self, hp, gen_weights, dis_weights, mode='f32',
               loss_scaling=False):
    self.hp = hp
    self.mode = mode
    t = lambda ws: [torch.tensor(np.asarray(w), dtype=torch.float32) for w in ws]
    self.gen, self.dis = t(gen_weights), t(dis_weights)
    self.gen_m = [torch.zeros_like(w) for w in self.gen]
    self.gen_v = [torch.zeros_like(w) for w in self.gen]
    self.dis_m = [torch.zeros_like(w) for w in self.dis]
    self.dis_v = [torch.zeros_like(w) for w in self.dis]
    self.gen_steps = self.dis_steps = 0
    self.gen_scale = O.DynamicLossScale() if loss_scaling else None
    self.dis_scale = O.DynamicLossScale() if loss_scaling else None

  def _real(self, inputs):
    return torch.as_tensor(np.asarray(inputs), dtype=torch.float32)

  def train(self, inputs, r):
    """Returns (gen_loss, dis_loss, None, metrics) as floats and keeps the
    step's record in self.last."""
    real = self._real(inputs)
    res = step_grads(self.hp, self.gen, self.dis, real, r, self.mode)
    for i, v in res['bn_updates'].items():
      self.gen[i] = v
    lr = self.hp.learning_rate
    if self.dis_scale is None or self.dis_scale.update(res['d_grads']):
      self.dis_steps += 1
      for p, g, m, v in zip(self.dis, res['d_grads'], self.dis_m, self.dis_v):
        O.keras_adam(p, g, m, v, self.dis_steps, lr)
    if self.gen_scale is None or self.gen_scale.update(res['g_grads']):
      self.gen_steps += 1
      frozen = set(O.generator_nontrainable(self.hp))
      for i, (p, g, m, v) in enumerate(zip(self.gen, res['g_grads'], self.gen_m,
                                           self.gen_v)):
        if i not in frozen:
          O.keras_adam(p, g, m, v, self.gen_steps, lr)
    metrics = O.signal_metrics(real, res['fake'], self.hp.signals_min,
                               self.hp.signals_max, self.hp.normalize)
    res['metrics'] = {k: float(v) for k, v in metrics.items()}
    self.last = res
    return (float(res['gen_loss']), float(res['dis_loss']), None,
            res['metrics'])

  def validate(self, inputs, r):
    """gan.py:87-90: (fake, gen_loss, dis_loss, None, metrics), no update."""
    real = self._real(inputs)
    res = step_grads(self.hp, self.gen, self.dis, real, r, self.mode,
                     training=False)
    metrics = O.signal_metrics(real, res['fake'], self.hp.signals_min,
                               self.hp.signals_max, self.hp.normalize)
    return (res['fake'], float(res['gen_loss']), float(res['dis_loss']), None,
            {k: float(v) for k, v in metrics.items()})
