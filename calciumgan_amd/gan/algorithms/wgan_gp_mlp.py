"""WGAN-GP on an MLP pair (gan/models/mlp.py) -- gan/algorithms/wgan_gp.py:12-95
with dropout -- as eager launches of the float32 kernels in csrc/mlp.hip.
WGAN_GP (wgan_gp.py, registered as 'wgan-gp') hands an MLP pair to this class.

Critic update (reference :64-80) on a batch `real` of B samples:
  1. G(z, training=True), masks on                           -> fake
  2. cg_mlp_interp                                -> X0 = [real | fake | x^]
  3. D forward over the 3B samples as ONE pass: an element's mask depends on
     its index in the (3B L x width) output, so each segment has masks of its
     own (the reference makes three calls, :70-71 and :47)
  4. input-gradient chain from seeds of 1 down to the input; its x^ segment is g
     (the coefficients (-1/B, +1/B, 1) of the three loss terms enter at the
     weight gradients)
  5. cg_mlp_gp_loss: ||g||, gp, v = lambda dgp/dg, the critic loss
  6. tangent chain: v forward through the x^ segment's masked linear chain.  The
     model is piecewise linear given its masks: no second-derivative term, and
     the biases get no penalty gradient
  7. weight gradients over [h_real | h_fake | tangent] against
     [delta_real | delta_fake | delta_x^]; bias gradients from the first two
  8. Keras Adam
Generator update (:22-36): G forward with masks, D(fake) with fresh masks, D's
input-gradient chain from seeds of -1/B, G's backward, Adam, signal metrics.

validate() runs the critic schedule's steps 1-5 with training=False: the
penalty's inner gradient included, no dropout, no update.
"""
import torch

from ... import _lib
from . import draws
from .gan import GAN, _METRIC_KEYS


class MLP_WGAN_GP(GAN):
  _has_penalty = True
  _mlp_step = True

  def __init__(self, hparams, generator, discriminator, summary=None):
    super().__init__(hparams, generator, discriminator, summary)
    if self._sync.world > 1:
      raise ValueError('calciumgan_amd: --model mlp is single process only')
    if getattr(hparams, 'spike_metrics', False):
      raise ValueError('calciumgan_amd: --spike_metrics is not implemented for '
                       '--model mlp')
    self.penalty = float(hparams.gradient_penalty)
    self.n_critic = int(hparams.n_critic)
    self._use_graph = False  # eager launches only
    # the dropout streams of the last train() / validate(), for the parity
    # tests: per update ('critic' | 'gen', generator's, discriminator's), each a
    # list of per-layer stream ids (None: that launch ran no dropout)
    self.last_streams = []

  def _build_state(self, B):
    dev = self.device
    net_d = self.discriminator.net
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    nc = max(self.n_critic, 1)
    L, C = net_d.L, net_d.C
    return dict(
        x0=f32(3 * B, L * C),
        seed3=torch.ones(3 * B, dtype=torch.float32, device=dev),
        seed_g=torch.full((B,), -1.0 / B, dtype=torch.float32, device=dev),
        norm=f32(B), coef_gp=f32(B), v=f32(B * L, C),
        tangent=[f32(B * l.per, l.cout) for l in net_d.layers[:-1]],
        gp=f32(nc), loss=f32(nc, 2), gen_loss=f32(1), out=f32(7))

  # -- the critic schedule ----------------------------------------------------
  def _critic_forward(self, st, real, z, alpha, slot, training, want_v):
    """Steps 1-5; returns the fake batch (B L, C)."""
    net_g, net_d = self.generator.net, self.discriminator.net
    B = real.shape[0]
    s = _lib.stream()
    n = net_d.L * net_d.C
    fake = net_g.forward(z, B, training)
    _lib.call('cg_mlp_interp', real, fake, alpha.reshape(-1), st['x0'], B, n, s)
    d_out = net_d.forward(st['x0'], 3 * B, training)
    self.last_streams.append(('critic', list(net_g.buffers(B).streams),
                              list(net_d.buffers(3 * B).streams)))
    gin = net_d.backward(3 * B, st['seed3'])
    g = gin[2 * B * net_d.L:]
    _lib.call('cg_mlp_gp_loss', g, d_out, st['norm'], st['gp'][slot:],
              st['coef_gp'], st['v'] if want_v else None, st['loss'][slot], B,
              n, self.penalty, s)
    return fake

  def _draws(self, B, r, alpha=True):
    """(z, alpha) of one pass: no PhaseShuffle in an MLP pair, so no shifts."""
    return draws.latents(self._streams, self.device, [r], B,
                         self.noise_shape[0], alpha)[:2]

  def _critic_compute(self, real, r=None, slot=0):
    """wgan_gp.py:64-80 up to the optimizer update: the critic's gradients in
    discriminator.net.params.grad."""
    B = real.shape[0]
    st = self._get_state(B)
    net_d = self.discriminator.net
    z, alpha = self._draws(B, r)
    self._critic_forward(st, real, z, alpha, slot, True, True)
    net_d.tangent(3 * B, B, st['v'], st['tangent'])
    net_d.weight_grads(3 * B, st['x0'], tails=[st['v']] + st['tangent'], seg=B,
                       coef=(-1.0 / B, 1.0 / B, 1.0), bias_seg=2 * B)

  def _gen_compute(self, real, r=None):
    """wgan_gp.py:22-36 up to the optimizer update; returns the fake batch."""
    B = real.shape[0]
    st = self._get_state(B)
    net_g, net_d = self.generator.net, self.discriminator.net
    z, _ = self._draws(B, r, alpha=False)
    fake = net_g.forward(z, B, True)
    d_out = net_d.forward(fake, B, True)
    self.last_streams.append(('gen', list(net_g.buffers(B).streams),
                              list(net_d.buffers(B).streams)))
    _lib.call('cg_neg_mean', d_out, st['gen_loss'], B, _lib.stream())
    dfake = net_d.backward(B, st['seed_g'])
    net_g.backward(B, dfake, need_dx=False)
    net_g.weight_grads(B, z)
    return fake

  def _metrics_of(self, real, fake):
    net = self.generator.net
    return self.metrics(real, fake.reshape(real.shape[0], net.L, net.C),
                        fake_pitch=net.C)

  def train(self, inputs, rand=None):
    """wgan_gp.py:82-95: n_critic critic updates on the same batch, then one
    generator update.  Returns (gen_loss, dis_loss, gradient_penalty, metrics)
    as 0-d device tensors, no host sync.  `rand` injects the draws for parity
    tests: dict(critic=[dict(z=, alpha=)] * n_critic, gen=dict(z=)); the
    dropout masks are functions of the models' call counters either way."""
    _lib.use(self.precision)
    real = self._to_device(inputs)
    st = self._get_state(real.shape[0])
    n = self.n_critic
    self.last_streams = []
    rc, rg = draws.per_update(rand, n)
    for i in range(n):
      self._critic_compute(real, rc[i], slot=i)
      self.dis_optimizer.update(self.discriminator)
    fake = self._gen_compute(real, rg)
    self.gen_optimizer.update(self.generator)
    metrics = self._metrics_of(real, fake)
    _lib.call('cg_step_outputs', st['gen_loss'], st['loss'], st['gp'],
              metrics[_METRIC_KEYS[0]], n, st['out'], _lib.stream())
    return self._averaged(self._outputs(st['out']))

  def validate(self, inputs, rand=None):
    """gan.py:87-90 with the WGAN-GP loss: training=False (no dropout), the
    penalty's inner gradient included, no update.  Returns (fake, gen_loss,
    dis_loss, gp, metrics).  rand: dict(z=, alpha=)."""
    _lib.use(self.precision)
    real = self._to_device(inputs)
    B = real.shape[0]
    st = self._get_state(B)
    net = self.generator.net
    z, alpha = self._draws(B, rand)
    self.last_streams = []
    fake = self._critic_forward(st, real, z, alpha, 0, False, False)
    metrics = self._metrics_of(real, fake)
    loss = st['loss'][0]
    return (fake.reshape(B, net.L, net.C).clone(),) + self._outputs(
        torch.stack([loss[1], loss[0], st['gp'][0]] +
                    [metrics[k] for k in _METRIC_KEYS]))
