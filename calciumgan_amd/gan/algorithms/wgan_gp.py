"""WGAN-GP train step -- gan/algorithms/wgan_gp.py:12-95 -- as a hand-scheduled
sequence of gfx950 kernels (no autograd graph).

Critic step (reference :64-80).  real, fake and the interpolate x^ run through
the discriminator as ONE batch of 3B samples (per-segment phase shifts):
  1. G forward                       -> fake
  2. interpolate + pack              -> X0 = [real | fake | x^]       (:38-41)
  3. D forward over 3B               -> outputs, activations h_l
  4. delta_5 = c_seg * w_d * lrelu'(h_5), c = (-1/B, +1/B, 1); input-gradient
     chain over 3B down to layer 2, layer 1 only for the x^ segment -> g
  5. ||g||, gp = mean((||g||-1)^2), v = lambda*dgp/dg                 (:48-50)
  6. tangent-forward of v through the SAME masked linear chain (the second
     backward of the penalty; D is piecewise linear, so the mask derivative
     vanishes and biases get no penalty gradient), in place over the x^
     segment's activations
  7. weight gradients over the 3B batch: inputs [h_real | h_fake | tangent],
     output-gradients [delta_real | delta_fake | delta_x^]  == autodiff of
     -E[D(real)] + E[D(fake)] + lambda*gp
  8. (data parallel) all-reduce, Keras Adam, re-pack bf16 operands
Generator step (reference :22-36): G forward (activations kept), D forward and
input-gradient chain on fake, generator backward, Adam, signal metrics.
"""
import collections
import os
import types

import torch

from ... import _lib
from ... import nets
from . import draws
from .gan import GAN, _METRIC_KEYS
from .registry import register

# hipGraph capture of train(): the ~370 launches of one step replay as ONE
# graph on a single rank, and under data parallelism as 2 * n_critic + 3 graphs
# cut around the gradient all-reduces (the RCCL calls stay eager between
# replays and overlap the graphs that do not need their result), removing
# launch gaps (replay.py).  CALCIUMGAN_GRAPH=0 disables it.
# development knob: keep the multi-rank segmentation on a single rank
_FORCE_SPLIT = os.environ.get('CALCIUMGAN_SPLIT_SEGMENTS', '0') == '1'
# single rank: one generator pass for the fake batches of all critic updates
# of a step (CALCIUMGAN_BATCH_G=0: one pass per update, as under data
# parallelism, where each pass hides the previous update's all-reduce)
_BATCH_G = os.environ.get('CALCIUMGAN_BATCH_G', '1') != '0'
# the penalty norm's finishing sum, gp / coef / critic loss and v's per-sample
# scale as ONE launch (cg_gp_loss_scale) instead of three (A/B: =0)
_FUSE_GP = os.environ.get('CALCIUMGAN_FUSE_GP', '1') != '0'
# single rank, batched generator pass: the output Dense of that pass writes the
# critic's input buffers of ALL updates itself -- interpolation and packing in its
# epilogue (cg_dense_rows_interp), one input buffer per update -- instead of an
# f32 fake batch that n_critic cg_interp_pack launches read back (A/B: =0)
_FUSE_INTERP = os.environ.get('CALCIUMGAN_FUSE_INTERP', '1') != '0'

# what _generator_pass hands one critic update: the f32 fake batch, or (fake
# None) the index of the input buffer its output Dense packed [real | fake | x^]
# into; alpha: the update's interpolation factors when the pass drew them
_Fed = collections.namedtuple('_Fed', 'fake alpha x0_index')


@register('wgan-gp')
class WGAN_GP(GAN):
  _has_penalty = True
  _graph_under_dp = True  # (as segments cut around the all-reduces)

  def __new__(cls, hparams, generator, discriminator, summary=None):
    """An MLP pair (--model mlp) goes to the MLP step (wgan_gp_mlp.py): the
    schedule below is the convolutional models'."""
    if cls is WGAN_GP and getattr(generator, 'is_mlp', False):
      from .wgan_gp_mlp import MLP_WGAN_GP
      return MLP_WGAN_GP(hparams, generator, discriminator, summary)
    return super().__new__(cls)

  def __init__(self, hparams, generator, discriminator, summary=None):
    super().__init__(hparams, generator, discriminator, summary)
    self.penalty = float(hparams.gradient_penalty)
    self.n_critic = int(hparams.n_critic)
    self.conv2d = getattr(hparams, 'conv2d', False)
    if self.conv2d:
      raise ValueError('calciumgan_amd: conv2d models are out of scope')

  # -- per-batch-size state ---------------------------------------------------
  def _build_state(self, B):
    dev = self.device
    dws = self.discriminator.net.workspace(3 * B)
    nc = self.n_critic
    # host-drawn inputs of a step on the device; the plans read their
    # PhaseShuffle draws straight from it (draws.critic_stage)
    stage = torch.zeros(draws.critic_stage_words(nc), dtype=torch.int32,
                        device=dev)
    critic_shifts, gen_shifts, _ = draws.critic_stage(stage, nc)
    st = dict(
        gws=self.generator.net.workspace(B),
        dws=dws,
        stage_dev=stage,
        critic=dws.plan(3 * B, B, 2 * B,
                        shifts=critic_shifts[0] if nc > 0 else None),
        gen=dws.plan(B, B, 0, want_norm=False, shifts=gen_shifts),
        norm=torch.zeros(B, dtype=torch.float32, device=dev),
        coef_gp=torch.zeros(B, dtype=torch.float32, device=dev),
        gp=torch.zeros(max(self.n_critic, 1), dtype=torch.float32, device=dev),
        loss=torch.zeros(max(self.n_critic, 1), 2, dtype=torch.float32,
                         device=dev),
        gen_loss=torch.zeros(1, dtype=torch.float32, device=dev),
        # the step's outputs [gen_loss, dis_loss, gp, metrics x 4], written
        # by the last launches of train(); train() hands out a COPY
        out=torch.zeros(7, dtype=torch.float32, device=dev))
    st['critic'].coef.copy_(torch.tensor([-1.0 / B, 1.0 / B, 1.0]))
    st['critic'].bias_coef.copy_(torch.tensor([-1.0 / B, 1.0 / B, 0.0]))
    st['critic'].build_jvp(2, st['coef_gp'])
    st['gen'].coef.copy_(torch.tensor([-1.0 / B]))
    st['gen'].bias_coef.zero_()
    if self.dis_optimizer.loss_scale is not None:
      # mixed_float16: the seeds of the backward chains carry the loss scale
      # (get_scaled_loss, wgan_gp.py:32,76).  The x^ segment's chain is the
      # INNER gradient of the penalty (its own tape, wgan_gp.py:45-48): its
      # seed stays 1, the scale enters its second backward through v
      st['coef_base'] = dict(
          critic=(st['critic'].coef.clone(), st['critic'].bias_coef.clone(),
                  torch.tensor([1.0, 1.0, 0.0], device=dev)),
          gen=(st['gen'].coef.clone(), st['gen'].bias_coef.clone(),
               torch.tensor([1.0], device=dev)))
    # (fp16: the loss scale multiplies coef on the device afterwards -- three
    # launches as before)
    if _FUSE_GP and self.dis_optimizer.loss_scale is None:
      st['critic'].defer_norm()
    return st

  def _critic_plan(self, st, k):
    """The critic plan whose layer-1 launches read input buffer k of the step
    (_DisWorkspace.x0): plan 0 is st['critic']; the others are built on first use
    with the same seeds and tangent chain."""
    if k == 0:
      return st['critic']
    plans = st.setdefault('critic_alt', {})
    pl = plans.get(k)
    if pl is None:
      B = st['coef_gp'].shape[0]
      pl = plans[k] = st['dws'].plan(
          3 * B, B, 2 * B, x0_index=k,
          shifts=draws.critic_stage(st['stage_dev'], self.n_critic)[0][k])
      pl.coef.copy_(st['critic'].coef)
      pl.bias_coef.copy_(st['critic'].bias_coef)
      pl.build_jvp(2, st['coef_gp'])
      if st['critic'].norm_deferred:
        pl.defer_norm()
    return pl

  def _can_fuse_interp(self, B, n, gws=None):
    """cg_dense_rows_interp applies: the streaming output Dense (register form at
    pitch 128, LDS-panel form beyond), n <= 8 updates.  gws: the generator
    workspace of the pass (default: the forward-only one over n * B samples)."""
    if not _FUSE_INTERP:
      return False
    if gws is None:
      gws = self.generator.net.workspace(n * B, forward_only=True)
    lay = self.discriminator.net.layers[0]
    return gws.can_interp(n) and lay.cinp == self.generator.net.Cp

  def _scale_seeds(self, st, which, optimizer, plan=None):
    """coef = base * (S where the segment's loss term is scaled, else 1), on the
    plan the coming launches use (default: st[which])."""
    S = optimizer.loss_scale
    if S is None:
      return
    plan = st[which] if plan is None else plan
    coef, bias_coef, scaled = st['coef_base'][which]
    f = scaled * S + (1.0 - scaled)
    torch.mul(coef, f, out=plan.coef)
    torch.mul(bias_coef, f, out=plan.bias_coef)

  # -- losses (API parity; the fused kernels compute the same values) ---------
  def generator_loss(self, fake_output):
    """wgan_gp.py:19-20."""
    return -fake_output.mean()

  def _critic_forward(self, st, real, z, alpha, shifts, slot,
                      real_cached=False, fake=None, training=True, scale=None,
                      plan=None, packed=False):
    """Steps 1-5 of the critic schedule; leaves g in st['critic'].gin.  `fake`
    is G(z) when the generator forward already ran (_critic_generate).
    training=False (validate, gan.py:87-90): BatchNormalization layers use their
    moving statistics."""
    net_d = self.discriminator.net
    B = real.shape[0]
    lay = net_d.layers[0]
    plan = st['critic'] if plan is None else plan
    s = _lib.stream()
    # (host-drawn shifts of an eager step are a pageable temporary: a
    # non-blocking copy could read it after it is gone once the host runs ahead
    # of the GPU; the graph path hands a device view)
    if shifts.data_ptr() != plan.shifts.data_ptr():  # (else staged in place)
      plan.shifts.copy_(shifts, non_blocking=shifts.is_cuda)
    self._scale_seeds(st, 'critic', self.dis_optimizer, plan)
    if not packed:  # (packed: plan.x0 already holds [real | fake | x^])
      if fake is None:
        fake = st['gws'].forward(z, keep=False, training=training)
      # (a plan that mixes layer 1 of x^ never reads x^: [real | fake] only)
      _lib.call('cg_interp_pack', real, fake,
                None if plan.mixes_layer1 else alpha, plan.x0, B, lay.lin,
                lay.cin, lay.cin, self.generator.net.Cf, lay.cinp,
                0 if real_cached else 1, s)
    plan.forward(seed_backward=True,
                 mix=alpha.reshape(-1) if plan.mixes_layer1 else None)
    plan.backward_chain(seeded=True)
    n = lay.lin * lay.cinp
    if plan.norm_deferred:
      # slots of ||g||^2 -> norm, gp, coef, critic loss and (scale = (g, dst, n
      # per sample): the caller's v = coef_b * g pass) in one launch
      norm = plan.sumsq
      slots, P = plan.ssq
      g, dst, ns = scale if scale is not None else (None, None, 0)
      _lib.call('cg_gp_loss_scale', slots, P, norm, st['gp'][slot:],
                st['coef_gp'], st['dws'].d_out, st['loss'][slot], B,
                self.penalty, 1.0, g, dst, ns, s)
      st['norm_out'] = norm
      return fake
    if plan.sumsq is not None:  # ||g||^2 came out of the dgrad epilogue
      norm = plan.sumsq
      squared = 1
    else:
      norm = st['norm']
      squared = 0
      _lib.call('cg_rownorm', plan.gin, norm, B, n, nets.reduce_ws(self.device),
                s)
    # gp = mean((||g|| - 1)^2), v's per-sample factor and the critic loss: one
    # launch (two single-block reductions over the batch)
    _lib.call('cg_gp_critic_loss', norm, st['gp'][slot:], st['coef_gp'],
              st['dws'].d_out, st['loss'][slot], B, self.penalty, squared, 1.0,
              s)
    if self.dis_optimizer.loss_scale is not None:
      st['coef_gp'].mul_(self.dis_optimizer.loss_scale)  # d(S * lambda * gp)/dg
    st['norm_out'] = norm
    return fake

  # -- the step, cut at the all-reduce points ---------------------------------
  def _critic_generate(self, real, r=None, keep=False):
    """fake = G(z) of one critic update (wgan_gp.py:65-67).  It reads no
    discriminator state, so train() runs it while the previous update's
    gradient all-reduce is still in flight.  keep=True (the generator update's
    own forward): activations stay for GeneratorNet's backward."""
    B = real.shape[0]
    st = self._get_state(B)
    z = draws.latents(self._streams, self.device, [r], B, self.noise_shape[0],
                      alpha=False).z
    return st['gws'].forward(z, keep=keep)

  def _generator_pass(self, real, gws, rs):
    """ONE forward-only pass of G on workspace `gws` for the k = len(rs)
    consecutive critic updates whose draws come from `rs`; returns their _Fed
    records.  k = 1 on st['gws'] is a critic update's own pass; k = n_critic on
    the forward-only workspace is the batched pass of a single rank: the
    generator does not change between the updates (wgan_gp.py:84-90), and the
    small early layers run far better at 5 B.  Where cg_dense_rows_interp applies
    the output Dense writes [real | fake_j | x^_j] into input buffer x0(j) itself:
    no f32 fake batch, no cg_interp_pack (x0(0) is free for a per-update pass:
    every launch of the previous update that read it is ahead on the stream)."""
    B, k = real.shape[0], len(rs)
    st = self._get_state(B)
    fuse = self._can_fuse_interp(B, k, gws)
    # one draw each for the noise and the interpolation factors of all updates
    # (i.i.d.: four RNG launches fewer per step).  A per-update pass that does not
    # fuse leaves alpha to its critic update, behind the all-reduce wait
    z, alpha, _ = draws.latents(self._streams, self.device, rs, B,
                                self.noise_shape[0], alpha=fuse or k > 1)
    part = lambda t, j: None if t is None else t[j * B:(j + 1) * B]
    if fuse:
      # (plans that form layer 1 of x^ from the other two segments' never read x^)
      gws.forward(z, keep=False,
                  interp=(real, None if st['critic'].mixes_layer1 else alpha,
                          [st['dws'].x0(j) for j in range(k)]))
      return [_Fed(None, part(alpha, j), j) for j in range(k)]
    fake = gws.forward(z, keep=False)
    return [_Fed(part(fake, j), part(alpha, j), None) for j in range(k)]

  def _critic_compute(self, real, r=None, slot=0, real_cached=False,
                      fake=None, alpha=None, x0_index=None):
    """wgan_gp.py:64-80 up to (not including) the optimizer update: leaves the
    critic gradients in discriminator.net.params.grad.  fake, alpha, x0_index:
    the _Fed record of this update when a generator pass ran ahead of it."""
    B = real.shape[0]
    st = self._get_state(B)
    net_d = self.discriminator.net
    lay = net_d.layers[0]
    packed = x0_index is not None  # (the generator pass packed X0 itself)
    if fake is None and not packed:
      fake = self._critic_generate(real, r)
    if alpha is None:
      alpha = draws.latents(self._streams, self.device, [r], B).alpha
    shifts = draws.shifts(self._streams, r, 3)
    plan = self._critic_plan(st, x0_index or 0)
    n = lay.lin * lay.cinp
    if plan.jvp_folds:
      # g already sits over the x^ segment of X0; v = lambda * dgp/dg = coef_b * g
      # enters the tangent chain as a per-sample scale of its first launch and
      # the layer-1 weight gradient through delta_1's x^ segment (g (x) coef
      # delta == coef g (x) delta): a pass over 1/4 of the bytes
      d1 = st['dws'].delta[1][2 * B:3 * B]
      scale = (d1, d1, d1[0].numel())
    else:
      # v = lambda * dgp/dg, written over the x^ segment of X0 (in place when g
      # already sits there)
      scale = (plan.gin, plan.x0[2 * B:], n)
    self._critic_forward(st, real, None, alpha, shifts, slot, real_cached,
                         fake=fake, scale=scale, plan=plan, packed=packed)
    s = _lib.stream()
    if not plan.norm_deferred:  # (else cg_gp_loss_scale has scaled the rows)
      _lib.call('cg_scale_rows', scale[0], st['coef_gp'], scale[1], B, scale[2],
                s)
    plan.jvp_forward()
    if not nets.DETERMINISTIC:  # (the ordered reductions store every gradient)
      net_d.params.grad.zero_()
    # bias gradients: real + fake segments only (the penalty has none)
    plan.weight_grads(bias_rows=2 * B)

  def _critic_apply(self, lr_t_dev=None):
    self.dis_optimizer.update(self.discriminator, self._sync.grad_scale,
                              lr_t_dev=lr_t_dev)

  def _train_discriminator(self, inputs, r=None, slot=0, real_cached=False,
                           lr_t_dev=None):
    """wgan_gp.py:64-80."""
    real = self._to_device(inputs)
    st = self._get_state(real.shape[0])
    self._critic_compute(real, r, slot, real_cached)
    self._sync.all_reduce(self.discriminator.net.params.grad)
    self._critic_apply(lr_t_dev)
    return st['loss'][slot, 0], st['gp'][slot]

  def _gen_compute(self, real, r=None, fake=None):
    """wgan_gp.py:22-36 up to the optimizer update."""
    B = real.shape[0]
    st = self._get_state(B)
    net_g, net_d = self.generator.net, self.discriminator.net
    lay = net_d.layers[0]
    plan = st['gen']
    if fake is None:
      fake = self._critic_generate(real, r, keep=True)  # same op: fake = G(z)
    shifts = draws.shifts(self._streams, r, 1)
    s = _lib.stream()
    if shifts.data_ptr() != plan.shifts.data_ptr():
      plan.shifts.copy_(shifts, non_blocking=shifts.is_cuda)
    self._scale_seeds(st, 'gen', self.gen_optimizer)
    _lib.call('cg_cast_pad', fake, st['dws'].act[0], B * lay.lin, lay.cin,
              self.generator.net.Cf, lay.cinp, s)
    plan.forward(seed_backward=True)
    _lib.call('cg_neg_mean', st['dws'].d_out, st['gen_loss'], B, s)
    plan.backward_chain(seeded=True)
    if not nets.DETERMINISTIC:
      net_g.params.grad.zero_()
    st['gws'].backward(plan.gin)

  def _gen_metrics(self, real):
    """gan.py:32-41 on the fake batch of the generator update."""
    st = self._get_state(real.shape[0])
    return self.metrics(real, st['gws'].fake, fake_pitch=self.generator.net.Cf)

  def _gen_apply(self, real, lr_t_dev=None, metrics=None):
    self.gen_optimizer.update(self.generator, self._sync.grad_scale,
                              lr_t_dev=lr_t_dev)
    return self._gen_metrics(real) if metrics is None else metrics

  def _train_generator(self, inputs, r=None, lr_t_dev=None):
    """wgan_gp.py:22-36."""
    real = self._to_device(inputs)
    st = self._get_state(real.shape[0])
    self._gen_compute(real, r)
    self._sync.all_reduce(self.generator.net.params.grad)
    metrics = self._gen_apply(real, lr_t_dev)
    return st['gen_loss'][0], metrics

  def _segments(self, real, rand=None, staged=False):
    """One train() (wgan_gp.py:82-95: n_critic critic updates on the SAME
    batch, then one generator update) as launch segments cut around the
    gradient all-reduces.  `rand` optionally injects the random draws (same
    structure as oracle.draw_randomness) for parity tests.  Returns
    [(callable, flat_grad_or_None, wait)]: after a segment with a gradient
    buffer its all-reduce is STARTED; a segment with wait=True needs the
    pending all-reduce finished first.  Work that does not read the reduced
    gradients -- the next update's G(z), the signal metrics -- sits in
    wait=False segments and overlaps the collective:

      [G(z0) D-step0] ar | [G(z1)] wait [adam0 D-step1] ar | ... |
      [G(zg)] wait [adam D fwd/bwd, G bwd] ar | [metrics] wait [adam_G, outputs]

    The last callable stores the step's outputs in st['out'].  staged (graph
    replay): update k reads its shifts from the state's stage buffer (where the
    plans' own shifts are views of it) and its Adam step size behind them."""
    n = self.n_critic
    B = real.shape[0]
    st = self._get_state(B)
    lr = lambda i: None
    if staged:
      critic_shifts, gen_shifts, lr_dev = draws.critic_stage(st['stage_dev'], n)
      rand = dict(critic=[draws.staged(v) for v in critic_shifts],
                  gen=draws.staged(gen_shifts))
      lr = lambda i: lr_dev[i:]
    rc, rg = draws.per_update(rand, n)
    d_grad = self.discriminator.net.params.grad
    g_grad = self.generator.net.params.grad
    # what the step's closures hand each other: the _Fed record of every critic
    # update, the generator update's own fake batch, the signal metrics
    step = types.SimpleNamespace(fed=[None] * n, fake=None, metrics=None)
    chain = lambda *fns: lambda: [fn() for fn in fns]

    def generate(i0, k, gws):
      def run():
        step.fed[i0:i0 + k] = self._generator_pass(real, gws, rc[i0:i0 + k])
      return run

    def critic_seg(i):
      def run():
        if i > 0:
          self._critic_apply(lr(i - 1))
        # the bf16 copy of `real` in X0[0:B] survives a critic step (only the
        # x^ segment is overwritten): converted once per train()
        self._critic_compute(real, rc[i], slot=i, real_cached=i > 0,
                             **step.fed[i]._asdict())
        step.fed[i] = None
      return run

    def generate_g():
      # the only forward that is followed by a backward through G
      step.fake = self._critic_generate(real, rg, keep=True)

    def gen_seg():
      if n > 0:
        self._critic_apply(lr(n - 1))
      self._gen_compute(real, rg, fake=step.fake)

    def metrics_seg():
      step.metrics = self._gen_metrics(real)

    def last_seg():
      metrics = self._gen_apply(real, lr(n), metrics=step.metrics)
      # (metrics are views of one 4-float buffer: GAN.metrics)
      _lib.call('cg_step_outputs', st['gen_loss'], st['loss'], st['gp'],
                metrics[_METRIC_KEYS[0]], n, st['out'], _lib.stream())

    segs = []
    for i in range(n):
      segs += [(generate(i, 1, st['gws']), None, False),
               (critic_seg(i), d_grad, True)]
    if n > 0:  # [G(z0) D-step0]: no all-reduce is pending yet
      segs[:2] = [(chain(segs[0][0], segs[1][0]), d_grad, False)]
    tail = [(generate_g, None, False), (gen_seg, g_grad, True),
            (metrics_seg, None, False), (last_seg, None, True)]
    if self._sync.world > 1 or _FORCE_SPLIT:
      return segs + tail
    # no collective to cut around: the whole step is one segment (one graph)
    # (BatchNormalization: the batch statistics are those of ONE update's
    # fake batch -- no batched pass)
    if _BATCH_G and n > 1 and not self.generator.net.batch_norm:
      # ... and no all-reduce for G(z_i) to hide behind: all critic updates'
      # fake batches come from ONE generator pass at the start of the step
      segs = [(generate(0, n, self.generator.net.workspace(
          n * B, forward_only=True)), None, False)]
      segs += [(critic_seg(i), d_grad, True) for i in range(n)]
    return [(chain(*[fn for fn, _, _ in segs + tail]), None, False)]

  @property
  def _adam_steps(self):
    return self.n_critic, 1

  def _fill_stage(self, host):
    """[shifts int32 x (12 n + 4) | lr_t f32 x (n + 1)] of the coming step."""
    n = self.n_critic
    critic_shifts, gen_shifts, lr = draws.critic_stage(host, n)
    for view in critic_shifts:
      view.copy_(self._streams.shifts(3))
    gen_shifts.copy_(self._streams.shifts(1))
    for i in range(n):
      lr[i] = self.dis_optimizer.lr_t(self.dis_optimizer.host_steps + i + 1)
    lr[n] = self.gen_optimizer.lr_t(self.gen_optimizer.host_steps + 1)

  def validate(self, inputs, rand=None):
    """gan.py:87-90 / :58-70 with the WGAN-GP loss (inner-gradient penalty, no
    parameter update).  Returns (fake, gen_loss, dis_loss, gp, metrics)."""
    _lib.use(self.precision)
    real = self._to_device(inputs)
    B = real.shape[0]
    st = self._get_state(B)
    z, alpha, shifts = draws.draw(self._streams, self.device, rand, B,
                                  self.noise_shape[0], True, 3)
    fake = self._critic_forward(st, real, z, alpha, shifts, 0, training=False)
    C = self.generator.net.C
    metrics = self.metrics(real, fake, fake_pitch=self.generator.net.Cf)
    loss = st['loss'][0]
    return (fake[:, :, :C].clone(),) + self._outputs(
        torch.stack([loss[1], loss[0], st['gp'][0]] +
                    [metrics[k] for k in _METRIC_KEYS]))
