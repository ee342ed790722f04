"""Base GAN object -- gan/algorithms/gan.py:13-97: get_noise, metrics,
generate (which WGAN-GP inherits) and the vanilla GAN step with binary
cross-entropy from logits (gan.py:43-90), hand-scheduled on gfx950 kernels.

One train() (gan.py:72-85) on a batch `real` of B samples:
  1. G forward (activations kept)                          -> fake
  2. pack X0 = [fake | real] (bf16)                         (fake first: the
     B-sample plan of step 5 runs over the first B samples of the same
     workspace and reads the forward's fake-segment activations)
  3. D forward over 2B, one set of PhaseShuffle draws per segment
  4. cg_dense1_bce: logits, the two BCE means, the per-sample seeds
       c_d = S_d (s(x) - y) / B (y = 0 fake, 1 real),  c_g = S_g (s(f) - 1) / B
     and delta_5 of both chains
  5. D input-gradient chain over 2B, D weight gradients (bias rows 2B, head
     from the per-sample c_d)
  6. G chain: the D input-gradient chain over the fake segment only, down to
     layer 1, from delta_5 of c_g; generator backward
  7. signal metrics of this fake batch; (data parallel) all-reduce of both
     gradients; Adam on D, then on G -- after every read of D's weights
There is no n_critic loop and no penalty.  The state of the step lives under
`_bce_` names: WGAN_GP subclasses this class and never touches it.
"""
import os

import torch

from ... import _lib
from ... import nets
from ... import parallel
from .optimizer import Optimizer
from .registry import register

# main.py:11-12 (CALCIUMGAN_SEED: another draw of the noise / interpolation /
# shift streams, for seed-to-seed comparisons -- tools/e2e_seeds.sh)
_SEED = int(__import__('os').environ.get('CALCIUMGAN_SEED', '1234'))
_METRIC_KEYS = ('signals_metrics/min', 'signals_metrics/max',
                'signals_metrics/mean', 'signals_metrics/std')
# the BCE step replays as one hipGraph after this many eager calls per batch
# size (single rank; CALCIUMGAN_GRAPH=0 keeps it eager, as for WGAN-GP)
_BCE_GRAPH_WARMUP_CALLS = 2
# pinned staging slots of the host-drawn inputs of a replay (phase shifts, Adam
# step sizes): the host may run this many steps ahead before it waits
_BCE_STAGING_SLOTS = 4
# staged words per step: [2B plan shifts int32 (4, 2) | fake-segment plan
# shifts (4, 1) | Adam step sizes f32 (D, G)]
_BCE_STAGE_WORDS = 14


@register('gan')
class GAN(object):

  def __init__(self, hparams, generator, discriminator, summary=None):
    self.generator = generator
    self.discriminator = discriminator
    self._summary = summary
    self.noise_shape = tuple(hparams.noise_shape)
    self.signal_shape = tuple(hparams.signal_shape)
    self._normalize = hparams.normalize
    self._signals_min = float(getattr(hparams, 'signals_min', 0.0))
    self._signals_max = float(getattr(hparams, 'signals_max', 1.0))
    if not hparams.normalize:
      self._signals_min, self._signals_max = 0.0, 1.0

    self.device = generator.net.device
    # the build of the kernel library both models compute with ('f16' under
    # hparams.mixed_precision); every entry point re-selects it
    self.precision = generator.net.precision
    if discriminator.net.precision != self.precision:
      raise ValueError('generator and discriminator differ in precision')
    self.gen_optimizer = Optimizer(hparams, self.device)
    self.dis_optimizer = Optimizer(hparams, self.device)

    self._sync = parallel.GradSync()
    self._streams = parallel.RandomStreams(_SEED, self.device, hparams.m)
    self._metrics_buf = torch.zeros(4, dtype=torch.float32, device=self.device)

  # -- helpers ---------------------------------------------------------------
  def _to_device(self, x):
    if not torch.is_tensor(x):
      x = torch.as_tensor(x)
    return x.to(device=self.device, dtype=torch.float32).contiguous()

  def get_noise(self, batch_size):
    """gan.py:29-30: N(0,1) of shape (batch,) + noise_shape."""
    return self._streams.noise(batch_size, self.noise_shape[0])

  def metrics(self, real, fake, fake_pitch=None):
    """gan.py:32-41 + signals_metrics.py:9-28: MSE between real and fake of the
    per-(sample, timestep) min / max / mean / std over channels, after
    denormalisation.  real (B, L, C) f32 contiguous; fake f32 with row pitch
    fake_pitch (defaults to C)."""
    B, L, C = real.shape
    rows = B * L
    rws = nets.reduce_ws(self.device)
    if rws is not None:
      # ordered reduction: the finishing launch stores the means
      buf = torch.empty(4, dtype=torch.float32, device=self.device)
    else:
      buf = torch.zeros(4, dtype=torch.float32, device=self.device)
    _lib.call('cg_signal_metrics', nets._p(real), nets._p(fake), nets._p(buf),
              rows, C, C, fake_pitch or C, self._signals_min,
              self._signals_max, nets._p(rws), nets._stream())
    if rws is None:
      buf.mul_(1.0 / rows)
    return {
        'signals_metrics/min': buf[0],
        'signals_metrics/max': buf[1],
        'signals_metrics/mean': buf[2],
        'signals_metrics/std': buf[3],
    }

  # -- spike statistics of a validation batch (csrc/spikes.hip) ----------------
  def spike_real_statistics(self, real_spikes):
    """Device (rates (B, C), covariances (B, C (C + 1) / 2)) of the ground-truth
    trains (B, L, C) of a validation batch, taken as
    compute_dg_metrics.get_data_statistics takes them from a file with `spikes`
    (the trains as float32, no deconvolution).  An unshuffled validation set
    gives the same batches every epoch: the caller may keep the result."""
    from ..utils import spike_metrics
    if not torch.is_tensor(real_spikes):
      import numpy as np
      real_spikes = torch.from_numpy(
          np.ascontiguousarray(np.asarray(real_spikes), dtype=np.float32))
    spikes = real_spikes.to(device=self.device, dtype=torch.float32)
    return spike_metrics.batch_statistics_device(spikes)

  def spike_statistics(self, fake, real_spikes=None, real_stats=None):
    """The spike criterion of one validation batch, on the device: `fake`
    ((B, L, C) f32 as validate() returns it, or the channel-padded generator
    output: only the first C channels are read) is denormalised with this
    algorithm's signals_min / max, deconvolved (OASIS AR(1), g 0.95, s_min 0.55,
    threshold 0.5: spike_helper.deconvolve_signals bit for bit) and reduced to
    per-trial firing rates and binned covariances; the real side comes from
    the ground-truth trains `real_spikes` (B, L, C), or from `real_stats` =
    spike_real_statistics(real_spikes) kept by the caller; sample i is paired
    with sample i.  Returns 0-d device tensors: the sums of |d| and d^2 of both
    statistics (compute_dg_metrics.report's MAE / RMSE / MSE are these sums
    divided by the counts) and the two counts.  No host sync."""
    from ..utils import spike_helper, spike_metrics
    C = self.signal_shape[-1]
    fake = fake[:, :, :C]
    if real_stats is None:
      real_stats = self.spike_real_statistics(real_spikes)
    spikes = spike_helper.deconvolve_signals_device(
        fake, scale=self._signals_max - self._signals_min,
        offset=self._signals_min)
    rates, covs = spike_metrics.batch_statistics_device(spikes)
    if rates.shape != real_stats[0].shape:
      raise ValueError('fake batch {} and real trains {} differ in shape'.format(
          tuple(rates.shape), tuple(real_stats[0].shape)))
    sums = spike_metrics.error_sums_device(real_stats[0], rates, real_stats[1],
                                           covs)
    count = lambda t: torch.tensor(float(t.numel()), dtype=torch.float64,
                                   device=self.device)
    return {
        'firing_rate_abs_sum': sums[0],
        'firing_rate_sq_sum': sums[1],
        'covariance_abs_sum': sums[2],
        'covariance_sq_sum': sums[3],
        'firing_rate_count': count(rates),
        'covariance_count': count(covs),
    }

  # -- the BCE step (gan.py:43-90) ---------------------------------------------
  def _bce_get_state(self, B):
    states = self.__dict__.setdefault('_bce_states', {})
    st = states.get(B)
    if st is None:
      dev = self.device
      dws = self.discriminator.net.workspace(2 * B)
      stage = torch.zeros(_BCE_STAGE_WORDS, dtype=torch.int32, device=dev)
      f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
      st = dict(
          gws=self.generator.net.workspace(B),
          dws=dws,
          stage_dev=stage,
          # D chain over [fake | real]; segment 0 is the fake batch
          dis=dws.plan(2 * B, B, None, want_norm=False,
                       shifts=stage[0:8].view(4, 2)),
          # G chain: the same workspace's first B samples (the fake segment's
          # activations of the 2B forward), input gradient down to layer 1
          gen=dws.plan(B, B, 0, want_norm=False, shifts=stage[8:12].view(4, 1)),
          coef_d=f32(2 * B),
          coef_g=f32(B),
          delta_g=torch.zeros_like(dws.delta[-1][:B]),
          loss=f32(2),  # [gen_loss, dis_loss]
          zero=f32(1),  # (the penalty slot of cg_step_outputs)
          out=f32(7))
      states[B] = st
    return st

  def _bce_shifts(self, r):
    """Host int32 (12,): the (4, 2) [fake | real] shifts of the 2B plan, then the
    fake segment's 4 for the G chain's plan.  r None: ONE draw of the shared
    stream, (4, 2) = [shifts_real | shifts_fake] (z is drawn before it)."""
    if r is None:
      sh = self._streams.shifts(2)
      real_s, fake_s = sh[:, 0], sh[:, 1]
    else:
      real_s = torch.as_tensor(r['shifts_real'], dtype=torch.int32).reshape(4)
      fake_s = torch.as_tensor(r['shifts_fake'], dtype=torch.int32).reshape(4)
    return torch.cat([torch.stack([fake_s, real_s], 1).reshape(-1), fake_s])

  def _bce_forward(self, st, real, z, shifts, training=True, seeds=True):
    """Steps 1-4: G(z) -> X0 = [fake | real] -> D over 2B -> cg_dense1_bce.
    shifts: host int32 (12,) (_bce_shifts) or None when already staged.
    seeds=False (validate): losses only, no seeds."""
    net_g, net_d = self.generator.net, self.discriminator.net
    B = real.shape[0]
    lay, last = net_d.layers[0], net_d.layers[-1]
    dws, pd = st['dws'], st['dis']
    s = nets._stream()
    if shifts is not None:
      st['stage_dev'][:12].copy_(shifts)
    fake = st['gws'].forward(z, keep=training, training=training)
    x0 = pd.x0
    _lib.call('cg_cast_pad', nets._p(fake), nets._p(x0), B * lay.lin, lay.cin,
              net_g.Cf, lay.cinp, s)
    _lib.call('cg_cast_pad', nets._p(real), nets._p(x0[B:2 * B]), B * lay.lin,
              lay.cin, lay.cin, lay.cinp, s)
    pd.forward(head=False)
    rws = nets.reduce_ws(self.device)
    if rws is None:
      st['loss'].zero_()  # (the atomics form adds onto it)
    sd = self.dis_optimizer.loss_scale if seeds else None
    sg = self.gen_optimizer.loss_scale if seeds else None
    _lib.call('cg_dense1_bce', nets._p(dws.act[-1]), nets._p(net_d.dense_w),
              nets._p(net_d.dense_b), nets._p(dws.d_out),
              nets._p(st['coef_d'] if seeds else None),
              nets._p(st['coef_g'] if seeds else None),
              nets._p(dws.delta[-1] if seeds else None),
              nets._p(st['delta_g'] if seeds else None), nets._p(st['loss']),
              nets._p(sd), nets._p(sg), B, last.lout, last.cout, last.coutp,
              net_d.alpha, nets._p(rws), s)
    return fake

  def _bce_compute(self, real, r=None):
    """Steps 1-6: leaves both models' gradients in params.grad and the losses
    in the state's `loss`; updates nothing.  r: injected draws
    (dict(z=, shifts_real=, shifts_fake=)), dict(shifts_dev=True) when the
    shifts are staged on the device (graph replay), or None."""
    B = real.shape[0]
    st = self._bce_get_state(B)
    net_g, net_d = self.generator.net, self.discriminator.net
    if r is None or 'shifts_dev' in r:
      z = self.get_noise(B)
      shifts = None if r is not None else self._bce_shifts(None)
    else:
      z = self._to_device(r['z'])
      shifts = self._bce_shifts(r)
    self._bce_forward(st, real, z, shifts)
    dws, pd, pg = st['dws'], st['dis'], st['gen']
    # D chain over 2B: no layer-1 input gradient; every sample has a bias term
    pd.backward_chain(seeded=True)
    if not nets.DETERMINISTIC:  # (the ordered reductions store every gradient)
      net_d.params.grad.zero_()
    pd.weight_grads(bias_rows=2 * B, head_coef=st['coef_d'])
    # G chain over the fake segment with D's weights of this step (Adam on D
    # runs after it): its delta_5 replaces the D chain's, which the weight
    # gradients above have consumed
    dws.delta[-1][:B].copy_(st['delta_g'])
    pg.backward_chain(seeded=True)
    if not nets.DETERMINISTIC:
      net_g.params.grad.zero_()
    st['gws'].backward(pg.gin)

  def _bce_step(self, real, r=None, lr_dev=None):
    """One whole train(): compute, metrics, gradient sync, Adam on D then G,
    the outputs buffer.  lr_dev (graph replay): the staged Adam step sizes."""
    st = self._bce_get_state(real.shape[0])
    self._bce_compute(real, r)
    metrics = self.metrics(real, st['gws'].fake, fake_pitch=self.generator.net.Cf)
    self._sync.all_reduce(self.discriminator.net.params.grad)
    self._sync.all_reduce(self.generator.net.params.grad)
    self.dis_optimizer.update(self.discriminator, self._sync.grad_scale,
                              lr_t_dev=None if lr_dev is None else lr_dev[0:])
    self.gen_optimizer.update(self.generator, self._sync.grad_scale,
                              lr_t_dev=None if lr_dev is None else lr_dev[1:])
    return self._bce_outputs(st, metrics)

  def _bce_outputs(self, st, metrics):
    """[gen_loss, dis_loss, 0, metrics x 4] into the state's out buffer."""
    loss = st['loss']
    _lib.call('cg_step_outputs', nets._p(loss[0:1]), nets._p(loss[1:2]),
              nets._p(st['zero']), nets._p(metrics[_METRIC_KEYS[0]]), 1,
              nets._p(st['out']), nets._stream())
    return st['out']

  def _bce_returns(self, o):
    """(gen_loss, dis_loss, metrics) as views of a fresh copy of the outputs
    buffer (the next step rewrites it in place); the means over the ranks under
    data parallelism."""
    o = self._sync.mean_scalars(o.clone())
    return o[0], o[1], {k: o[3 + i] for i, k in enumerate(_METRIC_KEYS)}

  def batch_buffer(self, B):
    """The device buffer a replay of train() reads its batch of B samples from,
    (B,) + signal_shape f32: a loader that gathers each batch into it saves the
    copy in front of every replay (as WGAN_GP.batch_buffer)."""
    st = self._bce_get_state(B)
    g = st.get('graph')
    if g is not None:
      return g['real']
    if st.get('batch_buf') is None:
      st['batch_buf'] = torch.empty((B,) + self.signal_shape,
                                    dtype=torch.float32, device=self.device)
    return st['batch_buf']

  def _bce_capture(self, real, st):
    """Capture one train() as ONE hipGraph.  The shifts and the Adam step sizes
    of a replay are copied into the state's stage buffer ahead of it
    (_bce_stage); z comes from the graph-registered device generator."""
    g = dict(
        real=(st['batch_buf'] if st.get('batch_buf') is not None and
              st['batch_buf'].shape == real.shape else torch.empty_like(real)),
        stage_host=[torch.zeros(_BCE_STAGE_WORDS, dtype=torch.int32).pin_memory()
                    for _ in range(_BCE_STAGING_SLOTS)],
        stage_event=[None] * _BCE_STAGING_SLOTS,
        stage_next=0)
    if g['real'].data_ptr() != real.data_ptr():
      g['real'].copy_(real)
    lr_dev = st['stage_dev'][12:].view(torch.float32)
    steps = (self.dis_optimizer.host_steps, self.gen_optimizer.host_steps)
    torch.cuda.synchronize()
    try:
      graph = torch.cuda.CUDAGraph()
      graph.register_generator_state(self._streams.local)
      with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        g['out'] = self._bce_step(g['real'], dict(shifts_dev=True), lr_dev)
    finally:
      # capture only records: undo the host step counters it advanced
      self.dis_optimizer.host_steps, self.gen_optimizer.host_steps = steps
    g['graph'] = graph
    return g

  def _bce_stage(self, st, g):
    """Shifts and Adam step sizes of the coming replay -> the stage buffer,
    through a ring of pinned slots (an event per slot keeps the host from
    rewriting a slot whose copy has not run yet)."""
    k = g['stage_next']
    g['stage_next'] = (k + 1) % _BCE_STAGING_SLOTS
    if g['stage_event'][k] is not None:
      g['stage_event'][k].synchronize()
    host = g['stage_host'][k]
    host[:12] = self._bce_shifts(None)
    lr = host[12:].view(torch.float32)
    lr[0] = self.dis_optimizer.lr_t(self.dis_optimizer.host_steps + 1)
    lr[1] = self.gen_optimizer.lr_t(self.gen_optimizer.host_steps + 1)
    st['stage_dev'].copy_(host, non_blocking=True)
    ev = g['stage_event'][k] = torch.cuda.Event()
    ev.record()

  def _bce_train_graphed(self, real, st):
    g = st.get('graph')
    if g is None:
      try:
        g = st['graph'] = self._bce_capture(real, st)
      except Exception as e:  # noqa: BLE001 -- any capture failure
        import warnings
        warnings.warn('calciumgan_amd: hipGraph capture of train() failed '
                      '({}: {}); continuing with eager launches'.format(
                          type(e).__name__, e))
        self._use_graph = False
        torch.cuda.synchronize()
        return self._bce_step(real)
    if g['real'].data_ptr() != real.data_ptr():
      g['real'].copy_(real)
    # (the draw order of an eager step: z on the device generator inside the
    # graph, then the shifts here)
    self._bce_stage(st, g)
    g['graph'].replay()
    self.dis_optimizer.host_steps += 1
    self.gen_optimizer.host_steps += 1
    return g['out']

  def train(self, inputs, rand=None):
    """gan.py:72-85: ONE forward of G and D on [fake | real], both models'
    gradients from it with D's weights before either update, then Adam on D and
    on G.  Returns (gen_loss, dis_loss, None, metrics) as 0-d device tensors (no
    host sync; views of a copy, valid across later steps; the means over the
    ranks under data parallelism).  rand = dict(z=, shifts_real=, shifts_fake=)
    injects the draws; otherwise z (per-rank device stream), then one (4, 2)
    draw [shifts_real | shifts_fake] of the shared stream.  A single rank
    replays the step as a hipGraph after two eager calls per batch size."""
    _lib.use(self.precision)
    real = self._to_device(inputs)
    st = self._bce_get_state(real.shape[0])
    # (set on first use, not in __init__: WGAN_GP sets its own.  main.py's
    # --profile window switches it off and back through the same attribute)
    use_graph = self.__dict__.setdefault(
        '_use_graph', os.environ.get('CALCIUMGAN_GRAPH', '1') != '0')
    if rand is None and use_graph and self._sync.world == 1:
      st['calls'] = st.get('calls', 0) + 1
      if st['calls'] > _BCE_GRAPH_WARMUP_CALLS:
        o = self._bce_train_graphed(real, st)
        gen_loss, dis_loss, metrics = self._bce_returns(o)
        return gen_loss, dis_loss, None, metrics
    o = self._bce_step(real, rand)
    gen_loss, dis_loss, metrics = self._bce_returns(o)
    return gen_loss, dis_loss, None, metrics

  def validate(self, inputs, rand=None):
    """gan.py:87-90 / :58-70: the same losses with training=False, no update.
    Returns (fake, gen_loss, dis_loss, None, metrics)."""
    _lib.use(self.precision)
    real = self._to_device(inputs)
    B = real.shape[0]
    st = self._bce_get_state(B)
    if rand is None:
      z = self.get_noise(B)
      shifts = self._bce_shifts(None)
    else:
      z = self._to_device(rand['z'])
      shifts = self._bce_shifts(rand)
    # (the staged shifts of a captured step are rewritten before each replay)
    fake = self._bce_forward(st, real, z, shifts, training=False, seeds=False)
    metrics = self.metrics(real, fake, fake_pitch=self.generator.net.Cf)
    gen_loss, dis_loss, metrics = self._bce_returns(
        self._bce_outputs(st, metrics))
    C = self.generator.net.C
    return fake[:, :, :C].clone(), gen_loss, dis_loss, None, metrics

  def generate(self, noise, denorm=False):
    """gan.py:92-97."""
    fake = self.generator(noise, training=False)
    if denorm:
      fake = fake * (self._signals_max - self._signals_min) + self._signals_min
    return fake
