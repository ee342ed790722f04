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
There is no n_critic loop and no penalty.

GAN is also the base of every algorithm: train() is a template over the
per-class pieces (_build_state, _segments, _fill_stage, _adam_steps,
_graph_under_dp) that replay.py drives, eagerly or as hipGraph replays.
"""
import contextlib
import os

import torch

from ... import _lib
from ... import nets
from ... import parallel
from . import averaging
from . import draws
from . import replay
from .optimizer import Optimizer
from .registry import register

# main.py:11-12 (CALCIUMGAN_SEED: another draw of the noise / interpolation /
# shift streams, for seed-to-seed comparisons -- tools/e2e_seeds.sh)
_SEED = int(os.environ.get('CALCIUMGAN_SEED', '1234'))
_METRIC_KEYS = ('signals_metrics/min', 'signals_metrics/max',
                'signals_metrics/mean', 'signals_metrics/std')


@register('gan')
class GAN(object):
  # the BCE step replays as a graph on a single rank only
  _graph_under_dp = False
  # train() returns None in the penalty position
  _has_penalty = False
  # whether the class's step drives an MLP pair (models/mlp.py): wgan_gp_mlp only
  _mlp_step = False

  def __init__(self, hparams, generator, discriminator, summary=None):
    for model in (generator, discriminator):
      if getattr(model, 'is_mlp', False) != self._mlp_step:
        raise ValueError(
            'calciumgan_amd: the MLP step needs an MLP generator and '
            'discriminator' if self._mlp_step else
            'calciumgan_amd: --model mlp trains under --algorithm wgan-gp only '
            '(the {} step is scheduled for the convolutional models)'.format(
                type(self).__name__))
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
    # an FFT dataset (info['fft']): the channels are [real | imag] spectra of
    # num_neurons traces; the spike statistics are taken of the traces
    self._fft = bool(getattr(hparams, 'fft', False))
    self._num_neurons = int(getattr(hparams, 'num_neurons',
                                    self.signal_shape[-1]))

    self.device = generator.net.device
    # the build of the kernel library both models compute with ('f16' under
    # hparams.mixed_precision); every entry point re-selects it
    self.precision = generator.net.precision
    if discriminator.net.precision != self.precision:
      raise ValueError('generator and discriminator differ in precision')
    self.gen_optimizer = Optimizer(hparams, self.device)
    self.dis_optimizer = Optimizer(hparams, self.device)
    # --ema_decay: the running average of the generator's weights
    # (averaging.py); None without the flag, and then nothing below runs
    self.average = None
    if hasattr(hparams, 'ema_decay'):
      self.average = averaging.WeightAverage(
          generator.net.params, averaging.check_decay(hparams.ema_decay))

    self._sync = parallel.GradSync()
    self._streams = parallel.RandomStreams(_SEED, self.device, hparams.m)
    self._metrics_buf = torch.zeros(4, dtype=torch.float32, device=self.device)
    # per-batch-size state of the step (workspaces, plans, captured graphs)
    self._state = {}
    # CALCIUMGAN_GRAPH=0 keeps every step eager; main.py's --profile window
    # switches it off and back through the same attribute
    self._use_graph = os.environ.get('CALCIUMGAN_GRAPH', '1') != '0'

  # -- helpers ---------------------------------------------------------------
  def _to_device(self, x):
    return draws.to_device(x, self.device)

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
    _lib.call('cg_signal_metrics', real, fake, buf, rows, C, C, fake_pitch or C,
              self._signals_min, self._signals_max, rws, _lib.stream())
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
    divided by the counts) and the two counts.  On an FFT dataset (hparams.fft)
    the C channels are the [real | imag] spectra of hparams.num_neurons traces:
    they are denormalised and inverted by utils.ifft_channels_device first and
    the statistics are those of the traces.  No host sync."""
    from ..utils import spike_helper, spike_metrics
    C = self.signal_shape[-1]
    fake = fake[:, :, :C]
    if real_stats is None:
      real_stats = self.spike_real_statistics(real_spikes)
    if self._fft:
      # [real | imag] spectra: denormalise and invert in one launch, then
      # deconvolve the num_neurons traces as they are
      from ..utils import utils
      spikes = spike_helper.deconvolve_signals_device(
          utils.ifft_channels_device(
              fake, self._num_neurons,
              scale=self._signals_max - self._signals_min,
              offset=self._signals_min))
    else:
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
  def _get_state(self, B):
    st = self._state.get(B)
    if st is None:
      st = self._state[B] = self._build_state(B)
    return st

  def _build_state(self, B):
    dev = self.device
    dws = self.discriminator.net.workspace(2 * B)
    stage = torch.zeros(draws.BCE_STAGE_WORDS, dtype=torch.int32, device=dev)
    _, dis_shifts, gen_shifts, _ = draws.bce_stage(stage)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    return dict(
        gws=self.generator.net.workspace(B),
        dws=dws,
        stage_dev=stage,
        # D chain over [fake | real]; segment 0 is the fake batch
        dis=dws.plan(2 * B, B, None, want_norm=False, shifts=dis_shifts),
        # G chain: the same workspace's first B samples (the fake segment's
        # activations of the 2B forward), input gradient down to layer 1
        gen=dws.plan(B, B, 0, want_norm=False, shifts=gen_shifts),
        coef_d=f32(2 * B),
        coef_g=f32(B),
        delta_g=torch.zeros_like(dws.delta[-1][:B]),
        loss=f32(2),  # [gen_loss, dis_loss]
        zero=f32(1),  # (the penalty slot of cg_step_outputs)
        # the step's outputs [gen_loss, dis_loss, 0, metrics x 4], written by
        # the last launches of train(); train() hands out a COPY
        out=f32(7))

  def _bce_forward(self, st, real, z, shifts, training=True, seeds=True):
    """Steps 1-4: G(z) -> X0 = [fake | real] -> D over 2B -> cg_dense1_bce.
    shifts: the 12 ints of draws.shifts(., ., 2), on the host or staged.
    seeds=False (validate): losses only, no seeds."""
    net_g, net_d = self.generator.net, self.discriminator.net
    B = real.shape[0]
    lay, last = net_d.layers[0], net_d.layers[-1]
    dws, pd = st['dws'], st['dis']
    s = _lib.stream()
    staged = draws.bce_stage(st['stage_dev'])[0]
    if shifts.data_ptr() != staged.data_ptr():  # (else staged in place)
      staged.copy_(shifts)
    fake = st['gws'].forward(z, keep=training, training=training)
    x0 = pd.x0
    _lib.call('cg_cast_pad', fake, x0, B * lay.lin, lay.cin, net_g.Cf, lay.cinp,
              s)
    _lib.call('cg_cast_pad', real, x0[B:2 * B], B * lay.lin, lay.cin, lay.cin,
              lay.cinp, s)
    pd.forward(head=False)
    rws = nets.reduce_ws(self.device)
    if rws is None:
      st['loss'].zero_()  # (the atomics form adds onto it)
    sd = self.dis_optimizer.loss_scale if seeds else None
    sg = self.gen_optimizer.loss_scale if seeds else None
    _lib.call('cg_dense1_bce', dws.act[-1], net_d.dense_w, net_d.dense_b,
              dws.d_out, st['coef_d'] if seeds else None,
              st['coef_g'] if seeds else None, dws.delta[-1] if seeds else None,
              st['delta_g'] if seeds else None, st['loss'], sd, sg, B,
              last.lout, last.cout, last.coutp, net_d.alpha, rws, s)
    return fake

  def _bce_compute(self, real, r=None):
    """Steps 1-6: leaves both models' gradients in params.grad and the losses
    in the state's `loss`; updates nothing.  r: the source of the draws
    (draws.py; injected: dict(z=, shifts_real=, shifts_fake=))."""
    B = real.shape[0]
    st = self._get_state(B)
    net_g, net_d = self.generator.net, self.discriminator.net
    z, _, shifts = draws.draw(self._streams, self.device, r, B,
                              self.noise_shape[0], False, 2)
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
    st = self._get_state(real.shape[0])
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
    _lib.call('cg_step_outputs', loss[0:1], loss[1:2], st['zero'],
              metrics[_METRIC_KEYS[0]], 1, st['out'], _lib.stream())
    return st['out']

  def _outputs(self, o):
    """(gen_loss, dis_loss, gradient_penalty or None, metrics) as views of a
    fresh COPY of the step's output buffer: the buffer itself is rewritten by
    the next train() -- in place, when the step replays as a graph -- so callers
    may keep the returned tensors across steps without a host sync (main.py
    averages them at the end of the epoch).  Data parallel: averaged over the
    ranks, one 7-float all-reduce per step."""
    o = self._sync.mean_scalars(o.clone())
    return (o[0], o[1], o[2] if self._has_penalty else None,
            {k: o[3 + i] for i, k in enumerate(_METRIC_KEYS)})

  # -- the pieces replay.py drives ---------------------------------------------
  @property
  def _adam_steps(self):
    """Adam steps per train() of (discriminator, generator)."""
    return 1, 1

  def _segments(self, real, rand=None, staged=False):
    """The whole BCE step as one segment.  staged (graph replay): the shifts
    and the Adam step sizes are read from the state's stage buffer."""
    lr_dev = None
    if staged:
      st = self._get_state(real.shape[0])
      shifts, _, _, lr_dev = draws.bce_stage(st['stage_dev'])
      rand = draws.staged(shifts)
    return [(lambda: self._bce_step(real, rand, lr_dev), None, False)]

  def _fill_stage(self, host):
    shifts, _, _, lr = draws.bce_stage(host)
    shifts.copy_(draws.shifts(self._streams, None, 2))
    lr[0] = self.dis_optimizer.lr_t(self.dis_optimizer.host_steps + 1)
    lr[1] = self.gen_optimizer.lr_t(self.gen_optimizer.host_steps + 1)

  def batch_buffer(self, B):
    """The device buffer train() reads a batch of B samples from when it replays
    its hipGraph: (B,) + signal_shape, f32.  A data loader that gathers every
    batch INTO it (torch.index_select(..., out=buffer)) saves the copy train()
    otherwise makes in front of each replay; passing any other tensor stays
    valid.  One buffer per batch size, alive as long as this object."""
    return replay.batch_buffer(self._get_state(B), (B,) + self.signal_shape,
                               self.device)

  def train(self, inputs, rand=None):
    """One step of the algorithm (the class's module docstring; gan.py:72-85
    here).  Returns (gen_loss, dis_loss, gradient_penalty or None, metrics) as
    0-d device tensors (no host sync inside; each call returns views of its own
    small buffer, so they stay valid across later steps; under data parallelism
    they are the means over all ranks).  `rand` optionally injects the random
    draws for parity tests (here dict(z=, shifts_real=, shifts_fake=); otherwise
    z from the per-rank device stream, then one (4, 2) draw [shifts_real |
    shifts_fake] of the shared stream).  After two eager calls per batch size a
    graphable step replays as hipGraphs."""
    _lib.use(self.precision)
    real = self._to_device(inputs)
    st = self._get_state(real.shape[0])
    if (rand is None and self._use_graph and
        (self._graph_under_dp or self._sync.world == 1)):
      st['calls'] = st.get('calls', 0) + 1
      if st['calls'] > replay.GRAPH_WARMUP_CALLS:
        return self._averaged(self._outputs(replay.replay(self, st, real)))
    # an eager step between replays (injected randomness, main.py's --profile
    # window).  The captured graphs stay valid: they hold pointers to buffers
    # that live as long as this object, and nothing in them depends on what ran
    # in between.  (Round 2 dropped them here after "stale graph" penalties of
    # 1e25; the cause was a hipMemsetAsync NODE inside the captured step --
    # cg_rownorm's -- not stale memory: DESIGN.md section 8.)
    return self._averaged(self._outputs(replay.eager(self, st, real, rand)))

  def _averaged(self, outputs):
    """The end of every train(): the generator has had its one update, the
    average takes its one (after the step on the same stream, outside the
    captured graphs; under mixed precision also when the loss scaler skipped
    the Adam step, as StyleGAN does).  Hands `outputs` through."""
    if self.average is not None:
      self.average.update()
    return outputs

  def averaged_generator(self):
    """Context manager: inside, the generator computes with its averaged
    weights (validate / generate / checkpoints of --ema_decay); a null context
    when averaging is off."""
    if self.average is None:
      return contextlib.nullcontext()
    return self.average.applied(self.generator.net)

  def validate(self, inputs, rand=None):
    """gan.py:87-90 / :58-70: the same losses with training=False, no update.
    Returns (fake, gen_loss, dis_loss, None, metrics)."""
    _lib.use(self.precision)
    real = self._to_device(inputs)
    B = real.shape[0]
    st = self._get_state(B)
    z, _, shifts = draws.draw(self._streams, self.device, rand, B,
                              self.noise_shape[0], False, 2)
    # (the staged shifts of a captured step are rewritten before each replay)
    fake = self._bce_forward(st, real, z, shifts, training=False, seeds=False)
    metrics = self.metrics(real, fake, fake_pitch=self.generator.net.Cf)
    C = self.generator.net.C
    return (fake[:, :, :C].clone(),) + self._outputs(
        self._bce_outputs(st, metrics))

  def generate(self, noise, denorm=False):
    """gan.py:92-97."""
    fake = self.generator(noise, training=False)
    if denorm:
      fake = fake * (self._signals_max - self._signals_min) + self._signals_min
    return fake
