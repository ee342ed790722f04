"""Launch-by-launch checking of the critic and generator passes ("teacher
forcing"): every launch of one eager update is compared with float64 arithmetic
(tests/layer_ref.py) on the inputs that launch read, as snapshotted from device
memory in front of it.  (The generator's stages, GenChecker / GenSim / GenTracer,
follow the critic's below.)

Three parts share one statement of each stage (the stage_* functions: buffers
read -> expected buffers written, with the bar of each):

  * Checker      walks a trace (a list of events, each with the watched buffers
                 before and after one launch) and asserts values, frame, pad
                 channels and coverage;
  * CriticSim    the same schedule in numpy on the CPU, each output rounded to the
                 storage type: a simulated trace, into which
                 tests/test_layer_ref.py plants faults (and, without rounding,
                 the closure against float64 autograd);
  * Tracer       records a trace from the real launches on the GPU
                 (tests/test_hip_layers.py).

A snapshot is a dict key -> float64 numpy array (every storage type converts
exactly).  Keys of the critic: x0 (the plan's [real | fake | x^] input), act.1-5,
e.1-4, delta.1-5, d_out, gin (when it is not the x^ segment of x0), sumsq, ssq (the
unsummed slots of the ordered norm), side.i, coef, bias_coef, shifts, norm,
coef_gp, gp, loss, D.data / D.grad / D.m / D.v and D.pack.<j>.

Bars (no constants of their own): activation-typed outputs |got - round_act(want)|
<= ulp_act(round_act(want)) + err, f32 outputs |got - want| <= err, with err the f32
accumulation bound gamma(K) sum |x| |w| of the contraction carried through the
epilogue as swconv_ref.epilogue_bound does, sum_bound for the plain sums and the
bars of pointwise_ref for the scalar chain.  A group that stores an intermediate
in the activation type (e[i], side[i], the value masked after its rounding) adds
half an activation ulp per stored rounding, by its form (stage_dgrad).  In the
fp16 build a subnormal operand of a contraction counts at 2^-14 (operand_floor)."""
import numpy as np

import layer_ref as LR
import pointwise_ref as R
import swconv_ref as S
import wgrad_ref as W

NUM_CONVS = 5
# The power-of-two loss scale of the f16 case `tiny`: tests/test_layer_ref.py
# asserts that no value the float64 reference stores under it exceeds half the
# fp16 maximum (and that twice the scale would).
F16_SCALE_TINY = 2.0**14
# ... and of the fp16 generator updates (test_layer_ref.GEN_CASES), asserted there
# the same way: the gradient buffers hold normal numbers under them
F16_GEN_SCALE = {'tiny': 2.0**18, 'tiny_noln': 2.0**18, 'mid': 2.0**21, 'odd_c': 2.0**19,
                 'tiny_bn': 2.0**18, 'tiny_bn_ln': 2.0**18, 'tiny_linear': 2.0**18,
                 'tiny-no_fuse_ln': 2.0**18, 'tiny-no_defer_finish': 2.0**18,
                 'k6_c40': 2.0**18, 'k14_c102': 2.0**18, 'k22_u24': 2.0**19,
                 'l6144': 2.0**19}


class StageError(AssertionError):
  """A stage missed a check; .stage names it."""

  def __init__(self, stage, msg):
    super().__init__('{}: {}'.format(stage, msg))
    self.stage = stage


def pitch(c):
  return max(32, -(-c // 32) * 32)


def same(a, b):
  return a is b or (a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and
                    np.array_equal(np.signbit(a), np.signbit(b)))


def operand_floor(f16, exact=False):
  """The magnitude a non-zero operand of a matrix-core contraction counts with at
  least (layer_ref.nabs): fp16's smallest normal number in the fp16 build -- its
  gradients go subnormal under small loss scales; nothing for bf16, whose
  subnormals (below 2^-126) no case reaches, and in the float64 closure."""
  return 2.0**-14 if (f16 and not exact) else 0.0


class Layer(object):

  def __init__(self, cin, cout, lin):
    self.cin, self.cout, self.lin, self.lout = cin, cout, lin, lin // 2
    self.cinp, self.coutp = pitch(cin), pitch(cout)


class Ctx(object):
  """What the stages of one critic plan need to know, from the model definition
  (hparams) and the caller's choices -- not from launch descriptors.

  flags: folded / sided (sets of layers whose input-gradient launch folds the
  reflected rows in / goes through side + cg_unshuffle_fixup; every other layer
  goes through e + cg_unshuffle_mask), jvp_folds, norm_deferred, has_sumsq,
  mixes_layer1, gin_in_x0; they select the SCHEDULE (which launches exist), never
  what a stage computes."""

  def __init__(self, hp, B, f16, nseg=3, input_grad_from=None, bias_rows=None,
               slot=0, mix=None, real=None, exact=False, **flags):
    L, C = hp.signal_shape
    u = hp.num_units
    self.k = hp.kernel_size
    self.layers = []
    cin, lin = C, L
    for cout in (u, 2 * u, 3 * u, 4 * u, 5 * u):
      self.layers.append(Layer(cin, cout, lin))
      cin, lin = cout, lin // 2
    self.B, self.seg, self.nseg, self.nB = B, B, nseg, nseg * B
    self.f16 = f16
    # exact: float64 throughout (no storage type, no f32 scalars): the closure
    self.exact = exact
    self.alpha = 0.3 if exact else R.f32(0.3)
    self.floor = operand_floor(f16, exact)
    self.penalty = float(hp.gradient_penalty) if exact else R.f32(hp.gradient_penalty)
    self.igf = (2 * B if nseg == 3 else 0) if input_grad_from is None else input_grad_from
    self.bias_rows = 2 * B if bias_rows is None else bias_rows
    self.slot = slot
    self.mix = mix      # the interpolation draws (f32), for cg_lrelu_mix / interp
    self.real = real    # (B, L, C) f32 batch, for cg_interp_pack
    self.scale = None   # the loss scale S (f16 build), else None
    self.folded = set(flags.pop('folded', ()))
    self.sided = set(flags.pop('sided', ()))
    self.jvp_folds = flags.pop('jvp_folds', False)
    self.norm_deferred = flags.pop('norm_deferred', False)
    self.has_sumsq = flags.pop('has_sumsq', False)
    self.mixes = flags.pop('mixes_layer1', False)
    self.gin_in_x0 = flags.pop('gin_in_x0', False)
    self.P = flags.pop('P', 1)
    assert not flags, flags
    # flat parameter layout of the critic (every tensor padded to 4 floats)
    self.shapes = []
    for lay in self.layers:
      self.shapes += [(self.k, lay.cin, lay.cout), (lay.cout,)]
    last = self.layers[-1]
    self.shapes += [(last.lout * last.cout, 1), (1,)]
    self.offsets, off = [], 0
    for s in self.shapes:
      self.offsets.append(off)
      off += -(-int(np.prod(s)) // 4) * 4
    self.numel = off

  # -- parameters as the launches read them ---------------------------------
  def param(self, flat, i):
    o, s = self.offsets[i], self.shapes[i]
    return flat[o:o + int(np.prod(s))].reshape(s)

  def pslice(self, i):
    o = self.offsets[i]
    return slice(o, o + int(np.prod(self.shapes[i])))

  def qw(self, w):
    return w if self.exact else R.round_act(w, self.f16)

  def Wq(self, snap, l):
    """Conv weights of layer l as the packed operand holds them."""
    return self.qw(self.param(snap['D.data'], 2 * l))

  def bias(self, snap, l):
    return self.param(snap['D.data'], 2 * l + 1)

  def head(self, snap):
    last = self.layers[-1]
    wq = self.qw(self.param(snap['D.data'], 10))
    return wq.reshape(last.lout, last.cout), float(self.param(snap['D.data'], 11)[0])

  def sh(self, snap, l, lo, hi):
    """Per-sample shifts of the read in front of layer l (0-based; none for 0)."""
    if l == 0:
      return np.zeros(hi - lo, np.int64)
    row = snap['shifts'][l - 1]
    return np.asarray([int(row[b // self.seg]) for b in range(lo, hi)], np.int64)

  def src(self, l):
    return 'x0' if l == 0 else 'act.{}'.format(l)

  def gin_key(self):
    return 'x0' if self.gin_in_x0 else 'gin'

  def gin_idx(self):
    return (slice(self.igf, self.nB),) if self.gin_in_x0 else (slice(None),)


def out(key, idx, want, err=0.0, kind='act', creal=None):
  """One expected output: after[key][idx] (real channels [:creal] when given; the
  pad channels behind them must be zero) against want within err."""
  return dict(key=key, idx=idx, want=want, err=err, kind=kind, creal=creal)


# ---------------------------------------------------------------------------
# stages: snapshot before -> expected outputs
# ---------------------------------------------------------------------------
def stage_interp_pack(ctx, b, write_real):
  """x0 <- [real | fake | x^] (x^ only when the plan reads it)."""
  B, lay = ctx.B, ctx.layers[0]
  C = lay.cin
  fake = b['G.fake'][:, :, :C]
  outs = []
  if write_real:
    outs.append(out('x0', (slice(0, B),), np.asarray(ctx.real, np.float64), creal=C))
  outs.append(out('x0', (slice(B, 2 * B),), fake, creal=C))
  if not ctx.mixes:
    outs.append(out('x0', (slice(2 * B, 3 * B),), R.interp(ctx.real, fake, ctx.mix),
                    creal=C))
  return outs


def stage_fwd(ctx, b, l, lo, hi, reflect_off=0, shifts_from=None):
  lay = ctx.layers[l]
  x = b[ctx.src(l)][lo:hi, :, :lay.cin]
  sh = ctx.sh(b if shifts_from is None else shifts_from, l, lo, hi)
  want, pre, mag = LR.critic_fwd(x, ctx.Wq(b, l), ctx.bias(b, l), sh, ctx.alpha,
                                 reflect_off, ctx.floor)
  err = LR.gamma(ctx.k * lay.cinp + 1) * mag + LR.U * np.abs(want)
  return [out('act.{}'.format(l + 1), (slice(lo, hi),), want, err, creal=lay.cout)]


def stage_mix(ctx, b):
  B, lay = ctx.B, ctx.layers[0]
  a1 = b['act.1']
  n = lay.lout * lay.coutp
  ha, hb = a1[:B].reshape(B, n), a1[B:2 * B].reshape(B, n)
  pa, pb = R.lrelu_mix_parts(ha, hb, ctx.mix, ctx.alpha)
  want = R.lrelu_mix(ha, hb, ctx.mix, ctx.alpha).reshape(a1[:B].shape)
  err = (6 * R.U32 * (np.abs(pa) + np.abs(pb))).reshape(want.shape)
  return [out('act.1', (slice(2 * B, 3 * B),), want[:, :, :lay.cout],
              err[:, :, :lay.cout], creal=lay.cout)]


def stage_head(ctx, b, seeded):
  last, nB = ctx.layers[-1], ctx.nB
  h = b['act.5'][:nB, :, :last.cout]
  wq, bd = ctx.head(b)
  d, bar = LR.head_fwd(h, wq, bd)
  outs = [out('d_out', (slice(0, nB),), d, bar, kind='f32')]
  if seeded:
    outs += stage_seed(ctx, b)
  return outs


def stage_seed(ctx, b):
  last, nB = ctx.layers[-1], ctx.nB
  h = b['act.5'][:nB, :, :last.cout]
  wq, _ = ctx.head(b)
  return [out('delta.5', (slice(0, nB),),
              LR.head_seed(h, wq, b['coef'], ctx.seg, ctx.alpha), creal=last.cout)]


def stage_cast_real(ctx, b):
  """The BCE step's x0 = [fake | real]: the real batch cast into segment 1."""
  C = ctx.layers[0].cin
  return [out('x0', (slice(ctx.B, 2 * ctx.B),),
              R.round_act(np.asarray(ctx.real, np.float64), ctx.f16), kind='bits', creal=C)]


def stage_bce(ctx, b, a):
  """cg_dense1_bce over [fake | real] (pointwise_ref.bce_head): the logits within
  sum_bound; everything else from the logits the launch STORED (a: the snapshot
  after it) inside pointwise_ref.bce_bars, the seeds from the coefficients it
  stored -- as test_hip_pointwise states the head's checks."""
  B, last = ctx.B, ctx.layers[-1]
  n2 = 2 * B
  h = b['act.5'][:n2, :, :last.cout]
  wq, bd = ctx.head(b)
  d, bar = LR.head_fwd(h, wq, bd)
  S_d = b['D.ls'][0] if 'D.ls' in b else 1.0
  S_g = b['G.ls'][0] if 'G.ls' in b else 1.0
  x = a['d_out'][:n2]
  r, e = R.bce_from_logits(x, B, S_d, S_g), R.bce_bars(x, B, S_d, S_g)
  g = wq[None] * LR.mask(h, ctx.alpha)
  wd = a['coef_d'][:, None, None] * g
  wg = a['coef_g'][:, None, None] * g[:B]
  f = lambda w: 2 * R.U32 * np.abs(w) + 2 * 2.0**-149
  return [out('d_out', (slice(0, n2),), d, bar, kind='f32'),
          out('coef_d', (), r['coef_d'], e['coef_d'], kind='f32'),
          out('coef_g', (), r['coef_g'], e['coef_g'], kind='f32'),
          out('loss', (), r['loss'], e['loss'], kind='f32'),
          out('delta.5', (slice(0, n2),), wd, f(wd), creal=last.cout),
          out('delta_g', (), wg, f(wg), creal=last.cout)]


def stage_head_wgrad_samples(ctx, b):
  """The head's gradients from a per-SAMPLE seed (the BCE step's coef_d)."""
  last, nB = ctx.layers[-1], ctx.nB
  x = b['act.5'][:nB, :, :last.cout]
  dW, eW, db, eb = LR.head_wgrad(x, b['coef_d'], b['coef_d'], 1)
  return [out('D.grad', (ctx.pslice(10),), dW.reshape(-1), eW.reshape(-1), kind='f32'),
          out('D.grad', (ctx.pslice(11),), np.array([db]), np.array([eb]), kind='f32')]


def stage_dgrad(ctx, b, i):
  """The input-gradient group of layer i (1..4): final delta[i], and the
  intermediates a launch may leave (kind 'free': written, not compared)."""
  lay, nB = ctx.layers[i], ctx.nB
  dn = b['delta.{}'.format(i + 1)][:nB, :, :lay.cout]
  hi = b['act.{}'.format(i)][:nB, :, :lay.cin]
  sh = ctx.sh(b, i, 0, nB)
  want, (d, r), mag = LR.critic_dgrad(dn, ctx.Wq(b, i), lay.lin, sh, hi, ctx.alpha,
                                            ctx.floor)
  md, mr = mag
  g = LR.gamma((ctx.k // 2) * lay.coutp)
  m = LR.mask(hi, ctx.alpha)
  # one rounding of a value stored in the activation type: half an ulp, taken at
  # the far end of the f32 value's own bar
  half = lambda v, acc: 0.5 * R.ulp_act(np.abs(v) + acc, ctx.f16)
  if ctx.exact:
    stored = 0.0
  elif i in ctx.sided or i in ctx.folded:
    # the direct part is rounded, masked and (where a reflected row lands on it)
    # stored before the sum; the reflected part is stored unmasked in `side`.  The
    # folded launch leaves bit for bit what side + cg_unshuffle_fixup leave
    # (include/calciumgan_hip.h), so it rounds at the same points
    stored = m * half(d, g * md) + np.where(r != 0, half(d * m, g * md) +
                                            m * half(r, g * mr), 0.0)
  else:
    # e[i] holds both parts, each rounded once; cg_unshuffle_mask sums in f32
    stored = m * (np.where(d != 0, half(d, g * md), 0.0) +
                  np.where(r != 0, half(r, g * mr), 0.0))
  err = g * (md + mr) + stored + 2 * LR.U * np.abs(want)
  return [out('delta.{}'.format(i), (slice(0, nB),), want, err, creal=lay.cin)], (d, r)


def stage_gin(ctx, b):
  lay = ctx.layers[0]
  d1 = b['delta.1'][ctx.igf:ctx.nB, :, :lay.cout]
  want, mag = LR.critic_gin(d1, ctx.Wq(b, 0), lay.lin, ctx.floor)
  err = LR.gamma((ctx.k // 2) * lay.coutp) * mag
  outs = [out(ctx.gin_key(), ctx.gin_idx(), want, err, creal=lay.cin)]
  if ctx.has_sumsq:
    own = np.ones(lay.lin, bool)
    ss, bar = LR.sumsq(want), S.rowsumsq_bound(want, err, own)
    if ctx.norm_deferred:
      outs.append(out('ssq', (), ss, bar, kind='slots'))
    else:
      outs.append(out('sumsq', (), ss, bar, kind='f32'))
  return outs


def _g_rows(ctx, b):
  g = b[ctx.gin_key()][ctx.gin_idx()]
  return g.reshape(g.shape[0], -1)


def stage_rownorm(ctx, b):
  g = _g_rows(ctx, b)
  want = R.rownorm(g)
  sb = R.sum_bound(g * g, axis=1)
  bar = np.where(want > 0, sb / (2 * np.where(want > 0, want, 1.0)), 0.0) + \
      2 * R.ulp_f32(want)
  bar[want == 0] = 0.0
  return [out('norm', (), want, bar, kind='f32')]


def _gp_outs(ctx, b, nv, e_nv, norm_key):
  B, slot = ctx.B, ctx.slot
  _, gpr, cr = R.gp_finalize(nv, ctx.penalty, 0, 1.0)
  egp, ecoef = R.gp_bars(nv, ctx.penalty, 1.0, e_nv)
  d = b['d_out']
  return [out(norm_key, (), nv, e_nv, kind='f32'),
          out('gp', (slice(slot, slot + 1),), np.array([gpr]), np.array([egp]), kind='f32'),
          out('coef_gp', (), cr, ecoef, kind='f32'),
          out('loss', (slot,), R.critic_loss(d, gpr, ctx.penalty, B),
              R.critic_loss_bars(d, gpr, egp, ctx.penalty, B), kind='f32')]


def stage_gp_critic_loss(ctx, b):
  if ctx.has_sumsq:
    nv = np.sqrt(b['sumsq'])
    return _gp_outs(ctx, b, nv, R.ulp_f32(nv), 'sumsq')
  return _gp_outs(ctx, b, b['norm'], np.zeros(ctx.B), 'norm')


def scaled_rows_target(ctx):
  """(source key, idx, destination key, idx) of v = coef_b * g."""
  x = slice(2 * ctx.B, 3 * ctx.B)
  if ctx.jvp_folds:
    return 'delta.1', (x,), 'delta.1', (x,)
  return ctx.gin_key(), ctx.gin_idx(), 'x0', (x,)


def stage_gp_loss_scale(ctx, b, a, rows=True):
  """cg_gp_loss_scale: slots -> norm, gp, coef, loss, and the rows scaled by the
  coefficients the launch STORED (a: the snapshot after it; as
  test_hip_pointwise.test_gp_loss_scale states it)."""
  B = ctx.B
  slots = b['ssq'].reshape(B, -1)
  nv = np.sqrt(slots.sum(axis=1))
  e_nv = R.sum_bound(slots, axis=1) / (2 * nv) + R.ulp_f32(nv)
  outs = _gp_outs(ctx, b, nv, e_nv, 'sumsq')
  if not rows:
    return outs
  sk, si, dk, di = scaled_rows_target(ctx)
  g = b[sk][si]
  want = R.scale_rows(g.reshape(B, -1), a['coef_gp']).reshape(g.shape)
  outs.append(out(dk, di, want))
  return outs


def stage_scale_rows(ctx, b):
  sk, si, dk, di = scaled_rows_target(ctx)
  g = b[sk][si]
  want = R.scale_rows(g.reshape(ctx.B, -1), b['coef_gp']).reshape(g.shape)
  return [out(dk, di, want)]


def stage_jvp(ctx, b, l, scale_rows=None):
  lay, B = ctx.layers[l], ctx.B
  x = slice(2 * B, 3 * B)
  t = b[ctx.src(l)][x, :, :lay.cin]
  key = 'act.{}'.format(l + 1)
  rs = None
  if l == 0 and ctx.jvp_folds:
    rs = b['coef_gp'] if scale_rows is None else scale_rows
  want, v, lin, mag = LR.tangent(t, ctx.Wq(b, l), ctx.sh(b, l, 2 * B, 3 * B),
                                 b[key][x, :, :lay.cout], ctx.alpha, rs, ctx.floor)
  err = S.epilogue_bound(LR.gamma(ctx.k * lay.cinp) * mag, lin, want, S.EPI_MASK, rs)
  return [out(key, (x,), want, err, creal=lay.cout)]


def stage_wgrad(ctx, b, l, x_override=None):
  lay, nB = ctx.layers[l], ctx.nB
  x = b[ctx.src(l)][:nB, :, :lay.cin] if x_override is None else x_override
  d = b['delta.{}'.format(l + 1)][:nB, :, :lay.cout]
  dW, mag = LR.critic_wgrad(x, d, ctx.k, ctx.sh(b, l, 0, nB), ctx.floor)
  rows = nB * lay.lout
  joins = -(-rows // 64)
  brows = ctx.bias_rows * lay.lout
  db, bmag = LR.dbias(d, brows)
  return [out('D.grad', (ctx.pslice(2 * l),), dW.reshape(-1),
              (LR.gamma(rows + joins) * mag).reshape(-1), kind='f32'),
          out('D.grad', (ctx.pslice(2 * l + 1),), db, LR.gamma(brows + joins) * bmag,
              kind='f32')]


def stage_head_wgrad(ctx, b):
  last, nB = ctx.layers[-1], ctx.nB
  x = b['act.5'][:nB, :, :last.cout]
  dW, eW, db, eb = LR.head_wgrad(x, b['coef'], b['bias_coef'], ctx.seg)
  return [out('D.grad', (ctx.pslice(10),), dW.reshape(-1), eW.reshape(-1), kind='f32'),
          out('D.grad', (ctx.pslice(11),), np.array([db]), np.array([eb]), kind='f32')]


ADAM = dict(b1=R.f32(0.9), b2=R.f32(0.999), eps=R.f32(1e-7))


def stage_adam(ctx, b, net, lr_t, grad_scale=1.0):
  p, g, m, v = (b[net + s] for s in ('.data', '.grad', '.m', '.v'))
  lr_t = R.f32(lr_t)
  want = R.adam(p, g, m, v, lr_t, ADAM['b1'], ADAM['b2'], ADAM['eps'], grad_scale)
  bars = R.adam_bars(p, g, m, v, lr_t, ADAM['b1'], ADAM['b2'], ADAM['eps'], grad_scale)
  return [out(net + k, (), w, e, kind='f32')
          for k, w, e in zip(('.data', '.m', '.v'), want, bars)]


def stage_grad_finite(ctx, b, net):
  """cg_grad_finite: ls[3] = gradients all finite; the rest of the state stays."""
  ls = b[net + '.ls'].copy()
  ls[3] = 1.0 if np.isfinite(b[net + '.grad']).all() else 0.0
  return [out(net + '.ls', (), ls, kind='bits')]


def stage_adam_scaled(ctx, b, net, lr, grad_scale):
  """cg_adam_scaled: skipped bit for bit when ls[3] == 0; else Adam on grad *
  grad_scale / S with the step size of t = ls[2] + 1 computed on the device (bars as
  test_hip_pointwise.test_grad_finite_and_adam_scaled derives them)."""
  S_, _, t, flag = b[net + '.ls']
  if flag == 0:
    return []
  tt = t + 1.0
  b1, b2, eps = ADAM['b1'], ADAM['b2'], ADAM['eps']
  lr_t = R.adam_lr_t(R.f32(lr), b1, b2, tt)
  U = R.U32
  rel = 4 * U * b2**tt / (1 - b2**tt) / 2 + 4 * U * b1**tt / (1 - b1**tt) + 5 * U
  p, g, m, v = (b[net + k] for k in ('.data', '.grad', '.m', '.v'))
  gs = R.f32(grad_scale) / S_
  want = R.adam(p, g, m, v, lr_t, b1, b2, eps, gs)
  bars = R.adam_bars(p, g, m, v, lr_t, b1, b2, eps, gs, lr_t_rel=rel, g_roundings=2)
  return [out(net + k, (), w, e, kind='f32')
          for k, w, e in zip(('.data', '.m', '.v'), want, bars)]


def stage_ls_update(ctx, b, net, interval):
  return [out(net + '.ls', (), R.loss_scale_update(b[net + '.ls'], interval).astype(
      np.float64), kind='bits')]


def stage_pack(ctx, b, net, descs):
  """Every packed operand equals wgrad_ref.pack of the weights in front of the
  launch.  descs: [(key, offset of the tensor in the flat buffer, [PackDesc])]."""
  outs = []
  for key, off, pds in descs:
    want = np.concatenate([W.pack(b[net + '.data'][off:], d, ctx.f16) for d in pds])
    outs.append(out(key, (), want, kind='bits'))
  return outs


# ---------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------
class Checker(object):
  """Claims the events of a trace one by one.  ratios[stage] is the worst
  error / bound met (recorded, not asserted beyond <= 1)."""

  def __init__(self, ctx):
    self.ctx = ctx
    self.ratios = {}
    self.group = None   # (layer, snapshot in front of the group's first launch)
    self.claimed = 0
    self.collect = False  # True: go on after a failed stage, report all of them

  # -- comparison -------------------------------------------------------------
  def _ratio(self, stage, diff, bar):
    with np.errstate(invalid='ignore', divide='ignore'):
      r = np.where(bar > 0, diff / np.where(bar > 0, bar, 1.0),
                   np.where(diff > 0, np.inf, 0.0))
    worst = float(np.max(r)) if r.size else 0.0
    self.ratios[stage] = max(self.ratios.get(stage, 0.0), worst)
    return r

  def _compare(self, stage, o, got_full):
    ctx = self.ctx
    got = got_full[o['idx']] if o['idx'] != () else got_full
    want = np.asarray(o['want'], np.float64)
    if o['kind'] == 'slots':
      got = got.reshape(want.shape[0], -1).sum(axis=1)
    if o['creal'] is not None:
      pad = got[..., o['creal']:]
      if pad.size and not (pad == 0).all():
        raise StageError(stage, 'pad channels of {} are not zero at {}'.format(
            o['key'], np.argwhere(pad != 0)[:3].tolist()))
      got = got[..., :o['creal']]
    want = want.reshape(got.shape)
    err = np.broadcast_to(np.asarray(o['err'], np.float64), got.shape)
    if o['kind'] == 'bits':
      if not same(got, want):
        raise StageError(stage, '{} differs bit for bit at {}'.format(
            o['key'], np.argwhere(got != want)[:3].tolist()))
      return
    if o['kind'] == 'act':
      r = R.round_act(want, ctx.f16).reshape(got.shape)
      fin = np.isfinite(r)
      if not np.array_equal(got[~fin], r[~fin], equal_nan=True):
        raise StageError(stage, 'non-finite values of {} differ'.format(o['key']))
      bar = R.ulp_act(r, ctx.f16) + err
      diff = np.abs(np.where(fin, got - np.where(fin, r, 0.0), 0.0))
    else:
      bar = err
      diff = np.abs(got - want)
    ratio = self._ratio(stage, diff, bar)
    bad = np.argwhere(~(diff <= bar))
    if bad.size:
      i = tuple(bad[0])
      raise StageError(stage, '{}{}: {} elements off, first at {}: got {!r} want {!r} '
                       'bar {!r} (worst error / bound {:.3g})'.format(
                           o['key'], o['idx'], len(bad), i, float(got[i]),
                           float(want[i]), float(bar[i]), float(np.max(ratio))))

  def _frame(self, stage, before, after, outs, free=()):
    """Everything the stage is not declared to write is bit-identical."""
    for key in before:
      if key in free:
        continue
      a, b = after[key], before[key]
      written = [o for o in outs if o['key'] == key]
      if not written:
        if not same(a, b):
          raise StageError(stage, 'wrote {} (not declared) at {}'.format(
              key, np.argwhere((a != b) & ~(np.isnan(a) & np.isnan(b)))[:3].tolist()))
        continue
      keep = np.ones(a.shape, bool)
      for o in written:
        if o['idx'] == ():
          keep[...] = False
        else:
          keep[o['idx']] = False
      if not same(np.where(keep, a, 0.0), np.where(keep, b, 0.0)):
        raise StageError(stage, 'wrote {} outside its rows at {}'.format(
            key, np.argwhere(keep & (a != b))[:3].tolist()))

  def check(self, stage, ev, outs, free=(), before=None):
    before = ev['before'] if before is None else before
    for o in outs:
      if o['kind'] != 'free':
        self._compare(stage, o, ev['after'][o['key']])
    self._frame(stage, before, ev['after'], outs, free)

  # -- dispatch -----------------------------------------------------------------
  def gap(self, prev_after, before, role=()):
    """Between two launches only the declared host-side operations change a
    buffer: coef_gp *= S under the loss scale (wgan_gp._critic_forward); the
    staging of the injected shifts and the loss scale on the seeds, in front of
    the launch that fills the plan's input (role: the launch that follows)."""
    for key in before:
      if same(prev_after[key], before[key]):
        continue
      if key in ('shifts', 'coef', 'bias_coef') and role and \
          role[0] in ('cast_fake', 'interp_pack'):
        continue
      S_ = self.ctx.scale
      if key == 'coef_gp' and S_ is not None:
        want = (prev_after[key].astype(np.float32) * np.float32(S_)).astype(np.float64)
        if same(want, before[key]):
          continue
      if key == 'delta.5' and 'delta_g' in before:
        # the BCE step's G chain starts from its own seeds: delta[5][:B] = delta_g
        want = prev_after[key].copy()
        want[:before['delta_g'].shape[0]] = before['delta_g']
        if same(want, before[key]):
          continue
      if key == 'G.dz' and same(before[key], before['gin']):
        continue  # linear output: dz = dfake, a copy (GeneratorNet._backward)
      raise StageError('between launches', '{} changed'.format(key))

  def run(self, events):
    prev = None
    errors = []
    for ev in events:
      try:
        if prev is not None:
          self.gap(prev['after'], ev['before'], ev['role'])
        self.claim(ev)
      except StageError as e:
        if not self.collect:
          raise
        errors.append(e)
      self.claimed += 1
      prev = ev
    if errors:
      raise StageError(errors[0].stage, ' || '.join(str(e) for e in errors))
    if self.group is not None:
      raise StageError('dgrad {}'.format(self.group[0]), 'group left open')
    return self.ratios

  def claim(self, ev):
    ctx, role, b = self.ctx, ev['role'], ev['before']
    name = ' '.join(str(r) for r in role)
    if self.group is not None and role[0] not in ('fixup', 'unshuffle_mask'):
      raise StageError(name, 'launch inside the open group of layer {}'.format(
          self.group[0]))
    kind = role[0]
    if kind == 'interp_pack':
      self.check(name, ev, stage_interp_pack(ctx, b, role[1]))
    elif kind == 'fwd':
      self.check(name, ev, stage_fwd(ctx, b, role[1], 0, ctx.nB))
    elif kind == 'fwd_pair':
      self.check(name, ev, stage_fwd(ctx, b, 0, 0, 2 * ctx.B))
    elif kind == 'mix':
      self.check(name, ev, stage_mix(ctx, b))
    elif kind == 'head':
      self.check(name, ev, stage_head(ctx, b, role[1]))
    elif kind == 'dgrad':
      i = role[1]
      outs, _ = stage_dgrad(ctx, b, i)
      if i in ctx.folded:
        self.check(name, ev, outs)
        return
      free = ('delta.{}'.format(i), 'side.{}'.format(i)) if i in ctx.sided else \
          ('e.{}'.format(i),)
      self._frame(name, b, ev['after'], [], free)
      self.group = (i, b, outs, free)
    elif kind in ('fixup', 'unshuffle_mask'):
      if self.group is None or self.group[0] != role[1] or \
          (kind == 'fixup') != (role[1] in ctx.sided):
        raise StageError(name, 'no input-gradient launch of this form in front')
      i, gb, outs, free = self.group
      self.group = None
      stage = 'dgrad {}'.format(i)
      # the finishing launch writes delta[i] only; the group as a whole is held
      # against the snapshot in front of its first launch
      self._frame(stage, b, ev['after'], outs)
      self.check(stage, ev, outs, free, before=gb)
    elif kind == 'gin':
      self.check(name, ev, stage_gin(ctx, b))
    elif kind == 'rownorm':
      self.check(name, ev, stage_rownorm(ctx, b))
    elif kind == 'gp_critic_loss':
      self.check(name, ev, stage_gp_critic_loss(ctx, b))
    elif kind == 'gp_loss_scale':
      self.check(name, ev, stage_gp_loss_scale(ctx, b, ev['after'], ev.get('rows', True)))
    elif kind == 'scale_rows':
      self.check(name, ev, stage_scale_rows(ctx, b))
    elif kind == 'jvp':
      self.check(name, ev, stage_jvp(ctx, b, role[1]))
    elif kind == 'wgrads':
      outs = []
      for l in role[1]:  # one stage name per layer, so a fault is named by its layer
        mine = stage_wgrad(ctx, b, l)
        for o in mine:
          self._compare('wgrad {}'.format(l), o, ev['after'][o['key']])
        outs += mine
      self._frame(name, b, ev['after'], outs)
    elif kind == 'cast_real':
      self.check(name, ev, stage_cast_real(ctx, b))
    elif kind == 'bce':
      self.check(name, ev, stage_bce(ctx, b, ev['after']))
    elif kind == 'head_wgrad_samples':
      self.check(name, ev, stage_head_wgrad_samples(ctx, b))
    elif kind == 'head_wgrad':
      self.check(name, ev, stage_head_wgrad(ctx, b))
    elif kind == 'adam':
      self.check(name, ev, stage_adam(ctx, b, role[1], ev['lr_t'], ev.get('grad_scale', 1.0)))
    elif kind == 'grad_finite':
      self.check(name, ev, stage_grad_finite(ctx, b, role[1]))
    elif kind == 'adam_scaled':
      self.check(name, ev, stage_adam_scaled(ctx, b, role[1], ev['lr'], ev['grad_scale']))
    elif kind == 'ls_update':
      self.check(name, ev, stage_ls_update(ctx, b, role[1], ev['interval']))
    elif kind == 'pack':
      self.check(name, ev, stage_pack(ctx, b, role[1], ev['descs']))
    else:
      raise StageError(name, 'unclaimed launch')


# ---------------------------------------------------------------------------
# the schedule on the CPU
# ---------------------------------------------------------------------------
class CriticSim(object):
  """The critic update of wgan_gp._critic_compute as a chain of the stage
  statements, each output stored through q (round_act: the simulated trace;
  None: float64 throughout, for the closure test).  fault: a dict naming ONE
  planted fault (tests/test_layer_ref.py)."""

  def __init__(self, ctx, dis_weights, real, fake, alpha, shifts, fault=None,
               coef=None, bias_coef=None):
    self.ctx = ctx
    self.rounded = rounded = not ctx.exact
    self.fault = fault or {}
    self.events = []
    c, B, nB = ctx, ctx.B, ctx.nB
    L0 = c.layers[0]
    z = lambda *s: np.zeros(s)
    st = self.st = {}
    st['x0'] = z(nB, L0.lin, L0.cinp)
    for l, lay in enumerate(c.layers):
      st['act.{}'.format(l + 1)] = z(nB, lay.lout, lay.coutp)
      st['delta.{}'.format(l + 1)] = z(nB, lay.lout, lay.coutp)
      if l < 4:
        st['e.{}'.format(l + 1)] = z(nB, lay.lout, lay.coutp)
    for i in c.sided:
      st['side.{}'.format(i)] = z(nB, max(1, 2), c.layers[i].cinp)
    st['d_out'] = z(nB)
    if not c.gin_in_x0:
      st['gin'] = z(nB - c.igf, L0.lin, L0.cinp)
    if c.has_sumsq:
      st['sumsq'] = z(B)
      if c.norm_deferred:
        st['ssq'] = z(B * c.P)
    # (under a loss scale the real and fake seeds carry it, the x^ seed stays 1)
    f = np.array([c.scale, c.scale, 1.0]) if c.scale is not None else 1.0
    if c.nseg == 1:  # the generator update's pass over the fake batch
      coef, bias_coef, f = coef or [-1.0 / B], bias_coef or [0.0], (c.scale or 1.0)
    st['coef'] = self.q32(np.array(coef or [-1.0 / B, 1.0 / B, 1.0])) * f
    st['bias_coef'] = self.q32(np.array(bias_coef or [-1.0 / B, 1.0 / B, 0.0])) * f
    st['shifts'] = np.asarray(shifts, np.float64).reshape(4, c.nseg)
    st['norm'], st['coef_gp'] = z(B), z(B)
    st['gp'], st['loss'] = z(1), z(1, 2)
    flat = z(c.numel)
    for i, w in enumerate(dis_weights):
      flat[c.pslice(i)] = np.asarray(w, np.float64).reshape(-1)
    st['D.data'], st['D.grad'] = flat, z(c.numel)
    st['G.fake'] = np.zeros((B, L0.lin, L0.cin))
    st['G.fake'][...] = np.asarray(fake, np.float64)
    c.real, c.mix = np.asarray(real, np.float64), np.asarray(alpha, np.float64)

  def q32(self, v):
    return v.astype(np.float32).astype(np.float64) if self.rounded else v

  def store(self, o):
    """Write one expected output as a launch would: rounded to its type, pad
    channels zero."""
    if o['kind'] == 'free':
      return
    buf = self.st[o['key']]
    want = np.asarray(o['want'], np.float64)
    if o['kind'] == 'act' and self.rounded:
      want = R.round_act(want, self.ctx.f16)
    elif o['kind'] in ('f32', 'slots') and self.rounded:
      want = self.q32(want)
    if o['kind'] == 'slots':
      v = np.zeros((want.shape[0], self.ctx.P))
      v[:, 0] = want
      buf[...] = v.reshape(buf.shape)
      return
    view = buf[o['idx']] if o['idx'] != () else buf
    if o['creal'] is not None:
      view[..., o['creal']:] = 0.0
      view[..., :o['creal']] = want.reshape(view[..., :o['creal']].shape)
    else:
      view[...] = want.reshape(view.shape)

  def emit(self, role, outs, extra=None, **info):
    before = {k: v.copy() for k, v in self.st.items()}
    for o in outs:
      self.store(o)
    if extra is not None:
      extra(self.st)
    ev = dict(role=role, before=before,
              after={k: v.copy() for k, v in self.st.items()})
    ev.update(info)
    self.events.append(ev)

  def run(self):
    c, st, f = self.ctx, self.st, self.fault
    B, nB = c.B, c.nB
    self.emit(('interp_pack', True), stage_interp_pack(c, st, True))
    self.forward()
    self.chain()
    self.penalty_and_grads()
    return self.events

  def forward(self):
    c, st, f = self.ctx, self.st, self.fault
    B, nB = c.B, c.nB
    for l in range(NUM_CONVS):
      kw = {}
      if f.get('reflect_off') == l:
        kw['reflect_off'] = 1
      if f.get('wrong_shift_row') == l:
        # segment 1 reads segment 0's row of the shift table
        bad = dict(st)
        bad['shifts'] = st['shifts'].copy()
        bad['shifts'][l - 1][1] = st['shifts'][l - 1][0]
        kw['shifts_from'] = bad
      extra = None
      if f.get('pad_nonzero') == l:
        lay = c.layers[l]
        extra = lambda s, l=l, lay=lay: s['act.{}'.format(l + 1)].__setitem__(
            (1, 0, lay.cout), 2.0**-6)
      if l == 0 and c.mixes:
        self.emit(('fwd_pair',), stage_fwd(c, st, 0, 0, 2 * B, **kw), extra)
        self.emit(('mix',), stage_mix(c, st))
      else:
        self.emit(('fwd', l), stage_fwd(c, st, l, 0, nB, **kw), extra)
    self.emit(('head', True), stage_head(c, st, True))

  def chain(self):
    c, st, f = self.ctx, self.st, self.fault
    B, nB = c.B, c.nB
    for i in range(NUM_CONVS - 1, 0, -1):
      outs, (d, r) = stage_dgrad(c, st, i)
      if i in c.folded:
        self.emit(('dgrad', i), outs)
        continue
      lay = c.layers[i]
      if i in c.sided:
        def first(s, i=i, lay=lay, d=d, r=r):
          m = LR.mask(s['act.{}'.format(i)][:nB, :, :lay.cin], c.alpha)
          s['delta.{}'.format(i)][:nB, :, :lay.cin] = self.qa(self.qa(d) * m)
          s['side.{}'.format(i)][:nB, 0, :lay.cin] = self.qa(r[:, 0])
        self.emit(('dgrad', i), [], first)
        self.emit(('fixup', i), outs)
      else:
        def first(s, i=i, lay=lay, d=d, r=r):
          s['e.{}'.format(i)][:nB, :, :lay.cin] = self.qa(d + r)
        self.emit(('dgrad', i), [], first)
        self.emit(('unshuffle_mask', i), outs)
    self.emit(('gin',), stage_gin(c, st))

  def penalty_and_grads(self):
    c, st, f = self.ctx, self.st, self.fault
    B, nB = c.B, c.nB
    if c.norm_deferred:
      self._gp_loss_scale()
    else:
      if not c.has_sumsq:
        self.emit(('rownorm',), stage_rownorm(c, st))
      self.emit(('gp_critic_loss',), stage_gp_critic_loss(c, st))
      if c.scale is not None:  # d(S lambda gp) / dg: a host-side product
        st['coef_gp'] = self.q32(st['coef_gp'] * np.float32(c.scale))
      self.emit(('scale_rows',), stage_scale_rows(c, st))
    # ---- tangent chain
    for l in range(NUM_CONVS):
      kw, extra = {}, None
      if l == 0 and f.get('coef_missing') is not None and c.jvp_folds:
        rs = st['coef_gp'].copy()
        rs[f['coef_missing']] = 1.0
        kw['scale_rows'] = rs
      if f.get('overwrite_other_segment') == l:
        key = 'act.{}'.format(l + 1)
        extra = lambda s, key=key: s[key].__setitem__(
            (B, 0), s[key][B, 0] + np.where(np.arange(s[key].shape[2]) == 0, 2.0**-4, 0))
      self.emit(('jvp', l), stage_jvp(c, st, l, **kw), extra)
    # ---- weight gradients
    outs = []
    for l in range(NUM_CONVS):
      cc, kw = c, {}
      if f.get('bias_rows_3B') and l == f['bias_rows_3B'] - 1:
        cc = _with(c, bias_rows=3 * B)
      if l == 0 and f.get('xhat_in_wgrad'):
        # the x^ rows of the layer-1 operand still hold x^, not v
        x = st['x0'][:nB, :, :c.layers[0].cin].copy()
        x[2 * B:] = R.round_act(R.interp(c.real, st['G.fake'], c.mix), c.f16)
        kw['x_override'] = x
      outs += stage_wgrad(cc, st, l, **kw)
    self.emit(('wgrads', tuple(range(NUM_CONVS))), outs)
    self.emit(('head_wgrad',), stage_head_wgrad(c, st))

  def qa(self, v):
    return R.round_act(v, self.ctx.f16) if self.rounded else v

  def _gp_loss_scale(self):
    c, st = self.ctx, self.st
    # the launch scales the rows by the coefficients it stores: two passes here
    outs = stage_gp_loss_scale(c, st, dict(coef_gp=np.zeros(c.B)))[:-1]
    tmp = {k: v for k, v in st.items()}
    coef = [o for o in outs if o['key'] == 'coef_gp'][0]['want']
    outs = stage_gp_loss_scale(c, tmp, dict(coef_gp=self.q32(coef)))
    if self.fault.get('coef_missing') is not None and not c.jvp_folds:
      o = outs[-1]
      w = np.array(o['want'])
      sk, si, _, _ = scaled_rows_target(c)
      w[self.fault['coef_missing']] = st[sk][si][self.fault['coef_missing']]
      o['want'] = w
    self.emit(('gp_loss_scale',), outs)


def _with(ctx, **kw):
  import copy
  c = copy.copy(ctx)
  for k, v in kw.items():
    setattr(c, k, v)
  return c


def critic_grads(sim):
  """The critic gradients of a finished CriticSim, in get_weights() order."""
  c = sim.ctx
  return [c.param(sim.st['D.grad'], i).copy() for i in range(len(c.shapes))]


# ---------------------------------------------------------------------------
# the tracer (GPU)
# ---------------------------------------------------------------------------
def plan_flags(plan):
  """The schedule's form, as the plan chose it (which launches exist)."""
  return dict(folded=set(plan.folded), sided=set(plan.side),
              jvp_folds=bool(getattr(plan, 'jvp_folds', False)),
              norm_deferred=bool(plan.norm_deferred),
              has_sumsq=getattr(plan, 'sumsq', None) is not None,
              mixes_layer1=bool(plan.mixes_layer1),
              gin_in_x0=bool(plan.gin_in_x0),
              P=plan.ssq[1] if plan.ssq is not None else 1)


def pack_descs(net):
  """[(key, offset of the source tensor in the flat parameters, [PackDesc])] of
  every packed operand of a net, in the order of its pack plan."""
  base = net.params.data.data_ptr()
  res = []
  for j, op in enumerate(net._pack_plan._keep):
    pds = [W.PackDesc(d.taps, d.C_real, d.N_real, d.Cx, d.CK, d.tap0, d.tap_step,
                      d.s_tap, d.s_c, d.s_n, d.parity_major, d.narrow_last)
           for d in op.descs]
    res.append(('pack.{}'.format(j), (op.src.data_ptr() - base) // 4, pds))
  return res


class Tracer(object):
  """Records one event per launch of an eager pass: nets._run_conv, _run_wgrad,
  _run_wgrads and _lib.call are wrapped; around each launch the device is
  synchronised and every watched tensor copied to the host.  Convolution and
  weight-gradient launches are identified by id() of their descriptor, _lib.call
  launches by name and pointer arguments."""

  def __init__(self, gan, B, plan=None):
    from calciumgan_amd import nets
    self.nets = nets
    st = gan._get_state(B)
    dws, dnet = st['dws'], gan.discriminator.net
    self.plan = plan = st['critic'] if plan is None else plan
    self.coef_ptrs = {plan.coef.data_ptr()}
    self.dws = dws
    w = self.watch = {}
    w['x0'] = plan.x0
    for l in range(1, NUM_CONVS + 1):
      w['act.{}'.format(l)] = dws.act[l]
      w['delta.{}'.format(l)] = dws.delta[l]
      if l < NUM_CONVS:
        w['e.{}'.format(l)] = dws.e[l]
    w['d_out'] = dws.d_out
    if plan.gin is not None and not plan.gin_in_x0:
      w['gin'] = plan.gin
    if plan.sumsq is not None:
      w['sumsq'] = plan.sumsq
    if plan.norm_deferred:
      w['ssq'] = plan.ssq[0]
    for i, t in plan.side.items():
      w['side.{}'.format(i)] = t
    w['coef'], w['bias_coef'], w['shifts'] = plan.coef, plan.bias_coef, plan.shifts
    for k in ('norm', 'coef_gp', 'gp', 'loss'):
      w[k] = st[k]
    for k in ('data', 'grad', 'm', 'v'):
      w['D.' + k] = getattr(dnet.params, k)
    self.packs = pack_descs(dnet)
    self.pack_plans = [('D', dnet._pack_plan, self.packs)]
    for (key, _, _), op in zip(self.packs, dnet._pack_plan._keep):
      w['D.' + key] = op.buf
    w['G.fake'] = st['gws'].fake
    # the step's other input buffers, its outputs and the loss-scale states: only
    # the frame assertion reads them
    for k in sorted(dws._x0_alt):
      if dws._x0_alt[k] is not plan.x0:
        w['x0.{}'.format(k)] = dws._x0_alt[k]
    if plan.x0 is not dws.act[0]:
      w['x0.0'] = dws.act[0]
    w['out'] = st['out']
    for net, opt in (('D', gan.dis_optimizer), ('G', gan.gen_optimizer)):
      if opt.loss_scale is not None:
        w[net + '.ls'] = opt.loss_scale_state
    self.roles = {}
    for l, d in enumerate(plan.fwd):
      self.roles[id(d)] = ('fwd', l)
    if plan.fwd_l1_pair is not None:
      self.roles[id(plan.fwd_l1_pair)] = ('fwd_pair',)
    for i, d in plan.dgrad:
      self.roles[id(d)] = ('dgrad', i)
    if plan.input_grad is not None:
      self.roles[id(plan.input_grad)] = ('gin',)
    for l, d in enumerate(plan.jvp):
      self.roles[id(d)] = ('jvp', l)
    self.wgrad_of = {id(d): l for l, d in enumerate(plan.wgrad)}
    self.delta_of = {dws.delta[i].data_ptr(): i for i in range(1, NUM_CONVS + 1)}
    self.events = []
    self.depth = 0
    self.last = None

  def snap(self):
    import torch
    torch.cuda.synchronize()
    new = {k: t.detach().cpu().double().numpy() for k, t in self.watch.items()}
    # an unchanged buffer keeps ONE host copy over the whole trace
    last = self.last
    if last is not None:
      for k, v in new.items():
        if same(v, last[k]):
          new[k] = last[k]
    self.last = new
    return new

  def _ptr(self, a):
    return a.data_ptr() if hasattr(a, 'data_ptr') else getattr(a, 'value', None)

  def identify(self, kind, args):
    if kind == 'conv':
      return self.roles.get(id(args[0]), ('conv', 'unknown descriptor')), {}
    if kind == 'wgrad':
      l = self.wgrad_of.get(id(args[0]))
      return (('wgrads', (l,)) if l is not None else ('wgrad', 'unknown')), {}
    if kind == 'wgrads':
      ls = tuple(self.wgrad_of.get(id(d)) for d in args[0])
      return (('wgrads', ls) if None not in ls else ('wgrads', 'unknown')), {}
    name, a = args[0], args[1:]
    if name == 'cg_interp_pack':
      return ('interp_pack', bool(a[10])), {}
    if name in ('cg_unshuffle_fixup', 'cg_unshuffle_mask'):
      i = self.delta_of.get(self._ptr(a[2]))
      return (name[len('cg_unshuffle_'):] if name.endswith('fixup') else
              'unshuffle_mask', i), {}
    if name == 'cg_dense1_wgrad':
      if self._ptr(a[1]) not in self.coef_ptrs:
        return ('call', name + ' with per-sample seeds'), {}  # (no stage claims it yet)
      return ('head_wgrad',), {}
    def net_of(t, suffix):
      for net in ('D', 'G'):
        w = self.watch.get(net + suffix)
        if w is not None and self._ptr(t) == w.data_ptr():
          return net
      return None
    if name == 'cg_adam' and a[10] is None:  # (a device step size: graph replay)
      return ('adam', net_of(a[0], '.data')), dict(lr_t=a[5], grad_scale=a[9])
    if name == 'cg_grad_finite':
      return ('grad_finite', net_of(a[0], '.grad')), {}
    if name == 'cg_adam_scaled':
      return ('adam_scaled', net_of(a[0], '.data')), dict(lr=a[5], grad_scale=a[9])
    if name == 'cg_loss_scale_update':
      return ('ls_update', net_of(a[0], '.ls')), dict(interval=a[1])
    if name == 'cg_pack_batched':
      for net, plan, packs in self.pack_plans:
        if self._ptr(a[0]) == plan.dev.data_ptr():
          return ('pack', net), dict(descs=[(net + '.' + k, o, p) for k, o, p in packs])
    if name == 'cg_gp_loss_scale':
      return ('gp_loss_scale',), dict(rows=a[10] is not None)
    if name == 'cg_signal_metrics':
      return ('metrics',), dict(
          _after=lambda: dict(metrics=a[2].detach().cpu().double().numpy()))
    simple = {'cg_lrelu_mix': ('mix',), 'cg_dense1_fwd_bwd': ('head', True),
              'cg_rownorm': ('rownorm',), 'cg_gp_critic_loss': ('gp_critic_loss',),
              'cg_scale_rows': ('scale_rows',)}
    return simple.get(name, ('call', name)), {}

  def _wrap(self, kind, orig):
    def run(*args):
      if self.depth:
        return orig(*args)
      role, info = self.identify(kind, args)
      before = self.snap()
      self.depth += 1
      try:
        res = orig(*args)
      finally:
        self.depth -= 1
      ev = dict(role=role, before=before, after=self.snap())
      post = info.pop('_after', None)
      ev.update(info)
      if post is not None:
        ev.update(post())
      self.events.append(ev)
      return res
    return run

  def install(self, monkeypatch):
    from calciumgan_amd import _lib
    nets = self.nets
    monkeypatch.setattr(nets, '_run_conv', self._wrap('conv', nets._run_conv))
    monkeypatch.setattr(nets, '_run_wgrad', self._wrap('wgrad', nets._run_wgrad))
    monkeypatch.setattr(nets, '_run_wgrads', self._wrap('wgrads', nets._run_wgrads))
    monkeypatch.setattr(_lib, 'call', self._wrap('call', _lib.call))


# ===========================================================================
# generator update (wgan_gp._gen_compute)
# ===========================================================================
import dense_ref as D
import norm_ref as NR


class GenCtx(object):
  """The generator's side of one generator update, from the model definition;
  ln_fused / defer / streaming_out / streaming_out_dgrad / Cf select the schedule
  and the output pitch (read from the workspace on the GPU)."""

  def __init__(self, hp, B, f16, z=None, exact=False, ln_fused=None, defer=False,
               streaming_out=True, streaming_out_dgrad=False, Cf=None):
    L, C = hp.signal_shape
    u, self.nd, self.k = hp.num_units, hp.noise_dim, hp.kernel_size
    self.w0 = L // 2**NUM_CONVS
    self.B, self.L, self.C, self.Cp, self.f16, self.exact = B, L, C, pitch(C), f16, exact
    self.Cf = self.Cp if Cf is None else Cf
    self.z = z
    self.alpha = 0.3 if exact else R.f32(0.3)
    self.floor = operand_floor(f16, exact)
    self.ln_eps = LR.LN_EPS if exact else R.f32(LR.LN_EPS)
    self.bn_eps = LR.BN_EPS if exact else R.f32(LR.BN_EPS)
    self.momentum = LR.BN_MOMENTUM if exact else R.f32(LR.BN_MOMENTUM)
    self.ln, self.bn = bool(hp.layer_norm), bool(getattr(hp, 'batch_norm', False))
    self.normalize = bool(hp.normalize)
    self.normed = self.ln or self.bn
    self.layers = []
    cin, lin = self.nd, self.w0
    for cout in (5 * u, 4 * u, 3 * u, 2 * u, C):
      lay = Layer(cin, cout, lin)
      lay.lout = 2 * lin
      self.layers.append(lay)
      cin, lin = cout, 2 * lin
    self.ln_fused = list(ln_fused) if ln_fused is not None else [False] * NUM_CONVS
    self.defer = defer
    self.streaming_out, self.streaming_out_dgrad = streaming_out, streaming_out_dgrad
    # keep: the forward keeps what backward() reads; training: BatchNormalization
    # takes batch statistics (False: the moving ones -- validate)
    self.keep, self.training = True, True
    self.smin, self.smax = float(hp.signals_min), float(hp.signals_max)
    nflat = self.w0 * self.nd
    self.shapes = [(self.nd, nflat), (nflat,)]
    self.idx_conv, self.idx_bn, self.idx_ln = [], [], []
    for lay in self.layers:
      self.idx_conv.append(len(self.shapes))
      self.shapes += [(self.k, 1, lay.cout, lay.cin), (lay.cout,)]
      self.idx_bn.append(len(self.shapes) if self.bn else None)
      if self.bn:
        self.shapes += [(lay.cout,)] * 4
      self.idx_ln.append(len(self.shapes) if self.ln else None)
      if self.ln:
        self.shapes += [(lay.cout,)] * 2
    self.idx_out = len(self.shapes)
    self.shapes += [(C, C), (C,)]
    self.offsets, off = [], 0
    for s in self.shapes:
      self.offsets.append(off)
      off += -(-int(np.prod(s)) // 4) * 4
    self.numel = off

  param = Ctx.param
  pslice = Ctx.pslice
  qw = Ctx.qw

  def V(self, snap, i):
    return self.param(snap['G.data'], i)

  def index_of(self, offset):
    return self.offsets.index(offset)


def _f32out(key, idx, want, err):
  return out(key, idx, want, err, kind='f32')


def g_cast_z(g, b):
  z = np.asarray(g.z, np.float64).reshape(g.B, 1, g.nd)
  return [out('G.z', (), z if g.exact else R.round_act(z, g.f16), kind='bits')]


def g_in(g, b):
  z = b['G.z'].reshape(g.B, g.nd)
  want, mag = LR.gen_in(z, g.qw(g.V(b, 0)), g.V(b, 1), g.alpha, g.floor)
  err = LR.gamma(g.nd + 1) * mag + LR.U * np.abs(want)
  shp = (g.B, g.w0, g.nd)
  return [out('G.h.0', (), want.reshape(shp), err.reshape(shp))]


def g_conv(g, b, i, keep=True):
  lay, ic = g.layers[i], g.idx_conv[i]
  h = b['G.h.{}'.format(i)][:, :, :lay.cin]
  y, mag = LR.gen_convt(h, g.qw(g.V(b, ic)), g.V(b, ic + 1), g.floor)
  acc = LR.gamma((g.k // 2) * lay.cinp + 1) * mag
  hk = 'G.h.{}'.format(i + 1)
  if not g.normed:
    want = LR.lrelu(y, g.alpha)
    return [out(hk, (), want, acc + LR.U * np.abs(want), creal=lay.cout)]
  if not g.ln_fused[i]:
    return [out('G.ypre.{}'.format(i + 1), (), y, acc, creal=lay.cout)]
  il = g.idx_ln[i]
  gam, bet = g.V(b, il), g.V(b, il + 1)
  if g.exact:
    hh, mean, rstd = LR.ln_lrelu(y, gam, bet, g.alpha)
    e_h = e_m = e_r = 0.0
  else:
    _, hh, mean, rstd = S.layernorm(y, gam, bet, g.ln_eps, g.alpha, g.f16)
    e_h, e_m, e_r = S.layernorm_bounds(y, acc, gam, bet, g.ln_eps, g.alpha, g.f16)
  outs = [out(hk, (), hh, e_h, creal=lay.cout)]
  if keep:
    outs += [out('G.ypre.{}'.format(i + 1), (), y, acc, creal=lay.cout),
             _f32out('G.mean.{}'.format(i + 1), (), mean.reshape(-1), np.reshape(e_m, -1)),
             _f32out('G.rstd.{}'.format(i + 1), (), rstd.reshape(-1), np.reshape(e_r, -1))]
  return outs


def _rows(a, c):
  return a[:, :, :c].reshape(-1, c)


def g_ln_fwd(g, b, i):
  lay, il = g.layers[i], g.idx_ln[i]
  src = 'G.ybn.{}' if g.bn else 'G.ypre.{}'
  y = _rows(b[src.format(i + 1)], lay.cout)
  if g.exact:  # (norm_ref's statement takes values of the activation type)
    h, mean, rstd = LR.ln_lrelu(y, g.V(b, il), g.V(b, il + 1), g.alpha)
    f = dict(h=h, mean=mean, rstd=rstd, e_h=np.zeros_like(h), e_mean=0.0, e_rstd=0.0)
  else:
    f = NR.ln_fwd(y, g.V(b, il), g.V(b, il + 1), g.ln_eps, g.alpha, g.f16)
  shp = (g.B, lay.lout, lay.cout)
  return [out('G.h.{}'.format(i + 1), (), f['h'].reshape(shp), f['e_h'].reshape(shp),
              creal=lay.cout),
          _f32out('G.mean.{}'.format(i + 1), (), f['mean'], f['e_mean']),
          _f32out('G.rstd.{}'.format(i + 1), (), f['rstd'], f['e_rstd'])]


def g_bn_stats(g, b, i):
  lay, ib = g.layers[i], g.idx_bn[i]
  y = _rows(b['G.ypre.{}'.format(i + 1)], lay.cout)
  s = NR.bn_stats(y, g.momentum, g.V(b, ib + 2), g.V(b, ib + 3),
                  rlanes=NR.bn_row_lanes(lay.coutp))
  return [_f32out('G.bn_mean.{}'.format(i + 1), (), s['mean'], s['e_mean']),
          _f32out('G.bn_var.{}'.format(i + 1), (), s['var'], s['e_var']),
          _f32out('G.data', (g.pslice(ib + 2),), s['mm'], s['e_mm']),
          _f32out('G.data', (g.pslice(ib + 3),), s['mv'], s['e_mv'])]


def g_bn_apply(g, b, i, training=True):
  lay, ib = g.layers[i], g.idx_bn[i]
  y = _rows(b['G.ypre.{}'.format(i + 1)], lay.cout)
  if training:
    mean, var = b['G.bn_mean.{}'.format(i + 1)], b['G.bn_var.{}'.format(i + 1)]
  else:
    mean, var = g.V(b, ib + 2), g.V(b, ib + 3)
  want, err = NR.bn_apply(y, mean, var, g.V(b, ib), g.V(b, ib + 1), g.bn_eps,
                          1.0 if g.ln else g.alpha)
  shp = (g.B, lay.lout, lay.cout)
  key = ('G.ybn.{}' if g.ln else 'G.h.{}').format(i + 1)
  return [out(key, (), want.reshape(shp), err.reshape(shp), creal=lay.cout)]


def g_out(g, b):
  x = _rows(b['G.h.5'], g.C)
  Wo, bo = g.qw(g.V(b, g.idx_out)), g.V(b, g.idx_out + 1)
  want, pre, mag = LR.gen_out(x, Wo, bo, g.normalize, g.floor)
  acc = (g.Cp + 1) * LR.U * mag
  err = D.sigmoid_bar(acc, want) if g.normalize else acc
  shp = (g.B, g.L, g.C)
  return [out('G.fake', (), want.reshape(shp), err.reshape(shp), kind='f32', creal=g.C)]


def g_out_interp(g, b, real, alphas, x0_keys):
  """cg_dense_rows_interp: the output Dense over the n fake batches of a step;
  update k's input buffer (x0_keys[k]) gets [real | fake_k | x^_k], x^ from the
  UNROUNDED fake (dense_ref.dense_rows_interp, dense_ref.xhat_err); alphas None:
  the x^ segments stay."""
  n, B = len(x0_keys), g.B // len(x0_keys)
  x = _rows(b['G.h.5'], g.C)
  Wo, bo = g.qw(g.V(b, g.idx_out)), g.V(b, g.idx_out + 1)
  want, pre, mag = LR.gen_out(x, Wo, bo, g.normalize, g.floor)
  acc = (g.Cp + 1) * LR.U * mag
  err = D.sigmoid_bar(acc, want) if g.normalize else acc
  fake, err = want.reshape(n, B, g.L, g.C), err.reshape(n, B, g.L, g.C)
  real = np.asarray(real, np.float64)
  outs = []
  for k, key in enumerate(x0_keys):
    outs.append(out(key, (slice(0, B),), R.round_act(real, g.f16), kind='bits', creal=g.C))
    outs.append(out(key, (slice(B, 2 * B),), fake[k], err[k], creal=g.C))
    if alphas is not None:
      a = np.asarray(alphas, np.float64)[k * B:(k + 1) * B]
      outs.append(out(key, (slice(2 * B, 3 * B),), R.interp(real, fake[k], a),
                      D.xhat_err(a, real, fake[k], err[k]), creal=g.C))
  return outs


def g_step_outputs(g, b, args, n):
  """cg_step_outputs: [gen_loss, mean loss[k][0], mean gp[k], metrics x 4], on what
  its pointer arguments addressed in front of the launch (args: gen_loss, the n
  loss[k][0], the n gp[k], the 4 metrics)."""
  gen_loss, loss0, gp, metrics = args
  loss = np.stack([loss0, np.zeros(n)], axis=1) if n else np.zeros((1, 2))
  want = R.step_outputs(gen_loss[0], loss, gp, metrics, n)
  bar = np.zeros(7)  # copies are exact; the means: the sum, then one quotient
  if n:
    bar[1] = R.sum_bound(loss0[:n]) / n + R.U32 * abs(want[1])
    bar[2] = R.sum_bound(gp[:n]) / n + R.U32 * abs(want[2])
  return [_f32out('out', (), want, bar)]


def g_cast_fake(g, b):
  fake = b['G.fake'][:, :, :g.C]
  return [out('x0', (slice(0, g.B),), fake if g.exact else R.round_act(fake, g.f16),
              kind='bits', creal=g.C)]


def g_neg_mean(g, b):
  d = b['d_out']
  want = R.neg_mean(d, g.B)
  return [_f32out('gen_loss', (), np.array([want]),
                  np.array([R.sum_bound(d[:g.B]) / g.B + R.U32 * abs(want)]))]


def g_sigmoid_bwd(g, b):
  want = R.sigmoid_bwd(b['gin'][:, :, :g.C], b['G.fake'][:, :, :g.C])
  return [out('G.dz', (), want, creal=g.C)]


def g_out_wgrad(g, b):
  x, dz = _rows(b['G.h.5'], g.C), _rows(b['G.dz'], g.C)
  return [_f32out('G.grad', (g.pslice(g.idx_out),), D.dense_wgrad(x, dz).reshape(-1),
                  D.wgrad_bound(x, dz).reshape(-1))]


def g_colsum(g, b, key, c, pidx):
  want, bar = NR.dbias(_rows(b[key], c))
  return [_f32out('G.grad', (g.pslice(pidx),), want, bar)]


def g_out_dgrad(g, b):
  dz = _rows(b['G.dz'], g.C)
  Wt = g.qw(g.V(b, g.idx_out)).T
  want = D.dense_rows(dz, Wt)
  err = (g.Cp + 1) * LR.U * (LR.nabs(dz, g.floor) @ LR.nabs(Wt, g.floor))
  shp = (g.B, g.L, g.C)
  return [out('G.dh.5', (), want.reshape(shp), err.reshape(shp), creal=g.C)]


def g_ln_bwd(g, b, a, i):
  """cg_ln_lrelu_bwd of layer i; the bias gradient is the column sum of the dy the
  launch STORED (a: the snapshot after it), as norm_ref.dbias states."""
  lay, il, ic = g.layers[i], g.idx_ln[i], g.idx_conv[i]
  c = lay.cout
  ykey = ('G.ybn.{}' if g.bn else 'G.ypre.{}').format(i + 1)
  dkey = ('G.dybn.{}' if g.bn else 'G.dy.{}').format(i + 1)
  r = NR.ln_bwd(_rows(b['G.dh.{}'.format(i + 1)], c), _rows(b['G.h.{}'.format(i + 1)], c),
                _rows(b[ykey], c), b['G.mean.{}'.format(i + 1)],
                b['G.rstd.{}'.format(i + 1)], g.V(b, il), g.alpha)
  shp = (g.B, lay.lout, c)
  outs = [out(dkey, (), r['dy'].reshape(shp), r['e_dy'].reshape(shp), creal=c)]
  sums = [_f32out('G.grad', (g.pslice(il),), r['dgamma'], r['e_dgamma']),
          _f32out('G.grad', (g.pslice(il + 1),), r['dbeta'], r['e_dbeta'])]
  if not g.bn:
    if g.exact or a is None:
      db, e_db = r['dy'].sum(axis=0), 0.0
    else:
      db, e_db = NR.dbias(_rows(a[dkey], c))
    sums.append(_f32out('G.grad', (g.pslice(ic + 1),), db, e_db))
  return outs, sums


def g_bn_bwd(g, b, a, i):
  lay, ib = g.layers[i], g.idx_bn[i]
  c = lay.cout
  if g.ln:
    dout, h, act = _rows(b['G.dybn.{}'.format(i + 1)], c), None, 0
  else:
    dout, h, act = (_rows(b['G.dh.{}'.format(i + 1)], c),
                    _rows(b['G.h.{}'.format(i + 1)], c), 1)
  args = (dout, h, _rows(b['G.ypre.{}'.format(i + 1)], c),
          b['G.bn_mean.{}'.format(i + 1)], b['G.bn_var.{}'.format(i + 1)], g.V(b, ib),
          g.bn_eps, g.alpha, act)
  pure = NR.bn_bwd(*args)
  own = pure if g.exact else NR.bn_bwd(*args, dgamma=g.param(a['G.grad'], ib),
                                       dbeta=g.param(a['G.grad'], ib + 1))
  shp = (g.B, lay.lout, c)
  return [out('G.dy.{}'.format(i + 1), (), own['dy'].reshape(shp),
              own['e_dy'].reshape(shp), creal=c),
          _f32out('G.grad', (g.pslice(ib),), pure['dgamma'], pure['e_dgamma']),
          _f32out('G.grad', (g.pslice(ib + 1),), pure['dbeta'], pure['e_dbeta'])]


def g_lrelu_bwd(g, b, i):
  """i = -1: the input Dense's activation."""
  k = i + 1
  want = R.lrelu_bwd(b['G.dh.{}'.format(k)], b['G.h.{}'.format(k)], g.alpha)
  return [out('G.dy.{}'.format(k), (), want.reshape(b['G.dy.{}'.format(k)].shape))]


def g_dgrad(g, b, i):
  lay, ic = g.layers[i], g.idx_conv[i]
  dy = b['G.dy.{}'.format(i + 1)][:, :, :lay.cout]
  want, mag = LR.gen_convt_dgrad(dy, g.qw(g.V(b, ic)), lay.lin, g.floor)
  err = LR.gamma(g.k * lay.coutp) * mag
  return [out('G.dh.{}'.format(i), (), want, err,
              creal=lay.cin if i > 0 else None)]


def g_in_wgrad(g, b):
  z, dy = b['G.z'].reshape(g.B, g.nd), b['G.dy.0'].reshape(g.B, -1)
  dW, mag = LR.dense_wgrad(z, dy, g.floor)
  joins = 8 * -(-g.B // 256)
  return [_f32out('G.grad', (g.pslice(0),), dW.reshape(-1),
                  (LR.gamma(g.B + joins) * mag).reshape(-1))]


def g_wgrad(g, b, i):
  lay, ic = g.layers[i], g.idx_conv[i]
  h = b['G.h.{}'.format(i)][:, :, :lay.cin]
  dy = b['G.dy.{}'.format(i + 1)][:, :, :lay.cout]
  dW, mag = LR.gen_convt_wgrad(h, dy, g.k, g.floor)
  rows = g.B * lay.lin
  joins = -(-rows // 64)
  return [_f32out('G.grad', (g.pslice(ic),), dW.reshape(-1),
                  (LR.gamma(rows + joins) * mag).reshape(-1))]


class GenChecker(Checker):
  """The generator update: the critic's stages over the fake segment (ctx: a Ctx
  with nseg = 1) plus the generator's own (g: a GenCtx)."""

  def __init__(self, ctx, g):
    Checker.__init__(self, ctx)
    self.g = g
    self.pending = []  # column sums whose finish is deferred to cg_finish_flush

  def sums(self, name, ev, outs, sums):
    """Check a stage whose column sums may be deferred."""
    if self.g.defer:
      self.pending += [(name, o) for o in sums]
      free = [dict(o, kind='free') for o in sums]
      self.check(name, ev, outs + free)
    else:
      self.check(name, ev, outs + sums)

  def claim(self, ev):
    g, role, b = self.g, ev['role'], ev['before']
    name = ' '.join(str(r) for r in role)
    kind = role[0]
    if not kind.startswith('g_') and kind not in ('cast_fake', 'neg_mean',
                                                   'finish_flush', 'metrics'):
      return Checker.claim(self, ev)
    if self.group is not None:
      raise StageError(name, 'launch inside an open group')
    if kind == 'g_cast_z':
      self.check(name, ev, g_cast_z(g, b))
    elif kind == 'g_in':
      self.check(name, ev, g_in(g, b))
    elif kind == 'g_conv':
      self.check(name, ev, g_conv(g, b, role[1], g.keep))
    elif kind == 'g_ln_fwd':
      self.check(name, ev, g_ln_fwd(g, b, role[1]))
    elif kind == 'g_bn_stats':
      self.check(name, ev, g_bn_stats(g, b, role[1]))
    elif kind == 'g_bn_apply':
      self.check(name, ev, g_bn_apply(g, b, role[1], g.training))
    elif kind == 'g_out':
      self.check(name, ev, g_out(g, b))
    elif kind == 'g_out_interp':
      self.check(name, ev, g_out_interp(g, b, self.ctx.real, ev['alphas'], ev['x0_keys']))
    elif kind == 'g_step_outputs':
      self.check(name, ev, g_step_outputs(g, b, ev['args_in'], ev['n']))
    elif kind == 'cast_fake':
      self.check(name, ev, g_cast_fake(g, b))
    elif kind == 'neg_mean':
      self.check(name, ev, g_neg_mean(g, b))
    elif kind == 'g_sigmoid_bwd':
      self.check(name, ev, g_sigmoid_bwd(g, b))
    elif kind == 'g_out_wgrad':
      self.check(name, ev, g_out_wgrad(g, b))
    elif kind == 'g_colsum':
      which = role[1]
      if which == 'out':
        s = g_colsum(g, b, 'G.dz', g.C, g.idx_out + 1)
      elif which == 'in':
        s = g_colsum(g, b, 'G.dy.0', g.w0 * g.nd, 1)
      else:
        s = g_colsum(g, b, 'G.dy.{}'.format(which + 1), g.layers[which].cout,
                     g.idx_conv[which] + 1)
      self.sums(name, ev, [], s)
    elif kind == 'g_out_dgrad':
      self.check(name, ev, g_out_dgrad(g, b))
    elif kind == 'g_ln_bwd':
      outs, s = g_ln_bwd(g, b, ev['after'], role[1])
      self.sums(name, ev, outs, s)
    elif kind == 'g_bn_bwd':
      self.check(name, ev, g_bn_bwd(g, b, ev['after'], role[1]))
    elif kind == 'g_lrelu_bwd':
      self.check(name, ev, g_lrelu_bwd(g, b, role[1]))
    elif kind == 'g_dgrad':
      self.check(name, ev, g_dgrad(g, b, role[1]))
    elif kind == 'g_in_wgrad':
      self.check(name, ev, g_in_wgrad(g, b))
    elif kind == 'g_wgrads':
      outs = []
      for i in role[1]:
        mine = g_wgrad(g, b, i)
        for o in mine:
          self._compare('g_wgrad {}'.format(i), o, ev['after'][o['key']])
        outs += mine
      self._frame(name, b, ev['after'], outs)
    elif kind == 'metrics':
      # cg_signal_metrics on (real, fake): the launch's own 4-float output
      fake = _rows(b['G.fake'], g.C)
      real = np.asarray(self.ctx.real, np.float64).reshape(-1, g.C)
      want = R.signal_metrics(real, fake, g.smin, g.smax)
      bar = R.signal_metrics_bars(real, fake, g.smin, g.smax)
      self._compare(name, _f32out('metrics', (), want, bar), ev['metrics'])
      self._frame(name, b, ev['after'], [])
    elif kind == 'finish_flush':
      for stage, o in self.pending:
        self._compare(stage, o, ev['after'][o['key']])
      self._frame(name, b, ev['after'], [o for _, o in self.pending])
      self.pending = []
    else:
      raise StageError(name, 'unclaimed launch')

  def run(self, events):
    res = Checker.run(self, events)
    if self.pending:
      raise StageError('finish_flush', 'deferred column sums never finished')
    return res


class GenSim(object):
  """wgan_gp._gen_compute as a chain of the stage statements (see CriticSim)."""

  def __init__(self, ctx, g, gen_weights, dis_weights, z, shifts):
    self.g = g
    B = g.B
    self.cs = cs = CriticSim(ctx, dis_weights, np.zeros((B, g.L, g.C)),
                             np.zeros((B, g.L, g.C)), np.zeros(B), shifts)
    st = self.st = cs.st
    zz = lambda *s: np.zeros(s)
    g.z = np.asarray(z, np.float64)
    st['G.z'] = zz(B, 1, g.nd)
    st['G.h.0'], st['G.dh.0'] = zz(B, g.w0, g.nd), zz(B, g.w0, g.nd)
    st['G.dy.0'] = zz(B, 1, g.w0 * g.nd)
    for i, lay in enumerate(g.layers):
      for k in ('G.h', 'G.ypre', 'G.dh', 'G.dy') + (('G.ybn', 'G.dybn') if g.bn and
                                                     g.ln else ()):
        st['{}.{}'.format(k, i + 1)] = zz(B, lay.lout, lay.coutp)
      for k in ('G.mean', 'G.rstd'):
        st['{}.{}'.format(k, i + 1)] = zz(B * lay.lout)
      if g.bn:
        st['G.bn_mean.{}'.format(i + 1)] = zz(lay.cout)
        st['G.bn_var.{}'.format(i + 1)] = zz(lay.cout)
    st['G.fake'], st['G.dz'] = zz(B, g.L, g.Cf), zz(B, g.L, g.Cp)
    st['gen_loss'] = zz(1)
    flat = zz(g.numel)
    for i, w in enumerate(gen_weights):
      flat[g.pslice(i)] = np.asarray(w, np.float64).reshape(-1)
    st['G.data'], st['G.grad'] = flat, zz(g.numel)
    self.deferred = []

  def sums(self, role, outs, sums):
    if self.g.defer:
      self.deferred += sums
      self.cs.emit(role, outs)
    else:
      self.cs.emit(role, outs + sums)

  def run(self):
    g, st, emit = self.g, self.st, self.cs.emit
    emit(('g_cast_z',), g_cast_z(g, st))
    emit(('g_in',), g_in(g, st))
    for i in range(NUM_CONVS):
      emit(('g_conv', i), g_conv(g, st, i))
      if g.bn:
        emit(('g_bn_stats', i), g_bn_stats(g, st, i))
        emit(('g_bn_apply', i), g_bn_apply(g, st, i))
      if g.ln and not g.ln_fused[i]:
        emit(('g_ln_fwd', i), g_ln_fwd(g, st, i))
    emit(('g_out',), g_out(g, st))
    emit(('cast_fake',), g_cast_fake(g, st))
    self.cs.forward()
    emit(('neg_mean',), g_neg_mean(g, st))
    self.cs.chain()
    if g.normalize:
      emit(('g_sigmoid_bwd',), g_sigmoid_bwd(g, st))
    else:
      st['G.dz'][...] = st['gin']  # a copy on the host's side of the schedule
    emit(('g_out_wgrad',), g_out_wgrad(g, st))
    self.sums(('g_colsum', 'out'), [], g_colsum(g, st, 'G.dz', g.C, g.idx_out + 1))
    emit(('g_out_dgrad',), g_out_dgrad(g, st))
    for i in range(NUM_CONVS - 1, -1, -1):
      lay = g.layers[i]
      conv_bias = lambda: g_colsum(g, st, 'G.dy.{}'.format(i + 1), lay.cout,
                                   g.idx_conv[i] + 1)
      if g.ln:
        outs, s = g_ln_bwd(g, st, None, i)
        if not g.bn:
          # the bias gradient sums the dy the launch stores
          dy = self.cs.qa(np.asarray(outs[0]['want']))
          s[-1] = g_ln_bwd(g, st, {outs[0]['key']: _padded(dy, lay.coutp)}, i)[1][-1]
        self.sums(('g_ln_bwd', i), outs, s)
      if g.bn:
        o = g_bn_bwd(g, st, None, i) if g.exact else self._bn_bwd(i)
        emit(('g_bn_bwd', i), o)
        self.sums(('g_colsum', i), [], conv_bias())
      elif not g.ln:
        emit(('g_lrelu_bwd', i), g_lrelu_bwd(g, st, i))
        self.sums(('g_colsum', i), [], conv_bias())
      emit(('g_dgrad', i), g_dgrad(g, st, i))
    emit(('g_lrelu_bwd', -1), g_lrelu_bwd(g, st, -1))
    emit(('g_in_wgrad',), g_in_wgrad(g, st))
    self.sums(('g_colsum', 'in'), [], g_colsum(g, st, 'G.dy.0', g.w0 * g.nd, 1))
    outs = []
    for i in range(NUM_CONVS):
      outs += g_wgrad(g, st, i)
    emit(('g_wgrads', tuple(range(NUM_CONVS))), outs)
    if g.defer:
      emit(('finish_flush',), self.deferred)
    return self.cs.events

  def _bn_bwd(self, i):
    """dy is evaluated with the sums the launch stores (f32)."""
    g, st = self.g, self.st
    ib = g.idx_bn[i]
    pure = g_bn_bwd(_with(g, exact=True), st, None, i)
    a = {'G.grad': st['G.grad'].copy()}
    for o in pure[1:]:
      a['G.grad'][o['idx']] = self.cs.q32(np.asarray(o['want']))
    return g_bn_bwd(g, st, a, i)


def _padded(v, cp):
  o = np.zeros(v.shape[:-1] + (cp,))
  o[..., :v.shape[-1]] = v
  return o


def gen_grads(sim):
  g = sim.g
  return [g.param(sim.st['G.grad'], i).copy() for i in range(len(g.shapes))]


def gen_flags(gan, B):
  """The generator schedule's form, as the workspace chose it."""
  from calciumgan_amd import nets
  net = gan.generator.net
  gws = gan._get_state(B)['gws']
  return dict(ln_fused=list(gws.ln_fused), Cf=net.Cf,
              defer=bool(nets._DEFER_FINISH and nets.DETERMINISTIC and net.layer_norm
                         and not net.batch_norm),
              streaming_out=bool(net.streaming_out),
              streaming_out_dgrad=bool(net.streaming_out_dgrad))


class GenTracer(Tracer):
  """Tracer of one generator update: the critic's plan over the fake segment plus
  the whole generator workspace."""

  def __init__(self, gan, B, plan=None):
    st = gan._get_state(B)
    Tracer.__init__(self, gan, B, plan=st['gen'] if plan is None else plan)
    gws, net = st['gws'], gan.generator.net
    self.gws, self.gnet = gws, net
    w = self.watch
    w['G.z'], w['G.dz'], w['gen_loss'] = gws.z, gws.dz, st['gen_loss']
    for i in range(NUM_CONVS + 1):
      w['G.h.{}'.format(i)], w['G.dh.{}'.format(i)] = gws.h[i], gws.dh[i]
      w['G.dy.{}'.format(i)] = gws.dy[i]
      if i == 0:
        continue
      for k, lst in (('ypre', gws.ypre), ('mean', gws.mean), ('rstd', gws.rstd),
                     ('bn_mean', getattr(gws, 'bn_mean', None)),
                     ('bn_var', getattr(gws, 'bn_var', None)),
                     ('ybn', getattr(gws, 'ybn', None)),
                     ('dybn', getattr(gws, 'dybn', None))):
        if lst is not None and lst[i] is not None:
          w['G.{}.{}'.format(k, i)] = lst[i]
    for k in ('data', 'grad', 'm', 'v'):
      w['G.' + k] = getattr(net.params, k)
    self.gpacks = pack_descs(net)
    self.pack_plans.append(('G', net._pack_plan, self.gpacks))
    for (key, _, _), op in zip(self.gpacks, net._pack_plan._keep):
      w['G.' + key] = op.buf
    self.roles[id(gws.f_in)] = ('g_in',)
    for i in range(NUM_CONVS):
      self.roles[id(gws.f_conv[i])] = ('g_conv', i)
      self.roles[id(gws.f_conv_fwd_only[i])] = ('g_conv', i)
      self.roles[id(gws.b_dgrad[i])] = ('g_dgrad', i)
    if gws.f_out is not None:
      self.roles[id(gws.f_out)] = ('g_out',)
    if gws.b_out_dgrad is not None:
      self.roles[id(gws.b_out_dgrad)] = ('g_out_dgrad',)
    self.g_wgrad_of = {id(d): i for i, d in enumerate(gws.b_wgrad)}
    self.in_wgrads = {id(gws.b_in_wgrad)}
    self.z_ptrs = {gws.z.data_ptr()}
    self.ptr = {}
    for i in range(NUM_CONVS + 1):
      for k, lst in (('h', gws.h), ('dh', gws.dh), ('dy', gws.dy), ('ypre', gws.ypre)):
        if lst[i] is not None:
          self.ptr[lst[i].data_ptr()] = (k, i)

  def identify(self, kind, args):
    gws, net = self.gws, self.gnet
    if kind == 'wgrad' and id(args[0]) in self.in_wgrads:
      return ('g_in_wgrad',), {}
    if kind in ('wgrad', 'wgrads'):
      ds = [args[0]] if kind == 'wgrad' else list(args[0])
      ls = tuple(self.g_wgrad_of.get(id(d)) for d in ds)
      if None not in ls:
        return ('g_wgrads', ls), {}
    if kind != 'call':
      return Tracer.identify(self, kind, args)
    name, a = args[0], args[1:]
    at = lambda j: self.ptr.get(self._ptr(a[j]), (None, None))
    if name == 'cg_cast_pad':
      if self._ptr(a[1]) in self.z_ptrs:
        return ('g_cast_z',), {}
      if self._ptr(a[1]) == self.dws.act[0].data_ptr():
        return ('cast_fake',), {}
    elif name in ('cg_bn_stats', 'cg_bn_apply') and at(0)[0] == 'ypre':
      return ('g_' + name[3:], at(0)[1] - 1), {}
    elif name == 'cg_ln_lrelu_fwd' and at(3)[0] == 'h':
      return ('g_ln_fwd', at(3)[1] - 1), {}
    elif name == 'cg_ln_lrelu_bwd' and at(0)[0] == 'dh':
      return ('g_ln_bwd', at(0)[1] - 1), {}
    elif name == 'cg_bn_bwd' and at(2)[0] == 'ypre':
      return ('g_bn_bwd', at(2)[1] - 1), {}
    elif name == 'cg_lrelu_bwd' and at(2)[0] == 'dy':
      return ('g_lrelu_bwd', at(2)[1] - 1), {}
    elif name == 'cg_colsum':
      off = (self._ptr(a[1]) - net.params.grad.data_ptr()) // 4
      offs = list(net.params.offsets)
      if off in offs:
        p = offs.index(off)
        if p == net.idx_out + 1:
          return ('g_colsum', 'out'), {}
        if p == 1:
          return ('g_colsum', 'in'), {}
        if p - 1 in net.idx_conv:
          return ('g_colsum', net.idx_conv.index(p - 1)), {}
    simple = {'cg_dense_rows': ('g_out',), 'cg_neg_mean': ('neg_mean',),
              'cg_sigmoid_bwd': ('g_sigmoid_bwd',), 'cg_dense_wgrad': ('g_out_wgrad',),
              'cg_dense_rows_act': ('g_out_dgrad',), 'cg_finish_flush': ('finish_flush',)}
    if name in simple:
      return simple[name], {}
    return Tracer.identify(self, kind, args)



# ===========================================================================
# a whole eager train(): several plans and generator workspaces over one trace
# ===========================================================================
class StepTracer(GenTracer):
  """Tracer of one eager WGAN_GP.train(): every critic plan of the step (update k
  reads input buffer x0(k) and its own words of the stage buffer), the generator
  update's plan, the generator workspace of that update (GA) and the forward-only
  one of the batched G(z) (GB).  A buffer that belongs to one plan or workspace is
  watched under its plain key if it is the first of that name, else under
  '<space>:<key>'; spaces[space] maps plain -> watched key, and view() renames a
  snapshot so that the stages of the active spaces find their buffers under the
  plain keys (every other buffer stays in the snapshot, under the frame check).
  Each event carries the space of its descriptor (None: the launch before it)."""

  def __init__(self, gan, B, n):
    from calciumgan_amd import nets
    self.nets = nets
    st = gan._get_state(B)
    dws, dnet, gnet = st['dws'], gan.discriminator.net, gan.generator.net
    self.dws, self.gnet = dws, gnet
    self.watch, self.spaces, self._seen = {}, {}, {}
    self.roles, self.space_of = {}, {}
    self.wgrad_of, self.g_wgrad_of, self.in_wgrads = {}, {}, set()
    self.coef_ptrs, self.z_ptrs, self.ptr = set(), {}, {}
    reg = self.reg
    for l in range(1, NUM_CONVS + 1):
      reg(None, 'act.{}'.format(l), dws.act[l])
      reg(None, 'delta.{}'.format(l), dws.delta[l])
      if l < NUM_CONVS:
        reg(None, 'e.{}'.format(l), dws.e[l])
    reg(None, 'd_out', dws.d_out)
    for k in ('norm', 'coef_gp', 'gp', 'loss', 'gen_loss', 'out', 'coef_d', 'coef_g',
              'delta_g'):
      if k in st:
        reg(None, k, st[k])
    self.pack_plans = []
    for name, net, opt in (('D', dnet, gan.dis_optimizer), ('G', gnet, gan.gen_optimizer)):
      for k in ('data', 'grad', 'm', 'v'):
        reg(None, name + '.' + k, getattr(net.params, k))
      packs = pack_descs(net)
      self.pack_plans.append((name, net._pack_plan, packs))
      for (key, _, _), op in zip(packs, net._pack_plan._keep):
        reg(None, name + '.' + key, op.buf)
      if opt.loss_scale is not None:
        reg(None, name + '.ls', opt.loss_scale_state)
    if 'dis' in st:  # the BCE step: D's chain over [fake | real], G's over fake
      self.plans = {'dis': st['dis']}
    else:
      self.plans = {'p{}'.format(k): gan._critic_plan(st, k) for k in range(n)}
    self.plans['gen'] = st['gen']
    for sp, plan in self.plans.items():
      reg(sp, 'x0', plan.x0)
      if plan.gin is not None and not plan.gin_in_x0:
        reg(sp, 'gin', plan.gin)
      if getattr(plan, 'sumsq', None) is not None:
        reg(sp, 'sumsq', plan.sumsq)
      if plan.norm_deferred:
        reg(sp, 'ssq', plan.ssq[0])
      for i, t in plan.side.items():
        reg(sp, 'side.{}'.format(i), t)
      for k in ('coef', 'bias_coef', 'shifts'):
        reg(sp, k, getattr(plan, k))
      self.coef_ptrs.add(plan.coef.data_ptr())
      descs = [(('fwd', l), d) for l, d in enumerate(plan.fwd)]
      descs += [(('dgrad', i), d) for i, d in plan.dgrad]
      descs += [(('jvp', l), d) for l, d in enumerate(plan.jvp)]
      if plan.fwd_l1_pair is not None:
        descs.append((('fwd_pair',), plan.fwd_l1_pair))
      if plan.input_grad is not None:
        descs.append((('gin',), plan.input_grad))
      for role, d in descs:
        self.roles[id(d)], self.space_of[id(d)] = role, sp
      for l, d in enumerate(plan.wgrad):
        self.wgrad_of[id(d)], self.space_of[id(d)] = l, sp
    self.gwss = {'GA': st['gws']}
    if n > 1:
      self.gwss['GB'] = gnet.workspace(n * B, forward_only=True)
    for sp, gws in self.gwss.items():
      reg(sp, 'G.z', gws.z)
      reg(sp, 'G.fake', gws.fake)
      self.z_ptrs[gws.z.data_ptr()] = sp
      full = not gws.forward_only
      if full:
        reg(sp, 'G.dz', gws.dz)
      for i in range(NUM_CONVS + 1):
        lists = [('h', gws.h)] + ([('dh', gws.dh), ('dy', gws.dy)] if full else [])
        if i:
          lists += [('ypre', gws.ypre), ('mean', gws.mean), ('rstd', gws.rstd)]
        for k, lst in lists:
          reg(sp, 'G.{}.{}'.format(k, i), lst[i])
          self.ptr[lst[i].data_ptr()] = (k, i)
      descs = [(('g_in',), gws.f_in)]
      for i in range(NUM_CONVS):
        descs += [(('g_conv', i), gws.f_conv[i]), (('g_conv', i), gws.f_conv_fwd_only[i])]
        if full:
          descs.append((('g_dgrad', i), gws.b_dgrad[i]))
          self.g_wgrad_of[id(gws.b_wgrad[i])] = i
          self.space_of[id(gws.b_wgrad[i])] = sp
      if gws.f_out is not None:
        descs.append((('g_out',), gws.f_out))
      if full:
        if gws.b_out_dgrad is not None:
          descs.append((('g_out_dgrad',), gws.b_out_dgrad))
        self.in_wgrads.add(id(gws.b_in_wgrad))
        self.space_of[id(gws.b_in_wgrad)] = sp
      for role, d in descs:
        self.roles[id(d)], self.space_of[id(d)] = role, sp
    self.gws = self.gwss['GA']
    self.delta_of = {dws.delta[i].data_ptr(): i for i in range(1, NUM_CONVS + 1)}
    self.x0_keys = [self.spaces['p{}'.format(k)]['x0'] for k in range(n)
                    if 'p{}'.format(k) in self.spaces]
    self.real_ptr = dws.act[0][B:2 * B].data_ptr()
    self.events, self.depth, self.last = [], 0, None

  def reg(self, space, key, t):
    """Watch t; a tensor already watched (same memory, shape and type) keeps its
    first key."""
    ident = (t.data_ptr(), tuple(t.shape), t.dtype)
    name = self._seen.get(ident)
    if name is None:
      name = key if key not in self.watch else '{}:{}'.format(space, key)
      self.watch[name] = t
      self._seen[ident] = name
    if space is not None:
      self.spaces.setdefault(space, {})[key] = name

  def identify(self, kind, args):
    role, info = GenTracer.identify(self, kind, args)
    space = None
    if kind == 'wgrads':
      space = self.space_of.get(id(args[0][0]))
    elif kind != 'call':
      space = self.space_of.get(id(args[0]))
    else:
      name, a = args[0], args[1:]
      if name == 'cg_cast_pad' and role == ('g_cast_z',):
        space = self.z_ptrs[self._ptr(a[1])]
      elif name == 'cg_cast_pad' and self._ptr(a[1]) == self.real_ptr:
        role = ('cast_real',)
      elif name == 'cg_dense1_bce':
        role = ('bce',)
      elif name == 'cg_dense1_wgrad' and self._ptr(a[1]) not in self.coef_ptrs:
        role = ('head_wgrad_samples',)
      elif name == 'cg_dense_rows_interp':
        al = a[4]
        role = ('g_out_interp',)
        info = dict(alphas=None if al is None else al.detach().cpu().double().numpy(),
                    x0_keys=list(self.x0_keys[:a[6]]))
      elif name == 'cg_step_outputs':
        role = ('g_step_outputs',)
        import torch
        torch.cuda.synchronize()
        take = lambda t, k, step=1: t.as_strided((k,), (step,)).detach().cpu().double().numpy()
        info = dict(args_in=(take(a[0], 1), take(a[1], a[4], 2), take(a[2], a[4]),
                             take(a[3], 4)), n=a[4])
    info['space'] = space
    return role, info


def view(snap, spaces, active):
  """snap with the buffers of the active spaces under their plain keys."""
  res = dict(snap)
  for sp in active:
    for key, name in spaces[sp].items():
      if key != name:
        if key in res:
          res['~' + key] = res.pop(key)
        res[key] = res.pop(name)
  return res


def run_step(events, spaces, checkers):
  """Check the trace of a whole step.  checkers: space -> (checker, the spaces whose
  buffers its stages address by their plain keys).  Between launches only the host's
  staging may change a buffer: a plan's shifts and seeds, coef_gp under the loss
  scale, dz = dfake of a linear output."""
  space, prev, ratios = None, None, {}
  for n, ev in enumerate(events):
    space = ev.get('space') or space
    if space not in checkers:
      raise StageError(' '.join(map(str, ev['role'])), 'launch {} belongs to no pass'.format(n))
    ck, active = checkers[space]
    if prev is not None:
      staged = {k: v for k, v in ev['before'].items()
                if k.split(':')[-1] not in ('shifts', 'coef', 'bias_coef')}
      ck.gap({k: prev[k] for k in staged}, staged)
    v = dict(ev, before=view(ev['before'], spaces, active),
             after=view(ev['after'], spaces, active))
    try:
      ck.claim(v)
    except StageError as e:
      raise StageError('{} (launch {}, {})'.format(e.stage, n, space), str(e))
    prev = ev['after']
  for ck, _ in checkers.values():
    if ck.group is not None or getattr(ck, 'pending', None):
      raise StageError('end of step', 'a group or a deferred sum was left open')
    for k, r in ck.ratios.items():
      ratios[k] = max(ratios.get(k, 0.0), r)
  return ratios
