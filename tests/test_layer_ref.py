"""CPU checks of the launch-by-launch references (tests/layer_ref.py,
tests/layer_trace.py):

  * closure: the stage statements chained in float64 with no rounding give the
    gradients of float64 torch.autograd through the oracle's d_step_grads, per
    term and together, to 1e-12;
  * discrimination: the checker passes a simulated trace (every output rounded to
    the storage type) and names the stage of each planted fault;
  * inputs: the hand-built phase-shuffle draws differ between the three segments
    in every layer and reach +m, -m and 0 in every layer."""
import numpy as np
import pytest
import torch

import oracle as O

import layer_trace as LT

TINY = dict(L=64, C=6, U=8, k=24, m=2, B=4)

# The cases of tests/test_hip_layers.py (kept here, on the CPU's side: the range
# test of the fp16 loss scales below builds the same inputs).
# (L, C, U, k, m, B), as in test_hip_step.CONFIGS
SHAPES = {
    'tiny': (64, 6, 8, 24, 2, 4),     # deepest layer lin = 4 < 2m + 1: cg_unshuffle_mask
    'long': (2048, 6, 8, 24, 10, 2),  # norm fused into the input-gradient launch
    'odd_c': (128, 102, 16, 24, 3, 3),  # pitch 128
    'c40': (128, 40, 16, 24, 3, 2),
    'm0_k8': (128, 6, 8, 8, 0, 3),    # classic tiles, tangent scale not folded
    'b1': (64, 6, 8, 24, 2, 1),
    'mid': (256, 16, 32, 24, 2, 6),
    # kernel sizes other than 24: the classic tiles, and with them the unfolded forms
    # of the critic schedule (side buffer + cg_unshuffle_fixup) with m > 0
    'k2': (64, 6, 8, 2, 2, 3),
    'k6_c40': (128, 40, 16, 6, 3, 2),    # narrow first layer, half_taps 3
    'k12': (128, 6, 8, 12, 3, 2),
    'k14_c102': (128, 102, 16, 14, 3, 2),  # pitch 128, narrow
    'k22_u24': (128, 6, 24, 22, 3, 2),   # pitches 32 / 64 / 96 / 96 / 128, narrow at layer 4
    'k4_u40': (64, 6, 40, 4, 2, 2),      # last width 200 -> pitch 224
    # 192 rows per sample in the generator's first layer: no LayerNorm tile fits them
    # (generator case only)
    'l6144': (6144, 6, 8, 24, 2, 1),
}
SEED = 42
# generator cases: name -> (shape, hparams, nets flags set before the model is built)
GEN_CASES = {
    'tiny': ('tiny', {}, {}),
    'tiny_noln': ('tiny', dict(layer_norm=False), {}),
    'mid': ('mid', {}, {}),
    'odd_c': ('odd_c', {}, {}),   # streaming output Dense, Cf = 104, streaming dh
    'tiny_bn': ('tiny', dict(layer_norm=False, batch_norm=True), {}),
    'tiny_bn_ln': ('tiny', dict(batch_norm=True), {}),
    'tiny_linear': ('tiny', dict(normalize=False), {}),
    'tiny-no_fuse_ln': ('tiny', {}, {'_FUSE_LN': False}),
    'tiny-no_defer_finish': ('tiny', {}, {'_DEFER_FINISH': False}),
    'k6_c40': ('k6_c40', {}, {}),
    'k14_c102': ('k14_c102', {}, {}),
    'k22_u24': ('k22_u24', {}, {}),
    'l6144': ('l6144', {}, {}),   # LayerNorm fused from the second layer on only
}


def shift_case(case):
  """Which of the hand-built draws (SHIFT_CASES) a case takes."""
  return len(case) % 3


# Hand-built draws (4 layers x [real, fake, x^]): per layer the three segments
# differ pairwise; over the list every layer meets +m, -m and 0.
SHIFT_CASES = [
    [[2, -2, 0], [-2, 0, 2], [0, 2, -2], [1, -1, 0]],
    [[-1, 1, 2], [0, 1, -1], [2, -2, 1], [-2, 0, 2]],
    [[0, -1, 1], [2, -1, 1], [-2, -1, 0], [0, 2, -2]],
]


def scaled_cases(m):
  """SHIFT_CASES for a model with another m: +-2 -> +-m, +-1 -> +-(m // 2 or 1)
  (kept distinct from 0 and from +-m for m >= 2)."""
  def f(s):
    if abs(s) == 2:
      return int(np.sign(s)) * m
    return int(np.sign(s)) * max(1, m // 2) if s else 0
  return [[[f(s) for s in row] for row in case] for case in SHIFT_CASES]


def test_shift_cases_cover_every_layer():
  m = TINY['m']
  for case in SHIFT_CASES:
    for row in case:
      assert len(set(row)) == 3, row
      assert all(abs(s) <= m for s in row)
  for layer in range(4):
    seen = {s for case in SHIFT_CASES for s in case[layer]}
    assert {m, -m, 0} <= seen, (layer, seen)
  for mm in (3, 10):
    for case in scaled_cases(mm):
      for row in case:
        assert len(set(row)) == 3, row


def case_inputs(shape, seed, case, **hpkw):
  """Weights and draws of one case, shared with tests/test_hip_layers.py (the GPU
  models are given these weights): (L, C, U, k, m, B) -> hparams, generator and
  critic weights (biases and norm parameters moved off their trivial initial
  values), real batch, z, alpha (float64; the callers cast) and the hand-built
  (4, 3) shifts."""
  L, C, U, k, m, B = shape
  hp = O.make_hparams(L, C, U, kernel_size=k, m=m, **hpkw)
  rng = np.random.RandomState(seed)
  gw = O.init_generator(hp, rng)
  dw = O.init_discriminator(hp, rng)
  for w in gw + dw:
    if w.ndim == 1:
      w += rng.randn(*w.shape).astype(np.float32) * 0.05
  real = rng.uniform(0, 1, (B, L, C))
  z = rng.standard_normal((B, hp.noise_dim))
  alpha = rng.uniform(0, 1, B)
  shifts = np.array(scaled_cases(m)[case % len(SHIFT_CASES)])  # (4, 3)
  return hp, gw, dw, real, z, alpha, shifts, B


def _setup(seed=3, case=0, **hpkw):
  c = TINY
  return case_inputs((c['L'], c['C'], c['U'], c['k'], c['m'], c['B']), seed, case,
                     **hpkw)


def _t64(ws):
  return [torch.tensor(np.asarray(w, np.float64)) for w in ws]


def _relmax(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---------------------------------------------------------------------------
# closure
# ---------------------------------------------------------------------------
def _oracle_terms(hp, gw, dw, real, z, alpha, shifts, terms):
  """float64 autograd of wr (-E D(real)) + wf E D(fake) + wp lambda gp."""
  wr, wf, wp = terms
  gen = _t64(gw)
  dis = [w.requires_grad_(True) for w in _t64(dw)]
  realt = torch.tensor(real)
  with torch.no_grad():
    fake = O.generator_forward(gen, torch.tensor(z), hp)
  loss = 0.0
  if wr:
    loss = loss - O.discriminator_forward(dis, realt, shifts[:, 0], hp).mean()
  if wf:
    loss = loss + O.discriminator_forward(dis, fake, shifts[:, 1], hp).mean()
  if wp:
    gp, _, _ = O.gradient_penalty(dis, realt, fake, torch.tensor(alpha),
                                  shifts[:, 2], hp)
    loss = loss + float(hp.gradient_penalty) * gp
  grads = torch.autograd.grad(loss, dis, allow_unused=True)
  return fake.numpy(), [np.zeros(w.shape) if g is None else g.numpy()
                        for g, w in zip(grads, dis)]


VARIANTS = {
    # the schedule's forms: which launches exist, never what a stage computes
    'folded': dict(folded=(1, 2, 3), gin_in_x0=True, jvp_folds=True,
                   norm_deferred=True, has_sumsq=True, P=3),
    'side': dict(sided=(1, 2, 3), gin_in_x0=True, jvp_folds=True),
    'plain': dict(),
    'mix': dict(folded=(1, 2, 3), gin_in_x0=True, jvp_folds=False,
                mixes_layer1=True, has_sumsq=True, norm_deferred=True),
}


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('terms', [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)],
                         ids=['real', 'fake', 'gp', 'all'])
def test_critic_closure(terms, variant):
  _critic_closure(_setup(case=1), terms, variant)


@pytest.mark.parametrize('variant', ['side', 'plain'])
def test_critic_closure_at_kernel_size_6(variant):
  """k = 2 (mod 4): both phases of the input gradient share one window offset and
  phase 0 starts on an even tap; three taps per phase.  The forms a kernel size
  other than 24 takes (no folded fix-up)."""
  _critic_closure(case_inputs(SHAPES['k6_c40'], SEED, shift_case('k6_c40')), (1, 1, 1),
                  variant)


def _critic_closure(inputs, terms, variant):
  hp, gw, dw, real, z, alpha, shifts, B = inputs
  fake, want = _oracle_terms(hp, gw, dw, real, z, alpha, shifts, terms)
  wr, wf, wp = terms
  hp.gradient_penalty = hp.gradient_penalty if wp else 0.0
  ctx = LT.Ctx(hp, B, False, exact=True, **VARIANTS[variant])
  sim = LT.CriticSim(ctx, [np.asarray(w, np.float64) for w in dw], real, fake, alpha,
                     shifts, coef=[-wr / B, wf / B, 1.0],
                     bias_coef=[-wr / B, wf / B, 0.0])
  sim.run()
  got = LT.critic_grads(sim)
  for i, (g, w) in enumerate(zip(got, want)):
    if np.abs(w).max() == 0:
      assert np.abs(g).max() <= 1e-15, i
    else:
      assert _relmax(g, w) <= 1e-12, (i, _relmax(g, w))
  if terms == (1, 1, 1):
    res = O.d_step_grads(_t64(gw), _t64(dw), torch.tensor(real), torch.tensor(z),
                         torch.tensor(alpha), shifts[:, 0], shifts[:, 1],
                         shifts[:, 2], hp)
    for i, (g, w) in enumerate(zip(got, res['grads'])):
      if float(w.abs().max()) > 0:
        assert _relmax(g, w.numpy()) <= 1e-12, i
    assert _relmax(sim.st['loss'][0, 0], float(res['loss'])) <= 1e-12
    assert _relmax(sim.st['gp'][0], float(res['gp'])) <= 1e-12
    norm = sim.st['sumsq'] if ctx.has_sumsq else sim.st['norm']
    assert _relmax(norm, res['norm'].numpy()) <= 1e-12


# ---------------------------------------------------------------------------
# discrimination
# ---------------------------------------------------------------------------
def _trace(variant, f16, fault=None, case=0):
  hp, gw, dw, real, z, alpha, shifts, B = _setup(case=case)
  with torch.no_grad():
    fake = O.generator_forward([torch.tensor(w) for w in gw],
                               torch.tensor(z, dtype=torch.float32), hp).numpy()
  real = real.astype(np.float32)
  alpha = alpha.astype(np.float32)
  ctx = LT.Ctx(hp, B, f16, **VARIANTS[variant])
  sim = LT.CriticSim(ctx, dw, real, fake, alpha, shifts, fault=fault)
  return ctx, sim.run()


@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'f16'])
@pytest.mark.parametrize('case', range(len(SHIFT_CASES)))
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_simulated_trace_passes(variant, case, f16):
  ctx, events = _trace(variant, f16, case=case)
  ratios = LT.Checker(ctx).run(events)
  assert ratios and max(ratios.values()) <= 1.0
  assert len(events) >= 20


FAULTS = [
    # (fault, variant, the stage the checker must name)
    (dict(wrong_shift_row=2), 'folded', 'fwd 2'),
    (dict(wrong_shift_row=4), 'side', 'fwd 4'),
    (dict(reflect_off=1), 'folded', 'fwd 1'),
    (dict(reflect_off=3), 'plain', 'fwd 3'),
    (dict(bias_rows_3B=1), 'folded', 'wgrad 0'),
    (dict(bias_rows_3B=4), 'plain', 'wgrad 3'),
    (dict(xhat_in_wgrad=True), 'folded', 'wgrad 0'),
    (dict(coef_missing=1), 'folded', 'jvp 0'),
    (dict(coef_missing=2), 'mix', 'gp_loss_scale'),
    (dict(pad_nonzero=1), 'folded', 'fwd 1'),
    (dict(pad_nonzero=4), 'side', 'fwd 4'),
    (dict(overwrite_other_segment=0), 'folded', 'jvp 0'),
    (dict(overwrite_other_segment=3), 'plain', 'jvp 3'),
]


@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'f16'])
@pytest.mark.parametrize('fault,variant,stage', FAULTS,
                         ids=['{}-{}'.format(list(f)[0], list(f.values())[0])
                              for f, _, _ in FAULTS])
def test_planted_fault_is_named(fault, variant, stage, f16):
  ctx, events = _trace(variant, f16, fault=fault)
  with pytest.raises(LT.StageError) as e:
    LT.Checker(ctx).run(events)
  assert e.value.stage == stage, str(e.value)


def test_unclaimed_launch_fails():
  ctx, events = _trace('folded', False)
  ev = dict(events[3])
  ev['role'] = ('call', 'cg_some_new_fusion')
  with pytest.raises(LT.StageError, match='unclaimed'):
    LT.Checker(ctx).run(events[:3] + [ev])


# ---------------------------------------------------------------------------
# generator update
# ---------------------------------------------------------------------------
GEN_NORMS = {'ln': dict(layer_norm=True), 'plain': dict(layer_norm=False),
             'bn': dict(layer_norm=False, batch_norm=True),
             'bn_ln': dict(layer_norm=True, batch_norm=True)}
GEN_FLAGS = dict(folded=(1, 2, 3))


def _gen_sim(norm, exact, f16=False, fused=False, defer=False, shape=None, **hpkw):
  hpkw = dict(GEN_NORMS[norm], **hpkw)
  hp, gw, dw, real, z, alpha, shifts, B = (
      _setup(case=2, **hpkw) if shape is None else
      case_inputs(SHAPES[shape], SEED + 1, shift_case(shape), **hpkw))
  ctx = LT.Ctx(hp, B, f16, nseg=1, exact=exact, **GEN_FLAGS)
  g = LT.GenCtx(hp, B, f16, exact=exact, ln_fused=[fused] * 5, defer=defer,
                Cf=-(-hp.num_channels // 8) * 8)
  if not exact:
    z = z.astype(np.float32)
  sim = LT.GenSim(ctx, g, gw, dw, z, shifts[:, 1])
  return hp, gw, dw, z, shifts[:, 1], ctx, g, sim


@pytest.mark.parametrize('norm,shape', [(n, None) for n in GEN_NORMS] + [('ln', 'k6_c40')],
                         ids=list(GEN_NORMS) + ['ln-k6_c40'])
def test_generator_closure(norm, shape):
  hp, gw, dw, z, sh, ctx, g, sim = _gen_sim(norm, True, fused=(norm == 'ln'), shape=shape)
  sim.run()
  res = O.g_step_grads(_t64(gw), _t64(dw), torch.tensor(z), sh, hp)
  got = LT.gen_grads(sim)
  assert len(got) == len(res['grads'])
  for i, (a, w) in enumerate(zip(got, res['grads'])):
    w = w.numpy()
    if np.abs(w).max() <= 1e-13 * max(1.0, np.abs(a).max()):
      # (BatchNormalization removes the column mean: the conv bias gradient is
      # zero up to float64 rounding; the moving statistics take none)
      assert np.abs(a).max() <= 1e-12, (i, np.abs(a).max())
    else:
      assert _relmax(a, w) <= 1e-12, (i, _relmax(a, w))
  assert _relmax(sim.st['gen_loss'][0], float(res['loss'])) <= 1e-12
  assert _relmax(sim.st['G.fake'][:, :, :g.C], res['fake'].numpy()) <= 1e-12


@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'f16'])
@pytest.mark.parametrize('norm,fused,defer,kw', [
    ('ln', True, True, {}), ('ln', False, False, {}), ('plain', False, False, {}),
    ('bn', False, False, {}), ('bn_ln', False, False, {}),
    ('ln', True, True, dict(normalize=False))])
def test_simulated_generator_trace_passes(norm, fused, defer, kw, f16):
  hp, gw, dw, z, sh, ctx, g, sim = _gen_sim(norm, False, f16, fused, defer, **kw)
  events = sim.run()
  ratios = LT.GenChecker(ctx, g).run(events)
  assert ratios and max(ratios.values()) <= 1.0


def test_f16_loss_scale_keeps_stored_values_in_range():
  """layer_trace.F16_SCALE_TINY, the loss scale of the GPU case tiny-scale (same
  weights and draws: test_hip_layers._build): under it no value the float64
  reference stores in the activation type exceeds half the fp16 maximum; under
  twice the scale one would."""
  shape = SHAPES['tiny']

  def worst(S):
    hp, gw, dw, real, z, alpha, shifts, B = case_inputs(shape, SEED, shift_case('tiny'))
    with torch.no_grad():
      fake = O.generator_forward([torch.tensor(w) for w in gw],
                                 torch.tensor(z, dtype=torch.float32), hp).numpy()
    ctx = LT.Ctx(hp, B, True, folded=(1, 2, 3), gin_in_x0=True, jvp_folds=True)
    ctx.scale = S
    sim = LT.CriticSim(ctx, dw, real.astype(np.float32), fake, alpha.astype(np.float32),
                       shifts)
    events = sim.run()
    LT.Checker(ctx).run(events)
    keys = [k for k in events[-1]['after']
            if k.split('.')[0] in ('x0', 'act', 'delta', 'e', 'side', 'gin')]
    return max(float(np.abs(ev['after'][k]).max()) for ev in events for k in keys)

  S = LT.F16_SCALE_TINY
  assert np.log2(S) == int(np.log2(S))
  assert worst(S) <= 65504.0 / 2
  assert worst(2 * S) > 65504.0 / 2


def test_stale_packed_operand_is_named():
  """The optimizer stages: Adam on the flat critic parameters, then the repack.
  A packed operand left one Adam step stale is named by the repack stage."""
  import pointwise_ref as R
  import wgrad_ref as W
  hp, gw, dw, real, z, alpha, shifts, B = _setup()
  ctx = LT.Ctx(hp, B, False)
  rng = np.random.RandomState(5)
  f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
  st = {'D.data': np.zeros(ctx.numel)}
  for i, w in enumerate(dw):
    st['D.data'][ctx.pslice(i)] = np.asarray(w, np.float64).reshape(-1)
  st['D.grad'] = f32(rng.randn(ctx.numel) * 1e-2)
  st['D.m'], st['D.v'] = np.zeros(ctx.numel), np.zeros(ctx.numel)
  lay = ctx.layers[1]
  # the forward operand of critic layer 2: (k, cin, cout) row-major, parity-major taps
  pd = W.PackDesc(ctx.k, lay.cin, lay.cout, lay.cinp, 32, 0, 1, lay.cin * lay.cout,
                  lay.cout, 1, 1, 0)
  descs = [('D.pack.1', ctx.offsets[2], [pd])]
  st['D.pack.1'] = W.pack(st['D.data'][ctx.offsets[2]:], pd, False)
  lr_t = float(R.adam_lr_t(1e-4, 0.9, 0.999, 1))

  def trace(stale):
    s = {k: v.copy() for k, v in st.items()}
    events = []
    for role, info in ((('adam', 'D'), dict(lr_t=lr_t)), (('pack', 'D'), dict(descs=descs))):
      before = {k: v.copy() for k, v in s.items()}
      if role[0] == 'adam':
        for o in LT.stage_adam(ctx, s, 'D', lr_t):
          s[o['key']] = f32(o['want'])
      elif not stale:
        for o in LT.stage_pack(ctx, s, 'D', descs):
          s[o['key']] = o['want']
      events.append(dict(role=role, before=before,
                         after={k: v.copy() for k, v in s.items()}, **info))
    return events

  LT.Checker(ctx).run(trace(False))
  with pytest.raises(LT.StageError) as e:
    LT.Checker(ctx).run(trace(True))
  assert e.value.stage == 'pack D'


def _gen_backward_worst(case, S):
  """Largest magnitude the float64 reference stores in an activation-typed
  gradient buffer of the fp16 generator update `case` under loss scale S."""
  shape, hpkw, _ = GEN_CASES[case]
  hp, gw, dw, real, z, alpha, shifts, B = case_inputs(SHAPES[shape], SEED + 1,
                                                      shift_case(case), **hpkw)
  ctx = LT.Ctx(hp, B, True, nseg=1, folded=(1, 2, 3))
  ctx.scale = S
  g = LT.GenCtx(hp, B, True, Cf=LT.pitch(hp.num_channels))
  events = LT.GenSim(ctx, g, gw, dw, z.astype(np.float32), shifts[:, 1]).run()
  last = events[-1]['after']
  keys = [k for k in last if k.split('.')[0] in ('delta', 'e', 'gin') or
          k.split('.')[:2] in (['G', 'dz'], ['G', 'dh'], ['G', 'dy'], ['G', 'dybn'])]
  return max(float(np.abs(last[k]).max()) for k in keys)


@pytest.mark.parametrize('case', list(GEN_CASES))
def test_f16_generator_loss_scales_keep_gradients_in_range(case):
  """layer_trace.F16_GEN_SCALE[case]: a power of two under which no gradient the
  float64 reference stores exceeds half the fp16 maximum, and twice which would
  (the gradients are linear in the scale)."""
  S = LT.F16_GEN_SCALE[case]
  assert np.log2(S) == int(np.log2(S))
  worst = _gen_backward_worst(case, S)
  assert worst <= 65504.0 / 2 < 2 * worst
