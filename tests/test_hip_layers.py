"""Launch-by-launch float64 parity of the critic update, the generator update,
validate(), a whole train() and an --algorithm gan step on the GPU, in both
precision builds: one eager wgan_gp._critic_compute / _gen_compute / validate /
train is traced
(tests/layer_trace.py) and every launch is held against float64 arithmetic on
the buffers it read (tests/layer_ref.py) -- values within one storage ulp plus
the f32 accumulation bound, everything it does not declare bit-identical, pad
channels zero, and no launch unclaimed.

CALCIUMGAN_LAYER_PARITY_OUT=<file.jsonl>: every case appends its worst
error / bound per stage (profiles/layer_parity.txt is made from it)."""
import json
import os

import numpy as np
import pytest
import torch

import oracle as O

import layer_trace as LT
from test_hip_pointwise import _back_to_bf16, precision  # noqa: F401 (fixtures)
from test_layer_ref import GEN_CASES, SEED, SHAPES, case_inputs, shift_case

pytestmark = pytest.mark.gpu

# name -> (shape, {(module, attribute): value} set before the model is built)
CRITIC_CASES = {n: (n, {}) for n in SHAPES if n not in ('mid', 'l6144')}
for _n in ('tiny', 'long'):
  CRITIC_CASES[_n + '-mix'] = (_n, {('nets', '_L1_LINEAR_MIN_ROWS'): 0})
for _n in ('tiny', 'odd_c'):
  for _mod, _flag in (('nets', '_FOLD_FIXUP'), ('nets', '_FUSE_UNSHUFFLE'),
                      ('nets', '_FOLD_SCALE'), ('wgan_gp', '_FUSE_GP')):
    CRITIC_CASES['{}-no{}'.format(_n, _flag.lower())] = (_n, {(_mod, _flag): False})


def _build(case, f16, monkeypatch, scale=1.0):
  from calciumgan_amd import nets
  from calciumgan_amd.gan.algorithms import get_algorithm, wgan_gp
  from calciumgan_amd.gan.models import get_models
  shape, flags = CRITIC_CASES[case]
  for (mod, attr), v in flags.items():
    monkeypatch.setattr({'nets': nets, 'wgan_gp': wgan_gp}[mod], attr, v)
  assert nets.DETERMINISTIC
  hp, gw, dw, real, z, alpha, sh, B = case_inputs(SHAPES[shape], SEED, shift_case(case))
  hp.verbose = 0
  hp.mixed_precision = bool(f16)
  gen, dis = get_models(hp, None)
  gan = get_algorithm(hp, gen, dis, None)
  gen.set_weights(gw)
  dis.set_weights(dw)
  if f16:
    gan.dis_optimizer.loss_scale_state[0] = scale
    gan.gen_optimizer.loss_scale_state[0] = scale
  sh = sh.astype(np.int32)  # (4, 3), hand-built
  r = dict(z=z.astype(np.float32), alpha=alpha.astype(np.float32),
           shifts_real=sh[:, 0], shifts_fake=sh[:, 1], shifts_inter=sh[:, 2])
  return hp, gan, real.astype(np.float32), r, B


def _record(case, f16, ratios):
  path = os.environ.get('CALCIUMGAN_LAYER_PARITY_OUT')
  if path:
    with open(path, 'a') as f:
      f.write(json.dumps(dict(case=case, build='f16' if f16 else 'bf16',
                              ratios=ratios)) + '\n')


def _assert_staged(ev, shifts, coef, bias_coef):
  """The plan's shift table, seeds and bias seeds in front of its first launch
  equal the injected draws, segment by segment."""
  b = ev['before']
  np.testing.assert_array_equal(b['shifts'], np.asarray(shifts, np.float64))
  f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
  np.testing.assert_array_equal(b['coef'], f32(coef))
  np.testing.assert_array_equal(b['bias_coef'], f32(bias_coef))


def _trace_critic(case, f16, monkeypatch, scale=1.0, apply=False):
  hp, gan, real, r, B = _build(case, f16, monkeypatch, scale)
  real_d = gan._to_device(real)
  fake = gan._critic_generate(real_d, r)  # G(z): the generator cases trace it
  torch.cuda.synchronize()
  st = gan._get_state(B)
  tr = LT.Tracer(gan, B)
  with monkeypatch.context() as mp:
    tr.install(mp)
    gan._critic_compute(real_d, r, fake=fake)
    if apply:  # the optimizer update and the repack behind it
      gan._critic_apply()
    torch.cuda.synchronize()
  ctx = LT.Ctx(hp, B, f16, real=real, mix=r['alpha'], **LT.plan_flags(st['critic']))
  if f16:
    ctx.scale = scale
  S = np.float32(scale if f16 else 1.0)
  one = np.float32(1.0) / np.float32(B)
  first = [e for e in tr.events if e['role'][0] == 'interp_pack'][0]
  _assert_staged(first, np.stack([r['shifts_real'], r['shifts_fake'],
                                  r['shifts_inter']], axis=1),
                 [-one * S, one * S, 1.0], [-one * S, one * S, 0.0])
  return ctx, tr.events, st


@pytest.mark.parametrize('case', list(CRITIC_CASES))
def test_critic_update(case, precision, monkeypatch, fixed_tiles):
  f16 = precision
  apply = case in ('tiny', 'odd_c')
  ctx, events, st = _trace_critic(case, f16, monkeypatch, apply=apply)
  ratios = LT.Checker(ctx).run(events)
  _record(case, f16, ratios)
  roles = [e['role'][0] for e in events]
  for need in ('interp_pack', 'head', 'gin', 'jvp', 'wgrads', 'head_wgrad'):
    assert need in roles, roles
  if apply:
    tail = ['grad_finite', 'adam_scaled', 'ls_update', 'pack'] if f16 else ['adam', 'pack']
    assert roles[-len(tail):] == tail, roles
    assert all(e['role'][1] == 'D' for e in events[-len(tail):])
  if f16:
    # the seeds carry the loss scale on the real and fake segments, not on x^
    B = ctx.B
    np.testing.assert_array_equal(
        events[0]['before']['coef'],
        np.array([-1.0 / B, 1.0 / B, 1.0], np.float32).astype(np.float64))


def test_critic_update_under_a_loss_scale(monkeypatch, fixed_tiles):
  """The f16 build with the power-of-two loss scale that
  tests/test_layer_ref.py shows to keep every stored value of this case below
  half the fp16 maximum."""
  from calciumgan_amd import _lib
  _lib.use('f16')
  S = LT.F16_SCALE_TINY
  ctx, events, st = _trace_critic('tiny', True, monkeypatch, scale=S)
  _record('tiny-scale', True, LT.Checker(ctx).run(events))
  B = ctx.B
  np.testing.assert_array_equal(
      events[0]['before']['coef'],
      (np.array([-1.0 / B, 1.0 / B, 1.0], np.float32) *
       np.array([S, S, 1.0], np.float32)).astype(np.float64))


def test_case_list_reaches_every_path(precision, monkeypatch, fixed_tiles):
  """From the plans: folded, side + fix-up, cg_unshuffle_mask, jvp_folds,
  norm_deferred and mixes_layer1 each true somewhere and false somewhere."""
  f16 = precision
  from calciumgan_amd import _lib
  seen = dict(folded=set(), sided=set(), masked=set(), jvp_folds=set(),
              norm_deferred=set(), mixes_layer1=set())
  classic_sided = set()  # m > 0, classic tiles only, side buffer + fix-up, nothing folded
  for case in CRITIC_CASES:
    with monkeypatch.context() as mp:
      hp, gan, real, r, B = _build(case, f16, mp)
      plan = gan._get_state(B)['critic']
      fl = LT.plan_flags(plan)
      tiles = [d.tile for d in plan.fwd] + [d.tile for _, d in plan.dgrad] + [
          plan.input_grad.tile]
      if (hp.m > 0 and all(t in _lib.TILES for t in tiles) and fl['sided'] and
          not fl['folded']):
        classic_sided.add(case)
        assert hp.kernel_size != 24, case
    seen['folded'].add(bool(fl['folded']))
    seen['sided'].add(bool(fl['sided']))
    seen['masked'].add(bool(set(range(1, 5)) - fl['folded'] - fl['sided']))
    for k in ('jvp_folds', 'norm_deferred', 'mixes_layer1'):
      seen[k].add(fl[k])
  assert seen['folded'] == {True, False}, seen
  assert True in seen['sided'] and True in seen['masked'], seen
  # the forms of every kernel size but 24: no software-pipelined tile anywhere in the
  # plan, the reflected rows through the side buffer and cg_unshuffle_fixup
  assert {'k6_c40', 'k12', 'k14_c102', 'k22_u24'} <= classic_sided, classic_sided
  assert seen['jvp_folds'] == {True, False}, seen
  assert seen['mixes_layer1'] == {True, False}, seen
  # (the f16 build never defers the norm: its loss scale multiplies the
  # coefficients between the two launches)
  assert seen['norm_deferred'] == ({False} if f16 else {True, False}), seen


# ---------------------------------------------------------------------------
# generator update
# ---------------------------------------------------------------------------
def _build_gen(case, f16, monkeypatch, scale=1.0):
  from calciumgan_amd import nets
  from calciumgan_amd.gan.algorithms import get_algorithm
  from calciumgan_amd.gan.models import get_models
  shape, hpkw, flags = GEN_CASES[case]
  for attr, v in flags.items():
    monkeypatch.setattr(nets, attr, v)
  assert nets.DETERMINISTIC
  hp, gw, dw, real, z, alpha, sh, B = case_inputs(SHAPES[shape], SEED + 1,
                                                  shift_case(case), **hpkw)
  hp.verbose = 0
  hp.mixed_precision = bool(f16)
  gen, dis = get_models(hp, None)
  gan = get_algorithm(hp, gen, dis, None)
  gen.set_weights(gw)
  dis.set_weights(dw)
  if f16:
    gan.dis_optimizer.loss_scale_state[0] = scale
    gan.gen_optimizer.loss_scale_state[0] = scale
  r = dict(z=z.astype(np.float32), shifts=sh.astype(np.int32)[:, 1])
  return hp, gan, real.astype(np.float32), r, B


def _generator_update(case, f16, monkeypatch, scale=1.0, tag='gen-'):
  hp, gan, real, r, B = _build_gen(case, f16, monkeypatch, scale)
  real_d = gan._to_device(real)
  st = gan._get_state(B)
  apply = case == 'tiny'
  tr = LT.GenTracer(gan, B)
  with monkeypatch.context() as mp:
    tr.install(mp)
    gan._gen_compute(real_d, r)
    if apply:  # the optimizer update and the repack behind it
      gan.gen_optimizer.update(gan.generator)
    torch.cuda.synchronize()
  ctx = LT.Ctx(hp, B, f16, nseg=1, **LT.plan_flags(st['gen']))
  if f16:
    ctx.scale = scale
  g = LT.GenCtx(hp, B, f16, z=r['z'], **LT.gen_flags(gan, B))
  ratios = LT.GenChecker(ctx, g).run(tr.events)
  _record(tag + case, f16, ratios)
  S = np.float32(scale if f16 else 1.0)
  first = [e for e in tr.events if e['role'][0] == 'cast_fake'][0]
  _assert_staged(first, np.asarray(r['shifts']).reshape(4, 1),
                 [-(np.float32(1.0) / np.float32(B)) * S], [0.0])
  roles = [e['role'][0] for e in tr.events]
  if apply:
    tail = ['grad_finite', 'adam_scaled', 'ls_update', 'pack'] if f16 else ['adam', 'pack']
    assert roles[-len(tail):] == tail, roles
    assert all(e['role'][1] == 'G' for e in tr.events[-len(tail):])
  return roles


@pytest.mark.parametrize('case', list(GEN_CASES))
def test_generator_update_under_a_loss_scale(case, monkeypatch, fixed_tiles):
  """The f16 build under the power-of-two loss scale that tests/test_layer_ref.py
  shows to keep this case's gradients below half the fp16 maximum: the bulk of the
  gradients is normal there and counts in gamma(K) sum |x| |w| at its own magnitude
  (layer_trace.operand_floor still lifts an entry that is subnormal)."""
  from calciumgan_amd import _lib
  _lib.use('f16')
  _generator_update(case, True, monkeypatch, LT.F16_GEN_SCALE[case], 'gen-scaled-')


@pytest.mark.parametrize('case', list(GEN_CASES))
def test_generator_update(case, precision, monkeypatch, fixed_tiles):
  roles = _generator_update(case, precision, monkeypatch)
  for need in ('g_cast_z', 'g_in', 'g_conv', 'g_out', 'cast_fake', 'head', 'neg_mean',
               'gin', 'g_out_wgrad', 'g_out_dgrad', 'g_dgrad', 'g_in_wgrad',
               'g_wgrads'):
    assert need in roles, roles


def test_generator_cases_reach_both_layernorm_forms(monkeypatch, fixed_tiles):
  seen = set()
  for case in GEN_CASES:
    with monkeypatch.context() as mp:
      hp, gan, real, r, B = _build_gen(case, False, mp)
      fused = list(LT.gen_flags(gan, B)['ln_fused'])
      seen |= set(fused)
      if case == 'l6144':  # 192, 384, 768, ... rows: only the first fit no 128-row tile
        assert fused == [False, True, True, True, True]
  assert seen == {True, False}


# ---------------------------------------------------------------------------
# validate()
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['tiny_bn', 'tiny_bn_ln'])
def test_validate(case, precision, monkeypatch, fixed_tiles):
  """validate() under BatchNormalization: the forward uses the MOVING statistics
  (the reference of cg_bn_apply takes them from the parameters), every launch is
  claimed, and no parameter, moment, moving statistic or packed operand changes."""
  f16 = precision
  hp, gan, real, r, B = _build_gen(case, f16, monkeypatch)
  shape = SHAPES[GEN_CASES[case][0]]
  _, _, _, _, _, alpha, sh, _ = case_inputs(shape, SEED + 1, shift_case(case),
                                            **GEN_CASES[case][1])
  sh = sh.astype(np.int32)
  rand = dict(z=r['z'], alpha=alpha.astype(np.float32), shifts_real=sh[:, 0],
              shifts_fake=sh[:, 1], shifts_inter=sh[:, 2])
  st = gan._get_state(B)
  tr = LT.GenTracer(gan, B, plan=st['critic'])
  with monkeypatch.context() as mp:
    tr.install(mp)
    gan.validate(real, rand)
    torch.cuda.synchronize()
  ctx = LT.Ctx(hp, B, f16, real=real, mix=rand['alpha'], **LT.plan_flags(st['critic']))
  if f16:
    ctx.scale = 1.0
  g = LT.GenCtx(hp, B, f16, z=r['z'], **LT.gen_flags(gan, B))
  g.keep, g.training = False, False
  ratios = LT.GenChecker(ctx, g).run(tr.events)
  _record('validate-' + case, f16, ratios)
  roles = [e['role'][0] for e in tr.events]
  assert 'g_bn_stats' not in roles and 'g_bn_apply' in roles and 'metrics' in roles
  assert not any(x in roles for x in ('jvp', 'wgrads', 'adam', 'pack')), roles
  first, last = tr.events[0]['before'], tr.events[-1]['after']
  for key in first:
    if key.split('.')[0] in ('G', 'D') and key.split('.')[1] in ('data', 'm', 'v',
                                                                  'pack'):
      assert LT.same(first[key], last[key]), key


# ---------------------------------------------------------------------------
# a whole eager train()
# ---------------------------------------------------------------------------
def test_whole_train(precision, monkeypatch, fixed_tiles):
  """One eager WGAN_GP.train() with n_critic = 2, every launch claimed: the batched
  G(z) whose output Dense writes [real | fake_k | x^_k] into x0(0) and x0(1)
  (cg_dense_rows_interp), update 0 on plan 0, Adam and repack, update 1 on its own
  plan (input buffer x0(1), stage words 12..23), Adam and repack, the generator
  update with its Adam and repack, the metrics and cg_step_outputs.  At odd_c:
  cg_dense_rows_interp needs a channel pitch of 128 or more (at `tiny`, pitch 32,
  train() packs through cg_interp_pack on plan 0 instead)."""
  from calciumgan_amd import nets
  from calciumgan_amd.gan.algorithms import get_algorithm
  from calciumgan_amd.gan.models import get_models
  f16, n = precision, 2
  assert nets.DETERMINISTIC
  hp, gw, dw, real, _, _, _, B = case_inputs(SHAPES['odd_c'], SEED + 2, 0, n_critic=n)
  hp.verbose = 0
  hp.mixed_precision = bool(f16)
  gen, dis = get_models(hp, None)
  gan = get_algorithm(hp, gen, dis, None)
  gen.set_weights(gw)
  dis.set_weights(dw)
  if f16:
    gan.dis_optimizer.loss_scale_state[0] = 1.0
    gan.gen_optimizer.loss_scale_state[0] = 1.0
  real = real.astype(np.float32)
  rng = np.random.RandomState(SEED + 3)
  from test_layer_ref import scaled_cases
  draws = [np.array(c, np.int32) for c in scaled_cases(hp.m)]
  z = lambda: rng.standard_normal((B, hp.noise_dim)).astype(np.float32)
  rand = dict(critic=[dict(z=z(), alpha=rng.uniform(0, 1, B).astype(np.float32),
                           shifts_real=draws[k][:, 0], shifts_fake=draws[k][:, 1],
                           shifts_inter=draws[k][:, 2]) for k in range(n)],
              gen=dict(z=z(), shifts=draws[2][:, 1]))
  st = gan._get_state(B)
  assert gan._can_fuse_interp(B, n)
  tr = LT.StepTracer(gan, B, n)
  with monkeypatch.context() as mp:
    tr.install(mp)
    gan.train(real, rand)
    torch.cuda.synchronize()
  events, spaces = tr.events, tr.spaces
  ctxs = [LT.Ctx(hp, B, f16, real=real, mix=rand['critic'][k]['alpha'], slot=k,
                 **LT.plan_flags(tr.plans['p{}'.format(k)])) for k in range(n)]
  ctx_gen = LT.Ctx(hp, B, f16, nseg=1, real=real, **LT.plan_flags(st['gen']))
  flags = LT.gen_flags(gan, B)
  gA = LT.GenCtx(hp, B, f16, z=rand['gen']['z'], **flags)
  gB = LT.GenCtx(hp, n * B, f16, z=np.concatenate([r['z'] for r in rand['critic']]),
                 **dict(flags, ln_fused=list(tr.gwss['GB'].ln_fused)))
  gB.keep = False
  for c in ctxs + [ctx_gen]:
    c.scale = 1.0 if f16 else None
  ckG = LT.GenChecker(ctx_gen, gA)
  checkers = {'GB': (LT.GenChecker(ctxs[0], gB), ['GB']), 'GA': (ckG, ['gen']),
              'gen': (ckG, ['gen'])}
  for k in range(n):
    checkers['p{}'.format(k)] = (LT.Checker(ctxs[k]), ['p{}'.format(k)])
  ratios = LT.run_step(events, spaces, checkers)
  _record('train-odd_c', f16, ratios)
  # coverage: the launches this case is about, in their order
  roles = [' '.join(str(x) for x in e['role'][:2]) if e['role'][0] in (
      'adam', 'adam_scaled', 'pack') else e['role'][0] for e in events]
  opt = 'adam_scaled' if f16 else 'adam'
  assert roles.count('g_out_interp') == 1 and 'interp_pack' not in roles
  assert roles.count(opt + ' D') == n and roles.count('pack D') == n
  assert roles.count(opt + ' G') == 1 and roles.count('pack G') == 1
  assert roles[-1] == 'g_step_outputs' and roles.count('metrics') == 1
  assert roles.count('head_wgrad') == n and roles.count('gin') == n + 1
  # the spaces in the order of the step, and each plan's staged draws
  order = []
  for e in events:
    if e.get('space') and (not order or order[-1] != e['space']):
      order.append(e['space'])
  assert order[:3] == ['GB', 'p0', 'p1'] and set(order[3:]) == {'GA', 'gen'}, order
  S = np.float32(1.0)
  one = np.float32(1.0) / np.float32(B)
  for k in range(n):
    sp = 'p{}'.format(k)
    first = [e for e in events if e.get('space') == sp][0]
    r = rand['critic'][k]
    b = LT.view(first['before'], spaces, [sp])
    _assert_staged(dict(before=b), np.stack([r['shifts_real'], r['shifts_fake'],
                                             r['shifts_inter']], axis=1),
                   [-one * S, one * S, 1.0], [-one * S, one * S, 0.0])
    # update k reads x0(k); update 0 leaves x0(1) alone
    assert spaces[sp]['x0'] == tr.x0_keys[k]
  x1 = tr.x0_keys[1]
  assert x1 != tr.x0_keys[0]
  for e in events:
    if e.get('space') == 'p0':
      assert LT.same(e['before'][x1], e['after'][x1])
  # update 1's shift table is stage words 12..23
  assert tr.plans['p1'].shifts.data_ptr() == st['stage_dev'].data_ptr() + 12 * 4


# ---------------------------------------------------------------------------
# --algorithm gan: one eager step
# ---------------------------------------------------------------------------
def test_gan_step(precision, monkeypatch, fixed_tiles):
  """One eager BCE step at `tiny`, every launch claimed: G forward, x0 = [fake |
  real], D's convolutions over 2B with head=False, cg_dense1_bce (logits, losses,
  both models' seeds), D's chain and weight gradients with the per-sample head_coef
  form, G's chain from its own seeds on the fake segment, the generator backward,
  the metrics, Adam and repack of D then G, cg_step_outputs."""
  from calciumgan_amd import nets
  from calciumgan_amd.gan.algorithms import get_algorithm
  from calciumgan_amd.gan.models import get_models
  f16 = precision
  assert nets.DETERMINISTIC
  hp, gw, dw, real, z, _, sh, B = case_inputs(SHAPES['tiny'], SEED + 4, 1)
  hp.verbose = 0
  hp.algorithm = 'gan'
  hp.mixed_precision = bool(f16)
  gen, dis = get_models(hp, None)
  gan = get_algorithm(hp, gen, dis, None)
  gen.set_weights(gw)
  dis.set_weights(dw)
  if f16:
    gan.dis_optimizer.loss_scale_state[0] = 4.0
    gan.gen_optimizer.loss_scale_state[0] = 2.0
  real = real.astype(np.float32)
  sh = sh.astype(np.int32)
  rand = dict(z=z.astype(np.float32), shifts_real=sh[:, 0], shifts_fake=sh[:, 1])
  st = gan._get_state(B)
  tr = LT.StepTracer(gan, B, 1)
  with monkeypatch.context() as mp:
    tr.install(mp)
    gan.train(real, rand)
    torch.cuda.synchronize()
  events, spaces = tr.events, tr.spaces
  ctx_dis = LT.Ctx(hp, B, f16, nseg=2, real=real, **LT.plan_flags(st['dis']))
  ctx_gen = LT.Ctx(hp, B, f16, nseg=1, real=real, **LT.plan_flags(st['gen']))
  g = LT.GenCtx(hp, B, f16, z=rand['z'], **LT.gen_flags(gan, B))
  ckG = LT.GenChecker(ctx_gen, g)
  checkers = {'GA': (ckG, ['gen']), 'gen': (ckG, ['gen']),
              'dis': (LT.GenChecker(ctx_dis, g), ['dis'])}
  ratios = LT.run_step(events, spaces, checkers)
  _record('gan-tiny', f16, ratios)
  roles = [' '.join(str(x) for x in e['role'][:2]) if e['role'][0] in (
      'adam', 'adam_scaled', 'pack') else e['role'][0] for e in events]
  opt = 'adam_scaled' if f16 else 'adam'
  for need in ('cast_fake', 'cast_real', 'bce', 'head_wgrad_samples', 'gin', 'metrics',
               opt + ' D', 'pack D', opt + ' G', 'pack G'):
    assert roles.count(need) == 1, (need, roles)
  assert 'head' not in roles and 'head_wgrad' not in roles and 'jvp' not in roles
  assert roles[-1] == 'g_step_outputs'
  assert roles.index(opt + ' D') < roles.index(opt + ' G')
  # the staged draws: D's plan [fake | real], G's plan the fake segment's
  first = events[0]['before']
  np.testing.assert_array_equal(first[spaces['dis']['shifts']],
                                np.stack([sh[:, 1], sh[:, 0]], axis=1).astype(np.float64))
  np.testing.assert_array_equal(first[spaces['gen']['shifts']],
                                sh[:, 1:2].astype(np.float64))
