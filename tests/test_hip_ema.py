"""GPU tests of --ema_decay: cg_ema_update against averaging.update_statement
bit for bit (every path of the kernel: 16-byte and scalar, tails, more than one
pass of its bounded grid), its refusals, and the layers above it -- the train
steps of both algorithms and both model families leave the trajectory alone
and the shadow on the host recurrence, the contents swap of
averaged_generator(), checkpoints, and main.py end to end.

Bits are compared with tobytes().  Where a result is NaN the sign and payload
are not compared: IEEE 754 leaves them open, and the host's x86 default NaN
(sign set) is not the device's (sign clear); NaNs must stand in the same places
and every other element must have the same bits."""
import glob
import json
import os
import pickle

import numpy as np
import pytest
import torch

import main as cli
import oracle as O
from calciumgan_amd import _lib
from calciumgan_amd.data import dg
from calciumgan_amd.gan.algorithms import averaging as A
from calciumgan_amd.gan.algorithms import get_algorithm
from calciumgan_amd.gan.models import get_models
from calciumgan_amd.gan.utils import dataset_helper, utils
from test_mlp_host import make_hparams as mlp_hparams

pytestmark = pytest.mark.gpu

# the kernel's grid is bounded at kEmaMaxBlocks = 2048 blocks of 256 threads
# (csrc/pointwise.hip): one pass covers 2048 * 256 quads on the 16-byte path
# and 2048 * 256 elements on the scalar path
ONE_PASS_VEC = 2048 * 256 * 4
ONE_PASS_SCALAR = 2048 * 256
N_PAST_ONE_PASS = ONE_PASS_VEC + 5
SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 4099, N_PAST_ONE_PASS]
# (ema, p) offsets in floats from a 16-byte boundary: separately and together
OFFSETS = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 1),
           (2, 2), (3, 3)]
OMS = [0.0, 0.001, 0.9, 1.0]
SENTINEL = np.float32(-7.25)


@pytest.fixture(autouse=True)
def _bf16_build():
  _lib.use('bf16')
  yield
  _lib.use('bf16')


def _same_bits(got, want):
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
  nan = np.isnan(want)
  if not nan.any():
    return got.tobytes() == want.tobytes()
  return (np.array_equal(np.isnan(got), nan) and
          got[~nan].tobytes() == want[~nan].tobytes())


def _launch(e, p, n, om, e_off=0, p_off=0, guard=8):
  """The kernel on copies of e / p placed e_off / p_off floats past a 16-byte
  boundary inside sentinel-filled buffers; returns (ema after, p after) and
  checks that nothing outside [0, n) was written."""
  be = torch.full((e_off + n + guard,), float(SENTINEL), dtype=torch.float32,
                  device='cuda')
  bp = torch.full((p_off + n + guard,), float(SENTINEL), dtype=torch.float32,
                  device='cuda')
  assert be.data_ptr() % 16 == 0 and bp.data_ptr() % 16 == 0
  ve, vp = be[e_off:e_off + n], bp[p_off:p_off + n]
  ve.copy_(torch.from_numpy(e))
  vp.copy_(torch.from_numpy(p))
  _lib.call('cg_ema_update', ve, vp, n, float(om), _lib.stream())
  torch.cuda.synchronize()
  he, hp = be.cpu().numpy(), bp.cpu().numpy()
  assert (he[:e_off] == SENTINEL).all() and (he[e_off + n:] == SENTINEL).all()
  assert hp[p_off:p_off + n].tobytes() == p.tobytes()
  assert (hp[:p_off] == SENTINEL).all() and (hp[p_off + n:] == SENTINEL).all()
  return he[e_off:e_off + n]


def _inputs(n, seed):
  rng = np.random.RandomState(seed)
  e = (rng.standard_normal(n) * np.exp(rng.uniform(-6, 6, n))).astype(np.float32)
  p = (rng.standard_normal(n) * np.exp(rng.uniform(-6, 6, n))).astype(np.float32)
  k = n // 3
  p[:k] = e[:k]  # (e == p stays e)
  return e, p


@pytest.mark.parametrize('n', SIZES)
def test_kernel_is_the_statement_bit_for_bit(n):
  e, p = _inputs(n, seed=n % 1000)
  # (the references once per om; every alignment sees the same values)
  want = {om: A.update_statement(e, p, np.float32(om)) for om in OMS}
  assert want[0.0].tobytes() == e.tobytes()
  for e_off, p_off in OFFSETS:
    for om in OMS:
      got = _launch(e, p, n, om, e_off, p_off)
      assert got.tobytes() == want[om].tobytes(), (n, e_off, p_off, om)


def test_sizes_cover_more_than_one_pass_of_the_grid():
  assert N_PAST_ONE_PASS > ONE_PASS_VEC > ONE_PASS_SCALAR
  assert N_PAST_ONE_PASS % 4  # (and a scalar tail behind the quads)


@pytest.mark.parametrize('offsets', [(0, 0), (1, 0), (0, 2), (3, 3)])
@pytest.mark.parametrize('om', OMS)
def test_special_values_at_known_places(om, offsets):
  inf, nan, tiny = np.inf, np.nan, 1e-45
  sub = 1e-39  # (a float32 denormal)
  specials = [(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (tiny, tiny),
              (tiny, 0.0), (3 * tiny, tiny), (sub, -sub), (-sub, 1.0),
              (1.0, sub), (inf, 1.0), (1.0, inf), (-inf, 1.0), (1.0, -inf),
              (inf, inf), (inf, -inf), (-inf, -inf), (nan, 1.0), (1.0, nan),
              (nan, nan), (nan, inf), (3.0e38, -3.0e38), (-3.0e38, 3.0e38)]
  n = 4099
  e, p = _inputs(n, seed=7)
  # at the head (the quads of the 16-byte path), in the middle and in the tail
  for start in (0, 2001, n - len(specials)):
    for i, (a, b) in enumerate(specials):
      e[start + i], p[start + i] = a, b
  want = A.update_statement(e, p, np.float32(om))
  got = _launch(e, p, n, om, *offsets)
  assert _same_bits(got, want)
  # what the statement promises, on the device's own output
  at = lambda i: got[2001 + i]
  assert not np.signbit(at(0)) and np.signbit(at(1))
  assert at(4) == np.float32(tiny) and at(4) != 0  # denormals are kept
  assert np.isnan(at(14)) and np.isnan(at(17)) and np.isnan(at(18))
  if om > 0:
    assert at(11) == np.float32(inf) and at(13) == np.float32(-inf)
    assert np.isnan(at(10)) and np.isnan(at(12))


def test_refusals_write_nothing():
  n = 64
  e = torch.full((n,), float(SENTINEL), dtype=torch.float32, device='cuda')
  p = torch.full((n,), 3.0, dtype=torch.float32, device='cuda')
  s = _lib.stream()
  for args in [(None, p, n, 0.5), (e, None, n, 0.5), (e, p, 0, 0.5),
               (e, p, -1, 0.5), (e, p, n, -0.001), (e, p, n, 1.001),
               (e, p, n, float('nan')), (e, p, n, float('inf'))]:
    with pytest.raises(ValueError, match='CG_EINVAL'):
      _lib.call('cg_ema_update', *args, s)
  torch.cuda.synchronize()
  assert (e.cpu().numpy() == SENTINEL).all() and (p.cpu().numpy() == 3.0).all()


def test_two_calls_on_equal_inputs_give_equal_bits():
  n = N_PAST_ONE_PASS
  e, p = _inputs(n, seed=3)
  a = _launch(e, p, n, 0.1, 0, 0)
  b = _launch(e, p, n, 0.1, 0, 0)
  c = _launch(e, p, n, 0.1, 1, 2)
  assert a.tobytes() == b.tobytes() == c.tobytes()


# -- the train steps ------------------------------------------------------------
DECAY = 0.9
B = 4


def _conv_hparams(algorithm='wgan-gp', **kw):
  hp = O.make_hparams(64, 6, 8, m=2, **kw)
  hp.n_critic = 2
  hp.algorithm = algorithm
  hp.verbose = 0
  return hp


def _gan(hp, ema):
  if ema:
    hp = type(hp)(**vars(hp))
    hp.ema_decay = DECAY
  gen, dis = get_models(hp, None)
  return get_algorithm(hp, gen, dis, None)


def _flat(gan):
  return gan.generator.net.params.data.cpu().numpy().copy()


def _weights_bytes(model):
  return [w.tobytes() for w in model.get_weights()]


def _out_bytes(out):
  g, d, gp, metrics = out
  vals = [g, d] + ([] if gp is None else [gp]) + [metrics[k] for k in sorted(metrics)]
  return torch.stack([v.float() for v in vals]).cpu().numpy().tobytes()


def _recurrence(shadow, weights, t0=0):
  """The host statement over the generator's flat buffers after each call."""
  s = shadow.copy()
  for t, w in enumerate(weights, start=t0):
    s = A.update_statement(s, w, A.one_minus(A.decay_at(DECAY, t)))
  return s


def _batch(seed=0, shape=(B, 64, 6)):
  return np.random.RandomState(seed).uniform(0, 1, shape).astype(np.float32)


def _lockstep(control, averaged, real, calls):
  """`calls` train() on both objects; (a) outputs and both models' weights
  equal bit for bit after every call, (b) the shadow on the host recurrence.
  Returns the generator's flat buffer after each call."""
  avg = averaged.average
  assert control.average is None and avg is not None
  start, t0 = avg.shadow.cpu().numpy().copy(), avg.updates
  seen = []
  for k in range(calls):
    oc, oa = control.train(real), averaged.train(real)
    torch.cuda.synchronize()
    assert _out_bytes(oc) == _out_bytes(oa), k
    for mc, ma in ((control.generator, averaged.generator),
                   (control.discriminator, averaged.discriminator)):
      assert _weights_bytes(mc) == _weights_bytes(ma), k
    seen.append(_flat(averaged))
    assert avg.updates == t0 + k + 1
    assert _same_bits(avg.shadow.cpu().numpy(), _recurrence(start, seen, t0)), k
  return seen


CONV = {'wgan_gp_ln': ('wgan-gp', {}),
        'wgan_gp_bn': ('wgan-gp', dict(layer_norm=False, batch_norm=True)),
        'gan_ln': ('gan', {})}


@pytest.mark.parametrize('case', sorted(CONV))
def test_conv_step_trajectory_is_untouched_and_the_shadow_is_the_recurrence(case):
  algorithm, kw = CONV[case]
  hp = _conv_hparams(algorithm, **kw)
  control, averaged = _gan(hp, False), _gan(hp, True)
  params = averaged.generator.net.params
  assert averaged.average.shadow.numel() == params.numel
  seen = _lockstep(control, averaged, _batch(), 5)
  # two eager warm-up calls, then replays
  st = averaged._get_state(B)
  assert st['calls'] == 5 and st.get('graph') is not None
  assert averaged._use_graph
  # the weights moved, and the shadow trails them
  assert seen[0].tobytes() != seen[-1].tobytes()
  shadow = averaged.average.shadow.cpu().numpy()
  assert shadow.tobytes() != seen[-1].tobytes()
  # get_weights(): Keras order, the views of the flat shadow; padding stays 0
  got = averaged.average.get_weights()
  sizes = [int(np.prod(s)) for s in params.shapes]
  covered = np.zeros(params.numel, bool)
  for w, o, n, s in zip(got, params.offsets, sizes, params.shapes):
    assert w.shape == tuple(s) and w.tobytes() == shadow[o:o + n].tobytes()
    covered[o:o + n] = True
  assert (shadow[~covered] == 0).all()
  if kw.get('batch_norm'):
    # the moving statistics (frozen entries) are averaged like the rest
    assert params.frozen
    for i in params.frozen:
      o, n = params.offsets[i], sizes[i]
      assert seen[0][o:o + n].tobytes() != seen[-1][o:o + n].tobytes()
      assert shadow[o:o + n].tobytes() != seen[-1][o:o + n].tobytes()


def test_mlp_step_shadow_is_the_recurrence():
  hp = mlp_hparams(L=6, C=2, noise_dim=32, num_units=32, n_critic=2)
  control, averaged = _gan(hp, False), _gan(hp, True)
  real = _batch(1, (3, 6, 2))
  seen = _lockstep(control, averaged, real, 3)
  assert seen[0].tobytes() != seen[-1].tobytes()


# -- the swap --------------------------------------------------------------------
def test_averaged_generator_swaps_contents_and_gives_them_back():
  hp = _conv_hparams()
  control, averaged = _gan(hp, False), _gan(hp, True)
  real = _batch()
  _lockstep(control, averaged, real, 5)
  avg, net = averaged.average, averaged.generator.net
  z = torch.randn(B, hp.noise_dim, generator=torch.Generator().manual_seed(5))
  raw = _weights_bytes(averaged.generator)
  ptr = net.params.data.data_ptr()
  shadow = [w.tobytes() for w in avg.get_weights()]
  assert raw != shadow
  with averaged.averaged_generator() as inside:
    assert inside is avg
    assert _weights_bytes(averaged.generator) == shadow
    fake = averaged.generate(z).cpu().numpy()
  fresh, _ = get_models(hp, None)
  fresh.set_weights(avg.get_weights())
  want = fresh(z, training=False).cpu().numpy()
  assert fake.tobytes() == want.tobytes()
  assert fake.tobytes() != averaged.generate(z).cpu().numpy().tobytes()
  assert _weights_bytes(averaged.generator) == raw
  assert net.params.data.data_ptr() == ptr
  assert [w.tobytes() for w in avg.get_weights()] == shadow
  # the packed operands came back too: the next replay is the control's
  _lockstep(control, averaged, real, 1)
  # an exception inside restores the same way
  raw = _weights_bytes(averaged.generator)
  with pytest.raises(RuntimeError, match='inside'):
    with averaged.averaged_generator():
      assert _weights_bytes(averaged.generator) != raw
      raise RuntimeError('inside')
  assert _weights_bytes(averaged.generator) == raw
  _lockstep(control, averaged, real, 1)
  # averaging off: a null context
  with control.averaged_generator() as nothing:
    assert nothing is None


# -- checkpoints ------------------------------------------------------------------
OLD_KEYS = {'epoch', 'gen_weights', 'dis_weights', 'gen_steps', 'dis_steps'}


def _ckpt_hparams(tmp_path, name, ema):
  hp = _conv_hparams()
  hp.ckpt_dir = str(tmp_path / name)
  hp.output_dir = str(tmp_path)
  if ema:
    hp.ema_decay = DECAY
  return hp


def _load_pickle(hp):
  files = sorted(glob.glob(os.path.join(hp.ckpt_dir, 'epoch-*.pkl')))
  assert len(files) == 1
  with open(files[0], 'rb') as f:
    return pickle.load(f)


def test_checkpoint_round_trip_resumes_the_shadow(tmp_path):
  """The checkpoint format carries neither Adam's moments nor the random
  streams (as before this flag): to compare a sixth step with the uninterrupted
  run's, the test copies the moments over and injects the same draws on both
  sides."""
  hp = _ckpt_hparams(tmp_path, 'ema', True)
  first = _gan(hp, False)
  real = _batch()
  for _ in range(5):
    first.train(real)
  utils.save_models(hp, first, 0)
  ck = _load_pickle(hp)
  assert set(ck) == OLD_KEYS | {'gen_ema_weights', 'ema_updates'}
  assert ck['ema_updates'] == 5
  assert [w.tobytes() for w in ck['gen_ema_weights']] == [
      w.tobytes() for w in first.average.get_weights()]
  assert [w.tobytes() for w in ck['gen_weights']] == _weights_bytes(first.generator)

  resumed = _gan(hp, False)
  utils.load_models(hp, resumed)
  assert hp.start_epoch == 1
  assert resumed.average.updates == 5
  assert (resumed.average.shadow.cpu().numpy().tobytes() ==
          first.average.shadow.cpu().numpy().tobytes())
  for a, b in ((first.generator, resumed.generator),
               (first.discriminator, resumed.discriminator)):
    assert _weights_bytes(a) == _weights_bytes(b)
    b.net.params.m.copy_(a.net.params.m)
    b.net.params.v.copy_(a.net.params.v)
  rand = O.draw_randomness(hp, B, seed=3)
  first.train(real, rand)
  resumed.train(real, rand)
  torch.cuda.synchronize()
  assert _weights_bytes(first.generator) == _weights_bytes(resumed.generator)
  assert first.average.updates == resumed.average.updates == 6
  assert (resumed.average.shadow.cpu().numpy().tobytes() ==
          first.average.shadow.cpu().numpy().tobytes())


def test_checkpoints_across_the_flag(tmp_path):
  # written without the flag: exactly the old keys
  plain_hp = _ckpt_hparams(tmp_path, 'plain', False)
  plain = _gan(plain_hp, False)
  real = _batch()
  for _ in range(2):
    plain.train(real)
  utils.save_models(plain_hp, plain, 3)
  assert set(_load_pickle(plain_hp)) == OLD_KEYS
  # flag on, keys absent: the shadow is the loaded weights, no update counted
  on_hp = _ckpt_hparams(tmp_path, 'plain', True)
  on = _gan(on_hp, False)
  on.train(real)  # (a shadow and a count of its own to be replaced)
  assert on.average.updates == 1
  utils.load_models(on_hp, on)
  assert on_hp.start_epoch == 4 and on.average.updates == 0
  assert _weights_bytes(on.generator) == _weights_bytes(plain.generator)
  assert [w.tobytes() for w in on.average.get_weights()] == _weights_bytes(
      plain.generator)
  # flag off, keys present: ignored, and what is written has the old keys
  ema_hp = _ckpt_hparams(tmp_path, 'with_keys', True)
  utils.save_models(ema_hp, on, 0)
  assert 'gen_ema_weights' in _load_pickle(ema_hp)
  off_hp = _ckpt_hparams(tmp_path, 'with_keys', False)
  off = _gan(off_hp, False)
  utils.load_models(off_hp, off)
  assert off.average is None and off_hp.start_epoch == 1
  assert _weights_bytes(off.generator) == _weights_bytes(on.generator)
  off_hp.ckpt_dir = str(tmp_path / 'rewritten')
  utils.save_models(off_hp, off, 1)
  assert set(_load_pickle(off_hp)) == OLD_KEYS


# -- main.py ------------------------------------------------------------------------
# wall-clock scalars of the training writer: different in any two runs
_TIMED = ('elapse', 'samples_per_sec')


def _args(input_dir, output_dir, *extra):
  a = cli.build_parser().parse_args([
      '--input_dir', input_dir, '--output_dir', output_dir, '--model',
      'calciumgan', '--algorithm', 'wgan-gp', '--batch_size', '8', '--num_units',
      '8', '--m', '2', '--layer_norm', '--epochs', '2', '--n_critic', '2',
      '--save_generated', 'last', '--verbose', '0'] + list(extra))
  a.global_step = 0
  a.surrogate_ds = False
  return a


def _scalars(path):
  return [json.loads(l) for l in open(path)]


def test_main_with_and_without_the_flag(tmp_path, monkeypatch):
  d = dg.make_dataset(num_neurons=6, sequence_length=64, num_segments=40)
  info = {k: v for k, v in d['info'].items() if k != 'rates_hz'}
  ds = str(tmp_path / 'ds')
  dataset_helper.write_dataset(ds, d['signals'], d['spikes'], info,
                               validation_size=8)
  launches = []
  call = _lib.call

  def counting(name, *args):
    launches.append(name)
    return call(name, *args)

  monkeypatch.setattr(_lib, 'call', counting)
  plain_dir, ema_dir = str(tmp_path / 'plain'), str(tmp_path / 'ema')
  plain_hp = _args(ds, plain_dir)
  cli.main(plain_hp)
  assert launches and launches.count('cg_ema_update') == 0
  del launches[:]
  ema_hp = _args(ds, ema_dir, '--ema_decay', '0.9')
  cli.main(ema_hp)
  # 32 training segments / batch 8: 4 train() per epoch, one update each
  assert plain_hp.global_step == ema_hp.global_step == 8
  assert launches.count('cg_ema_update') == 8

  def training(run):
    return [(r['tag'], r['step'], r['value'])
            for r in _scalars(os.path.join(run, 'scalars.jsonl'))
            if not r['tag'].startswith(_TIMED)]

  tp, te = training(plain_dir), training(ema_dir)
  assert len(tp) >= 4 and tp == te
  # validation ran on the averaged generator: other figures
  va = lambda run: [r['value'] for r in _scalars(
      os.path.join(run, 'validation', 'scalars.jsonl'))
                    if r['tag'] == 'signals_metrics/mean']
  assert len(va(plain_dir)) == 2 and va(plain_dir) != va(ema_dir)
  hp_p = json.load(open(os.path.join(plain_dir, 'hparams.json')))
  hp_e = json.load(open(os.path.join(ema_dir, 'hparams.json')))
  assert 'ema_decay' not in hp_p and hp_e.pop('ema_decay') == 0.9
  # (paths under the runs' own output directories aside)
  rel = lambda hp, run: {k: v.replace(run, '<run>') if isinstance(v, str) else v
                         for k, v in hp.items()}
  assert rel(hp_p, plain_dir) == rel(hp_e, ema_dir)
  cp = pickle.load(open(os.path.join(plain_dir, 'checkpoints', 'epoch-001.pkl'),
                        'rb'))
  ce = pickle.load(open(os.path.join(ema_dir, 'checkpoints', 'epoch-001.pkl'),
                        'rb'))
  assert set(cp) == OLD_KEYS
  assert set(ce) == OLD_KEYS | {'gen_ema_weights', 'ema_updates'}
  assert ce['ema_updates'] == 8
  # the same raw weights in both; the average is another set
  for k in ('gen_weights', 'dis_weights'):
    assert [w.tobytes() for w in cp[k]] == [w.tobytes() for w in ce[k]]
  assert [w.tobytes() for w in ce['gen_ema_weights']] != [
      w.tobytes() for w in ce['gen_weights']]
