"""GPU tests of `--model mlp` under WGAN-GP: one critic update, one generator
update and a whole train() against tests/mlp_oracle.py with the same noise,
alpha and masks on both sides (the masks are read back from the device through
cg_mlp_dropout_mask), validate / generate without masks, bitwise
reproducibility, and main.py end to end on a surrogate directory.

The bar is mlp_oracle.check_parity's: within 4 x the distance of the float32
oracle from the float64 one, per tensor (floor 1e-6)."""
import glob
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import main as cli
import mlp_oracle as M
from calciumgan_amd import _lib
from calciumgan_amd.gan.algorithms import get_algorithm
from calciumgan_amd.gan.algorithms.wgan_gp_mlp import MLP_WGAN_GP
from calciumgan_amd.gan.models import get_models, mlp
from calciumgan_amd.gan.utils import utils
from test_mlp_host import ROOT, make_hparams

pytestmark = pytest.mark.gpu

CASES = [dict(B=3, L=6, C=2, U=8, nd=5), dict(B=70, L=6, C=2, U=40, nd=5)]
IDS = ['B3_U8', 'B70_U40']
P = 0.5


@pytest.fixture(autouse=True)
def _bf16_build():
  _lib.use('bf16')
  yield


def _hp(case, **kw):
  return make_hparams(L=case['L'], C=case['C'], noise_dim=case['nd'],
                      num_units=case['U'], dropout=P, **kw)


def _gan(hp, randomise=True):
  gen, dis = get_models(hp, None)
  if randomise:
    # (zero biases and Glorot kernels are a mild test: every tensor random)
    rng = np.random.RandomState(11)
    for model in (gen, dis):
      model.set_weights([
          (rng.standard_normal(w.shape) * (0.3 if w.ndim == 1 else
                                           1.0 / np.sqrt(w.shape[0]))
           ).astype(np.float32) for w in model.get_weights()])
    # the critic's outputs away from zero: the compared losses are MEANS of them,
    # and the relative error of a mean of mixed-sign terms measures its
    # conditioning, not the kernels.  (With a head bias near 0 the generator
    # loss at B 70 was a mean of 0.046 over terms of mean magnitude 0.75,
    # condition 16: the float32 oracle's per-sample errors were 6.9e-6 of that
    # mean, i.e. 8e-7 expected in the mean of 70, and its own 1.4e-7 a lucky
    # draw that the device's 1.3e-6 was then held against.)
    w = dis.get_weights()
    w[9] = np.full(1, 2.0, np.float32)
    dis.set_weights(w)
  gan = get_algorithm(hp, gen, dis, None)
  assert isinstance(gan, MLP_WGAN_GP)
  return gan


def _device_mask(stream, shape, p):
  n = int(np.prod(shape))
  out = torch.empty(n, dtype=torch.uint8, device='cuda')
  _lib.call('cg_mlp_dropout_mask', out, n, mlp.DROPOUT_SEED, stream, p,
            _lib.stream())
  torch.cuda.synchronize()
  got = out.cpu().numpy().astype(bool)
  np.testing.assert_array_equal(
      got, mlp.dropout_keep_mask(mlp.DROPOUT_SEED, stream, n, p))
  return got.reshape(shape)


def _masks(record, n_d, case):
  """(masks_g, masks_d) of one update from the streams the device used."""
  _, g_streams, d_streams = record
  B, L, U = case['B'], case['L'], case['U']
  assert g_streams[0] is None and g_streams[4] is None and d_streams[4] is None
  mg = [_device_mask(s, (B, L, w), P)
        for s, w in zip(g_streams[1:4], (U, 2 * U, 3 * U))]
  md = [_device_mask(s, (n_d, L, w), P)
        for s, w in zip(d_streams[:4], (4 * U, 3 * U, 2 * U, U))]
  return mg, md


def _draws(case, seed, n_critic):
  rng = np.random.RandomState(seed)
  B, nd = case['B'], case['nd']
  f = lambda *s: rng.standard_normal(s).astype(np.float32)
  return dict(
      critic=[dict(z=f(B, nd), alpha=rng.uniform(0, 1, B).astype(np.float32))
              for _ in range(n_critic)],
      gen=dict(z=f(B, nd)))


def _real(case, seed=5):
  return np.random.RandomState(seed).uniform(
      0, 1, (case['B'], case['L'], case['C'])).astype(np.float32)


def _host(t):
  torch.cuda.synchronize()
  return t.detach().cpu().numpy()


def _oracles(hp, gan):
  gw, dw = gan.generator.get_weights(), gan.discriminator.get_weights()
  return (M.OracleMLPGAN(hp, gw, dw, torch.float64),
          M.OracleMLPGAN(hp, gw, dw, torch.float32))


def _cmp_list(name, dev, a64, a32):
  assert len(dev) == len(a64) == len(a32)
  for i, (d, x, y) in enumerate(zip(dev, a64, a32)):
    M.check_parity('{}[{}]'.format(name, i), _host(d) if torch.is_tensor(d) else d,
                   x.numpy().reshape(np.shape(d)), y.numpy().reshape(np.shape(d)))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_critic_update(case):
  hp = _hp(case)
  gan = _gan(hp)
  o64, o32 = _oracles(hp, gan)
  real = _real(case)
  r = _draws(case, 1, 1)['critic'][0]
  B = case['B']
  gan._critic_compute(gan._to_device(real), r, slot=0)
  st = gan._get_state(B)
  r['masks_g'], r['masks_d'] = _masks(gan.last_streams[-1], 3 * B, case)
  loss, gp = _host(st['loss'][0, 0]), _host(st['gp'][0])
  grads = [_host(g).copy() for g in gan.discriminator.net.params.grad_views]
  gan.dis_optimizer.update(gan.discriminator)
  a, b = o64.critic_update(real, r), o32.critic_update(real, r)
  tag = 'critic B{} '.format(B)
  M.check_parity(tag + 'loss', loss, a['loss'].numpy(), b['loss'].numpy())
  M.check_parity(tag + 'gp', gp, a['gp'].numpy(), b['gp'].numpy())
  M.check_parity(tag + 'gen_loss', _host(st['loss'][0, 1]),
                 a['gen_loss'].numpy(), b['gen_loss'].numpy())
  assert float(a['gp']) > 0
  _cmp_list(tag + 'grad', grads, a['grads'], b['grads'])
  _cmp_list(tag + 'weights', gan.discriminator.get_weights(), o64.dis, o32.dis)
  # the masks did their work: dropped elements are exactly zero
  h = _host(gan.discriminator.net.buffers(3 * B).h[0]).reshape(3 * B, case['L'], -1)
  assert (h[~r['masks_d'][0]] == 0).all() and (h[r['masks_d'][0]] != 0).any()


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_generator_update(case):
  hp = _hp(case)
  gan = _gan(hp)
  o64, o32 = _oracles(hp, gan)
  real = _real(case)
  r = _draws(case, 2, 0)['gen']
  B = case['B']
  fake = gan._gen_compute(gan._to_device(real), r)
  st = gan._get_state(B)
  r['masks_g'], r['masks_d'] = _masks(gan.last_streams[-1], B, case)
  loss = _host(st['gen_loss'][0])
  fake = _host(fake).copy()
  grads = [_host(g).copy() for g in gan.generator.net.params.grad_views]
  gan.gen_optimizer.update(gan.generator)
  a, b = o64.generator_update(real, r), o32.generator_update(real, r)
  tag = 'gen B{} '.format(B)
  M.check_parity(tag + 'loss', loss, a['loss'].numpy(), b['loss'].numpy())
  M.check_parity(tag + 'fake', fake.reshape(B, case['L'], case['C']),
                 a['fake'].numpy(), b['fake'].numpy())
  _cmp_list(tag + 'grad', grads, a['grads'], b['grads'])
  _cmp_list(tag + 'weights', gan.generator.get_weights(), o64.gen, o32.gen)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_whole_train_step(case):
  hp = _hp(case, n_critic=2)
  gan = _gan(hp)
  o64, o32 = _oracles(hp, gan)
  real = _real(case)
  rand = _draws(case, 3, 2)
  B = case['B']
  got = gan.train(real, rand)
  assert [k for k, _, _ in gan.last_streams] == ['critic', 'critic', 'gen']
  for rec, r in zip(gan.last_streams, rand['critic'] + [rand['gen']]):
    r['masks_g'], r['masks_d'] = _masks(rec, 3 * B if rec[0] == 'critic' else B,
                                        case)
  # every (model call, layer) has a stream of its own
  ids = [s for _, g, d in gan.last_streams for s in g + d if s is not None]
  assert len(ids) == len(set(ids)) == 3 * 7
  a, b = o64.train(real, rand), o32.train(real, rand)
  tag = 'train B{} '.format(B)
  for i, name in enumerate(('gen_loss', 'dis_loss', 'gp')):
    M.check_parity(tag + name, _host(got[i]), np.float64(a[i]), np.float64(b[i]))
  _cmp_list(tag + 'last critic grad',
            list(gan.discriminator.net.params.grad_views),
            o64.last['critic'][-1]['grads'], o32.last['critic'][-1]['grads'])
  _cmp_list(tag + 'gen grad', list(gan.generator.net.params.grad_views),
            o64.last['gen']['grads'], o32.last['gen']['grads'])
  _cmp_list(tag + 'dis weights', gan.discriminator.get_weights(), o64.dis,
            o32.dis)
  _cmp_list(tag + 'gen weights', gan.generator.get_weights(), o64.gen, o32.gen)
  assert gan.dis_optimizer.iterations == 2 and gan.gen_optimizer.iterations == 1
  metrics = got[3]
  want = M.O.signal_metrics(torch.as_tensor(real, dtype=torch.float64),
                            o64.last['gen']['fake'], 0.0, 1.0, True)
  for k, v in want.items():
    assert abs(float(metrics[k]) - float(v)) < 1e-5 * max(1.0, abs(float(v))), k


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_validate_and_generate_apply_no_dropout(case):
  hp = _hp(case)
  gan = _gan(hp)
  o64, o32 = _oracles(hp, gan)
  real = _real(case)
  r = _draws(case, 4, 1)['critic'][0]
  B = case['B']
  before = gan.discriminator.get_weights()
  got = gan.validate(real, r)
  assert all(s is None for _, g, d in gan.last_streams for s in g + d)
  a, b = o64.validate(real, r), o32.validate(real, r)
  tag = 'validate B{} '.format(B)
  M.check_parity(tag + 'fake', _host(got[0]), a[0].numpy(), b[0].numpy())
  for i, name in ((1, 'gen_loss'), (2, 'dis_loss'), (3, 'gp')):
    M.check_parity(tag + name, _host(got[i]), np.float64(a[i]), np.float64(b[i]))
  again = gan.validate(real, r)
  for x, y in zip(got[:4], again[:4]):
    assert np.array_equal(_host(x).view(np.int32), _host(y).view(np.int32))
  for x, y in zip(before, gan.discriminator.get_weights()):
    assert np.array_equal(x, y)
  # G(noise, training=False) and generate()
  w64 = [torch.as_tensor(w, dtype=torch.float64) for w in gan.generator.get_weights()]
  w32 = [torch.as_tensor(w) for w in gan.generator.get_weights()]
  z = torch.as_tensor(r['z'])
  f = lambda w, zz: M.generator_forward(w, zz, case['L'], hp.alpha, None, 1.0,
                                        True).numpy()
  out = gan.generator(r['z'], training=False)
  assert tuple(out.shape) == (B, case['L'], case['C'])
  M.check_parity('G(training=False) B{}'.format(B), _host(out),
                 f(w64, z.double()), f(w32, z))
  assert np.array_equal(_host(out), _host(gan.generator(r['z'], training=False)))
  assert np.array_equal(_host(out), _host(gan.generate(r['z'])))
  # training=True draws masks: another result, and another one on the next call
  t1 = _host(gan.generator(r['z'], training=True))
  t2 = _host(gan.generator(r['z'], training=True))
  assert (t1 != _host(out)).any() and (t1 != t2).any()
  d = gan.discriminator(real, training=False)
  assert tuple(d.shape) == (B, 1)
  assert np.array_equal(_host(d), _host(gan.discriminator(real, training=False)))


def test_two_fresh_objects_train_to_the_same_bits():
  case = CASES[1]
  real = [_real(case, seed) for seed in (1, 2, 3)]
  weights = []
  for _ in range(2):
    gan = _gan(_hp(case, n_critic=2), randomise=False)
    for x in real:
      out = gan.train(x)
    weights.append((gan.generator.get_weights(), gan.discriminator.get_weights(),
                    [_host(v) for v in out[:3]]))
  for a, b in zip(weights[0], weights[1]):
    for x, y in zip(a, b):
      assert np.array_equal(np.asarray(x).view(np.int32),
                            np.asarray(y).view(np.int32))
  # and they did train: the weights left their initial values
  fresh = _gan(_hp(case, n_critic=2), randomise=False)
  assert any((x != y).any() for x, y in zip(fresh.discriminator.get_weights(),
                                            weights[0][1]))


def test_refusals():
  case = CASES[0]
  hp = _hp(case)
  hp.algorithm = 'gan'
  gen, dis = get_models(hp, None)
  with pytest.raises(ValueError, match='wgan-gp'):
    get_algorithm(hp, gen, dis, None)
  hp.algorithm = 'wgan-gp'
  hp.spike_metrics = True
  with pytest.raises(ValueError, match='spike_metrics'):
    get_algorithm(hp, gen, dis, None)


def test_main_end_to_end_on_a_surrogate_directory(tmp_path):
  sys.path.insert(0, os.path.join(ROOT, 'dataset'))
  try:
    import generate_surrogate_dataset as tool
  finally:
    sys.path.pop(0)
  data = str(tmp_path / 'surrogate')
  tool.generate(data, num_samples=9000, training_size=8192 + 512,
                sequence_length=6)
  out = str(tmp_path / 'run')
  hp = cli.build_parser().parse_args([
      '--input_dir', data, '--output_dir', out, '--model', 'mlp',
      '--algorithm', 'wgan-gp', '--batch_size', '512', '--epochs', '2',
      '--plot_weights', '--verbose', '0'])
  hp.global_step = 0
  hp.surrogate_ds = True
  # (main.main would go on to sample 2 * 10^6 signals: too slow for a test; the
  # sampling is called directly below)
  real_generate = utils.generate_dataset
  utils.generate_dataset = lambda *a, **k: None
  try:
    cli.main(hp)
  finally:
    utils.generate_dataset = real_generate
  assert hp.global_step == 2 * 16 and hp.signal_shape == (6, 2)
  import json
  scalars = [json.loads(l) for l in open(os.path.join(out, 'scalars.jsonl'))]
  losses = [r['value'] for r in scalars if 'loss' in r['tag']]
  assert len(losses) >= 4 and np.isfinite(losses).all()
  hists = [json.loads(l) for l in open(os.path.join(out, 'histograms.jsonl'))]
  tags = {r['tag'] for r in hists}
  assert any(t.endswith('dense/kernel:0') for t in tags)
  assert any(t.endswith('dense_9/bias:0') for t in tags)
  assert len(hists) == 2 * 20
  # the checkpoint restores to the same weights
  ck = sorted(glob.glob(os.path.join(out, 'checkpoints', 'epoch-*.pkl')))[-1]
  saved = pickle.load(open(ck, 'rb'))
  gen, dis = get_models(hp, None)
  gan = get_algorithm(hp, gen, dis, None)
  assert any((a != b).any() for a, b in zip(saved['gen_weights'],
                                            gen.get_weights()))
  utils.load_models(hp, gan)
  assert hp.start_epoch == 2
  for a, b in zip(saved['gen_weights'] + saved['dis_weights'],
                  gen.get_weights() + dis.get_weights()):
    assert np.array_equal(a, b)
  assert gan.dis_optimizer.iterations == 2 * 16 * 5
  utils.generate_dataset(hp, gan, num_samples=300)
  generated = pickle.load(open(os.path.join(out, 'generated.pkl'), 'rb'))
  assert sorted(generated) == ['signals']
  sig = generated['signals']
  assert sig.shape == (300, 6, 2) and sig.dtype == np.float32
  assert np.isfinite(sig).all() and sig.std() > 0
  span = hp.signals_max - hp.signals_min  # (sigmoid output, denormalised)
  assert sig.min() >= hp.signals_min - 1e-5 * span
  assert sig.max() <= hp.signals_max + 1e-5 * span
