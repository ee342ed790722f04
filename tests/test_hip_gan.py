"""GPU tests of the vanilla GAN step (--algorithm gan, reference
gan/algorithms/gan.py:43-90): the BCE head kernel (cg_dense1_bce) against a
float64 host computation, one step and twenty steps against the CPU oracle of
tests/bce_oracle.py, graph replay against eager launches, two processes, the
validate / normalisation / mixed-precision surfaces, data parallelism and
main.py --algorithm gan."""
import json
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import bce_oracle as BO
import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (L, C, U, k, m, B, layer_norm) -- test_hip_step.py's CONFIGS that the
# issue names, plus BASELINE configs[1]'s layer shapes at batch 8
CONFIGS = {
    'tiny': (64, 6, 8, 24, 2, 4, True),
    'mid': (256, 16, 32, 24, 2, 6, True),
    'odd_c': (128, 102, 16, 24, 3, 3, True),
    'b1': (64, 6, 8, 24, 2, 1, True),
    'm0_k8': (128, 6, 8, 8, 0, 3, True),
    'long': (2048, 6, 8, 24, 10, 2, True),
    'cfg2_b8': (2048, 102, 64, 24, 10, 8, True),
}


@pytest.fixture(autouse=True)
def _back_to_bf16():
  yield
  from calciumgan_amd import _lib
  _lib.use('bf16')


def _build(name, **hp_kw):
  from calciumgan_amd.gan.algorithms import get_algorithm
  from calciumgan_amd.gan.models import get_models
  L, C, U, k, m, B, ln = CONFIGS[name]
  hp = O.make_hparams(L, C, U, kernel_size=k, m=m, layer_norm=ln)
  for key, v in hp_kw.items():
    setattr(hp, key, v)
  hp.algorithm = 'gan'
  hp.verbose = 0
  gen, dis = get_models(hp, None)
  gan = get_algorithm(hp, gen, dis, None)
  rng = np.random.RandomState(42)
  gw, dw = gen.get_weights(), dis.get_weights()
  for w in gw + dw:
    if w.ndim == 1:
      w += rng.randn(*w.shape).astype(np.float32) * 0.05
  gen.set_weights(gw)
  dis.set_weights(dw)
  real = rng.uniform(0, 1, (B, L, C)).astype(np.float32)
  return hp, gen, dis, gan, real, B


def _flat(ts):
  return np.concatenate([
      (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).reshape(-1)
      for t in ts]).astype(np.float64)


def _ratio_cos(got, ref):
  g, r = _flat(got), _flat(ref)
  return (np.linalg.norm(g) / np.linalg.norm(r),
          float(g @ r / (np.linalg.norm(g) * np.linalg.norm(r))))


# ---------------------------------------------------------------------------
# 1. the head kernel
# ---------------------------------------------------------------------------
# (one ulp of the activation type at |x|; x rounded to it on the host)
from pointwise_ref import round_act as _round_act  # noqa: E402
from pointwise_ref import ulp_act as _ulp  # noqa: E402


@pytest.mark.parametrize('precision', ['bf16', 'f16'])
@pytest.mark.parametrize('shape', [(64, 320, 320, 8), (8, 12, 16, 3),
                                   (256, 320, 320, 2)],
                         ids=['cfg2_head_lds', 'small', 'reread'])
def test_bce_head_matches_float64(shape, precision):
  """logits == cg_dense1_fwd's (same loop, same reduction order); loss means
  within 1e-6 relative of float64 BCE of those logits; the seeds within 1e-6;
  every delta within one ulp of act(c_b * act(w) * act'(h)); two launches give
  the same bits.  fp16: the seeds carry a device loss scale per chain."""
  from calciumgan_amd import _lib, nets
  _lib.use(precision)
  f16 = precision == 'f16'
  dt = torch.float16 if f16 else torch.bfloat16
  Lt, C, Cp, B = shape
  n = 2 * B
  alpha = 0.3
  rng = np.random.RandomState(5)
  h = np.zeros((n, Lt, Cp), np.float32)
  h[:, :, :C] = rng.randn(n, Lt, C).astype(np.float32)
  w = (rng.randn(Lt * C) / np.sqrt(Lt * C)).astype(np.float32)
  bias = np.array([0.25], np.float32)
  wq = _round_act(w, f16).reshape(Lt, C)
  # logits spread over +-60 (a few at +-1e4): scale each sample's row
  target = rng.uniform(-60, 60, n)
  target[1], target[-1] = 1e4, -1e4
  if f16:
    target[1], target[-1] = 3e3, -3e3  # (|h| stays inside fp16's range)
  # (rows leaning towards sign(w) * sign(target): the unscaled logit is far
  # from zero, so the scaled rows stay inside fp16's range)
  sgn = np.sign(target - bias[0])
  h[:, :, :C] += sgn[:, None, None] * np.sign(wq)[None]
  for b in range(n):
    x0 = float((_round_act(h[b, :, :C], f16) * wq).sum())
    h[b] *= (target[b] - bias[0]) / x0
  hd = torch.tensor(h).to(dt).cuda()
  hq = hd.double().cpu().numpy()
  wd, bd = torch.tensor(w).cuda(), torch.tensor(bias).cuda()
  sd = torch.tensor([1024.0 if f16 else 1.0]).cuda()
  sg = torch.tensor([256.0 if f16 else 1.0]).cuda()
  ws = nets.reduce_ws(torch.device('cuda'))

  def launch():
    out = torch.full((n,), 7.0, device='cuda')
    cd = torch.full((n,), 7.0, device='cuda')
    cg = torch.full((B,), 7.0, device='cuda')
    dd = torch.full((n, Lt, Cp), 7.0, device='cuda').to(dt)
    dg = torch.full((B, Lt, Cp), 7.0, device='cuda').to(dt)
    loss = torch.full((2,), 7.0, device='cuda')
    _lib.call('cg_dense1_bce', nets._p(hd), nets._p(wd), nets._p(bd),
              nets._p(out), nets._p(cd), nets._p(cg), nets._p(dd), nets._p(dg),
              nets._p(loss), nets._p(sd), nets._p(sg), B, Lt, C, Cp, alpha,
              nets._p(ws), nets._stream())
    torch.cuda.synchronize()
    return [t.cpu() for t in (out, cd, cg, dd, dg, loss)]

  out, cd, cg, dd, dg, loss = launch()
  ref = torch.zeros(n, device='cuda')
  _lib.call('cg_dense1_fwd', nets._p(hd), nets._p(wd), nets._p(bd), nets._p(ref),
            n, Lt, C, Cp, nets._stream())
  torch.cuda.synchronize()
  # the logits: cg_dense1_fwd's own loop and reduction -> expected identical;
  # the bar allows 2 f32 ulp for a compiler that contracts the two copies of
  # the loop differently
  o, r = out.numpy(), ref.cpu().numpy()
  assert (np.abs(o - r) <= 2 * np.spacing(np.abs(r))).all(), (o, r)
  # and they are the float64 dot (f32 accumulation of F products)
  x64 = (hq[:, :, :C] * wq[None]).sum(axis=(1, 2)) + bias[0]
  mag = (np.abs(hq[:, :, :C]) * np.abs(wq[None])).sum(axis=(1, 2))
  assert (np.abs(o - x64) <= 1e-5 * mag + 1e-5).all()
  # losses and seeds from the kernel's logits, in float64
  x = o.astype(np.float64)
  sp = lambda v: np.maximum(v, 0) + np.log1p(np.exp(-np.abs(v)))  # softplus
  # (s(x) - 1 as -s(-x): exact for large x, as in the kernel)
  sig = lambda v: np.where(v >= 0, 1 / (1 + np.exp(-np.abs(v))),
                           np.exp(-np.abs(v)) / (1 + np.exp(-np.abs(v))))
  xf, xr = x[:B], x[B:]
  gen = sp(-xf).mean()
  dis = sp(-xr).mean() + sp(xf).mean()
  np.testing.assert_allclose(loss.numpy(), [gen, dis], rtol=1e-6)
  want_cd = np.r_[sig(xf), -sig(-xr)] / B * float(sd[0])
  want_cg = -sig(-xf) / B * float(sg[0])
  np.testing.assert_allclose(cd.numpy(), want_cd, rtol=1e-6, atol=1e-30)
  np.testing.assert_allclose(cg.numpy(), want_cg, rtol=1e-6, atol=1e-30)
  # deltas: act(c_b * act(w) * lrelu'(h)), channels >= C zero
  mask = np.where(hq > 0, 1.0, alpha)
  wpad = np.zeros((Lt, Cp))
  wpad[:, :C] = wq
  for got, c in ((dd, cd.numpy()), (dg, cg.numpy())):
    g = got.double().numpy()
    k = g.shape[0]
    want = _round_act(c[:k, None, None] * wpad[None] * mask[:k], f16)
    assert (np.abs(g - want) <= _ulp(want, f16)).all()
    assert (g[:, :, C:] == 0).all()
  # two launches: the same bits
  again = launch()
  for a, b in zip((out, cd, cg, dd, dg, loss), again):
    assert torch.equal(a.view(torch.int16) if a.dtype == dt else a,
                       b.view(torch.int16) if b.dtype == dt else b)


# ---------------------------------------------------------------------------
# 2. one step against the bf16-emulating oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CONFIGS))
def test_step_matches_bf16_oracle(name):
  hp, gen, dis, gan, real, B = _build(name)
  r = BO.draw_randomness(hp, B, seed=7)
  gw = [torch.tensor(w) for w in gen.get_weights()]
  dw = [torch.tensor(w) for w in dis.get_weights()]
  emu = BO.step_grads(hp, gw, dw, torch.tensor(real), r, 'bf16')
  gan._bce_compute(gan._to_device(real), r)
  torch.cuda.synchronize()
  st = gan._get_state(B)
  loss = st['loss'].cpu().numpy()
  np.testing.assert_allclose(loss, [float(emu['gen_loss']),
                                    float(emu['dis_loss'])], rtol=1e-2)
  d_out = st['dws'].d_out.cpu().numpy()
  ref_out = np.r_[emu['fake_out'].numpy().ravel(), emu['real_out'].numpy().ravel()]
  np.testing.assert_allclose(d_out, ref_out, rtol=1e-2,
                             atol=1e-2 * np.abs(ref_out).max())
  for what, got, ref in (('D', dis.net.params.grad_views, emu['d_grads']),
                         ('G', gen.net.params.grad_views, emu['g_grads'])):
    ratio, cos = _ratio_cos(got, ref)
    assert abs(ratio - 1) < 2e-2, (what, ratio)
    assert cos >= 0.985, (what, cos)
  # the same step through train(): Adam on both models, weights close
  hp, gen, dis, gan, real, B = _build(name)
  orc = BO.OracleBCEGAN(hp, gen.get_weights(), dis.get_weights(), 'bf16')
  w0 = _flat(gen.get_weights() + dis.get_weights())
  got = gan.train(real, r)
  ref = orc.train(real, r)
  torch.cuda.synchronize()
  assert got[2] is None
  np.testing.assert_allclose([float(got[0]), float(got[1])], ref[:2], rtol=1e-2)
  wh = _flat(gen.get_weights() + dis.get_weights())
  wo = _flat([t.numpy() for t in orc.gen + orc.dis])
  lr = hp.learning_rate
  # the first Adam step moves each weight by ~lr sign(g): a weight whose gradient
  # sign flips under bf16 rounding is 2 lr away, no weight further
  assert np.abs(wh - wo).max() <= 2.02 * lr
  cos = float((wh - w0) @ (wo - w0) / (np.linalg.norm(wh - w0) *
                                       np.linalg.norm(wo - w0)))
  assert cos > 0.8, cos


# ---------------------------------------------------------------------------
# 3. twenty steps against the f32 oracle
# ---------------------------------------------------------------------------
def test_train_tracks_f32_oracle_over_20_steps():
  hp, gen, dis, gan, real, B = _build('tiny')
  orc = BO.OracleBCEGAN(hp, gen.get_weights(), dis.get_weights(), 'f32')
  g0 = [w.copy() for w in gen.get_weights()]
  d0 = [w.copy() for w in dis.get_weights()]
  for step in range(20):
    r = BO.draw_randomness(hp, B, seed=100 + step)
    got = gan.train(real, r)
    ref = orc.train(real, r)
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(got[0]), ref[0], rtol=3e-2, atol=3e-3)
    np.testing.assert_allclose(float(got[1]), ref[1], rtol=3e-2, atol=3e-3)
    for k in ref[3]:
      np.testing.assert_allclose(float(got[3][k]), ref[3][k], rtol=2e-2)
  assert gan.dis_optimizer.iterations == 20 and gan.gen_optimizer.iterations == 20
  for w_h, w_o, w_i in zip(dis.get_weights() + gen.get_weights(),
                           orc.dis + orc.gen, d0 + g0):
    mv = np.linalg.norm(w_o.numpy() - w_i)
    if mv > 0:
      assert np.linalg.norm(w_h - w_o.numpy()) / mv < 0.25


# ---------------------------------------------------------------------------
# 4. graph replay against eager launches
# ---------------------------------------------------------------------------
def test_graph_replay_equals_eager(fixed_tiles):
  runs = []
  for graphed in (True, False):
    hp, gen, dis, gan, real, B = _build('mid')
    gan._use_graph = graphed
    outs = []
    for _ in range(6):
      gl, dl, gp, m = gan.train(real)
      assert gp is None
      outs.append(torch.stack([gl, dl] + [m[k] for k in sorted(m)]))
    torch.cuda.synchronize()
    if graphed:
      assert gan._get_state(B).get('graph') is not None
    else:
      assert gan._get_state(B).get('graph') is None
    runs.append((torch.stack(outs).cpu().numpy(),
                 gen.get_weights() + dis.get_weights()))
  (oa, wa), (ob, wb) = runs
  np.testing.assert_array_equal(oa, ob)
  for a, b in zip(wa, wb):
    np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------
# 5. two processes
# ---------------------------------------------------------------------------
def _det(steps, shape):
  env = dict(os.environ)
  env.pop('CALCIUMGAN_AUTOTUNE', None)
  env.pop('CALCIUMGAN_TILE_CACHE', None)
  out = subprocess.run(
      [sys.executable, os.path.join(ROOT, 'tests', 'gan_worker.py'), 'det',
       str(steps)] + [str(v) for v in shape],
      env=env, capture_output=True, text=True, timeout=900)
  assert out.returncode == 0, out.stderr[-2000:]
  return json.loads(out.stdout.strip().splitlines()[-1])


def test_two_processes_train_gan_to_identical_bits():
  """20 train() calls at BASELINE configs[1]'s full shapes (L 2048, C 102,
  num_units 64, batch 128) in two fresh processes: the same bits."""
  a = _det(20, (2048, 102, 64, 128))
  b = _det(20, (2048, 102, 64, 128))
  assert a['graph'] and b['graph']
  assert np.isfinite(a['last']).all()
  assert a['outputs'] == b['outputs'], (a['last'], b['last'])
  assert a['weights'] == b['weights']


# ---------------------------------------------------------------------------
# 6. surfaces
# ---------------------------------------------------------------------------
def test_validate_updates_nothing_and_matches_oracle():
  hp, gen, dis, gan, real, B = _build('mid')
  orc = BO.OracleBCEGAN(hp, gen.get_weights(), dis.get_weights(), 'bf16')
  r = BO.draw_randomness(hp, B, seed=9)
  w0 = _flat(gen.get_weights() + dis.get_weights())
  steps = (gan.dis_optimizer.iterations, gan.gen_optimizer.iterations)
  fake, gl, dl, gp, metrics = gan.validate(real, r)
  torch.cuda.synchronize()
  assert gp is None
  assert tuple(fake.shape) == real.shape
  assert np.isfinite([float(gl), float(dl)]).all()
  ref = orc.validate(real, r)
  np.testing.assert_allclose([float(gl), float(dl)], ref[1:3], rtol=1e-2)
  np.testing.assert_allclose(fake.cpu().numpy(), ref[0].numpy(), atol=2e-2)
  for k in ref[4]:
    np.testing.assert_allclose(float(metrics[k]), ref[4][k], rtol=2e-2)
  assert (gan.dis_optimizer.iterations, gan.gen_optimizer.iterations) == steps
  np.testing.assert_array_equal(_flat(gen.get_weights() + dis.get_weights()), w0)
  gan.validate(real)  # (own draws)


@pytest.mark.parametrize('norm', ['batch_norm', 'layer_norm'])
def test_normalised_generators_train(norm):
  kw = dict(batch_norm=norm == 'batch_norm', layer_norm=norm == 'layer_norm')
  hp, gen, dis, gan, real, B = _build('mid', **kw)
  orc = BO.OracleBCEGAN(hp, gen.get_weights(), dis.get_weights(), 'bf16')
  g0 = _flat(gen.get_weights())
  for step in range(3):
    r = BO.draw_randomness(hp, B, seed=30 + step)
    got = gan.train(real, r)
    ref = orc.train(real, r)
    torch.cuda.synchronize()
    np.testing.assert_allclose([float(got[0]), float(got[1])], ref[:2],
                               rtol=3e-2, atol=3e-3)
  for _ in range(4):  # own draws, graph replay from the third call
    got = gan.train(real)
  torch.cuda.synchronize()
  assert np.isfinite([float(got[0]), float(got[1])]).all()
  assert np.abs(_flat(gen.get_weights()) - g0).max() > 0


def test_mixed_precision_tracks_f16_oracle_with_loss_scaling():
  """Three injected-randomness steps follow the fp16-emulating oracle with its
  two DynamicLossScales (both started at 512, as test_hip_fp16.py does), then
  the free-running steps replay as a hipGraph with the scales on the device."""
  hp, gen, dis, gan, real, B = _build('tiny', mixed_precision=True)
  assert gan.precision == 'f16'
  gan.dis_optimizer.loss_scale_state[0] = 512.0
  gan.gen_optimizer.loss_scale_state[0] = 512.0
  orc = BO.OracleBCEGAN(hp, gen.get_weights(), dis.get_weights(), 'f16',
                        loss_scaling=True)
  orc.dis_scale.scale = orc.gen_scale.scale = 512.0
  d0 = [w.copy() for w in dis.get_weights()]
  g0 = [w.copy() for w in gen.get_weights()]
  for step in range(3):
    r = BO.draw_randomness(hp, B, seed=50 + step)
    got = gan.train(real, r)
    ref = orc.train(real, r)
    torch.cuda.synchronize()
    np.testing.assert_allclose([float(got[0]), float(got[1])], ref[:2],
                               rtol=1e-2, atol=1e-3)
  assert gan.dis_optimizer.iterations == orc.dis_steps == 3
  assert gan.gen_optimizer.iterations == orc.gen_steps == 3
  for w_h, w_o, w_i in zip(dis.get_weights() + gen.get_weights(),
                           orc.dis + orc.gen, d0 + g0):
    mv = np.linalg.norm(w_o.numpy() - w_i)
    if mv > 0:
      assert np.linalg.norm(w_h - w_o.numpy()) / mv < 0.25
  for _ in range(5):
    out = gan.train(real)
  torch.cuda.synchronize()
  assert gan._get_state(B).get('graph') is not None
  assert np.isfinite([float(out[0]), float(out[1])]).all()
  assert gan.dis_optimizer.iterations == 8 and gan.gen_optimizer.iterations == 8
  assert float(gan.dis_optimizer.loss_scale_state[1]) == 8.0


def test_forced_overflow_skips_only_that_optimizer():
  """A discriminator loss scale so large that its seeds overflow fp16: the
  critic's update is skipped and its scale halves; the generator's update (its
  own scale) goes ahead."""
  hp, gen, dis, gan, real, B = _build('tiny', mixed_precision=True)
  gan.dis_optimizer.loss_scale_state[0] = 2.0**120
  s_g = float(gan.gen_optimizer.loss_scale_state[0])
  d0, g0 = _flat(dis.get_weights()), _flat(gen.get_weights())
  gl, dl, gp, _ = gan.train(real, BO.draw_randomness(hp, B, seed=3))
  torch.cuda.synchronize()
  assert float(gan.dis_optimizer.loss_scale_state[0]) == 2.0**119
  assert float(gan.gen_optimizer.loss_scale_state[0]) == s_g
  assert gan.dis_optimizer.iterations == 0 and gan.gen_optimizer.iterations == 1
  np.testing.assert_array_equal(_flat(dis.get_weights()), d0)
  assert np.abs(_flat(gen.get_weights()) - g0).max() > 0
  assert np.isfinite([float(gl), float(dl)]).all()


# ---------------------------------------------------------------------------
# 7. data parallel: 2 ranks over gloo on one GPU
# ---------------------------------------------------------------------------
def _free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  p = s.getsockname()[1]
  s.close()
  return p


def test_two_rank_gan_equals_one_rank_on_global_batch(tmp_path):
  env = dict(os.environ)
  env['DP_WORKER_OUT'] = str(tmp_path)
  env['HSA_ENABLE_IPC_MODE_LEGACY'] = '0'
  cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
         '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
         '--master-port', str(_free_port()),
         os.path.join(ROOT, 'tests', 'gan_worker.py'), 'dp']
  out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
  assert out.returncode == 0, out.stderr[-2000:]
  recs = [np.load(os.path.join(str(tmp_path), 'gan_rank%d.npz' % r))
          for r in (0, 1)]
  for rec in recs:
    assert rec['same'].all() and rec['finite'].all()
  np.testing.assert_array_equal(recs[0]['d_grad'], recs[1]['d_grad'])
  # one rank on the global batch, same weights and draws
  sys.path.insert(0, os.path.join(ROOT, 'tests'))
  import gan_worker as W
  hp, gen, dis, gan = W._gan(W.DP['L'], W.DP['C'], W.DP['U'])
  real, r = W.dp_inputs(hp)
  gan._bce_compute(gan._to_device(real), r)
  torch.cuda.synchronize()
  rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
  assert rel(recs[0]['d_grad'], dis.net.params.grad.cpu().numpy()) < 2e-3
  assert rel(recs[0]['g_grad'], gen.net.params.grad.cpu().numpy()) < 2e-3
  np.testing.assert_allclose(recs[0]['loss'],
                             gan._get_state(W.DP['B'])['loss'].cpu().numpy(),
                             rtol=2e-3)


# ---------------------------------------------------------------------------
# 8. main.py --algorithm gan
# ---------------------------------------------------------------------------
def test_main_gan_trains_validates_saves_and_resumes(tmp_path):
  import main as cli
  from calciumgan_amd.data import dg
  from calciumgan_amd.gan.utils import dataset_helper, h5_helper
  d = dg.make_dataset(num_neurons=16, sequence_length=256, num_segments=70)
  info = {k: v for k, v in d['info'].items() if k != 'rates_hz'}
  ds = str(tmp_path / 'ds')
  dataset_helper.write_dataset(ds, d['signals'], d['spikes'], info,
                               validation_size=6)
  out = str(tmp_path / 'run')

  def args(epochs):
    a = cli.build_parser().parse_args([
        '--input_dir', ds, '--output_dir', out, '--model', 'calciumgan',
        '--algorithm', 'gan', '--batch_size', '8', '--num_units', '8', '--m',
        '2', '--layer_norm', '--epochs', str(epochs), '--save_generated',
        'last', '--verbose', '0'])
    a.global_step = 0
    a.surrogate_ds = False
    return a

  hp = args(2)
  metrics = cli.main(hp, return_metrics=True)
  assert all(np.isfinite(v) for v in metrics.values()), metrics
  assert hp.global_step == 16
  tr = [json.loads(l) for l in open(os.path.join(out, 'scalars.jsonl'))]
  tags = {r['tag'] for r in tr}
  assert {'loss/generator', 'loss/discriminator'} <= tags
  assert 'loss/gradient_penalty' not in tags
  assert all(np.isfinite(r['value']) for r in tr)
  va = [json.loads(l) for l in open(os.path.join(out, 'validation',
                                                 'scalars.jsonl'))]
  assert 'loss/gradient_penalty' not in {r['tag'] for r in va}
  ck = os.path.join(out, 'checkpoints', 'epoch-001.pkl')
  c1 = pickle.load(open(ck, 'rb'))
  assert int(c1['dis_steps']) == 16 and int(c1['gen_steps']) == 16
  gen = h5_helper.get(os.path.join(out, 'generated', 'epoch001_signals.h5'),
                      'signals')
  assert gen.shape == (6, 256, 16) and np.isfinite(gen).all()
  hp2 = args(3)
  cli.main(hp2)
  c2 = pickle.load(open(os.path.join(out, 'checkpoints', 'epoch-002.pkl'), 'rb'))
  assert int(c2['dis_steps']) == 24 and int(c2['gen_steps']) == 24
  moved = sum(float(np.abs(a - b).sum())
              for a, b in zip(c1['dis_weights'], c2['dis_weights']))
  assert moved > 0
