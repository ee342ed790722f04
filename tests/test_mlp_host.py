"""CPU tests of `--model mlp`: the registry, shapes and parameter counts, the
numpy statement of the dropout masks, the float64 oracle against its own hand
schedule, and the surrogate dataset tool."""
import os
import pickle
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mlp_oracle as M
from calciumgan_amd import geometry as geo
from calciumgan_amd.gan.models import mlp
from calciumgan_amd.gan.models.registry import _MODELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'surrogate_dg_reference.npz')


def make_hparams(L=6, C=2, noise_dim=32, num_units=32, dropout=0.2, **kw):
  hp = SimpleNamespace(
      signal_shape=(L, C), sequence_length=L, num_channels=C, num_neurons=C,
      noise_dim=noise_dim, noise_shape=(noise_dim,), num_units=num_units,
      dropout=dropout, activation='leakyrelu', normalize=True, m=2,
      gradient_penalty=10.0, n_critic=2, learning_rate=1e-4, signals_min=0.0,
      signals_max=1.0, batch_norm=False, layer_norm=False,
      mixed_precision=False, model='mlp', algorithm='wgan-gp', verbose=0)
  hp.__dict__.update(kw)
  hp.alpha = geo.PIECEWISE_LINEAR_ALPHA.get(hp.activation)  # (the oracle's)
  return hp


def test_mlp_is_registered():
  assert 'mlp' in _MODELS


def test_parameter_counts_and_keras_shapes():
  hp = make_hparams()
  gs, ds = mlp.generator_shapes(hp), mlp.discriminator_shapes(hp)
  assert sum(int(np.prod(s)) for s in gs) == 15938
  assert sum(int(np.prod(s)) for s in ds) == 21249
  assert gs == [(32, 192), (192,), (32, 32), (32,), (32, 64), (64,), (64, 96),
                (96,), (96, 2), (2,)]
  assert ds == [(2, 128), (128,), (128, 96), (96,), (96, 64), (64,), (64, 32),
                (32,), (192, 1), (1,)]


def test_objects_weights_round_trip_and_names():
  """The objects on a CPU device: weights can be read and set (they cannot
  compute there)."""
  hp = make_hparams()
  cpu = torch.device('cpu')
  gen, dis = mlp.generator(hp, cpu), mlp.discriminator(hp, cpu)
  assert gen.count_params() == 15938 and dis.count_params() == 21249
  assert [w.shape for w in gen.get_weights()] == mlp.generator_shapes(hp)
  assert [w.shape for w in dis.get_weights()] == mlp.discriminator_shapes(hp)
  assert len(gen.trainable_variables) == 10
  assert gen.net.params.names[:2] == ['dense/kernel:0', 'dense/bias:0']
  assert gen.net.params.names[-1] == 'dense_4/bias:0'
  assert dis.net.params.names[0] == 'dense_5/kernel:0'
  assert dis.net.params.names[-1] == 'dense_9/bias:0'
  for model in (gen, dis):
    w = model.get_weights()
    # Glorot uniform kernels, zero biases
    assert all(np.all(b == 0) for b in w[1::2])
    assert all(np.abs(k).max() <= np.sqrt(6.0 / sum(k.shape)) for k in w[0::2])
    new = [v + np.float32(i + 1) for i, v in enumerate(w)]
    model.set_weights(new)
    for a, b in zip(model.get_weights(), new):
      np.testing.assert_array_equal(a, b)
  # the same seeded streams: a second object starts from the same weights
  for a, b in zip(mlp.discriminator(hp, cpu).get_weights(),
                  mlp.discriminator(hp, cpu).get_weights()):
    np.testing.assert_array_equal(a, b)
  with pytest.raises(RuntimeError):
    gen(np.zeros((2, 32), np.float32))


@pytest.mark.parametrize('change', [
    dict(activation='tanh'), dict(mixed_precision=True), dict(batch_norm=True),
    dict(layer_norm=True), dict(world_size=2), dict(num_units=257),
    dict(sequence_length=4096, signal_shape=(4096, 2)), dict(noise_dim=0)])
def test_refusals(change):
  hp = make_hparams(**change)
  with pytest.raises(ValueError):
    mlp.generator(hp, torch.device('cpu'))


def test_noise_dim_is_free_of_the_convolution_rules():
  hp = make_hparams(noise_dim=5, num_units=8)
  assert mlp.generator(hp, torch.device('cpu')).count_params() > 0
  with pytest.raises(ValueError):
    geo.validate_hparams(SimpleNamespace(strides=2, kernel_size=24, noise_dim=5))


# -- dropout_keep_mask ------------------------------------------------------------
def test_philox_known_answer():
  """Random123's kat_vectors entry for philox4x32-10 with an all-zero counter
  and key.  The vector in the issue was quoted from memory; the statement --
  ten rounds, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
  0xBB67AE85 -- reproduces it as written, so nothing had to be settled either
  way."""
  got = mlp.philox4x32_10(np.zeros(4, np.uint32), (0, 0))
  assert ['{:08x}'.format(int(v)) for v in got] == [
      '6627e8d5', 'e169c58d', 'bc57ac4c', '9b00dbd8']


def test_philox_second_known_answer():
  """Random123's all-ones vector: counter and key 0xffffffff."""
  got = mlp.philox4x32_10(np.full(4, 0xFFFFFFFF, np.uint32),
                          (0xFFFFFFFF, 0xFFFFFFFF))
  assert ['{:08x}'.format(int(v)) for v in got] == [
      '408f276d', '41c83b0e', 'a20bc7c6', '6d5451fd']


@pytest.mark.parametrize('p', [0.2, 0.5])
def test_keep_rate(p):
  n = 10**6
  keep = mlp.dropout_keep_mask(1234, 7, n, p)
  assert keep.dtype == bool and keep.shape == (n,)
  sd = np.sqrt(p * (1 - p) / n)
  assert abs(keep.mean() - (1 - p)) < 4 * sd


def test_keep_mask_properties():
  assert mlp.dropout_keep_mask(1234, 7, 1001, 0.0).all()
  a = mlp.dropout_keep_mask(1234, 7, 4096, 0.5)
  b = mlp.dropout_keep_mask(1234, 8, 4096, 0.5)
  c = mlp.dropout_keep_mask(1235, 7, 4096, 0.5)
  assert (a != b).any() and (a != c).any()
  # a pure function of its arguments; a prefix of a longer mask
  np.testing.assert_array_equal(a, mlp.dropout_keep_mask(1234, 7, 4096, 0.5))
  np.testing.assert_array_equal(a[:1027],
                                mlp.dropout_keep_mask(1234, 7, 1027, 0.5))
  # word e & 3 of block e >> 2, 64-bit stream ids and seeds
  words = mlp.philox4x32_10(np.array([[1, 0, 5, 2]], np.uint32), (9, 3))
  big = mlp.dropout_keep_mask((3 << 32) | 9, (2 << 32) | 5, 8, 0.5)
  np.testing.assert_array_equal(big[4:], words[0] >= np.uint32(1 << 31))
  assert mlp.dropout_threshold(0.5) == 1 << 31
  assert mlp.dropout_scale(0.2) == np.float32(1.25)
  assert mlp.stream_id(3, 1, 2) == (3 << 8) | (1 << 4) | 2


# -- the oracle against itself ------------------------------------------------------
def _random_weights(shapes, rng):
  return [rng.standard_normal(s) * 0.5 for s in shapes]


def test_hand_schedule_equals_autograd():
  """The schedule the device runs -- input-gradient chain, v, tangent chain,
  weight gradients over three segments, no bias gradient from the penalty --
  equals autograd's gradients of -E[D(real)] + E[D(fake)] + lambda gp in
  float64: with fixed masks the model is piecewise linear, so the masks add no
  second-derivative term."""
  B, L, C, U, nd, p = 3, 5, 2, 8, 5, 0.5
  hp = make_hparams(L=L, C=C, noise_dim=nd, num_units=U, dropout=p)
  rng = np.random.RandomState(3)
  gen_w = _random_weights(mlp.generator_shapes(hp), rng)
  dis_w = _random_weights(mlp.discriminator_shapes(hp), rng)
  real = rng.uniform(0, 1, (B, L, C))
  r = dict(z=rng.standard_normal((B, nd)), alpha=rng.uniform(0, 1, B),
           masks_g=[rng.uniform(size=(B, L, w)) >= p for w in (U, 2 * U, 3 * U)],
           masks_d=[rng.uniform(size=(3 * B, L, w)) >= p
                    for w in (4 * U, 3 * U, 2 * U, U)])
  auto = M.critic_step(gen_w, dis_w, real, r, hp)
  loss, gp, grads = M.hand_critic_grads(dis_w, real, auto['fake'], r['alpha'],
                                        r['masks_d'], hp)
  assert abs(float(loss) - float(auto['loss'])) < 1e-10
  assert abs(float(gp) - float(auto['gp'])) < 1e-10
  assert float(auto['gp']) > 0
  for i, (a, b) in enumerate(zip(grads, auto['grads'])):
    b = b.reshape(a.shape)
    assert float((a - b).abs().max()) < 1e-10 * max(1.0, float(b.abs().max())), i
  # the penalty reaches the kernels and leaves the biases alone
  hp0 = make_hparams(L=L, C=C, noise_dim=nd, num_units=U, dropout=p,
                     gradient_penalty=0.0)
  plain = M.critic_step(gen_w, dis_w, real, r, hp0)['grads']
  assert float((plain[0] - auto['grads'][0]).abs().max()) > 1e-6
  for i in (1, 3, 5, 7, 9):
    assert float((plain[i] - auto['grads'][i]).abs().max()) < 1e-12


# -- the dataset tool ---------------------------------------------------------------
def _tool():
  sys.path.insert(0, os.path.join(ROOT, 'dataset'))
  try:
    import generate_surrogate_dataset as tool
  finally:
    sys.path.pop(0)
  return tool


def test_surrogate_tool_files(tmp_path):
  out = str(tmp_path / 'surrogate')
  subprocess.check_call([
      sys.executable, os.path.join(ROOT, 'dataset',
                                   'generate_surrogate_dataset.py'),
      '--output_dir', out, '--num_samples', '300', '--training_size', '200',
      '--sequence_length', '6'])
  load = lambda n: pickle.load(open(os.path.join(out, n), 'rb'))
  sur, gt, tr = (load(n) for n in ('surrogate.pkl', 'ground_truth.pkl',
                                   'training.pkl'))
  assert sorted(sur) == ['spikes'] and sorted(gt) == ['spikes']
  assert sorted(tr) == ['signals', 'spikes']
  assert sur['spikes'].shape == gt['spikes'].shape == (300, 2, 6)
  assert tr['spikes'].shape == tr['signals'].shape == (200, 2, 6)
  for a in (sur['spikes'], gt['spikes'], tr['spikes'], tr['signals']):
    assert a.dtype == np.float32
  assert set(np.unique(sur['spikes'])) <= {0.0, 1.0}
  assert (sur['spikes'] != gt['spikes']).any()
  # every training sample is one of the ground truth's
  gt_rows = {row.tobytes() for row in gt['spikes']}
  assert all(row.tobytes() in gt_rows for row in tr['spikes'])
  # calcium: spike + 0.95 * previous from t = 2 on, plus noise of sd 0.3
  c = tr['spikes'].copy()
  for j in range(2, 6):
    c[:, :, j] += np.float32(0.95) * c[:, :, j - 1]
  noise = tr['signals'] - c
  assert abs(noise.std() - 0.3) < 0.03 and abs(noise.mean()) < 0.03


def test_surrogate_statistics_against_the_reference():
  """tests/golden/surrogate_dg_reference.npz: per-neuron rates and the pair
  covariance (population form, over all bins) of 10^5 samples of 2 neurons x 6
  steps drawn by the reference's DichotGauss(2, mean=[[0.6, 0.8]],
  corr=[[1, .3], [.3, 1]], make_pd=True).sample(repeats=6), one call per
  sample as generate_surrogate_data.py:17-30 makes them, under
  np.random.seed(1234), on the CPU with numpy and scipy alone.

  Both sides are estimates over N = 6 * 10^5 independent bins, so a difference
  has the standard error sqrt(2) * sd / sqrt(N), with sd^2 = r (1 - r) for a
  rate and the variance of (x - r_x)(y - r_y) for the covariance."""
  gold = np.load(GOLDEN)
  n, L = int(gold['num_samples']), int(gold['sequence_length'])
  assert (n, L) == (10**5, 6)
  spikes = _tool().generate_dg_spikes(n, L, np.random.RandomState(99))
  assert spikes.shape == (n, 2, L)
  bins = spikes.transpose(1, 0, 2).reshape(2, -1).astype(np.float64)
  N = bins.shape[1]
  rates = bins.mean(1)
  for k in range(2):
    se = np.sqrt(2 * gold['rates'][k] * (1 - gold['rates'][k]) / N)
    assert abs(rates[k] - gold['rates'][k]) < 4 * se, (k, rates, gold['rates'])
  prod = (bins[0] - rates[0]) * (bins[1] - rates[1])
  se = np.sqrt(2 * prod.var() / N)
  assert abs(prod.mean() - gold['cov'][0, 1]) < 4 * se
  assert gold['cov'][0, 1] > 10 * se  # the correlation is there to be missed
  # bins of one sample are independent in time
  lag = np.mean((spikes[:, 0, 1:] - rates[0]) * (spikes[:, 0, :-1] - rates[0]))
  assert abs(lag) < 4 * gold['rates'][0] * (1 - gold['rates'][0]) / np.sqrt(n * 5)
