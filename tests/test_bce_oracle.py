"""CPU checks of the vanilla GAN step's pieces that need no GPU: the BCE
oracle's seed algebra and stability (tests/bce_oracle.py) and the ABI 20
declaration of the BCE head (cg_dense1_bce)."""
import os
import re
import subprocess
import sys

import numpy as np
import torch

import bce_oracle as BO
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seed_is_sigmoid_minus_label_under_autograd_f64():
  """d/dx of Keras BCE from logits, per sample, is s(x) - y: the per-sample
  coefficients the head kernel writes are this times S / B."""
  x = torch.tensor(np.r_[np.linspace(-60, 60, 41), [-1e4, 1e4]],
                   dtype=torch.float64, requires_grad=True)
  for y in (0.0, 1.0):
    t = torch.full_like(x, y)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(
        x, t, reduction='sum')
    (g,) = torch.autograd.grad(loss, x)
    np.testing.assert_allclose(g.numpy(), BO.bce_seed(x.detach(), y).numpy(),
                               rtol=1e-12, atol=1e-300)


def test_losses_finite_at_extreme_logits():
  for v in (1e4, -1e4):
    r = torch.full((3, 1), v)
    f = torch.full((3, 1), -v)
    gen, dis = BO.bce_losses(r, f)
    assert torch.isfinite(gen) and torch.isfinite(dis)
  gen, dis = BO.bce_losses(torch.full((2, 1), 1e4), torch.full((2, 1), 1e4))
  # BCE(1, 1e4) = 0, BCE(0, 1e4) = 1e4
  assert float(gen) == 0.0 and float(dis) == 1e4


def test_oracle_step_gradients_are_those_of_the_two_losses():
  """One tiny oracle step in float64: the discriminator's gradients are those
  of BCE(1, D(real)) + BCE(0, D(fake)), checked through the head's bias:
  dL_D/db = mean(s(r) - 1) + mean(s(f)).  (float64: the identity is exact to
  rounding, and the step stays off the f32 convolution kernels that the golden
  oracle tests of this process use.)"""
  hp = O.make_hparams(64, 6, 8, m=2)
  rng = np.random.RandomState(0)
  gw = O.init_generator(hp, rng)
  dw = O.init_discriminator(hp, rng)
  real = rng.uniform(0, 1, (4, 64, 6))
  r = BO.draw_randomness(hp, 4, seed=3)
  res = BO.step_grads(hp, gw, dw, real, r, 'f32', dtype=torch.float64)
  want = (torch.sigmoid(res['real_out']) - 1).mean() + torch.sigmoid(
      res['fake_out']).mean()
  np.testing.assert_allclose(float(res['d_grads'][-1][0]), float(want),
                             rtol=1e-12)
  assert all(torch.isfinite(g).all() for g in res['d_grads'] + res['g_grads'])
  gen, dis = BO.bce_losses(res['real_out'], res['fake_out'])
  assert float(gen) == float(res['gen_loss']) and float(dis) == float(
      res['dis_loss'])


def test_abi20_declares_the_bce_head():
  """Header, ctypes table and both builds of the library agree on ABI 20 and
  export cg_dense1_bce.  (The libraries are loaded in a child process: this
  test leaves the HIP runtime out of the test process.)"""
  header = open(os.path.join(ROOT, 'include', 'calciumgan_hip.h')).read()
  assert int(re.search(r'#define CG_ABI_VERSION (\d+)', header).group(1)) == 20
  assert re.search(r'\bint cg_dense1_bce\(', header)
  from calciumgan_amd import _lib
  assert len(_lib.SIGNATURES['cg_dense1_bce']) == 18
  code = ('import sys; sys.path.insert(0, {!r})\n'
          'from calciumgan_amd import _lib\n'
          'for p in ("bf16", "f16"):\n'
          '  lib = _lib.load(p)\n'
          '  assert lib.cg_abi_version() == 20, p\n'
          '  assert hasattr(lib, "cg_dense1_bce"), p\n'
          'print("ok")\n').format(ROOT)
  out = subprocess.run([sys.executable, '-c', code], capture_output=True,
                       text=True, timeout=300)
  assert out.returncode == 0 and out.stdout.strip().endswith('ok'), out.stderr
