"""CPU checks of tests/pointwise_ref.py: every float64 statement the GPU parity
tests of tests/test_hip_pointwise.py compare a kernel with is tied here to an
independent one -- torch autograd in float64 or the oracle of
oracle/calciumgan_oracle.py -- and the rounding helpers to hand-picked values."""
import numpy as np
import torch

import oracle as O
import pointwise_ref as R

F64 = torch.float64


def test_penalty_value_and_coefficient_under_autograd_f64():
  """gp = mean((||g_b|| - 1)^2) and d(scale gp)/dg_b = coef_b g_b: the
  coefficient cg_gp_finalize writes times the row cg_scale_rows multiplies."""
  rng = np.random.RandomState(0)
  for B, n, scale, mul in ((1, 8, 10.0, 1.0), (5, 24, 10.0, 1.0), (7, 16, 3.0, 0.5)):
    g = rng.randn(B, n) * rng.uniform(0.01, 3.0, (B, 1))
    gt = torch.tensor(g, dtype=F64, requires_grad=True)
    norm = gt.pow(2).sum(1).sqrt()
    gp = ((norm - 1)**2).mean()
    (scale * mul * gp).backward()
    nv, gpr, coef = R.gp_finalize(R.rownorm(g), scale, 0, mul)
    np.testing.assert_allclose(nv, norm.detach().numpy(), rtol=1e-14)
    np.testing.assert_allclose(gpr, gp.item(), rtol=1e-13)
    np.testing.assert_allclose(R.scale_rows(g, coef), gt.grad.numpy(), rtol=1e-12,
                               atol=1e-300)
    # from the sums of squares
    nv2, gp2, coef2 = R.gp_finalize((g * g).sum(1), scale, 1, mul)
    np.testing.assert_allclose(nv2, nv, rtol=1e-14)
    np.testing.assert_allclose(gp2, gpr, rtol=1e-12)
    np.testing.assert_allclose(coef2, coef, rtol=1e-12, atol=1e-300)


def test_critic_losses_match_the_oracle():
  rng = np.random.RandomState(1)
  B = 9
  d = rng.randn(3 * B)
  got = R.critic_loss(d, 0.37, 10.0, B)
  want = O.discriminator_loss(torch.tensor(d[:B]), torch.tensor(d[B:2 * B]), 0.37,
                              10.0)
  np.testing.assert_allclose(got[0], float(want), rtol=1e-14)
  np.testing.assert_allclose(got[1], -d[B:2 * B].mean(), rtol=1e-14)
  np.testing.assert_allclose(R.neg_mean(d, B), -d[:B].mean(), rtol=1e-14)


def test_adam_matches_keras_adam_of_the_oracle():
  rng = np.random.RandomState(2)
  n = 101
  p, g, m = rng.randn(n), rng.randn(n), rng.randn(n) * 0.1
  v = rng.rand(n) * 0.1
  for t, gs in ((1, 1.0), (3, 0.5), (20000, 2.0)):
    pt, mt, vt = (torch.tensor(a, dtype=F64) for a in (p, m, v))
    O.keras_adam(pt, torch.tensor(g * gs, dtype=F64), mt, vt, t, 1e-3)
    p1, m1, v1 = R.adam(p, g, m, v, R.adam_lr_t(1e-3, 0.9, 0.999, t), 0.9, 0.999,
                        1e-7, gs)
    np.testing.assert_allclose(p1, pt.numpy(), rtol=1e-13)
    np.testing.assert_allclose(m1, mt.numpy(), rtol=1e-13)
    np.testing.assert_allclose(v1, vt.numpy(), rtol=1e-13)
  # v = 0 and g = 0: the update is m / eps, and 0 for m = 0 -- never NaN
  p1, m1, v1 = R.adam([1.0, 1.0], [0.0, 0.0], [0.0, 0.5], [0.0, 0.0], 1e-3, 0.9,
                      0.999, 1e-7)
  assert p1[0] == 1.0 and np.isfinite(p1).all() and (v1 == 0).all()


def test_interpolation_and_signal_metrics_match_the_oracle():
  rng = np.random.RandomState(3)
  B, L, C = 3, 7, 11
  real, fake, alpha = rng.rand(B, L, C), rng.rand(B, L, C), rng.rand(B)
  want = O.interpolation(torch.tensor(real), torch.tensor(fake), torch.tensor(alpha))
  np.testing.assert_allclose(R.interp(real, fake, alpha), want.numpy(), rtol=1e-15)
  m = O.signal_metrics(torch.tensor(real), torch.tensor(fake), -0.5, 2.5, True)
  want = [float(m['signals_metrics/' + k]) for k in ('min', 'max', 'mean', 'std')]
  got = R.signal_metrics(real.reshape(-1, C), fake.reshape(-1, C), -0.5, 2.5)
  np.testing.assert_allclose(got, want, rtol=1e-12)
  # a row of identical values has std exactly 0
  flat = np.full((2, 5), 0.625)
  assert (R.signal_stats(flat, -1.0, 3.0)[3] == 0).all()


def test_elementwise_backward_pieces_under_autograd_f64():
  rng = np.random.RandomState(4)
  alpha = 0.3
  # LeakyReLU
  y = torch.tensor(rng.randn(50), dtype=F64, requires_grad=True)
  dh = rng.randn(50)
  h = torch.nn.functional.leaky_relu(y, alpha)
  h.backward(torch.tensor(dh))
  np.testing.assert_allclose(R.lrelu_bwd(dh, h.detach().numpy(), alpha),
                             y.grad.numpy(), rtol=1e-15)
  # h = +-0 takes the slope (tf.nn.leaky_relu's gradient: features > 0 ? g : alpha g)
  assert (R.lrelu_grad(np.array([0.0, -0.0]), alpha) == alpha).all()
  # sigmoid
  z = torch.tensor(rng.randn(50), dtype=F64, requires_grad=True)
  s = torch.sigmoid(z)
  s.backward(torch.tensor(dh))
  np.testing.assert_allclose(R.sigmoid_bwd(dh, s.detach().numpy()), z.grad.numpy(),
                             rtol=1e-13)
  # lrelu_mix: act(m act^-1(h_a) + (1 - m) act^-1(h_b)) on pre-activations
  ya, yb, mix = rng.randn(4, 16), rng.randn(4, 16), rng.rand(4)
  act = lambda t: np.maximum(t, alpha * t)
  want = act(mix[:, None] * ya + (1 - mix[:, None]) * yb)
  np.testing.assert_allclose(R.lrelu_mix(act(ya), act(yb), mix, alpha), want,
                             rtol=1e-12, atol=1e-15)


def test_head_seeds_and_weight_gradient_under_autograd_f64():
  """out = bias + <h, w>; with L = sum_b coef[b / seg] out_b over h =
  leaky_relu(y): dL/dy is cg_dense1_bwd's seed, dL/dw cg_dense1_wgrad's sum."""
  rng = np.random.RandomState(5)
  nB, Lt, C, seg, alpha = 6, 4, 5, 2, 0.3
  y = torch.tensor(rng.randn(nB, Lt, C), dtype=F64, requires_grad=True)
  w = torch.tensor(rng.randn(Lt, C), dtype=F64, requires_grad=True)
  bias = torch.tensor([0.25], dtype=F64, requires_grad=True)
  coef = rng.randn(nB // seg)
  h = torch.nn.functional.leaky_relu(y, alpha)
  out = (h * w[None]).sum((1, 2)) + bias
  cb = torch.tensor(np.repeat(coef, seg))
  (cb * out).sum().backward()
  hn, wn = h.detach().numpy(), w.detach().numpy()
  np.testing.assert_allclose(R.dense1_fwd(hn, wn, 0.25), out.detach().numpy(),
                             rtol=1e-14)
  np.testing.assert_allclose(R.dense1_bwd(hn, wn, coef, seg, alpha), y.grad.numpy(),
                             rtol=1e-14)
  np.testing.assert_allclose(R.dense1_wgrad_terms(hn, coef, seg).sum(0),
                             w.grad.numpy(), rtol=1e-13)
  np.testing.assert_allclose(np.repeat(coef, seg).sum(), bias.grad.item(), rtol=1e-13)


def test_step_outputs_statement():
  loss = np.array([[1.0, np.nan], [2.0, np.nan], [6.0, np.nan]])
  got = R.step_outputs(0.5, loss, [0.1, 0.2, 0.6], [1, 2, 3, 4], 3)
  np.testing.assert_allclose(got, [0.5, 3.0, 0.3, 1, 2, 3, 4], rtol=1e-15)
  assert (R.step_outputs(0.5, loss, [0.1], [1, 2, 3, 4], 0)[1:3] == 0).all()


def test_round_act_on_ties_subnormals_and_overflow():
  # ties go to the even neighbour
  assert R.round_act(1 + 2.0**-8, False) == 1.0
  assert R.round_act(1 + 3 * 2.0**-8, False) == 1 + 2.0**-6
  assert R.round_act(1 + 2.0**-11, True) == 1.0
  assert R.round_act(1 + 3 * 2.0**-11, True) == 1 + 2.0**-9
  # just past the tie: up
  assert R.round_act(1 + 2.0**-8 + 2.0**-20, False) == 1 + 2.0**-7
  assert R.round_act(1 + 2.0**-11 + 2.0**-22, True) == 1 + 2.0**-10
  # subnormals: kept; half the smallest one ties to zero, three halves to two
  for f16 in (False, True):
    tiny, big = R.act_limits(f16)
    assert R.round_act(tiny, f16) == tiny and R.round_act(-tiny, f16) == -tiny
    assert R.round_act(tiny / 2, f16) == 0.0
    assert R.round_act(1.5 * tiny, f16) == 2 * tiny
    assert R.round_act(big, f16) == big
    assert R.ulp_act(tiny, f16) == tiny and R.ulp_act(0.0, f16) == tiny
    # the largest finite value is one ulp below the next power of two
    assert big + R.ulp_act(big, f16) == 2.0**(16 if f16 else 128)
  # overflow: the halfway point to 2^16 already rounds to infinity
  assert R.round_act(65519.0, True) == 65504.0
  assert R.round_act(65520.0, True) == np.inf
  assert R.round_act(-1e5, True) == -np.inf
  assert R.round_act(1e5, False) == 99840.0
  assert np.signbit(R.round_act(-0.0, True)) and np.signbit(R.round_act(-0.0, False))
  assert R.round_act(1e39, False) == np.inf


def test_ulps_and_sum_bound():
  assert R.ulp_act(1.0, False) == 2.0**-7 and R.ulp_act(1.9, False) == 2.0**-7
  assert R.ulp_act(1.0, True) == 2.0**-10 and R.ulp_act(2.0**-14, True) == 2.0**-24
  assert R.ulp_act(2.0**-20, True) == 2.0**-24
  assert R.ulp_f32(1.0) == 2.0**-23 == float(np.spacing(np.float32(1.0)))
  assert R.ulp_f32(3e-41) == 2.0**-149
  x = np.random.RandomState(6).randn(1000) * 10
  np.testing.assert_array_equal(R.ulp_f32(x), np.spacing(np.abs(x.astype(np.float32))
                                                          ).astype(np.float64))
  assert R.sum_bound([1.0, -2.0, 4.0]) == 3 * 2.0**-24 * 7.0
  np.testing.assert_array_equal(R.sum_bound(np.ones((4, 3)), axis=0),
                                np.full(3, 4 * 2.0**-24 * 4.0))
  # an f32 sum in sequential and pairwise order stays inside it
  t = np.random.RandomState(7).randn(5000).astype(np.float32)
  seq = np.float32(0)
  for a in t:
    seq = np.float32(seq + a)
  exact = t.astype(np.float64).sum()
  assert abs(float(seq) - exact) <= R.sum_bound(t)
  assert abs(float(t.sum(dtype=np.float32)) - exact) <= R.sum_bound(t)
