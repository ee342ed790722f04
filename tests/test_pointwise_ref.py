"""CPU checks of tests/pointwise_ref.py: every float64 statement the GPU parity
tests of tests/test_hip_pointwise.py compare a kernel with is tied here to an
independent one -- torch autograd in float64 or the oracle of
oracle/calciumgan_oracle.py -- and the rounding helpers to hand-picked values."""
import decimal

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


# ---------------------------------------------------------------------------
# the BCE head and the loss-scale state machine
# ---------------------------------------------------------------------------
def test_bce_head_under_autograd_f64():
  """R.bce_head against binary_cross_entropy_with_logits on a LeakyReLU -> linear
  head in float64: the losses, d(S_d loss[1]) / dy = delta_d and, over the fake
  segment, d(S_g loss[0]) / dy = delta_g -- at logits within +-30, where autograd's
  own sigmoid is accurate."""
  bcel = torch.nn.functional.binary_cross_entropy_with_logits
  rng = np.random.RandomState(8)
  alpha = 0.3
  for B, Lt, C, Cp, S_d, S_g in ((1, 2, 3, 8, 1.0, 1.0), (5, 4, 6, 8, 1024.0, 256.0),
                                 (9, 3, 8, 8, 2.0, 0.5)):
    y = rng.randn(2 * B, Lt, Cp) * 8
    y[:, :, C:] = 0.0
    w = rng.randn(Lt, C) / np.sqrt(Lt * C)
    yt = torch.tensor(y, dtype=F64, requires_grad=True)
    ht = torch.nn.functional.leaky_relu(yt, alpha)
    x = (ht[:, :, :C] * torch.tensor(w)[None]).sum((1, 2)) + 0.25
    assert float(x.detach().abs().max()) <= 30
    loss0 = bcel(x[:B], torch.ones(B, dtype=F64))
    loss1 = bcel(x[B:], torch.ones(B, dtype=F64)) + bcel(x[:B],
                                                        torch.zeros(B, dtype=F64))
    gd, = torch.autograd.grad(S_d * loss1, yt, retain_graph=True)
    gg, = torch.autograd.grad(S_g * loss0, yt)
    r = R.bce_head(ht.detach().numpy(), w, 0.25, B, alpha, S_d, S_g)
    np.testing.assert_allclose(r['x'], x.detach().numpy(), rtol=1e-13)
    np.testing.assert_allclose(r['loss'], [loss0.item(), loss1.item()], rtol=1e-12)
    np.testing.assert_allclose(r['delta_d'], gd.numpy(), rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(r['delta_g'], gg.numpy()[:B], rtol=1e-11, atol=1e-300)
    assert (gg.numpy()[B:] == 0).all()
    assert (r['delta_d'][:, :, C:] == 0).all() and (r['delta_g'][:, :, C:] == 0).all()
    # the per-sample terms are the unreduced losses
    none = lambda t: bcel(x, torch.full((2 * B,), t, dtype=F64), reduction='none')
    # (torch's own log(1 + e) is absolute-accurate only: 1e-15 on terms of 1e-4)
    np.testing.assert_allclose(r['t0'], none(0.0).detach().numpy(), rtol=1e-12,
                               atol=1e-14)
    np.testing.assert_allclose(r['t1'], none(1.0).detach().numpy(), rtol=1e-12,
                               atol=1e-14)
    np.testing.assert_array_equal(r['td'], np.r_[r['t0'][:B], r['t1'][B:]])
    np.testing.assert_array_equal(r['tg'], r['t1'][:B])


def test_bce_statement_keeps_its_accuracy_at_the_planted_logits():
  """Against 60-digit closed forms where they are simple: x = +-0 gives log 2
  and +-1/2; at x = +-104 the small side is e^-104 to float64's accuracy."""
  x = np.array([0.0, -0.0, 104.0, -104.0])
  r = R.bce_from_logits(np.r_[x, x], 4, 8.0, 2.0)
  np.testing.assert_array_equal(r['t0'][:2], [np.log(2.0)] * 2)
  np.testing.assert_array_equal(r['coef_d'][:2], [8.0 / 8] * 2)        # S_d / (2B)
  np.testing.assert_array_equal(r['coef_d'][4:6], [-8.0 / 8] * 2)      # -S_d / (2B)
  np.testing.assert_array_equal(r['coef_g'][:2], [-2.0 / 8] * 2)       # -S_g / (2B)
  tiny = float(decimal.Context(prec=60).exp(decimal.Decimal(-104)))  # e^-104
  np.testing.assert_allclose([r['t1'][2], r['t0'][3]], [tiny] * 2, rtol=1e-14)
  np.testing.assert_allclose([r['t0'][2], r['t1'][3]], [104.0] * 2, rtol=1e-15)
  np.testing.assert_allclose(r['coef_d'][[3, 6]], [8 * tiny / 4, -8 * tiny / 4],
                             rtol=1e-14)
  np.testing.assert_allclose(r['coef_g'][2], -2 * tiny / 4, rtol=1e-14)


@np.errstate(over='ignore', divide='ignore')
def test_the_bce_bars_bite_on_the_naive_f32_forms():
  """The naive f32 forms -- log(1 + exp(-x)), 1 / (1 + exp(-x)) without the sign
  split, s(x) - 1 -- evaluated with numpy float32 at the planted logits each miss
  the bars the GPU test applies, by factors no libm allowance could hide; the
  bars themselves are a few spacings of the result everywhere."""
  f = np.float32
  for f16 in (False, True):
    x = R.bce_planted_logits(f16)
    B = len(x)
    x2 = np.r_[x, x]
    r, bar = R.bce_from_logits(x2, B), R.bce_bars(x2, B)
    x32 = x.astype(f)
    one = f(1)
    inv_b = one / f(B)
    # BCE(1, x) = log(1 + exp(-x)): overflows for x <= -89, loses e^-x from x = 17
    t1 = np.log(one + np.exp(-x32))
    miss = np.abs(t1.astype(np.float64) - r['t1'][:B]) / bar['t1'][:B]
    assert miss[x == -89].min() > 1e6 and miss[x == 20].min() > 1e6, miss
    # mutation of the kernel's line: logf(1 + expf(-|x|)) in place of log1pf
    t1m = np.maximum(x32, 0) - x32 + np.log(one + np.exp(-np.abs(x32)))
    miss = np.abs(t1m.astype(np.float64) - r['t1'][:B]) / bar['t1'][:B]
    assert miss[x == 20].min() > 1e6 and miss[x == 88].min() > 1e5, miss
    # s(x) without the sign split: exp(-x) overflows, the seed is flushed to 0
    s = one / (one + np.exp(-x32))
    cd = (s * inv_b).astype(np.float64)
    miss = np.abs(cd - r['coef_d'][:B]) / bar['coef_d'][:B]
    assert miss[x == -89].min() > 1e4, miss
    # s(x) - 1 on the real segment and for the generator: cancels from x = 17
    cr = ((s - one) * inv_b).astype(np.float64)
    miss = np.abs(cr - r['coef_d'][B:]) / bar['coef_d'][B:]
    assert miss[x == 20].min() > 1e6 and miss[x == 40].min() > 1e6, miss
    miss = np.abs(cr - r['coef_g']) / bar['coef_g']
    assert miss[x == 20].min() > 1e6, miss
    # every bar is a small number of spacings of its result (2^-149 at least)
    for k, width in (('t0', 5), ('t1', 5), ('coef_d', 9), ('coef_g', 9)):
      assert (bar[k] <= width * R.ulp_f32(r[k])).all(), k
      assert (bar[k] >= 0.5 * R.ulp_f32(r[k])).all(), k


def test_loss_scale_update_follows_the_oracles_dynamic_loss_scale():
  """Doubles on the interval-th finite update, halves on a non-finite one, sits on
  the floor of 1; t counts the applied updates only."""
  good, bad = [torch.ones(3)], [torch.tensor([1.0, float('inf')])]
  for S0, interval, flags in ((4.0, 2, [1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 1]),
                              (2.0**15, 3, [1, 1, 0, 1, 1, 1, 1, 1, 1, 0]),
                              (1.5, 1, [0, 0, 1, 1, 0])):
    orc = O.DynamicLossScale(S0, interval)
    ls = np.array([S0, 0.0, 0.0, 1.0], np.float32)
    applied = 0
    seen = set()
    for flag in flags:
      ls[3] = flag  # what cg_grad_finite leaves
      ls = R.loss_scale_update(ls, interval)
      applied += int(orc.update(good if flag else bad))
      assert list(ls) == [orc.scale, orc.good_steps, applied, 1.0], (S0, flag, ls)
      seen.add(float(ls[0]))
    if S0 == 4.0:  # this sequence doubles, halves and sits on the floor
      assert 1.0 in seen and max(seen) > S0
  # 2^127 doubles to infinity in f32: S stays, the count restarts
  np.testing.assert_array_equal(
      R.loss_scale_update([2.0**127, 4.0, 9.0, 1.0], 5), [2.0**127, 0.0, 10.0, 1.0])
  assert list(R.loss_scale_update([1.5, 3.0, 9.0, 0.0], 5)) == [1.0, 0.0, 9.0, 1.0]
