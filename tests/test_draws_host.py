"""The resolver of a train step's draws (gan/algorithms/draws.py) on the host:
for every order its docstring lists, the resolver's output equals, exactly, the
same calls made by hand on an identically seeded second RandomStreams; the two
generators are independent; injected draws come back in the documented layouts;
staged views come back as the same storage."""
import numpy as np
import torch

from calciumgan_amd import parallel
from calciumgan_amd.gan.algorithms import draws

B, ND, N, M = 3, 4, 3, 2
SEED = 1234
CPU = torch.device('cpu')


def _pair():
  return (parallel.RandomStreams(SEED, CPU, M),
          parallel.RandomStreams(SEED, CPU, M))


def _bce_layout(real_s, fake_s):
  """The 12 ints of a BCE step: [fake | real] pairs, then the fake segment's."""
  return torch.tensor([v for f, r in zip(fake_s, real_s) for v in (f, r)] +
                      list(fake_s), dtype=torch.int32)


def _same(got, want):
  assert got.dtype == want.dtype and got.shape == want.shape
  assert torch.equal(got, want)


def test_per_update_pass_order():
  """z_i, alpha_i and shifts(3) per critic update -- whether the pass draws z and
  alpha together (it fuses) or leaves alpha to the critic update -- then the
  generator update's z and shifts(1)."""
  for together in (True, False):
    s, h = _pair()
    for _ in range(N):
      if together:
        z, alpha, none = draws.latents(s, CPU, [None], B, ND)
        assert none is None
      else:
        z = draws.latents(s, CPU, [None], B, ND, alpha=False).z
        alpha = draws.latents(s, CPU, [None], B).alpha
      sh = draws.shifts(s, None, 3)
      _same(z, h.noise(B, ND))
      _same(alpha, h.alpha(B))
      _same(sh, h.shifts(3))
    d = draws.draw(s, CPU, None, B, ND, False, 1)
    _same(d.z, h.noise(B, ND))
    assert d.alpha is None
    _same(d.shifts, h.shifts(1))
    # nothing else was drawn: the streams are where the hand-made calls left them
    _same(s.noise(1, 1), h.noise(1, 1))
    _same(s.shifts(1), h.shifts(1))


def test_batched_pass_order():
  """z of all n B samples, then alpha of all n B, as ONE draw each."""
  s, h = _pair()
  z, alpha, _ = draws.latents(s, CPU, [None] * N, B, ND)
  _same(z, h.noise(N * B, ND))
  _same(alpha, h.alpha(N * B))
  for _ in range(N):
    _same(draws.shifts(s, None, 3), h.shifts(3))
  _same(draws.latents(s, CPU, [None], B, ND, alpha=False).z, h.noise(B, ND))
  _same(draws.shifts(s, None, 1), h.shifts(1))


def test_staged_updates_draw_latents_from_the_streams():
  """A replay: z / alpha from the streams as in an eager step; the shifts are
  the staged view itself."""
  s, h = _pair()
  stage = torch.zeros(draws.critic_stage_words(N), dtype=torch.int32)
  critic, gen, _ = draws.critic_stage(stage, N)
  rs = [draws.staged(v) for v in critic]
  z, alpha, _ = draws.latents(s, CPU, rs, B, ND)
  _same(z, h.noise(N * B, ND))
  _same(alpha, h.alpha(N * B))
  for r, v in zip(rs, critic):
    got = draws.shifts(s, r, 3)
    assert got.data_ptr() == v.data_ptr() and got.shape == (4, 3)
  got = draws.shifts(s, draws.staged(gen), 1)
  assert got.data_ptr() == gen.data_ptr() and got.shape == (4, 1)
  _same(s.shifts(3), h.shifts(3))  # (a staged pass drew none)


def test_bce_step_and_validate_order():
  """z, then ONE shifts(2) = [shifts_real | shifts_fake], laid out for the two
  plans; validate draws the same way."""
  s, h = _pair()
  for _ in range(2):  # (a train step, then a validate pass)
    d = draws.draw(s, CPU, None, B, ND, False, 2)
    _same(d.z, h.noise(B, ND))
    assert d.alpha is None
    sh = h.shifts(2)
    _same(d.shifts, _bce_layout(sh[:, 0].tolist(), sh[:, 1].tolist()))
  stage = torch.zeros(draws.BCE_STAGE_WORDS, dtype=torch.int32)
  words, dis, gen, lr = draws.bce_stage(stage)
  got = draws.draw(s, CPU, draws.staged(words), B, ND, False, 2)
  _same(got.z, h.noise(B, ND))
  assert got.shifts.data_ptr() == stage.data_ptr()
  # the plans' views of the 12 words, and the step sizes behind them
  words.copy_(torch.arange(12, dtype=torch.int32))
  _same(dis, torch.arange(8, dtype=torch.int32).view(4, 2))
  _same(gen, torch.arange(8, 12, dtype=torch.int32).view(4, 1))
  assert lr.dtype == torch.float32 and lr.numel() == 2
  assert lr.data_ptr() == stage[12:].data_ptr()


def test_wgan_validate_order():
  s, h = _pair()
  d = draws.draw(s, CPU, None, B, ND, True, 3)
  _same(d.z, h.noise(B, ND))
  _same(d.alpha, h.alpha(B))
  _same(d.shifts, h.shifts(3))


def test_local_and_shared_are_independent():
  """Shift draws between the z / alpha draws change neither sequence."""
  s, h = _pair()
  zs, alphas, shs = [], [], []
  for i in range(N):
    shs.append(draws.shifts(s, None, 3))
    zs.append(draws.latents(s, CPU, [None], B, ND, alpha=False).z)
    shs.append(draws.shifts(s, None, 1))
    shs.append(draws.shifts(s, None, 2))
    alphas.append(draws.latents(s, CPU, [None], B).alpha)
  for i in range(N):  # all of `local` first, then all of `shared`
    _same(zs[i], h.noise(B, ND))
    _same(alphas[i], h.alpha(B))
  for i in range(N):
    _same(shs[3 * i], h.shifts(3))
    _same(shs[3 * i + 1], h.shifts(1))
    sh = h.shifts(2)
    _same(shs[3 * i + 2], _bce_layout(sh[:, 0].tolist(), sh[:, 1].tolist()))


def _injected(rng):
  sh = lambda: rng.randint(-M, M + 1, size=4).astype(np.int32)
  return dict(z=rng.standard_normal((B, ND)).astype(np.float32),
              alpha=rng.uniform(0, 1, size=B).astype(np.float32),
              shifts_real=sh(), shifts_fake=sh(), shifts_inter=sh())


def test_injected_draws_layouts():
  rng = np.random.RandomState(3)
  s, h = _pair()
  rs = [_injected(rng) for _ in range(N)]
  z, alpha, _ = draws.latents(s, CPU, rs, B, ND)
  _same(z, torch.from_numpy(np.concatenate([r['z'] for r in rs], 0)))
  _same(alpha, torch.from_numpy(np.concatenate([r['alpha'] for r in rs])))
  d = draws.draw(s, CPU, rs[1], B, ND, True, 3)
  _same(d.z, torch.from_numpy(rs[1]['z']))
  _same(d.alpha, torch.from_numpy(rs[1]['alpha']))
  _same(d.shifts, torch.from_numpy(np.stack(
      [rs[1][k] for k in ('shifts_real', 'shifts_fake', 'shifts_inter')], 1)))
  # the generator update: shifts=, as one (4, 1) column
  g = dict(z=rs[0]['z'], shifts=rs[0]['shifts_inter'])
  d = draws.draw(s, CPU, g, B, ND, False, 1)
  assert d.alpha is None
  _same(d.shifts, torch.from_numpy(g['shifts']).reshape(4, 1))
  # the BCE step
  d = draws.draw(s, CPU, rs[2], B, ND, False, 2)
  _same(d.shifts, _bce_layout(rs[2]['shifts_real'].tolist(),
                              rs[2]['shifts_fake'].tolist()))
  # injected draws leave the streams alone
  _same(s.noise(B, ND), h.noise(B, ND))
  _same(s.shifts(3), h.shifts(3))
  # a step's injected structure splits per update; None stays None
  rand = dict(critic=rs, gen=g)
  rc, rg = draws.per_update(rand, N)
  assert rc is rs and rg is g
  assert draws.per_update(None, N) == ([None] * N, None)


def test_critic_stage_views_tile_the_buffer():
  """[shifts x (12 n + 4) | step sizes x (n + 1)]: the views are disjoint, in
  order, and cover every word."""
  words = draws.critic_stage_words(N)
  stage = torch.arange(words, dtype=torch.int32)
  critic, gen, lr = draws.critic_stage(stage, N)
  assert len(critic) == N and lr.dtype == torch.float32
  flat = torch.cat([v.reshape(-1) for v in critic] + [gen.reshape(-1),
                                                       lr.view(torch.int32)])
  _same(flat, stage)
  assert gen.shape == (4, 1) and all(v.shape == (4, 3) for v in critic)
  assert lr.numel() == N + 1
