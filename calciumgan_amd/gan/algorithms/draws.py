"""Where a train step's randomness comes from -- the only code that looks.

A step's random inputs are the noise z, the interpolation factors alpha and
the PhaseShuffle shifts.  `r` names their source for one update:
  None               the process's own streams (parallel.RandomStreams)
  staged(view)       a graph replay: z / alpha still come from the streams, the
                     shifts were copied to device memory ahead of the replay
                     (replay._stage, filled by the algorithm's _fill_stage) and
                     `view` is where the launches read them
  a dict             draws injected by a parity test: z=, alpha=, and
                     shifts_real= / shifts_fake= / shifts_inter= (a critic or
                     BCE pass) or shifts= (the generator update), 4 ints each

The contract.  z and alpha come from RandomStreams.local, the per-rank device
generator that the captured graphs register; the shifts come from
RandomStreams.shared, a host generator that is identical on all ranks.  The
two are independent: only the order WITHIN each must be preserved, and that
order is what makes a replayed step reproduce an eager one bit for bit
(tests/test_determinism.py).  Per schedule, with B samples and n critic
updates per step:

  per-update pass   local:  z_0 (B), alpha_0 (B), z_1, alpha_1, ... z_g (B)
  (data parallel, BatchNorm generators, CALCIUMGAN_BATCH_G=0)
                    shared: shifts(3) per critic update, then shifts(1)
  batched pass      local:  z (n B), alpha (n B), then z_g (B)
  (single rank)     shared: as above
  BCE step          local:  z (B)
                    shared: ONE shifts(2) = [shifts_real | shifts_fake]
  validate          local:  z (B), then (WGAN-GP, MLP) alpha (B)
                    shared: shifts(3) (WGAN-GP), one shifts(2) (BCE), none (MLP)
  MLP step          local:  z_0, alpha_0, ... z_g;  shared: none (no shuffle)

A replay draws its shifts on the host ahead of time (_fill_stage) in the same
`shared` order.  The functions below need neither a GPU nor a GAN object.
"""
import collections

import torch

# one discriminator pass: a field is None when the pass does not use it
Draws = collections.namedtuple('Draws', 'z alpha shifts')

_STAGED = 'shifts_dev'
# injected shifts of a pass with nseg segments, in the order of streams.shifts
_SHIFT_KEYS = {1: ('shifts',), 2: ('shifts_real', 'shifts_fake'),
               3: ('shifts_real', 'shifts_fake', 'shifts_inter')}


def staged(view):
  """The `r` of an update whose shifts sit in device memory at `view`."""
  return {_STAGED: view}


def per_update(rand, n):
  """([r of critic update i] * n, r of the generator update) of a step's
  injected draws `rand` (the structure of oracle.draw_randomness) or of None."""
  if rand is None:
    return [None] * n, None
  return rand['critic'], rand['gen']


def to_device(x, device):
  if not torch.is_tensor(x):
    x = torch.as_tensor(x)
  return x.to(device=device, dtype=torch.float32).contiguous()


def latents(streams, device, rs, B, noise_dim=None, alpha=True):
  """z and alpha of the len(rs) consecutive updates whose sources are `rs`, as
  ONE draw each: z (k B, noise_dim) when noise_dim is given, then alpha (k B,)
  when asked.  Injected draws are concatenated from the per-update dicts."""
  k = len(rs)
  if rs[0] is None or _STAGED in rs[0]:
    return Draws(
        None if noise_dim is None else streams.noise(k * B, noise_dim),
        streams.alpha(k * B) if alpha else None, None)
  cat = lambda ts: ts[0] if k == 1 else torch.cat(ts, 0)
  return Draws(
      None if noise_dim is None else
      cat([to_device(r['z'], device) for r in rs]),
      cat([to_device(r['alpha'], device).reshape(-1) for r in rs])
      if alpha else None, None)


def shifts(streams, r, nseg):
  """The PhaseShuffle draws of one discriminator pass with nseg segments: host
  int32 (4, nseg), columns [real | fake | x^] of a critic update or the one of
  the generator update -- or the staged device view.  nseg = 2 is the BCE step:
  its ONE draw [real | fake] comes back as the 12 ints its plans read, the (4, 2)
  [fake | real] of the 2B plan, then the fake segment's four for the G chain."""
  if r is not None and _STAGED in r:
    return r[_STAGED]
  if r is None:
    sh = streams.shifts(nseg)
  else:
    sh = torch.stack([torch.as_tensor(r[k], dtype=torch.int32).reshape(4)
                      for k in _SHIFT_KEYS[nseg]], dim=1)
  if nseg == 2:
    real_s, fake_s = sh[:, 0], sh[:, 1]
    return torch.cat([torch.stack([fake_s, real_s], 1).reshape(-1), fake_s])
  return sh


def draw(streams, device, r, B, noise_dim, alpha, nseg):
  """The Draws of one whole pass, in its order: z, alpha, shifts."""
  d = latents(streams, device, [r], B, noise_dim, alpha)
  return d._replace(shifts=shifts(streams, r, nseg))


# -- the staged words of a step: st['stage_dev'], replay.py's pinned slots ---
def critic_stage_words(n):
  return 13 * n + 5


def critic_stage(stage, n):
  """Views of a WGAN-GP step's [shifts int32 x (12 n + 4) | Adam step sizes f32
  x (n + 1)]: ([critic update i's (4, 3)] * n, the generator update's (4, 1),
  the step sizes).  The plans read their shifts straight from the device copy:
  a replay needs ONE staged copy and none into the plans."""
  return ([stage[12 * i:12 * i + 12].view(4, 3) for i in range(n)],
          stage[12 * n:12 * n + 4].view(4, 1),
          stage[12 * n + 4:].view(torch.float32))


BCE_STAGE_WORDS = 14


def bce_stage(stage):
  """Views of a BCE step's [2B plan shifts int32 (4, 2) | fake-segment plan
  shifts (4, 1) | Adam step sizes f32 (D, G)]: (the 12 shift words that
  shifts(., ., 2) lays out, the two plans' views of them, the step sizes)."""
  return (stage[:12], stage[0:8].view(4, 2), stage[8:12].view(4, 1),
          stage[12:].view(torch.float32))
