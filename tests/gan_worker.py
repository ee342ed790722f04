"""Worker of tests/test_hip_gan.py for the vanilla GAN step (--algorithm gan).

  gan_worker.py det STEPS L C U B
      a fresh process trains STEPS train() calls (two eager, then hipGraph
      replays) from fixed weights on a fixed batch and prints one JSON line:
      SHA-256 of every weight tensor + Adam moments, of every step's outputs.
  gan_worker.py dp   (under torch.distributed.run, 2 ranks, gloo)
      one rank of a data-parallel run on the shared GPU; writes
      $DP_WORKER_OUT/gan_rank<r>.npz: the all-reduced gradients of the global
      batch from the rank's shard, and whether the replicas held identical
      weights after every one of a few train() calls."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import bce_oracle as BO
import oracle as O

DP = dict(L=256, C=16, U=16, B=8, seed=11)  # shared with the test


def _gan(L, C, U, m=2):
  from calciumgan_amd.gan.algorithms import get_algorithm
  from calciumgan_amd.gan.models import get_models
  hp = O.make_hparams(L, C, U, kernel_size=24, m=m, layer_norm=True)
  hp.algorithm = 'gan'
  hp.verbose = 0
  gen, dis = get_models(hp, None)
  return hp, gen, dis, get_algorithm(hp, gen, dis, None)


def det():
  steps = int(sys.argv[2])
  L, C, U, B = (int(v) for v in sys.argv[3:7])
  np.random.seed(1234)
  torch.manual_seed(1234)
  hp, gen, dis, gan = _gan(L, C, U)
  rng = np.random.RandomState(7)
  real = torch.from_numpy(rng.uniform(0, 1, (B, L, C)).astype(np.float32)).cuda()
  h = hashlib.sha256()
  for _ in range(steps):
    gl, dl, gp, metrics = gan.train(real)
    assert gp is None
    vals = torch.stack([gl, dl] + list(metrics.values()))
    h.update(vals.cpu().numpy().tobytes())
  torch.cuda.synchronize()
  hw = hashlib.sha256()
  for w in gen.get_weights() + dis.get_weights():
    hw.update(np.ascontiguousarray(w).tobytes())
  for net in (gen.net, dis.net):
    hw.update(net.params.m.cpu().numpy().tobytes())
    hw.update(net.params.v.cpu().numpy().tobytes())
  print(json.dumps({'weights': hw.hexdigest(), 'outputs': h.hexdigest(),
                    'last': [float(v) for v in vals.cpu()],
                    'graph': gan._get_state(B).get('graph') is not None}))


def dp_inputs(hp):
  rng = np.random.RandomState(7)
  real = rng.uniform(0, 1, (DP['B'], DP['L'], DP['C'])).astype(np.float32)
  return real, BO.draw_randomness(hp, DP['B'], seed=DP['seed'])


def dp():
  import torch.distributed as dist
  from calciumgan_amd import parallel
  parallel.init_process_group('gloo')
  rank, world = parallel.rank(), parallel.world_size()
  hp, gen, dis, gan = _gan(DP['L'], DP['C'], DP['U'])
  assert gan._sync.world == world
  real, r = dp_inputs(hp)
  mine = torch.tensor(real[rank::world]).to(gan.device)
  # per-sample draws are sharded like the batch, the shifts are shared
  rm = dict(z=r['z'][rank::world], shifts_real=r['shifts_real'],
            shifts_fake=r['shifts_fake'])
  gan._bce_compute(mine, rm)
  gan._sync.all_reduce(dis.net.params.grad)
  gan._sync.all_reduce(gen.net.params.grad)
  d_grad = (dis.net.params.grad * gan._sync.grad_scale).cpu().numpy()
  g_grad = (gen.net.params.grad * gan._sync.grad_scale).cpu().numpy()
  st = gan._get_state(mine.shape[0])
  loss = st['loss'].double().cpu()
  dist.all_reduce(loss)
  # replicas after every step of eager data-parallel training
  same = []
  for _ in range(4):
    gl, dl, gp, _m = gan.train(mine)
    assert gp is None
    flat = torch.cat([gen.net.params.data, dis.net.params.data]).cpu()
    parts = [torch.empty_like(flat) for _ in range(world)]
    dist.all_gather(parts, flat)
    same.append(all(torch.equal(parts[0], p) for p in parts))
  np.savez(os.path.join(os.environ['DP_WORKER_OUT'],
                        'gan_rank{}.npz'.format(rank)),
           d_grad=d_grad, g_grad=g_grad, loss=(loss / world).numpy(),
           same=np.array(same), finite=np.isfinite([float(gl), float(dl)]))
  dist.barrier()
  dist.destroy_process_group()


if __name__ == '__main__':
  {'det': det, 'dp': dp}[sys.argv[1]]()
