#!/usr/bin/env python
"""Time of one WGAN-GP train() on the MLP pair (--model mlp) at the surrogate
experiment's shapes: batch 64, 6 time steps, 2 channels, num_units 32, noise 32,
dropout 0.2, n_critic 5, eager launches.

  python tools/bench_mlp.py [--steps 1000] [--warmup 50]
      [--json profiles/mlp_bench.json]

  ms_per_train        wall time of --steps train() calls between two
                      synchronizes, divided by --steps
  launches_per_train  kernels of the project's library per train(): entry-point
                      calls, cg_mlp_dense_wgrad counted twice (partial sums and
                      the finishing launch).  torch's own launches -- the noise
                      and alpha draws, the copy of the seven outputs -- are not
                      in it; torch_ops_per_train counts those calls

The step is launch-bound at these shapes (the largest Dense is 384 rows x 128
-> 96), so the time is mostly the host's.  Clocks are whatever the machine runs
at; nothing here is a pass criterion.  Prints ONE JSON line (and writes it to
--json)."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np
import torch


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--warmup', type=int, default=50)
  ap.add_argument('--batch_size', type=int, default=64)
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  from calciumgan_amd import _lib
  from calciumgan_amd.gan.algorithms import get_algorithm
  from calciumgan_amd.gan.models import get_models
  torch.cuda.set_device(0)
  B, L, C, U, nd = args.batch_size, 6, 2, 32, 32
  hp = SimpleNamespace(
      signal_shape=(L, C), sequence_length=L, num_channels=C, num_neurons=C,
      noise_dim=nd, noise_shape=(nd,), num_units=U, dropout=0.2,
      activation='leakyrelu', normalize=True, m=2, gradient_penalty=10.0,
      n_critic=5, learning_rate=1e-4, signals_min=0.0, signals_max=1.0,
      batch_norm=False, layer_norm=False, mixed_precision=False, model='mlp',
      algorithm='wgan-gp', verbose=0)
  gen, dis = get_models(hp, None)
  gan = get_algorithm(hp, gen, dis, None)
  real = torch.from_numpy(np.random.RandomState(0).uniform(
      0, 1, (B, L, C)).astype(np.float32)).cuda()

  for _ in range(args.warmup):
    out = gan.train(real)
  torch.cuda.synchronize()
  if not all(np.isfinite(float(v)) for v in out[:3]):
    raise SystemExit('non-finite losses after the warm-up: {}'.format(out[:3]))

  # count one step's launches
  counts = {'calls': 0, 'wgrad': 0}
  real_call = _lib.call

  def counting(name, *a):
    counts['calls'] += 1
    counts['wgrad'] += name == 'cg_mlp_dense_wgrad'
    return real_call(name, *a)

  _lib.call = counting
  try:
    gan.train(real)
  finally:
    _lib.call = real_call
  n = hp.n_critic
  torch_ops = 2 * n + 1 + 1  # z and alpha per critic update, z, the output copy

  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(args.steps):
    gan.train(real)
  torch.cuda.synchronize()
  ms = (time.perf_counter() - t0) * 1e3 / args.steps
  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  res = {
      'metric': 'WGAN-GP train() on the MLP pair: B {} L {} C {} U {} noise {}, '
                'dropout 0.2, n_critic {}, eager'.format(B, L, C, U, nd, n),
      'ms_per_train': ms,
      'launches_per_train': counts['calls'] + counts['wgrad'],
      'library_calls_per_train': counts['calls'],
      'torch_ops_per_train': torch_ops,
      'steps': args.steps,
      'warmup': args.warmup,
      'n_gpus': 1,
      'gpu': torch.cuda.get_device_name(0),
      'box': socket.gethostname(),
      'commit': commit,
      'conditions': 'one MI355X, one run, clocks not pinned, eager launches',
  }
  line = json.dumps(res)
  if args.json:
    with open(args.json, 'w') as f:
      f.write(line + '\n')
  print(line)


if __name__ == '__main__':
  main()
