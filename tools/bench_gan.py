#!/usr/bin/env python
"""Samples/s of the vanilla GAN step (--algorithm gan, reference
gan/algorithms/gan.py:72-85) at BASELINE configs[1]'s shapes: DG sl2048, 102
neurons, batch 128, num_units 64, k 24, s 2, m 10, layer_norm, bf16, hipGraph
replay of train() on one GPU.

  python tools/bench_gan.py --steps K --warmup W [--batch 128] [--mixed_precision]

The timing rules are bench.py's: a resident dataset of a few batches, every
step gathers ITS batch into gan.batch_buffer() inside the timed region,
synchronize on both sides of the K timed steps.  Prints ONE JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import torch


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--seq_len', type=int, default=2048)
  ap.add_argument('--neurons', type=int, default=102)
  ap.add_argument('--num_units', type=int, default=64)
  ap.add_argument('--m', type=int, default=10)
  ap.add_argument('--mixed_precision', action='store_true')
  args = ap.parse_args()
  if args.steps < 1:
    ap.error('--steps must be at least 1')
  import bench
  from calciumgan_amd.data import dg
  from calciumgan_amd.gan.algorithms import get_algorithm
  from calciumgan_amd.gan.models import get_models
  torch.cuda.set_device(0)
  hp = bench.make_hparams(args.seq_len, args.neurons, args.num_units, args.m,
                          args.mixed_precision)
  hp.algorithm = 'gan'
  gen, dis = get_models(hp, None)
  gan = get_algorithm(hp, gen, dis, None)
  B = args.batch
  nseg = B * 4
  data = dg.make_dataset(args.neurons, args.seq_len, num_segments=nseg,
                         seed=1234)
  dataset = torch.from_numpy(data['signals']).to(gan.device)
  real = gan.batch_buffer(B)
  gsteps = torch.Generator().manual_seed(99)
  total = args.warmup + args.steps
  index = [torch.randperm(nseg, generator=gsteps)[:B].to(gan.device)
           for _ in range(min(total, 64))]

  def next_batch(i):
    torch.index_select(dataset, 0, index[i % len(index)], out=real)
    return real

  for i in range(args.warmup):
    gan.train(next_batch(i))
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for i in range(args.steps):
    out = gan.train(next_batch(args.warmup + i))
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  st = gan._get_state(B)
  print(json.dumps({
      'metric': 'training samples/sec, --algorithm gan (seq_len={})'.format(
          args.seq_len),
      'value': B * args.steps / dt,
      'unit': 'samples/s',
      'n_gpus': 1,
      'steps': args.steps,
      'warmup': args.warmup,
      'ms_per_step': dt / args.steps * 1e3,
      'dtype': 'f16' if args.mixed_precision else 'bf16',
      'config': dict(seq_len=args.seq_len, neurons=args.neurons, batch=B,
                     num_units=args.num_units, m=args.m),
      'launch': ('hipGraph replay of train()' if st.get('graph') is not None
                 else 'eager launches'),
      'final_losses': [float(out[0]), float(out[1])],
  }))


if __name__ == '__main__':
  main()
