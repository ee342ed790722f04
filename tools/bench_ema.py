#!/usr/bin/env python
"""Cost of --ema_decay at BASELINE configs[1] shapes (DG sl2048, 102 neurons,
batch 128, num_units 64, m 10, layer_norm): the averaging launch on the
generator's flat buffer, and a whole train() with and without it.

  python tools/bench_ema.py [--reps 30] [--warmup 3] [--rounds 6] [--steps 10]
      [--json profiles/ema_bench.json]

  update_ms      WeightAverage.update() (cg_ema_update, one launch) between two
                 events recorded on the stream: median of --reps calls after
                 --warmup calls, min and max beside it
  adam_ms        cg_adam over a buffer of the same size in the same run, timed
                 the same way: the yardstick (28 bytes per element against 12)
  floor_ms       12 bytes x numel at 5.9 and at 6.6 TB/s, the rates the
                 project's streaming kernels reach (nothing here measures them)
  gb_per_s       12 bytes x numel over update_ms
  train_ms       ms per train() of two algorithm objects built alike, one with
                 ema_decay: --rounds rounds, each timing --steps replayed
                 steps of one object and then of the other (a host clock
                 around a window that ends in a synchronise), in alternating
                 order; the median round of each, and every round beside it.
                 The object without the flag is what a run without it executes.

Before anything is timed one update is compared with the host statement
(averaging.update_statement) bit for bit.  Clocks are whatever the machine runs
at; no time here is a pass criterion.  Prints ONE JSON line (and writes it to
--json)."""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np
import torch


def _each_event(fn, reps):
  out = []
  for _ in range(reps):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    out.append(start.elapsed_time(stop))
  return out


def _window(gan, batches, steps):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for i in range(steps):
    gan.train(batches(i))
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e3 / steps


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--rounds', type=int, default=6)
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--decay', type=float, default=0.999)
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  import bench
  from calciumgan_amd import _lib
  from calciumgan_amd.data import dg
  from calciumgan_amd.gan.algorithms import averaging, get_algorithm
  from calciumgan_amd.gan.models import get_models
  torch.cuda.set_device(0)
  L, C, U, m, B = 2048, 102, 64, 10, 128

  def build(ema):
    hp = bench.make_hparams(L, C, U, m)
    if ema:
      hp.ema_decay = args.decay
    gen, dis = get_models(hp, None)
    return get_algorithm(hp, gen, dis, None)

  plain, averaged = build(False), build(True)
  avg = averaged.average
  params = averaged.generator.net.params
  numel = params.numel

  # the check: one update of a shadow that differs from the weights
  avg.shadow.mul_(0.5)
  e, p = avg.shadow.cpu().numpy(), params.data.cpu().numpy()
  om = averaging.one_minus(averaging.decay_at(args.decay, avg.updates))
  avg.update()
  torch.cuda.synchronize()
  want = averaging.update_statement(e, p, om)
  if avg.shadow.cpu().numpy().tobytes() != want.tobytes():
    raise SystemExit('cg_ema_update differs from update_statement')
  avg.shadow.copy_(params.data)
  avg.updates = 0

  # the launch alone, and Adam on buffers of the same size beside it
  for _ in range(args.warmup):
    avg.update()
  update_ms = _each_event(avg.update, args.reps)
  avg.shadow.copy_(params.data)
  avg.updates = 0
  pa, ga = params.data.clone(), torch.randn_like(params.data) * 1e-3
  ma, va = torch.zeros_like(pa), torch.zeros_like(pa)

  def adam():
    _lib.call('cg_adam', pa, ga, ma, va, numel, 1e-4, 0.9, 0.999, 1e-7, 1.0,
              None, _lib.stream())

  for _ in range(args.warmup):
    adam()
  adam_ms = _each_event(adam, args.reps)
  del pa, ga, ma, va

  # train() with and without, alternating in this process
  data = dg.make_dataset(C, L, num_segments=4 * B, seed=1234)
  dataset = torch.from_numpy(data['signals']).to(plain.device)
  gsteps = torch.Generator().manual_seed(99)
  index = [torch.randperm(4 * B, generator=gsteps)[:B].to(plain.device)
           for _ in range(16)]

  def feeder(gan):
    real = gan.batch_buffer(B)

    def batches(i):
      torch.index_select(dataset, 0, index[i % len(index)], out=real)
      return real
    return batches

  feed = {id(plain): feeder(plain), id(averaged): feeder(averaged)}
  for gan in (plain, averaged):  # two eager calls, the capture, two replays
    _window(gan, feed[id(gan)], 5)
  rounds = {'plain': [], 'ema': []}
  for r in range(args.rounds):
    order = [('plain', plain), ('ema', averaged)]
    for name, gan in (order if r % 2 == 0 else order[::-1]):
      rounds[name].append(_window(gan, feed[id(gan)], args.steps))
  graphs = all(g._use_graph and g._get_state(B).get('graph') is not None
               for g in (plain, averaged))

  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  moved = 12 * numel
  up, ad = statistics.median(update_ms), statistics.median(adam_ms)
  tp, te = statistics.median(rounds['plain']), statistics.median(rounds['ema'])
  res = {
      'metric': 'cg_ema_update over the generator of cfg2 ({} floats, {:.1f} MB) '
                'and train() with / without --ema_decay'.format(numel,
                                                                4 * numel / 1e6),
      'numel': numel,
      'update_ms': up,
      'update_ms_min': min(update_ms),
      'update_ms_max': max(update_ms),
      'adam_ms': ad,
      'adam_ms_min': min(adam_ms),
      'adam_ms_max': max(adam_ms),
      'update_over_adam': up / ad,
      'moved_mb': moved / 1e6,
      'floor_ms_at_6p6_tb_s': moved / 6.6e12 * 1e3,
      'floor_ms_at_5p9_tb_s': moved / 5.9e12 * 1e3,
      'gb_per_s': moved / 1e9 / (up * 1e-3),
      'train_ms_plain': tp,
      'train_ms_ema': te,
      'train_ms_difference': te - tp,
      'train_ms_plain_rounds': rounds['plain'],
      'train_ms_ema_rounds': rounds['ema'],
      'train_replayed_as_graphs': graphs,
      'bit_exact_against_statement': True,
      'decay': args.decay,
      'reps': args.reps,
      'warmup': args.warmup,
      'rounds': args.rounds,
      'steps_per_round': args.steps,
      'n_gpus': 1,
      'gpu': torch.cuda.get_device_name(0),
      'box': socket.gethostname(),
      'commit': commit,
      'conditions': 'one MI355X, one run, clocks not pinned',
  }
  line = json.dumps(res)
  if args.json:
    with open(args.json, 'w') as f:
      f.write(line + '\n')
  print(line)


if __name__ == '__main__':
  main()
