#!/usr/bin/env python
"""Time of one epoch's --plot_weights work at BASELINE configs[2]'s models
(--num_units 64 --layer_norm on (2048, 102) signals): statistics and 30-bucket
histograms of every trainable variable of the generator and the discriminator.

  python tools/bench_tensor_summary.py [--reps 30] [--warmup 3]
      [--json profiles/tensor_summary_bench.json]

  event_ms       both models' FlatParams.summaries_host (one cg_tensor_summary
                 call of five launches and one device-to-host copy of the rows
                 per model) between two events recorded on the stream: median
                 of --reps warm runs; min and max beside it
  device_ms      the same runs on the host clock, a synchronize on both sides
  host_s         the route without the kernel: get_weights() (one device-to-host
                 copy per variable) and the numpy statements
                 (summary_helper.variable_statistics / histogram_buckets) on
                 this machine's CPU, best of two
  param_mb       bytes of the summarised variables; floor_us is two reads of
                 them at 6 TB/s (the streaming kernels of this library measure
                 5.9 - 6.6 TB/s): what the launches cannot go below
  copied_kb      what comes to the host: (8 + 3 x 30) float64 per variable

Before anything is timed the device result is compared with the statements:
counts, edges, minimum and maximum exactly, sum and sq within the summation
bounds of tests/test_hip_tensor_summary.py.  Clocks are whatever the machine
runs at; no time here is a pass criterion.  Prints ONE JSON line (and writes it
to --json)."""
import argparse
import json
import math
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

K = 30
U = 2.0**-53


def _each(fn, reps):
  """ms of every one of `reps` runs."""
  out = []
  for _ in range(reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    out.append((time.perf_counter() - t0) * 1e3)
  return out


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


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _check(params, stats, buckets):
  from calciumgan_amd.gan.utils import summary_helper as sh
  weights = params.get_weights()
  for row, i in enumerate(params.summary_indices(True)):
    d = weights[i].astype(np.float64).reshape(-1)
    n, st, what = float(d.size), stats[row], params.names[i]
    rows = sh.histogram_buckets(weights[i], K)
    got = buckets[row][:1] if st[1] == st[2] else buckets[row]
    ok = (st[0] == n and st[7] == 0 and st[1] == d.min() and st[2] == d.max() and
          np.array_equal(_bits(got), _bits(rows)) and
          abs(st[3] - math.fsum(d)) <= 2 * n * U * math.fsum(np.abs(d)))
    c = d - st[4]
    ok = ok and abs(st[5] - math.fsum(c * c)) <= 2 * (n + 4) * U * math.fsum(c * c)
    ok = ok and st[4] == st[3] / n and st[6] == math.sqrt(st[5] / n)
    if not ok:
      raise SystemExit('{}: the device summary differs from the statement'
                       .format(what))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--num_units', type=int, default=64)
  ap.add_argument('--seq_len', type=int, default=2048)
  ap.add_argument('--neurons', type=int, default=102)
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  import oracle as O
  from calciumgan_amd.gan.models import get_models
  from calciumgan_amd.gan.utils import summary_helper as sh
  torch.cuda.set_device(0)
  hp = O.make_hparams(args.seq_len, args.neurons, num_units=args.num_units,
                      m=10, layer_norm=True)
  hp.verbose = 0
  gen, dis = get_models(hp, None)
  models = [gen.net.params, dis.net.params]
  reps = max(args.reps, 20)

  def device():
    return [p.summaries_host(K, trainable_only=True) for p in models]

  for p, (stats, buckets) in zip(models, device()):
    _check(p, stats, buckets)

  host = []
  for _ in range(2):
    t0 = time.perf_counter()
    for p in models:
      weights = p.get_weights()
      for i in p.summary_indices(True):
        sh.variable_statistics(weights[i])
        sh.histogram_buckets(weights[i], K)
    host.append(time.perf_counter() - t0)

  for _ in range(args.warmup):
    device()
  wall_ms = _each(device, reps)
  event_ms = _each_event(device, reps)
  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  variables = sum(len(p.summary_indices(True)) for p in models)
  elements = sum(int(np.prod(p.shapes[i])) for p in models
                 for i in p.summary_indices(True))
  ev = statistics.median(event_ms)
  res = {
      'metric': 'statistics and {}-bucket histograms of the {} trainable '
                'variables ({} parameters) of generator and discriminator, '
                'num_units={}, L={}, C={}, layer_norm: one epoch of '
                '--plot_weights'.format(K, variables, elements, args.num_units,
                                        args.seq_len, args.neurons),
      'event_ms': ev,
      'event_ms_min': min(event_ms),
      'event_ms_max': max(event_ms),
      'device_ms': statistics.median(wall_ms),
      'device_ms_min': min(wall_ms),
      'device_ms_max': max(wall_ms),
      'host_s': min(host),
      'variables': variables,
      'parameters': elements,
      'param_mb': 4 * elements / 1e6,
      'read_mb': 2 * 4 * elements / 1e6,
      'floor_us': 2 * 4 * elements / 6e12 * 1e6,
      'copied_kb': 8 * variables * (8 + 3 * K) / 1e3,
      'host_copied_mb': 4 * elements / 1e6,
      'launches': 5 * len(models),
      'equal_to_the_statements': True,
      'device_faster_than_host': bool(statistics.median(wall_ms) * 1e-3 <
                                      min(host)),
      'reps': reps,
      'warmup': args.warmup,
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
