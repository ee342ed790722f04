#!/usr/bin/env python
"""Time of the validation-time spike statistics of ONE batch at BASELINE
configs[1]'s shapes (B = 128, L = 2048, C = 102, DG traces from data/dg.py) on
one GPU, beside the host path on the same traces:

  python tools/bench_spike_stats.py [--reps 10] [--warmup 2] [--batch 128]
      [--cpus 16] [--json profiles/spike_stats_bench.json]

  device_deconvolve_ms   cg_oasis_ar1_batched on the (B, L, 128-pitch) batch
  device_statistics_ms   cg_spike_stats of the fake trains + cg_spike_stats_error
                         against kept real-side statistics
  device_total_ms        (a) what GAN.spike_statistics costs per validation batch
  host_deconvolve_s      (b) spike_helper.deconvolve_signals on the same traces,
                         single-threaded as that code runs
  host_deconvolve_pool_s (b') (b) / --cpus: the best a process pool over the
                         CPUs a job may use could do (not run: a bound)

The timing rules are tools/bench_gan.py's: synchronize on both sides of the
timed launches, warm-up calls first (they also allocate the workspace and upload
the power table).  The device trains are checked against the host's before
anything is timed.  Prints ONE JSON line (and writes it to --json)."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np
import torch


def _timed(fn, reps):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(reps):
    out = fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / reps * 1e3, out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--seq_len', type=int, default=2048)
  ap.add_argument('--neurons', type=int, default=102)
  ap.add_argument('--cpus', type=int, default=16)
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  from calciumgan_amd import _lib
  from calciumgan_amd.data import dg
  from calciumgan_amd.gan.utils import spike_helper, spike_metrics
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  B, L, C = args.batch, args.seq_len, args.neurons
  d = dg.make_dataset(C, L, num_segments=B, seed=1234)
  smin, smax = float(d['info']['signals_min']), float(d['info']['signals_max'])
  sig = np.ascontiguousarray(d['signals'], dtype=np.float32)  # normalised
  # the generator's output layout: channel pitch 128
  buf = torch.zeros(B, L, 128 if C <= 128 else C, dtype=torch.float32, device=dev)
  buf[:, :, :C] = torch.from_numpy(sig).to(dev)
  fake = buf[:, :, :C]
  real = torch.from_numpy(np.ascontiguousarray(d['spikes'], dtype=np.float32)).to(dev)
  real_stats = spike_metrics.batch_statistics_device(real)

  deconv = lambda: spike_helper.deconvolve_signals_device(
      fake, scale=smax - smin, offset=smin)

  def stats(trains):
    r, c = spike_metrics.batch_statistics_device(trains)
    return spike_metrics.error_sums_device(real_stats[0], r, real_stats[1], c)

  for _ in range(args.warmup):
    trains = deconv()
    stats(trains)
  # (b) the host path on the same traces, and the check that both agree
  host_in = (sig * np.float32(smax - smin) + np.float32(smin)).transpose(
      0, 2, 1).reshape(B * C, L)
  t0 = time.perf_counter()
  host_trains = spike_helper.deconvolve_signals(host_in)
  host_s = time.perf_counter() - t0
  same = bool(np.array_equal(
      trains.cpu().numpy().transpose(0, 2, 1).reshape(B * C, L), host_trains))
  ms_deconv, trains = _timed(deconv, args.reps)
  ms_stats, sums = _timed(lambda: stats(trains), args.reps)
  ms_total, _ = _timed(lambda: stats(deconv()), args.reps)
  try:
    commit = args.commit or subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'],
                                     cwd=ROOT, stderr=subprocess.DEVNULL
                                     ).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  res = {
      'metric': 'spike statistics of one validation batch (B={}, L={}, C={})'.
                format(B, L, C),
      'device_deconvolve_ms': ms_deconv,
      'device_statistics_ms': ms_stats,
      'device_total_ms': ms_total,
      'host_deconvolve_s': host_s,
      'host_deconvolve_pool_s': host_s / args.cpus,
      'cpus': args.cpus,
      'device_beats_pool_bound': bool(ms_total * 1e-3 < host_s / args.cpus),
      'trains_identical_to_host': same,
      'spikes_per_trace': float(host_trains.sum() / len(host_trains)),
      'workspace_bytes': int(_lib.load().cg_oasis_ws_bytes(B * C, L)),
      'error_sums': [float(v) for v in sums],
      'reps': args.reps,
      'warmup': args.warmup,
      'n_gpus': 1,
      'gpu': torch.cuda.get_device_name(0),
      'box': socket.gethostname(),
      'commit': commit,
  }
  line = json.dumps(res)
  if args.json:
    with open(args.json, 'w') as f:
      f.write(line + '\n')
  print(line)


if __name__ == '__main__':
  main()
