#!/usr/bin/env python
"""Time of the histogram KL of compute_metrics.py --device gpu at BASELINE
configs[1]'s shapes: 128 trials (T = 2048, C = 102), the van Rossum matrices of
two different draws of DG spike trains (data/dg.py, two seeds) as the recorded
and the synthetic side, so a pair is 2 x 5 151 distances.

  python tools/bench_pair_kl.py [--reps 30] [--warmup 3] [--trials 128]
      [--host_pairs 32] [--json profiles/pair_kl_bench.json]

  device_ms      spike_metrics.pair_histograms_device (cg_pair_histogram, one
                 launch for all pairs), the copy of counts, sizes and status to
                 the host and compute_metrics.kl_from_counts per pair: what
                 pairs_kl_divergence_device does for one statistic.  Median of
                 --reps warm runs, each timed on its own with a synchronize on
                 both sides; min and max beside it
  kernel_ms      the launch alone, likewise
  host_s         compute_metrics.pairs_kl_divergence (pandas.cut per pair) on
                 the same triangles on this machine's CPU: --host_pairs pairs
                 timed, scaled to all
  transfer_ms    what the host path needs first: both (n, C, C) float64 batches
                 brought to the host

Before anything is timed the device counts, sizes, edges and status are compared
with the numpy statement (spike_metrics.pair_histograms), and the KL of the
--host_pairs pairs with pairs_kl_divergence, bit for bit.  Clocks are whatever
the machine runs at; no figure here is a pass criterion.  Prints ONE JSON line
(and writes it to --json)."""
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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--trials', type=int, default=128)
  ap.add_argument('--seq_len', type=int, default=2048)
  ap.add_argument('--neurons', type=int, default=102)
  ap.add_argument('--host_pairs', type=int, default=32,
                  help='pairs pairs_kl_divergence is timed (and the device KL '
                       'checked) on')
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  import compute_metrics as cm
  from calciumgan_amd.data import dg
  from calciumgan_amd.gan.utils import spike_metrics
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  B, T, C = args.trials, args.seq_len, args.neurons
  reps = max(args.reps, 20)
  sides = []
  for seed in (1234, 4321):
    d = dg.make_dataset(C, T, num_segments=B, seed=seed)
    x = torch.from_numpy(np.ascontiguousarray(d['spikes'], dtype=np.float32)
                         ).to(dev)
    sides.append(spike_metrics.van_rossum_distance_device(x))
  real, fake = sides
  torch.cuda.synchronize()
  full = C * (C - 1) // 2
  iu = np.triu_indices(C, k=1)

  def launch():
    return spike_metrics.pair_histograms_device(real, fake, cm.NUM_BINS,
                                                return_edges=False)

  def device_path():
    counts, valid, _, status = launch()
    counts, status = counts.cpu().numpy(), status.cpu().numpy()
    valid.cpu()
    assert not status.any()
    return np.array([cm.kl_from_counts(counts[i, 0], counts[i, 1], full, full)
                     for i in range(B)], dtype=np.float32)

  # the check: the statement's counts, sizes, edges and status ...
  got = [t.cpu().numpy() for t in
         spike_metrics.pair_histograms_device(real, fake, cm.NUM_BINS)]
  t0 = time.perf_counter()
  real_h, fake_h = real.cpu().numpy(), fake.cpu().numpy()
  transfer_ms = (time.perf_counter() - t0) * 1e3
  want = spike_metrics.pair_histograms(real_h, fake_h, cm.NUM_BINS)
  for name, g, w in zip(('counts', 'valid', 'edges', 'status'), got, want):
    same = (np.array_equal(g.view(np.int64), w.view(np.int64))
            if name == 'edges' else np.array_equal(g, w))
    if not same:
      raise SystemExit('{} differ from the statement'.format(name))
  if want[3].any() or not (want[1] == full).all():
    raise SystemExit('a degenerate pair in the benchmark data')
  # ... and the host's KL on the pairs it is timed on
  k = max(1, min(args.host_pairs, B))
  pairs = [(real_h[i][iu], fake_h[i][iu]) for i in range(k)]
  t0 = time.perf_counter()
  host_kl = cm.pairs_kl_divergence(pairs)
  host_s = (time.perf_counter() - t0) / k * B
  kl = device_path()
  if kl[:k].tobytes() != host_kl.tobytes():
    raise SystemExit('the KL differs from pairs_kl_divergence')

  for _ in range(args.warmup):
    device_path()
  path_ms = _each(device_path, reps)
  kernel_ms = _each(launch, reps)
  t0 = time.perf_counter()
  real.cpu(), fake.cpu()
  transfer_ms = min(transfer_ms, (time.perf_counter() - t0) * 1e3)
  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  device_ms = statistics.median(path_ms)
  res = {
      'metric': 'histogram KL of {} pairs of van Rossum matrices (T={}, C={}, '
                '{} bins, 2 x {} values a pair)'.format(B, T, C, cm.NUM_BINS,
                                                        full),
      'device_ms': device_ms,
      'device_ms_min': min(path_ms),
      'device_ms_max': max(path_ms),
      'kernel_ms': statistics.median(kernel_ms),
      'kernel_ms_min': min(kernel_ms),
      'kernel_ms_max': max(kernel_ms),
      'host_s': host_s,
      'host_ms_per_pair': host_s / B * 1e3,
      'host_pairs_timed': k,
      'transfer_ms': transfer_ms,
      'equal_to_statement': True,
      'kl_equal_to_host': True,
      'kl_mean': float(np.mean(kl)),
      'device_faster_than_host': bool(device_ms * 1e-3 < host_s),
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
