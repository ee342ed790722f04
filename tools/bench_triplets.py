#!/usr/bin/env python
"""Time of the packing and counting kernels of compute_metrics.py
--triplet_metrics on one GPU at three shapes (trials x frames x neurons, bin):
the report's 500 x 2048 x 102 at bin 12, the same trials at bin 1, and 500 x
8192 x 512 at bin 12; beside each its operations floor, one yardstick and the
host:

  python tools/bench_triplets.py [--runs 30] [--warmup 3]
      [--shapes 500x2048x102x12,500x2048x102x1,500x8192x512x12]
      [--json profiles/triplet_bench.json]

  pack_ms       cg_binary_words of one side, in batches of --batch_trials, and
                the join of their words
  count_ms      cg_triplet_counts of that side: singles, pairs and all C(C,3)
                triplets
  ops_floor_ms  2 Tr W lane operations (one AND and one popcount-accumulate per
                triplet and word; Tr = C(C,3), W words a neuron) at the vector
                rate of `valu_rate_source`: 256 CUs x 4 SIMDs x 32 lanes a
                cycle at 2.4 GHz = 78.6 T lane operations a second (not
                measured by this tool)
  yardstick_ms  the vendor-GEMM statement: for a neuron i one float32
                torch.matmul (x o x_i)^T x of the (S, C) states, exact below
                2^24; timed on --yardstick_neurons values of i spread over the
                neurons and SCALED to all C (`yardstick_scaled_from`)
  host_s_extrapolated   spike_metrics.triplet_counts' product for --host_neurons
                values of i on this machine's CPUs, scaled to C - 2:
                EXTRAPOLATED, not run whole

The device counts are first held to the statement: singles and pairs whole,
the triplets of the --host_neurons values of i (equality of integers), and the
yardstick's products to the device's.  Timing: --warmup calls first, then each
of --runs calls between two events on the current stream; the figure is the
median, the spread min .. max.  Outputs and workspace are allocated once,
outside the timed region.  Clocks are whatever the machine runs at; no figure
here is a pass criterion.  Prints ONE JSON line (and writes it to --json)."""
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

VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
VALU_RATE_SOURCE = (
    "MI355X_MICROARCH.md, Compute: 'A wave (64 lanes) is assigned to one SIMD "
    "and issues each VALU instruction over 2 cycles (32 lanes/cycle x 2)'; 256 "
    "CUs of 4 SIMDs at ~2.4 GHz (half its F32 vector peak of 157.3 TF, an FMA "
    "being two operations)")


def _event_ms(fn, warmup, runs):
  """Milliseconds of each of `runs` calls of fn, between two stream events."""
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(runs):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    times.append(start.elapsed_time(stop))
  return times


def _summary(times):
  return float(np.median(times)), float(min(times)), float(max(times))


def _trains(trials, T, C, seed, dev):
  """float32 device (trials, T, C): rate 0.04 a frame times a lognormal gain
  shared by the neurons and drawn per 12 frames."""
  g = torch.Generator(device=dev)
  g.manual_seed(seed)
  nb = -(-T // 12)
  gain = torch.exp(0.6 * torch.randn(trials, nb, 1, generator=g, device=dev))
  rate = 0.04 * gain.repeat_interleave(12, dim=1)[:, :T]
  out = torch.empty(trials, T, C, dtype=torch.float32, device=dev)
  for i in range(0, trials, 50):   # (the uniform draws of 50 trials at a time)
    out[i:i + 50] = torch.rand(out[i:i + 50].shape, generator=g,
                               device=dev) < rate[i:i + 50]
  return out


def _spread(C, n):
  """n values of i in 0 .. C - 3, spread evenly, ascending, distinct."""
  return sorted({int(round(v)) for v in np.linspace(0, C - 3, max(1, n))})


def bench_shape(args, sm, _lib, shape, dev):
  N, T, C, bin = shape
  trains = _trains(N, T, C, 1, dev)

  def pack():
    return sm.DeviceWords.cat(
        sm.binary_words_device(trains[i:i + args.batch_trials], bin)
        for i in range(0, N, args.batch_trials))

  words = pack()
  pack_ms = _summary(_event_ms(pack, args.warmup, args.runs))
  W = int(words.tensor.shape[1])
  S = len(words)
  Tr = C * (C - 1) * (C - 2) // 6
  lib = _lib.load()
  ws_bytes = lib.cg_triplet_counts_ws_bytes(C, W)
  ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
  singles = torch.empty(C, dtype=torch.int32, device=dev)
  pairs = torch.empty(C, C, dtype=torch.int32, device=dev)
  triplets = torch.empty(Tr, dtype=torch.int32, device=dev)

  def count():
    _lib.call('cg_triplet_counts', words.tensor, C, W, W, singles, pairs,
              triplets, ws, _lib.stream())

  count_ms = _summary(_event_ms(count, args.warmup, args.runs))
  torch.cuda.synchronize()

  # the states as float32 (S, C) on the device, from torch alone
  nb = T // bin
  x = torch.cat([
      (trains[i:i + 50, :nb * bin].reshape(-1, nb, bin, C) != 0).any(2).reshape(
          -1, C).float() for i in range(0, N, 50)])
  del trains
  assert tuple(x.shape) == (S, C) and S < 1 << 24
  # rank of the first triplet (i, i + 1, i + 2) and the size of i's block
  first = [C * (C - 1) * (C - 2) // 6 - (C - i) * (C - i - 1) * (C - i - 2) // 6
           for i in range(C - 1)]
  ju, ku = np.triu_indices(C, 1)
  after = np.concatenate([[0], np.cumsum(C - 1 - np.arange(C))])

  def block(m, i):   # the block of ranks of i from a (C, C) product
    sel = slice(after[i + 1], None)
    return m[ju[sel], ku[sel]]

  # the check and the host's time: the statement's products for a few i
  xh = x.cpu().numpy().astype(np.float64)
  got_t = triplets.cpu().numpy()
  hp = xh.T @ xh
  if not (np.array_equal(pairs.cpu().numpy(), hp.astype(np.int64)) and
          np.array_equal(singles.cpu().numpy(),
                         np.diagonal(hp).astype(np.int64))):
    raise SystemExit('the device pairs differ from the statement')
  host_i = _spread(C, args.host_neurons)
  t0 = time.perf_counter()
  host_m = [(xh * xh[:, i:i + 1]).T @ xh for i in host_i]
  host_s = (time.perf_counter() - t0) / len(host_i) * (C - 2)
  for i, m in zip(host_i, host_m):
    if not np.array_equal(got_t[first[i]:first[i + 1]],
                          block(m, i).astype(np.int64)):
      raise SystemExit('the device triplets differ from the statement')
  del xh, host_m

  # the yardstick: one vendor GEMM per neuron
  yard_i = _spread(C, args.yardstick_neurons)
  masked = torch.empty_like(x)
  out = torch.empty(len(yard_i), C, C, dtype=torch.float32, device=dev)

  def yardstick():
    for n, i in enumerate(yard_i):
      torch.mul(x, x[:, i:i + 1], out=masked)
      torch.matmul(masked.t(), x, out=out[n])

  yard = _summary(_event_ms(yardstick, args.warmup, args.runs))
  scale = float(C) / len(yard_i)
  yard_h = out.cpu().numpy()
  yardstick_agrees = all(
      np.array_equal(block(yard_h[n], i).astype(np.int64),
                     got_t[first[i]:first[i + 1]])
      for n, i in enumerate(yard_i))
  ops = 2.0 * Tr * W
  floor_ms = ops / VALU_LANE_OPS_PER_S * 1e3
  return {
      'shape': '{} trials x {} frames x {} neurons, bin {}'.format(N, T, C, bin),
      'states': S, 'words_per_neuron': W, 'triplets': Tr,
      'pack_ms': pack_ms[0], 'pack_ms_min_max': pack_ms[1:],
      'count_ms': count_ms[0], 'count_ms_min_max': count_ms[1:],
      'lane_ops': ops,
      'ops_floor_ms': floor_ms,
      'count_ms_over_ops_floor': count_ms[0] / floor_ms,
      'yardstick_ms': yard[0] * scale,
      'yardstick_ms_min_max': [yard[1] * scale, yard[2] * scale],
      'yardstick_scaled_from': '{} of {} neurons timed, times {:.3f}'.format(
          len(yard_i), C, scale),
      'yardstick_agrees': bool(yardstick_agrees),
      'count_ms_over_yardstick': count_ms[0] / (yard[0] * scale),
      'host_s_extrapolated': host_s,
      'host_neurons_timed': len(host_i),
      'device_equals_statement': 'singles, pairs, the triplets of {} neurons i'
                                 .format(len(host_i)),
      'workspace_bytes': int(ws_bytes),
  }


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--shapes', default='500x2048x102x12,500x2048x102x1,'
                  '500x8192x512x12', help='trials x frames x neurons x bin')
  ap.add_argument('--batch_trials', type=int, default=128)
  ap.add_argument('--host_neurons', type=int, default=2,
                  help='values of i checked against the statement and timed on '
                  'the host')
  ap.add_argument('--yardstick_neurons', type=int, default=8)
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  from calciumgan_amd import _lib
  from calciumgan_amd.gan.utils import spike_metrics as sm
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  shapes = [tuple(int(v) for v in s.split('x')) for s in args.shapes.split(',')]
  results = []
  for shape in shapes:
    results.append(bench_shape(args, sm, _lib, shape, dev))
    torch.cuda.empty_cache()
  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  res = {
      'metric': 'binary words and third-order counts of one side',
      'shapes': results,
      'valu_lane_ops_per_s': VALU_LANE_OPS_PER_S,
      'valu_rate_source': VALU_RATE_SOURCE,
      'host_cpus': os.cpu_count(),
      'runs': args.runs,
      'warmup': args.warmup,
      'clocks_pinned': False,
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
