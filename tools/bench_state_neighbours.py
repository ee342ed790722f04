#!/usr/bin/env python
"""Time of the neighbour queries of compute_metrics.py --state_metrics at the
report's shape (500 trials of 2048 frames of 102 neurons a side, bin 12, k 5:
85 000 states a side) on one GPU, beside its operations floor, one yardstick
and the host:

  python tools/bench_state_neighbours.py [--runs 30] [--warmup 3] [--trials 500]
      [--host_rows 1024] [--json profiles/state_neighbours_bench.json]

  states_ms     cg_population_states of one side, in batches of --batch_trials
  self_ms       cg_state_neighbours of a set against itself, self excluded, knn
                only (the radii of a set)
  cross_ms      cg_state_neighbours of one set against the other with radius_b:
                knn and within
  flop_floor_ms 2 Sa Sb Cp (Cp = C rounded up to the K step of 32) at the card's
                dense BF16 matrix rate, the datasheet's 2.5 PFLOP/s
                (`matrix_tflops_source`; not measured by this tool)
  yardstick_ms  the cross query's knn by torch.matmul in float32 over chunks of
                --yardstick_rows rows of A (the vendor GEMM; exact on these
                integers) with |b|^2 added, then torch.topk on the materialised
                chunk: it writes and reads the Sa Sb distances
                (`yardstick_matrix_bytes` in all) that the kernel never stores
  host_s_extrapolated   spike_metrics.state_neighbours (the numpy statement) of
                --host_rows rows of A against all of B on this machine's CPUs,
                scaled to Sa: EXTRAPOLATED from that slice, not run whole

The device result is first held to the statement on those --host_rows rows
(equality of integers), and the yardstick's knn to the device's.  Timing:
--warmup calls first, then each of --runs calls between two events on the
current stream; the figure is the median, the spread min .. max.  Outputs and
workspace are allocated once, outside the timed region.  Clocks are whatever
the machine runs at; no figure here is a pass criterion.  Prints ONE JSON line
(and writes it to --json)."""
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

BF16_MATRIX_TFLOPS = 2500.0    # datasheet, dense; not measured by this tool


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


def _trains(trials, T, C, bin, seed, dev):
  """float32 device (trials, T, C): rate 0.08 a frame times a lognormal gain
  shared by the neurons and drawn per bin."""
  g = torch.Generator(device=dev)
  g.manual_seed(seed)
  nb = -(-T // bin)
  gain = torch.exp(0.6 * torch.randn(trials, nb, 1, generator=g, device=dev))
  rate = 0.08 * gain.repeat_interleave(bin, dim=1)[:, :T]
  return (torch.rand(trials, T, C, generator=g, device=dev) < rate).float()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--trials', type=int, default=500)
  ap.add_argument('--seq_len', type=int, default=2048)
  ap.add_argument('--neurons', type=int, default=102)
  ap.add_argument('--bin', type=int, default=12)
  ap.add_argument('--k', type=int, default=5)
  ap.add_argument('--batch_trials', type=int, default=128)
  ap.add_argument('--host_rows', type=int, default=1024,
                  help='rows of A checked against the statement and timed on '
                  'the host')
  ap.add_argument('--yardstick_rows', type=int, default=4096)
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  from calciumgan_amd import _lib
  from calciumgan_amd.gan.utils import spike_metrics as sm
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  N, T, C, bin, k = args.trials, args.seq_len, args.neurons, args.bin, args.k
  tr_a, tr_b = _trains(N, T, C, bin, 1, dev), _trains(N, T, C, bin, 2, dev)

  def states(trains):
    return sm.DeviceStates.cat(
        sm.population_states_device(trains[i:i + args.batch_trials], bin)
        for i in range(0, N, args.batch_trials))

  a, b = states(tr_a), states(tr_b)
  S, Cp = len(a), a.tensor.shape[1]
  states_ms = _summary(_event_ms(lambda: states(tr_a), args.warmup, args.runs))
  del tr_a, tr_b
  lib = _lib.load()
  ws = torch.empty(lib.cg_state_neighbours_ws_bytes(S, S, C, bin, k),
                   dtype=torch.uint8, device=dev)
  knn = torch.empty(S, k, dtype=torch.int32, device=dev)
  within = torch.empty(S, dtype=torch.int32, device=dev)

  def query(x, y, exclude_self, radius):
    _lib.call('cg_state_neighbours', x.tensor, S, y.tensor, S, C, bin, k,
              1 if exclude_self else 0, radius,
              knn, None if radius is None else within, ws, _lib.stream())

  query(b, b, True, None)
  rad_b = knn[:, k - 1].contiguous()
  self_ms = _summary(_event_ms(lambda: query(b, b, True, None), args.warmup,
                               args.runs))
  cross_ms = _summary(_event_ms(lambda: query(a, b, False, rad_b), args.warmup,
                                args.runs))
  torch.cuda.synchronize()
  got_knn, got_within = knn.cpu().numpy(), within.cpu().numpy()

  # the check and the host's time: the statement on a slice of A
  n = max(1, min(args.host_rows, S))
  a_host, b_host = a.counts()[:n].cpu().numpy(), b.counts().cpu().numpy()
  t0 = time.perf_counter()
  want_knn, want_within = sm.state_neighbours(a_host, b_host, k,
                                              radius_b=rad_b.cpu().numpy())
  host_s = (time.perf_counter() - t0) / n * S
  if not (np.array_equal(got_knn[:n], want_knn) and
          np.array_equal(got_within[:n], want_within)):
    raise SystemExit('the device integers differ from the statement')

  # the yardstick: the vendor GEMM, the chunk materialised, torch.topk
  fa, fb = a.tensor.float(), b.tensor.float()
  nb2 = (fb * fb).sum(1)
  R = max(1, min(args.yardstick_rows, S))
  chunk = torch.empty(R, S, dtype=torch.float32, device=dev)
  yard = torch.empty(S, k, dtype=torch.float32, device=dev)

  def yardstick():
    for i in range(0, S, R):
      rows = fa[i:i + R]
      d = chunk[:len(rows)]
      torch.matmul(rows, fb.t(), out=d)
      d.mul_(-2.0).add_(nb2)
      yard[i:i + R] = torch.topk(d, k, dim=1, largest=False, sorted=True)[0]

  yard_ms = _summary(_event_ms(yardstick, args.warmup, args.runs))
  yard_d2 = (yard + (fa * fa).sum(1)[:, None]).cpu().numpy()
  yardstick_agrees = bool(np.array_equal(yard_d2.astype(np.int64),
                                         got_knn.astype(np.int64)))

  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  flop = 2.0 * S * S * Cp
  flop_floor_ms = flop / (BF16_MATRIX_TFLOPS * 1e12) * 1e3
  res = {
      'metric': 'state neighbours of {} trials x {} frames x {} neurons a side, '
                'bin {}, k {}: {} states, K padded to {}'.format(N, T, C, bin, k,
                                                                 S, Cp),
      'states': S,
      'states_ms': states_ms[0], 'states_ms_min_max': states_ms[1:],
      'self_ms': self_ms[0], 'self_ms_min_max': self_ms[1:],
      'cross_ms': cross_ms[0], 'cross_ms_min_max': cross_ms[1:],
      'tflop': flop * 1e-12,
      'cross_tflops': flop / (cross_ms[0] * 1e-3) * 1e-12,
      'flop_floor_ms': flop_floor_ms,
      'matrix_tflops': BF16_MATRIX_TFLOPS,
      'matrix_tflops_source': 'datasheet BF16 dense; not measured by this tool',
      'cross_ms_over_flop_floor': cross_ms[0] / flop_floor_ms,
      'yardstick_ms': yard_ms[0], 'yardstick_ms_min_max': yard_ms[1:],
      'yardstick_rows': R,
      'yardstick_matrix_bytes': S * S * 4,
      'yardstick_agrees': yardstick_agrees,
      'cross_ms_over_yardstick': cross_ms[0] / yard_ms[0],
      'host_s_extrapolated': host_s,
      'host_rows': n,
      'host_cpus': os.cpu_count(),
      'device_equals_statement_rows': n,
      'workspace_bytes': int(ws.numel()),
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
