#!/usr/bin/env python
"""Time of the cross-correlograms and population counts of compute_metrics.py
--temporal_metrics at BASELINE configs[1]'s report shape (128 trials, T = 2048,
C = 102, max_lag = 24; DG spike trains from data/dg.py) on one GPU, beside the
numpy statement on a few of the same trials, and on a batch of dense random
trains (the kernel's work does not depend on the spike density: the two times
say so):

  python tools/bench_spike_ccg.py [--runs 30] [--warmup 3] [--trials 128]
      [--host_trials 2] [--json profiles/spike_ccg_bench.json]

  ccg_ms               cg_spike_ccg on the (B, T, C) DG batch
  ccg_dense_ms         the same on B trials of density 0.5
  population_hist_ms   cg_spike_population_hist on the DG batch
  statement_s          spike_metrics.cross_correlogram on --host_trials of the
                       DG trials, scaled to the batch

Both device results are compared with the statements for equality (on the
--host_trials DG trials and as many dense ones) before anything is timed.
Timing: --warmup calls first, then each of --runs calls between two events on
the current stream; the figure is the median, the spread min .. max.  The
outputs are allocated once, outside the timed region.  Beside the time stand the
two floors of the batch, computed from the shapes: the bytes it has to move (the
spikes read once, the correlograms written once) at the 5.9 - 6.6 TB/s the
project's streaming kernels reach, and its 2 B (max_lag + 1) T C^2 operations at
the 2.5 PFLOP/s of the bf16 matrix pipe.  Clocks are whatever the machine runs
at; no figure here is a pass criterion.  Prints ONE JSON line (and writes it to
--json)."""
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

STREAM_TBS = (5.9, 6.6)   # the project's streaming kernels (README)
MFMA_BF16_PFLOPS = 2.5    # dense bf16 MFMA peak of the MI355X


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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--trials', type=int, default=128)
  ap.add_argument('--seq_len', type=int, default=2048)
  ap.add_argument('--neurons', type=int, default=102)
  ap.add_argument('--max_lag', type=int, default=24)
  ap.add_argument('--host_trials', type=int, default=2,
                  help='trials the statement is timed (and the device results '
                       'checked) on')
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  from calciumgan_amd import _lib
  from calciumgan_amd.data import dg
  from calciumgan_amd.gan.utils import spike_metrics
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  B, T, C, L = args.trials, args.seq_len, args.neurons, args.max_lag
  d = dg.make_dataset(C, T, num_segments=B, seed=1234)
  host = np.ascontiguousarray(d['spikes'], dtype=np.float32)  # (B, T, C)
  dense = (np.random.RandomState(7).uniform(size=(B, T, C)) < 0.5
           ).astype(np.float32)
  x, xd = (torch.from_numpy(a).to(dev) for a in (host, dense))
  ccg = torch.empty(B, L + 1, C, C, dtype=torch.int32, device=dev)
  hist = torch.empty(B, C + 1, dtype=torch.int32, device=dev)

  def run_ccg(t):
    _lib.call('cg_spike_ccg', t, B, T, C, t.stride(0), t.stride(1), t.stride(2),
              L, ccg, _lib.stream())

  def run_hist(t):
    _lib.call('cg_spike_population_hist', t, B, T, C, t.stride(0), t.stride(1),
              t.stride(2), hist, _lib.stream())

  # the check: the statements' integers, on the trials the host also runs
  k = max(1, min(args.host_trials, B))
  t0 = time.perf_counter()
  want = spike_metrics.cross_correlogram(host[:k], L)
  statement_s = (time.perf_counter() - t0) / k * B
  for name, t, array, expect in (
      ('DG', x, host, want),
      ('dense', xd, dense, spike_metrics.cross_correlogram(dense[:k], L))):
    run_ccg(t)
    run_hist(t)
    torch.cuda.synchronize()
    if not np.array_equal(ccg[:k].cpu().numpy(), expect):
      raise SystemExit('the {} correlograms differ from the statement'
                       .format(name))
    if not np.array_equal(hist[:k].cpu().numpy(),
                          spike_metrics.population_count_histogram(array[:k])):
      raise SystemExit('the {} population counts differ from the statement'
                       .format(name))

  ccg_ms = _summary(_event_ms(lambda: run_ccg(x), args.warmup, args.runs))
  dense_ms = _summary(_event_ms(lambda: run_ccg(xd), args.warmup, args.runs))
  hist_ms = _summary(_event_ms(lambda: run_hist(x), args.warmup, args.runs))
  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  read_bytes = B * T * C * 4
  write_bytes = B * (L + 1) * C * C * 4
  flop = 2.0 * B * (L + 1) * T * C * C
  bytes_floor_ms = [(read_bytes + write_bytes) / (r * 1e12) * 1e3
                    for r in reversed(STREAM_TBS)]
  mfma_floor_ms = flop / (MFMA_BF16_PFLOPS * 1e15) * 1e3
  res = {
      'metric': 'cross-correlograms of {} trials (T={}, C={}, max_lag={})'
                .format(B, T, C, L),
      'ccg_ms': ccg_ms[0], 'ccg_ms_min_max': ccg_ms[1:],
      'ccg_dense_ms': dense_ms[0], 'ccg_dense_ms_min_max': dense_ms[1:],
      'population_hist_ms': hist_ms[0], 'population_hist_ms_min_max': hist_ms[1:],
      'statement_s': statement_s,
      'host_trials_timed': k,
      'equal_to_statement': True,
      'spikes_per_train': float(host.sum(1).mean()),
      'read_bytes': read_bytes,
      'write_bytes': write_bytes,
      'flop': flop,
      'bytes_floor_ms': bytes_floor_ms,
      'mfma_floor_ms': mfma_floor_ms,
      'ccg_over_bytes_floor': ccg_ms[0] / bytes_floor_ms[1],
      'ccg_over_mfma_floor': ccg_ms[0] / mfma_floor_ms,
      'ccg_tflops': flop / (ccg_ms[0] * 1e-3) * 1e-12,
      'population_hist_read_tbs': read_bytes / (hist_ms[0] * 1e-3) * 1e-12,
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
