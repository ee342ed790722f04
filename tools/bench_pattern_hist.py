#!/usr/bin/env python
"""Time of the pattern counts of the surrogate experiment at its own shape:
2 * 10^6 samples of 6 time steps x 2 neurons (compute_surrogate_metrics.py).

  python tools/bench_pattern_hist.py [--reps 30] [--warmup 3] [--inner 10]
      [--samples 2000000] [--json profiles/pattern_hist_bench.json]

  hist_ms          spike_metrics.pattern_histogram_device (cg_pattern_histogram:
                   the zeroing launch and the counting launch) on a draw of the
                   dichotomised-Gaussian model, stored (n, neurons, L) and read
                   in place as its (n, L, neurons) view, as the tool reads
                   ground_truth.pkl
  hist_equal_ms    the same on an input whose samples all carry one pattern: the
                   worst contention
  *_gather_ms      both on a copy of the input that starts one element into its
                   buffer: no 16-byte alignment, so every frame is loaded on its
                   own (the form any other strides take) instead of a sample in
                   16-byte pieces
  deconv_ms        spike_helper.deconvolve_signals_device of the calcium traces
                   of the same batch, (n, L, C)
  statement_s      spike_metrics.pattern_histogram (numpy) on the same draw
  host_deconv_s    spike_helper.deconvolve_signals of the same traces

ms between two stream events around --inner (10) calls in a row, divided by
--inner, after --warmup calls; the median of --reps (at least 30) such runs, min
and max beside it; the variants take turns within a repetition.  Before
anything is timed the device counts of both inputs in both forms are
compared with the numpy statement, and the device trains with the host's, for
equality.  floor_us is the input's bytes at 6 TB/s (the streaming kernels reach
5.9 - 6.6).  Clocks are whatever the machine runs at; no figure here is a pass
criterion.  Prints ONE JSON line (and writes it to --json)."""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, 'dataset')):
  if path not in sys.path:
    sys.path.insert(0, path)

import numpy as np
import torch

def _once(fn, inner):
  """ms per call of `inner` calls between two stream events."""
  start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
  start.record()
  for _ in range(inner):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) / inner


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--inner', type=int, default=10)
  ap.add_argument('--samples', type=int, default=2 * 10**6)
  ap.add_argument('--sequence_length', type=int, default=6)
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  import generate_surrogate_dataset as gsd
  from calciumgan_amd.gan.utils import spike_helper, spike_metrics
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  n, L, C = args.samples, args.sequence_length, gsd.NUM_NEURONS
  reps = max(args.reps, 30)
  rng = np.random.RandomState(1234)
  spikes = gsd.generate_dg_spikes(n, L, rng)               # (n, C, L)
  signals = np.ascontiguousarray(
      gsd.spikes_to_signals(spikes, rng).transpose(0, 2, 1))  # (n, L, C)
  equal = np.ascontiguousarray(np.broadcast_to(spikes[:1], spikes.shape))

  def views(array):
    """The (n, L, C) view of the array on the device, and the same from a copy
    one element into its buffer."""
    flat = torch.empty(array.size + 1, dtype=torch.float32, device=dev)
    flat[1:] = torch.from_numpy(array).to(dev).reshape(-1)
    return (torch.from_numpy(array).to(dev).permute(0, 2, 1),
            flat[1:].view(array.shape).permute(0, 2, 1))

  d_spikes, d_spikes_odd = views(spikes)
  d_equal, d_equal_odd = views(equal)
  d_signals = torch.from_numpy(signals).to(dev)

  # the check, and the host's times
  t0 = time.perf_counter()
  want = spike_metrics.pattern_histogram(spikes.transpose(0, 2, 1))
  statement_s = time.perf_counter() - t0
  want_equal = spike_metrics.pattern_histogram(equal.transpose(0, 2, 1))
  for x, w in ((d_spikes, want), (d_equal, want_equal), (d_spikes_odd, want),
               (d_equal_odd, want_equal)):
    got = spike_metrics.pattern_histogram_device(x).cpu().numpy()
    if not np.array_equal(got, w):
      raise SystemExit('the counts differ from the statement')
  t0 = time.perf_counter()
  trains = spike_helper.deconvolve_signals(
      np.ascontiguousarray(signals.transpose(0, 2, 1)).reshape(n * C, L))
  host_deconv_s = time.perf_counter() - t0
  got = spike_helper.deconvolve_signals_device(d_signals).cpu().numpy()
  if not np.array_equal(got, trains.reshape(n, C, L).transpose(0, 2, 1)):
    raise SystemExit('the device trains differ from the host trains')

  def hist(x):
    return lambda: spike_metrics.pattern_histogram_device(x)

  runs = {
      'hist_ms': hist(d_spikes),
      'hist_gather_ms': hist(d_spikes_odd),
      'hist_equal_ms': hist(d_equal),
      'hist_equal_gather_ms': hist(d_equal_odd),
      'deconv_ms': lambda: spike_helper.deconvolve_signals_device(d_signals),
  }
  for _ in range(args.warmup):
    for fn in runs.values():
      fn()
  torch.cuda.synchronize()
  times = {name: [] for name in runs}
  for _ in range(reps):
    for name, fn in runs.items():
      times[name].append(_once(fn, max(args.inner, 1)))
  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  nbytes = n * L * C * 4
  floor_us = nbytes / 6e12 * 1e6
  res = {'metric': 'pattern counts of {} samples of {} x {} ({} codes, {} MB '
                   'read)'.format(n, L, C, 1 << (L * C), nbytes // 10**6)}
  for name, ms in times.items():
    res[name] = statistics.median(ms)
    res[name + '_min'] = min(ms)
    res[name + '_max'] = max(ms)
  res.update({
      'floor_us': floor_us,
      'hist_times_floor': res['hist_ms'] * 1e3 / floor_us,
      'hist_tb_per_s': nbytes / (res['hist_ms'] * 1e-3) / 1e12,
      'equal_over_dg': res['hist_equal_ms'] / res['hist_ms'],
      'gather_over_packed': res['hist_gather_ms'] / res['hist_ms'],
      'statement_s': statement_s,
      'host_deconv_s': host_deconv_s,
      'patterns_seen': int((want > 0).sum()),
      'top_pattern_fraction': float(want.max()) / n,
      'equal_to_statement': True,
      'trains_equal_to_host': True,
      'reps': reps,
      'warmup': args.warmup,
      'inner': max(args.inner, 1),
      'n_gpus': 1,
      'gpu': torch.cuda.get_device_name(0),
      'box': socket.gethostname(),
      'commit': commit,
      'conditions': 'one MI355X, one run, clocks not pinned',
  })
  line = json.dumps(res)
  if args.json:
    with open(args.json, 'w') as f:
      f.write(line + '\n')
  print(line)


if __name__ == '__main__':
  main()
