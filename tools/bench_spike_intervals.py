#!/usr/bin/env python
"""Time of the packing and counting kernels of compute_metrics.py
--interval_metrics on one GPU at two shapes (trials x frames x neurons): the
report's 500 x 2048 x 102 a side and 500 x 8192 x 512; beside each its bytes
floor, one yardstick and the host:

  python tools/bench_spike_intervals.py [--runs 30] [--warmup 3]
      [--shapes 500x2048x102,500x8192x512] [--max_isi 240]
      [--json profiles/spike_intervals_bench.json]

  pack_ms        cg_binary_words at bin 1 of one side, in batches of
                 --batch_trials, and the join of their words
  count_ms       cg_spike_intervals of that side: histograms, moments and the
                 counts of every train
  bytes_floor_ms the words read once (4 C trials wpt bytes) at 5.9 and at 6.6
                 TB/s, the rates of the project's streaming kernels (README)
  yardstick_ms   the same integers without a kernel of the project's:
                 torch.nonzero of the (neurons, trials, frames) spikes, the
                 difference of neighbouring rows and torch.bincount, in slices
                 of at most --yardstick_elements elements; nonzero synchronises
                 with the host, so this is wall time around a synchronise
  host_s         spike_metrics.interval_counts of the side on this machine's
                 CPUs: MEASURED, run whole, once

The device integers are first held to the statement (equality), and the
yardstick's to the device's.  Timing: --warmup calls first, then each of --runs
calls between two events on the current stream; the figure is the median, the
spread min .. max.  Outputs and workspace are allocated once, outside the timed
region.  Clocks are whatever the machine runs at; no figure here is a pass
criterion.  Prints ONE JSON line (and writes it to --json)."""
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
RATE = 13.0 / 2048        # spikes a frame: the trains of the report


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


def _wall_ms(fn, warmup, runs):
  """Milliseconds of each of `runs` calls of fn that synchronises itself."""
  for _ in range(warmup):
    fn()
  times = []
  for _ in range(runs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) * 1e3)
  return times


def _summary(times):
  return float(np.median(times)), float(min(times)), float(max(times))


def _trains(trials, T, C, seed, dev):
  """float32 device (trials, T, C): RATE a frame times a lognormal gain drawn
  per trial and shared by its neurons."""
  g = torch.Generator(device=dev)
  g.manual_seed(seed)
  rate = RATE * torch.exp(0.3 * torch.randn(trials, 1, 1, generator=g, device=dev))
  out = torch.empty(trials, T, C, dtype=torch.float32, device=dev)
  for i in range(0, trials, 50):   # (the uniform draws of 50 trials at a time)
    out[i:i + 50] = torch.rand(out[i:i + 50].shape, generator=g,
                               device=dev) < rate[i:i + 50]
  return out


def _yardstick(spikes, H):
  """(hist, moments, counts) of bool device (C, N, T) spikes from torch alone."""
  C, N, T = spikes.shape
  at = torch.nonzero(spikes)              # rows (c, n, t), sorted
  c, n, t = at[:, 0], at[:, 1], at[:, 2]
  same = (c[1:] == c[:-1]) & (n[1:] == n[:-1])
  d = t[1:] - t[:-1]
  I, owner = d[same], c[1:][same]
  hist = torch.bincount(owner * H + I.clamp(max=H) - 1,
                        minlength=C * H).view(C, H)
  both = same[1:] & same[:-1]
  pair_owner = c[2:][both]
  # (float64 weights: exact on these integers below 2^53)
  moments = torch.stack([
      torch.bincount(c, minlength=C).double(),
      torch.bincount(owner, minlength=C).double(),
      torch.bincount(owner, weights=I.double(), minlength=C),
      torch.bincount(owner, weights=(I * I).double(), minlength=C),
      torch.bincount(pair_owner, minlength=C).double(),
      torch.bincount(pair_owner, weights=(d[1:] * d[:-1])[both].double(),
                     minlength=C)], 1).long()
  return hist, moments, spikes.sum(2).t()


def bench_shape(args, sm, _lib, shape, dev):
  N, T, C = shape
  max_isi, H = args.max_isi, args.max_isi + 1
  trains = _trains(N, T, C, 1, dev)

  def pack():
    return sm.DeviceWords.cat(
        sm.binary_words_device(trains[i:i + args.batch_trials], 1)
        for i in range(0, N, args.batch_trials))

  words = pack()
  pack_ms = _summary(_event_ms(pack, args.warmup, args.runs))
  W = int(words.tensor.shape[1])
  wpt = W // N
  lib = _lib.load()
  ws_bytes = lib.cg_spike_intervals_ws_bytes(C, N, wpt, max_isi)
  ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
  hist = torch.empty(C, H, dtype=torch.int32, device=dev)
  moments = torch.empty(C, 6, dtype=torch.int64, device=dev)
  counts = torch.empty(N, C, dtype=torch.int32, device=dev)

  def count():
    _lib.call('cg_spike_intervals', words.tensor, C, N, wpt, W, max_isi, hist,
              moments, counts, ws, _lib.stream())

  count()
  torch.cuda.synchronize()
  got = [x.cpu().numpy().astype(np.int64) for x in (hist, moments, counts)]

  # the statement on the host, whole, and its time
  host_spikes = torch.cat([(trains[i:i + 50] != 0).to(torch.uint8).cpu()
                           for i in range(0, N, 50)]).numpy()
  t0 = time.perf_counter()
  want = sm.interval_counts(host_spikes, max_isi)
  host_s = time.perf_counter() - t0
  del host_spikes
  for name, g, w in zip(('hist', 'moments', 'counts'), got, want):
    if not np.array_equal(g, w):
      raise SystemExit('the device {} differ from the statement'.format(name))

  count_ms = _summary(_event_ms(count, args.warmup, args.runs))
  torch.cuda.synchronize()

  # the yardstick, in slices of neurons
  spikes = torch.empty(C, N, T, dtype=torch.bool, device=dev)
  for i in range(0, N, 50):
    spikes[:, i:i + 50] = (trains[i:i + 50] != 0).permute(2, 0, 1)
  del trains
  step = max(1, min(C, args.yardstick_elements // (N * T)))
  parts = []

  def yardstick():
    del parts[:]
    for c0 in range(0, C, step):
      parts.append(_yardstick(spikes[c0:c0 + step], H))

  yard = _summary(_wall_ms(yardstick, 1, args.yardstick_runs))
  yard_got = (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]),
              torch.cat([p[2] for p in parts], 1))
  yardstick_agrees = all(
      np.array_equal(y.cpu().numpy().astype(np.int64), g)
      for y, g in zip(yard_got, got))
  word_bytes = 4.0 * C * W
  floor_ms = [word_bytes / (r * 1e12) * 1e3 for r in STREAM_TBS]
  return {
      'shape': '{} trials x {} frames x {} neurons'.format(N, T, C),
      'max_isi': max_isi, 'words_per_trial': wpt, 'word_bytes': word_bytes,
      'spikes': int(got[1][:, 0].sum()), 'intervals': int(got[1][:, 1].sum()),
      'pack_ms': pack_ms[0], 'pack_ms_min_max': pack_ms[1:],
      'count_ms': count_ms[0], 'count_ms_min_max': count_ms[1:],
      'bytes_floor_ms': [floor_ms[1], floor_ms[0]],
      'count_ms_over_bytes_floor': count_ms[0] / floor_ms[0],
      'yardstick_ms': yard[0], 'yardstick_ms_min_max': yard[1:],
      'yardstick_runs': args.yardstick_runs,
      'yardstick_neurons_a_slice': step,
      'yardstick_agrees': bool(yardstick_agrees),
      'count_ms_over_yardstick': count_ms[0] / yard[0],
      'host_s': host_s,
      'device_equals_statement': 'hist, moments and counts, whole',
      'workspace_bytes': int(ws_bytes),
  }


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--shapes', default='500x2048x102,500x8192x512',
                  help='trials x frames x neurons')
  ap.add_argument('--max_isi', type=int, default=240)
  ap.add_argument('--batch_trials', type=int, default=128)
  ap.add_argument('--yardstick_runs', type=int, default=5)
  ap.add_argument('--yardstick_elements', type=int, default=1 << 28,
                  help='spikes of at most this many frames go through one '
                  'torch.nonzero')
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
      'metric': 'binary words and inter-spike-interval counts of one side',
      'shapes': results,
      'stream_tb_per_s': list(STREAM_TBS),
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
