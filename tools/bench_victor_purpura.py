#!/usr/bin/env python
"""Time of the per-trial Victor-Purpura distance matrices of compute_metrics.py
--victor_purpura at BASELINE configs[1]'s shapes (128 trials, T = 2048, C = 102,
DG spike trains from data/dg.py) on one GPU, beside the numpy statement and the
old pair loop on the same trials, and on a second batch of dense random trains:

  python tools/bench_victor_purpura.py [--reps 10] [--warmup 2] [--trials 128]
      [--dense_trials 4] [--host_trials 2] [--json profiles/victor_purpura_bench.json]

  device_ms            cg_victor_purpura (both launches) on the (B, T, C) DG batch
  device_dense_ms      the same on --dense_trials trials of density 0.5 (about
                       T / 2 spikes a train: a pair is about T^2 / 4 cells)
  statement_s          spike_metrics.victor_purpura_distance_frames on
                       --host_trials of the DG trials, scaled to the batch
  pair_loop_s          spike_metrics.victor_purpura_distance (the triple Python
                       loop) on the first --loop_trains trains of those trials,
                       scaled to all pairs of the batch
  dense_statement_s    the statement on the first --dense_check_trains trains
                       of ONE dense trial, scaled to all pairs of the dense batch

The device results are compared bit for bit with the statement (on the
--host_trials DG trials and those trains of one dense trial: a pair's distance
does not depend on the other trains) before anything is timed.  Timing
rules as tools/bench_van_rossum.py: warm-up calls first, synchronize on both
sides of the timed launches; the workspace is allocated once, outside the timed
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


def _timed(fn, reps):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(reps):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / reps * 1e3


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--trials', type=int, default=128)
  ap.add_argument('--dense_trials', type=int, default=4)
  ap.add_argument('--seq_len', type=int, default=2048)
  ap.add_argument('--neurons', type=int, default=102)
  ap.add_argument('--host_trials', type=int, default=2,
                  help='DG trials the host functions are timed (and the device '
                       'result checked) on')
  ap.add_argument('--loop_trains', type=int, default=24,
                  help='trains of a trial the old pair loop is timed on')
  ap.add_argument('--dense_check_trains', type=int, default=12)
  ap.add_argument('--q', type=float, default=1.0)
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  from calciumgan_amd import _lib, nets
  from calciumgan_amd.data import dg
  from calciumgan_amd.gan.utils import spike_metrics
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  B, T, C = args.trials, args.seq_len, args.neurons
  qf = spike_metrics.victor_purpura_cost(args.q)
  d = dg.make_dataset(C, T, num_segments=B, seed=1234)
  host = np.ascontiguousarray(d['spikes'], dtype=np.float32)  # (B, T, C)
  dense = (np.random.RandomState(7).uniform(size=(args.dense_trials, T, C)) < 0.5
           ).astype(np.float32)

  def prepare(array):
    x = torch.from_numpy(array).to(dev)
    n = x.shape[0]
    nbytes = _lib.load().cg_victor_purpura_ws_bytes(n, T, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dist = torch.empty(n, C, C, dtype=torch.float64, device=dev)

    def launch():
      _lib.call('cg_victor_purpura', nets._p(x), n, T, C, x.stride(0),
                x.stride(1), x.stride(2), qf, nets._p(dist), nets._p(ws), nbytes,
                nets._stream())
    return launch, dist, nbytes

  run_dg, dist_dg, ws_dg = prepare(host)
  run_dense, dist_dense, ws_dense = prepare(dense)
  for _ in range(args.warmup):
    run_dg()
  run_dense()
  torch.cuda.synchronize()

  # the check: the statement's bits, on the trials the host also runs
  k = max(1, min(args.host_trials, B))
  got = dist_dg.cpu().numpy()
  t0 = time.perf_counter()
  want = [spike_metrics.victor_purpura_distance_frames(host[b].T, q=args.q)
          for b in range(k)]
  statement_s = (time.perf_counter() - t0) / k * B
  for b in range(k):
    if not np.array_equal(got[b].view(np.int64), want[b].view(np.int64)):
      raise SystemExit('DG trial {} differs from the statement'.format(b))
  dm = max(2, min(args.dense_check_trains, C))
  t0 = time.perf_counter()
  want_dense = spike_metrics.victor_purpura_distance_frames(dense[0, :, :dm].T,
                                                            q=args.q)
  dense_statement_s = ((time.perf_counter() - t0) / (dm * (dm - 1) / 2) *
                       (C * (C - 1) / 2) * args.dense_trials)
  got_dense = np.ascontiguousarray(dist_dense.cpu().numpy()[0, :dm, :dm])
  if not np.array_equal(got_dense.view(np.int64), want_dense.view(np.int64)):
    raise SystemExit('the dense trial differs from the statement')
  m = min(args.loop_trains, C)
  t0 = time.perf_counter()
  for b in range(k):
    spike_metrics.victor_purpura_distance(host[b, :, :m].T, q=args.q)
  pair_loop_s = ((time.perf_counter() - t0) / k / (m * (m - 1) / 2) *
                 (C * (C - 1) / 2) * B)

  ms_dg = _timed(run_dg, args.reps)
  ms_dense = _timed(run_dense, max(1, min(args.reps, 3)))
  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  counts = host.sum(1)                                   # (B, C)
  iu = np.triu_indices(C, k=1)
  cells = float(sum((n[iu[0]] * n[iu[1]]).sum() for n in counts))
  dcounts = dense.sum(1)
  dense_cells = float(sum((n[iu[0]] * n[iu[1]]).sum() for n in dcounts))
  res = {
      'metric': 'Victor-Purpura matrices of {} trials (T={}, C={}, q={})'
                .format(B, T, C, args.q),
      'device_ms': ms_dg,
      'device_dense_ms': ms_dense,
      'dense_trials': args.dense_trials,
      'statement_s': statement_s,
      'pair_loop_s': pair_loop_s,
      'dense_statement_s': dense_statement_s,
      'host_trials_timed': k,
      'pair_loop_trains_timed': m,
      'dense_statement_trains_timed': dm,
      'bit_equal_to_statement': True,
      'device_faster_than_statement': bool(ms_dg * 1e-3 < statement_s),
      'spikes_per_train': float(counts.mean()),
      'spikes_per_train_max': float(counts.max()),
      'dense_spikes_per_train': float(dcounts.mean()),
      'cells': cells,
      'gcells_per_s': cells / (ms_dg * 1e-3) * 1e-9,
      'dense_cells': dense_cells,
      'dense_gcells_per_s': dense_cells / (ms_dense * 1e-3) * 1e-9,
      'workspace_bytes': int(ws_dg),
      'dense_workspace_bytes': int(ws_dense),
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
