#!/usr/bin/env python
"""Time of the per-trial van Rossum matrices and correlation coefficients of
compute_metrics.py at BASELINE configs[1]'s shapes (128 trials, T = 2048, C =
102, DG spike trains from data/dg.py) on one GPU, beside the host functions on
the same trials:

  python tools/bench_van_rossum.py [--reps 20] [--warmup 3] [--trials 128]
      [--host_trials 0] [--json profiles/van_rossum_bench.json]

  device_van_rossum_ms    cg_van_rossum (gram and dist) on the (B, T, C) batch
  device_distance_only_ms the same with gram = NULL (what compute_metrics asks)
  device_corrcoef_ms      cg_spike_corrcoef on the same batch
  host_van_rossum_s       spike_metrics.van_rossum_distance, one trial after the
                          other (scaled to the batch when --host_trials < trials)
  host_corrcoef_s         spike_metrics.correlation_coefficients likewise

The device results are checked against the numpy statements before anything is
timed (gram within (2 T + 2) 2^-53 S of van_rossum_gram_frames on the trials the
host also runs; correlations within 2 ulp of correlation_coefficients_exact).
Timing rules as tools/bench_spike_stats.py: warm-up calls first, synchronize on
both sides of the timed launches.  Clocks are whatever the machine runs at; no
figure here is a pass criterion.  Prints ONE JSON line (and writes it to
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


def _timed(fn, reps):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(reps):
    out = fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / reps * 1e3, out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--trials', type=int, default=128)
  ap.add_argument('--seq_len', type=int, default=2048)
  ap.add_argument('--neurons', type=int, default=102)
  ap.add_argument('--host_trials', type=int, default=0,
                  help='trials the host functions are timed (and the device '
                       'results checked) on; 0: all of them')
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
  d = dg.make_dataset(C, T, num_segments=B, seed=1234)
  host = np.ascontiguousarray(d['spikes'], dtype=np.float32)  # (B, T, C)
  x = torch.from_numpy(host).to(dev)
  decay = spike_metrics.van_rossum_decay(1.0)
  gram = torch.empty(B, C, C, dtype=torch.float64, device=dev)
  dist = torch.empty_like(gram)

  def van_rossum(with_gram=True):
    _lib.call('cg_van_rossum', nets._p(x), B, T, C, x.stride(0), x.stride(1),
              x.stride(2), decay, nets._p(gram) if with_gram else None,
              nets._p(dist), nets._stream())

  corrcoef = lambda: spike_metrics.correlation_coefficients_device(x)
  for _ in range(args.warmup):
    van_rossum()
    van_rossum(False)
    corr = corrcoef()
  torch.cuda.synchronize()
  # the check, on the trials the host functions run on
  k = min(args.host_trials, B) if args.host_trials > 0 else B
  S, r = gram.cpu().numpy(), corr.cpu().numpy()
  worst_gram, corr_ulps = 0.0, 0
  for b in range(k):
    rec = spike_metrics.van_rossum_gram_frames(host[b].T, decay)
    bound = (2 * T + 2) * 2.0**-53 * rec
    err = np.abs(S[b] - rec)
    ok = bound > 0
    worst_gram = max(worst_gram, float((err[ok] / bound[ok]).max()))
    if not np.all(err <= bound):
      raise SystemExit('gram of trial {} misses its bound'.format(b))
    want = spike_metrics.correlation_coefficients_exact(host[b].T)
    if not np.array_equal(np.isnan(want), np.isnan(r[b])):
      raise SystemExit('correlation NaNs of trial {} differ'.format(b))
    fin = np.isfinite(want)
    corr_ulps = max(corr_ulps, int(np.abs(
        r[b][fin].view(np.int64) - want[fin].view(np.int64)).max()))
  if corr_ulps > 2:
    raise SystemExit('correlations {} ulp from the statement'.format(corr_ulps))
  t0 = time.perf_counter()
  for b in range(k):
    spike_metrics.van_rossum_distance(host[b].T)
  host_vr = (time.perf_counter() - t0) / k * B
  t0 = time.perf_counter()
  for b in range(k):
    spike_metrics.correlation_coefficients(host[b].T)
  host_cc = (time.perf_counter() - t0) / k * B
  ms_vr, _ = _timed(van_rossum, args.reps)
  ms_d, _ = _timed(lambda: van_rossum(False), args.reps)
  ms_cc, _ = _timed(corrcoef, args.reps)
  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  # two products (G and G^T) per pair of 16-train tiles, upper triangle of tiles
  tiles = (C + 15) // 16
  flop = 2.0 * 16 * 16 * T * 2 * (tiles * (tiles + 1) // 2) * B
  res = {
      'metric': 'van Rossum matrices and correlations of {} trials (T={}, C={})'
                .format(B, T, C),
      'device_van_rossum_ms': ms_vr,
      'device_distance_only_ms': ms_d,
      'device_corrcoef_ms': ms_cc,
      'host_van_rossum_s': host_vr,
      'host_corrcoef_s': host_cc,
      'host_trials_timed': k,
      'mfma_f64_gflops': flop / (ms_vr * 1e-3) * 1e-9,
      'gram_worst_fraction_of_bound': worst_gram,
      'corrcoef_worst_ulps': corr_ulps,
      'spikes_per_train': float(host.sum() / (B * C)),
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
