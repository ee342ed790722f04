#!/usr/bin/env python
"""Time of the trace power spectra of compute_metrics.py --spectral_metrics at
BASELINE configs[1]'s report shape (128 trials, T = 2048, C = 102; DG calcium
traces from data/dg.py) on one GPU, beside the yardstick -- cg_ifft_channels on
as many traces of the same length in the same run: the same stages, one neuron
per complex trace -- and the numpy statement on a few of the same trials:

  python tools/bench_trace_psd.py [--runs 30] [--warmup 3] [--trials 128]
      [--host_trials 8] [--json profiles/trace_psd_bench.json]

  psd_ms        cg_trace_psd on the (B, T, C) batch, both launches
  ifft_ms       utils.ifft_channels_device on a (B, T, 2 C) batch of spectra
  statement_s   signals_metrics.trace_power_spectrum on --host_trials of the
                trials, scaled to the batch

The device totals are held to the statement first: e1 = sum_k |P - P64| / sum_k
P64 per neuron against the float64 statement, which must not exceed 4 x that of
the single-precision statement (the bar of tests/trace_psd_cases.py).  Timing:
--warmup calls first, then each of --runs calls between two events on the
current stream; the figure is the median, the spread min .. max.  Outputs and
workspace are allocated once, outside the timed region.  Beside the time stands
the floor of the batch: its bytes (the traces read once; the partial sums
written and read once are counted too) at the 5.9 - 6.6 TB/s the project's
streaming kernels reach.  Clocks are whatever the machine runs at; no figure
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

STREAM_TBS = (5.9, 6.6)   # the project's streaming kernels (README)


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


def _float64_totals(x):
  """The statement wholly in float64 (mean, window, transform)."""
  from calciumgan_amd.gan.utils import signals_metrics
  x = np.asarray(x, dtype=np.float64)
  T = x.shape[1]
  w = 0.5 - 0.5 * signals_metrics._cospi(2.0 * np.arange(T) / T)
  X = np.fft.rfft((x - x.mean(axis=1, keepdims=True)) * w[None, :, None], axis=1)
  return (X.real ** 2 + X.imag ** 2).sum(axis=0)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--trials', type=int, default=128)
  ap.add_argument('--seq_len', type=int, default=2048)
  ap.add_argument('--neurons', type=int, default=102)
  ap.add_argument('--host_trials', type=int, default=8,
                  help='trials the statement is timed on')
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  from calciumgan_amd import _lib
  from calciumgan_amd.data import dg
  from calciumgan_amd.gan.utils import signals_metrics, utils
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  B, T, C = args.trials, args.seq_len, args.neurons
  d = dg.make_dataset(C, T, num_segments=B, seed=1234)
  host = np.ascontiguousarray(d['signals'], dtype=np.float32)  # (B, T, C)
  x = torch.from_numpy(host).to(dev)
  nbytes = _lib.load().cg_trace_psd_ws_bytes(B, T, C)
  ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
  totals = torch.empty(T // 2 + 1, C, dtype=torch.float64, device=dev)

  def run_psd():
    _lib.call('cg_trace_psd', x, B, T, C, x.stride(0), x.stride(1), x.stride(2),
              totals, ws, _lib.stream())

  # the check: both statements on the whole batch
  k = max(1, min(args.host_trials, B))
  t0 = time.perf_counter()
  signals_metrics.trace_power_spectrum(host[:k])
  statement_s = (time.perf_counter() - t0) / k * B
  P64 = _float64_totals(host)
  norm = P64.sum(axis=0)
  single = signals_metrics.trace_power_spectrum(host, single_precision=True)
  run_psd()
  torch.cuda.synchronize()
  got = totals.cpu().numpy()
  e1 = float((np.abs(got - P64).sum(axis=0) / norm).max())
  e1_single = float((np.abs(single - P64).sum(axis=0) / norm).max())
  if not e1 <= 4 * e1_single:
    raise SystemExit('the device totals miss the statement: e1 {:.3g}, single '
                     'precision {:.3g}'.format(e1, e1_single))

  spectra = torch.from_numpy(np.random.RandomState(7).standard_normal(
      (B, T, 2 * C)).astype(np.float32)).to(dev)
  psd_ms = _summary(_event_ms(run_psd, args.warmup, args.runs))
  ifft_ms = _summary(_event_ms(
      lambda: utils.ifft_channels_device(spectra, C), args.warmup, args.runs))
  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  read_bytes = B * T * C * 4
  partial_bytes = 2 * nbytes
  bytes_floor_ms = [(read_bytes + partial_bytes) / (r * 1e12) * 1e3
                    for r in reversed(STREAM_TBS)]
  res = {
      'metric': 'power spectra of {} trials (T={}, C={})'.format(B, T, C),
      'psd_ms': psd_ms[0], 'psd_ms_min_max': psd_ms[1:],
      'ifft_ms': ifft_ms[0], 'ifft_ms_min_max': ifft_ms[1:],
      'psd_over_ifft': psd_ms[0] / ifft_ms[0],
      'statement_s': statement_s,
      'host_trials_timed': k,
      'e1': e1, 'e1_single_precision': e1_single,
      'read_bytes': read_bytes,
      'partial_bytes_written_and_read': partial_bytes,
      'bytes_floor_ms': bytes_floor_ms,
      'psd_over_bytes_floor': psd_ms[0] / bytes_floor_ms[1],
      'psd_read_tbs': read_bytes / (psd_ms[0] * 1e-3) * 1e-12,
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
