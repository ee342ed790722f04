#!/usr/bin/env python
"""Time of the nearest-stretch distances of compute_metrics.py --novelty_metrics
at BASELINE configs[2]'s report shape (128 trials of L = 2048 frames of C = 102
neurons against a DG recording of T_raw = 20432 rows at step 2: S = 9193
stretches, K = 208896, 0.49 TFLOP) on one GPU, beside its floors, one yardstick
and the host:

  python tools/bench_nearest_stretch.py [--runs 30] [--warmup 3] [--trials 128]
      [--host_trials 2] [--json profiles/nearest_stretch_bench.json]

  ms_with_d2 / ms_without_d2   cg_nearest_stretch, all five launches, with the
                (N, S) profile stored and with d2 = NULL
  host_expanded_s   signals_metrics.nearest_stretch(expanded=True) on
                --host_trials of the trials on this machine's CPUs, scaled to
                the batch (a float64 BLAS matmul against a strided view)
  bytes_floor_ms    queries and recording read once, partial sums written and
                read once, d2 written, at the 5.9 - 6.6 TB/s the project's
                streaming kernels reach
  flop_floor_ms     2 N K S at the card's dense FP64 matrix rate: the
                datasheet's 78.6 TFLOP/s (`fp64_matrix_tflops_source`; a loop of
                the instruction on registers alone, tools/probe/
                mfma_f64_probe.hip, sustains 77.9 -- not measured by this tool)
  matmul_ms_scaled  the yardstick: torch.matmul in float64 (the vendor GEMM) of
                the same queries against --yardstick_windows MATERIALISED windows
                of the same recording, scaled to S.  It is handed
                `yardstick_operand_bytes` for those windows and would need
                `yardstick_all_windows_bytes` for all of them; the kernel reads
                the `recording_bytes` of the recording.

The device result is first held to the statement (the direct difference form) on
--host_trials of the trials under the bar of tests/nearest_stretch_cases.py:
|d2 - d2_stmt| <= 4 K 2^-53 (|q|^2 + W).  Timing: --warmup calls first, then each
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

STREAM_TBS = (5.9, 6.6)        # the project's streaming kernels (README)
FP64_MATRIX_TFLOPS = 78.6      # datasheet, dense; not measured by this tool


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
  ap.add_argument('--duration', type=int, default=20432)
  ap.add_argument('--step', type=int, default=2)
  ap.add_argument('--host_trials', type=int, default=2,
                  help='trials checked against the statement and timed on the '
                  'host')
  ap.add_argument('--yardstick_windows', type=int, default=1024)
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  from calciumgan_amd import _lib
  from calciumgan_amd.data import dg
  from calciumgan_amd.gan.utils import signals_metrics as sm
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  N, L, C, T_raw, step = (args.trials, args.seq_len, args.neurons, args.duration,
                          args.step)
  K, S = L * C, sm.stretch_offsets(T_raw, L, step)
  signals, _, _ = dg.make_recording(C, T_raw, seed=1234)
  raw_host = np.ascontiguousarray(signals.T, dtype=np.float32)
  rng = np.random.RandomState(7)
  starts = rng.randint(0, T_raw - L + 1, size=N)
  q_host = np.stack([raw_host[v:v + L] for v in starts]) + np.float32(
      0.05) * rng.standard_normal((N, L, C)).astype(np.float32)
  q_host = np.ascontiguousarray(q_host, dtype=np.float32)
  raw, q = torch.from_numpy(raw_host).to(dev), torch.from_numpy(q_host).to(dev)
  nbytes = _lib.load().cg_nearest_stretch_ws_bytes(N, L, C, T_raw, step)
  ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
  d2 = torch.empty(N, S, dtype=torch.float64, device=dev)
  nearest = torch.empty(N, dtype=torch.float64, device=dev)
  index = torch.empty(N, dtype=torch.int32, device=dev)

  def run(profile):
    _lib.call('cg_nearest_stretch', q, N, L, C, q.stride(0), q.stride(1),
              q.stride(2), raw, T_raw, raw.stride(0), raw.stride(1), step, None,
              0, d2 if profile else None, nearest, index, ws, _lib.stream())

  # the check: the statement on a few of the trials
  k = max(1, min(args.host_trials, N))
  want_n, want_i, want_d2 = sm.nearest_stretch(q_host[:k], raw_host, step,
                                               return_profile=True)
  t0 = time.perf_counter()
  sm.nearest_stretch(q_host[:k], raw_host, step, expanded=True)
  host_expanded_s = (time.perf_counter() - t0) / k * N
  run(True)
  torch.cuda.synchronize()
  got_d2 = d2[:k].cpu().numpy()
  r64 = raw_host.astype(np.float64)
  rows = (r64 * r64).sum(axis=1)
  w = np.array([rows[j * step:j * step + L].sum() for j in range(S)])
  q2 = (q_host[:k].astype(np.float64) ** 2).sum(axis=(1, 2))
  bar = 4.0 * K * 2.0 ** -53 * (q2[:, None] + w[None, :])
  ratio = float((np.abs(got_d2 - want_d2) / bar).max())
  got_i = index[:k].cpu().numpy()
  near_ok = bool((np.abs(nearest[:k].cpu().numpy() - want_n) <=
                  bar[np.arange(k), want_i]).all())
  if not (ratio <= 1.0 and near_ok):
    raise SystemExit('the device distances miss the statement: err / bar '
                     '{:.3g}'.format(ratio))

  with_d2 = _summary(_event_ms(lambda: run(True), args.warmup, args.runs))
  without = _summary(_event_ms(lambda: run(False), args.warmup, args.runs))

  # the yardstick: the vendor GEMM on materialised windows
  Y = max(1, min(args.yardstick_windows, S))
  idx = (torch.arange(Y, device=dev) * step)[:, None] + torch.arange(
      L, device=dev)[None, :]
  windows = raw[idx].reshape(Y, K).double()          # (Y, K) float64
  q64 = q.reshape(N, K).double()
  out = torch.empty(N, Y, dtype=torch.float64, device=dev)
  matmul = _summary(_event_ms(
      lambda: torch.matmul(q64, windows.t(), out=out), args.warmup, args.runs))
  x = (q2[:, None] + w[None, :Y] - got_d2[:, :Y]) / 2   # the kernel's products
  matmul_agrees = bool(np.allclose(out[:k].cpu().numpy(), x, rtol=1e-9, atol=1e-6))

  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  flop = 2.0 * N * K * S
  S_pad = (S + 63) // 64 * 64
  partial_bytes = nbytes - 8 * (N + T_raw + S)
  stream_bytes = N * K * 4 + T_raw * C * 4 + 2 * partial_bytes + N * S * 8
  bytes_floor_ms = [stream_bytes / (r * 1e12) * 1e3 for r in reversed(STREAM_TBS)]
  flop_floor_ms = flop / (FP64_MATRIX_TFLOPS * 1e12) * 1e3
  matmul_scaled = matmul[0] * S / Y
  res = {
      'metric': 'nearest stretch of {} trials (L={}, C={}) in a recording of {} '
                'rows, step {}: S={}, K={}'.format(N, L, C, T_raw, step, S, K),
      'ms_with_d2': with_d2[0], 'ms_with_d2_min_max': with_d2[1:],
      'ms_without_d2': without[0], 'ms_without_d2_min_max': without[1:],
      'tflop': flop * 1e-12,
      'tflops_with_d2': flop / (with_d2[0] * 1e-3) * 1e-12,
      'host_expanded_s': host_expanded_s,
      'host_trials': k,
      'host_cpus': os.cpu_count(),
      'err_over_bar': ratio,
      'index_equals_statement': bool((got_i == want_i).all()),
      'bytes_floor_ms': bytes_floor_ms,
      'stream_bytes': stream_bytes,
      'flop_floor_ms': flop_floor_ms,
      'fp64_matrix_tflops': FP64_MATRIX_TFLOPS,
      'fp64_matrix_tflops_source': 'datasheet (dense); not measured by this tool',
      'ms_over_flop_floor': with_d2[0] / flop_floor_ms,
      'matmul_ms': matmul[0], 'matmul_ms_min_max': matmul[1:],
      'matmul_windows': Y,
      'matmul_ms_scaled': matmul_scaled,
      'ms_over_matmul_scaled': with_d2[0] / matmul_scaled,
      'matmul_agrees': matmul_agrees,
      'yardstick_operand_bytes': Y * K * 8,
      'yardstick_all_windows_bytes': S * K * 8,
      'recording_bytes': T_raw * C * 4,
      'workspace_bytes': nbytes,
      'padded_offsets': S_pad,
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
