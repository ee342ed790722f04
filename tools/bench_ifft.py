#!/usr/bin/env python
"""Time of the inverse FFT of a generated batch of an FFT dataset at BASELINE
configs[1]'s validation shapes: 128 samples of [real | imag] spectra (T = 2048,
2 x 102 channels), the normalised spectra of DG traces (data/dg.py,
make_dataset(fft=True)), denormalised and inverted to (128, 2048, 102) traces.

  python tools/bench_ifft.py [--reps 30] [--warmup 3] [--samples 128]
      [--json profiles/ifft_bench.json]

  device_ms      utils.ifft_channels_device (cg_ifft_channels, one launch):
                 median of --reps warm runs, each timed on its own with a
                 synchronize on both sides; min and max beside it
  event_ms       the same launches between two events recorded on the stream
  gb_per_s       bytes the launch has to move (the spectra in, the traces out)
                 over event_ms; floor_mb is that number of bytes
  host_s         utils.ifft_channels (numpy, complex64) of the same denormalised
                 batch on this machine's CPU, best of two
  transfer_ms    what a host transform in the middle of the validation chain
                 would add: the batch down and the traces up again

Before anything is timed the device result is compared with the float64 inverse
transform of the float32 input: per trace e = ||y - y64|| / ||y64||, held to
Higham's bound log2(T) eta and to 4 x the same error of single-precision
pocketfft (scipy.fft.ifft on complex64), as tests/ifft_cases.py states them.
Clocks are whatever the machine runs at; no time here is a pass criterion.
Prints ONE JSON line (and writes it to --json)."""
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


def _each_event(fn, reps):
  out = []
  for _ in range(reps):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    out.append(start.elapsed_time(stop))
  return out


def _errors(y, y64):
  norm = np.sqrt((y64 * y64).sum(axis=1))
  return np.sqrt(((y.astype(np.float64) - y64) ** 2).sum(axis=1)) / norm


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--samples', type=int, default=128)
  ap.add_argument('--seq_len', type=int, default=2048)
  ap.add_argument('--neurons', type=int, default=102)
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  import scipy.fft
  from calciumgan_amd.data import dg
  from calciumgan_amd.gan.utils import utils
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  B, T, C = args.samples, args.seq_len, args.neurons
  reps = max(args.reps, 20)
  d = dg.make_dataset(C, T, num_segments=B, fft=True)
  x_host = np.ascontiguousarray(d['signals'], dtype=np.float32)
  smin, smax = d['info']['signals_min'], d['info']['signals_max']
  scale, offset = smax - smin, smin
  x = torch.from_numpy(x_host).to(dev)

  def launch():
    return utils.ifft_channels_device(x, C, scale=scale, offset=offset)

  # the check: the float64 transform of the float32 input the kernel forms
  got = launch().cpu().numpy()
  xin = (x_host * np.float32(scale)).astype(np.float32) + np.float32(offset)
  z = xin[..., :C].astype(np.complex128) + 1j * xin[..., C:].astype(np.complex128)
  y64 = np.fft.ifft(z, axis=1).real
  e = float(_errors(got, y64).max())
  e_ref = float(_errors(scipy.fft.ifft(z.astype(np.complex64), axis=1).real,
                        y64).max())
  u = 2.0 ** -24
  bound = float(np.log2(T) * (2 * u + 4 * u / (1 - 4 * u) * (np.sqrt(2.0) + 2 * u)))
  if not (e <= bound and e <= 4 * e_ref):
    raise SystemExit('error {} against the float64 transform: bound {}, '
                     'single-precision pocketfft {}'.format(e, bound, e_ref))

  host = []
  for _ in range(2):
    t0 = time.perf_counter()
    utils.ifft_channels(utils.denormalize(x_host, smin, smax))
    host.append(time.perf_counter() - t0)
  t0 = time.perf_counter()
  down = x.cpu()
  torch.from_numpy(got).to(dev)
  torch.cuda.synchronize()
  transfer_ms = (time.perf_counter() - t0) * 1e3
  del down

  for _ in range(args.warmup):
    launch()
  wall_ms = _each(launch, reps)
  event_ms = _each_event(launch, reps)
  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  moved = 4 * B * T * 3 * C
  ev = statistics.median(event_ms)
  res = {
      'metric': 'inverse FFT of {} samples of [real | imag] spectra (T={}, '
                '2 x {} channels) to traces'.format(B, T, C),
      'device_ms': statistics.median(wall_ms),
      'device_ms_min': min(wall_ms),
      'device_ms_max': max(wall_ms),
      'event_ms': ev,
      'event_ms_min': min(event_ms),
      'event_ms_max': max(event_ms),
      'floor_mb': moved / 1e6,
      'gb_per_s': moved / 1e9 / (ev * 1e-3),
      'host_s': min(host),
      'transfer_ms': transfer_ms,
      'max_error': e,
      'max_error_pocketfft_f32': e_ref,
      'higham_bound': bound,
      'within_bounds': True,
      'device_faster_than_host': bool(ev * 1e-3 < min(host)),
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
