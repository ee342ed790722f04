#!/usr/bin/env python
"""Time of cutting one training batch out of a resident recording at BASELINE
configs[1]'s shapes -- 128 windows of 2048 rows of 102 neurons, stride-2 starts
of a DG recording (data/dg.py make_recording) -- against gathering the same
batch from the materialised resident set, which is what an array / TFRecord
directory trains from (ArrayDataset: torch.index_select(..., out=)).

  python tools/bench_window_batch.py [--reps 30] [--warmup 3] [--inner 10]
      [--segments 1024] [--json profiles/window_batch_bench.json]

Every variant writes into one (128, 2048, channels) batch buffer, as main.py
binds GAN.batch_buffer; each rep draws another sorted batch of windows (uploaded
before anything is timed).  A rep times --inner launches of one variant between
two events recorded on the stream and divides; the four variants alternate
inside every rep, so they share the box and the moment.

  window_plain_ms   cg_window_batch, fft = 0, normalised: median (min, max)
  window_fft_ms     cg_window_batch, fft = 1, normalised
  select_plain_ms   torch.index_select from the materialised (N, 2048, 102) set
  select_fft_ms     torch.index_select from the materialised (N, 2048, 204) set
  *_tb_per_s        bytes the launch has to move (*_mb: the windows in, the batch
                    out) over the median
  host_plain_s / host_fft_s   dataset_helper.window_batch (numpy) of one batch on
                    this machine's CPU, best of two
  resident_*        bytes a run keeps in HBM at configs[1]'s 9192 segments: the
                    recording, against the windows as traces and as spectra
                    (computed from shapes; the timed sets hold --segments windows)

Before anything is timed the plain launch is compared with the numpy statement
byte for byte, and the FFT launch with the float64 transform of the float32
windows (Higham's bound and 4 x single-precision pocketfft, as
tests/window_cases.py states them).  Clocks are whatever the machine runs at;
no time here is a pass criterion.  Prints ONE JSON line (and writes it to
--json)."""
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

CFG_SEGMENTS = 9192  # BASELINE configs[1]: segments of the whole set


def _stats(ms):
  return statistics.median(ms), min(ms), max(ms)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--inner', type=int, default=10)
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--seq_len', type=int, default=2048)
  ap.add_argument('--neurons', type=int, default=102)
  ap.add_argument('--segments', type=int, default=1024,
                  help='windows of the materialised sets the gathers read')
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  import scipy.fft
  from calciumgan_amd.data import dg, recording
  from calciumgan_amd.gan.utils import dataset_helper as dh
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  B, L, C, N = args.batch, args.seq_len, args.neurons, args.segments
  reps, inner = max(args.reps, 20), max(args.inner, 1)
  signals, spikes, _ = dg.make_recording(C, L + 2 * N, 1234)
  recs = {fft: recording.build(signals, spikes, L, fft=fft, validation_size=0,
                               max_segments=N, device=dev if fft else None)
          for fft in (False, True)}
  raw_host = recs[False]['raw']
  raw = torch.from_numpy(raw_host).to(dev)
  norm = {fft: recording.normalisation(recs[fft]['info']) for fft in recs}

  # the batches: sorted positions of B windows, window i begins at row 2 i
  rng = np.random.RandomState(7)
  pos = [np.sort(rng.permutation(N)[:B]) for _ in range(reps + args.warmup)]
  dev_pos = [torch.from_numpy(p).to(dev) for p in pos]
  dev_starts = [torch.from_numpy((2 * p).astype(np.int32)).to(dev) for p in pos]
  out = {fft: torch.empty((B, L, 2 * C if fft else C), device=dev)
         for fft in recs}

  def window(fft, k):
    return dh.window_batch_device(raw, dev_starts[k], L, fft, *norm[fft],
                                  out=out[fft])

  # the checks, on the first batch
  plain = window(False, 0).cpu().numpy()
  want = dh.window_batch(raw_host, 2 * pos[0], L, False, *norm[False])
  if plain.tobytes() != want.tobytes():
    raise SystemExit('the plain launch differs from the numpy statement')
  spec = dh.window_batch_device(raw, dev_starts[0], L, True).cpu().numpy()
  z64 = np.fft.fft(dh.window_batch(raw_host, 2 * pos[0], L).astype(np.float64),
                   axis=1)

  def errors(z):
    return float((np.sqrt((np.abs(z - z64) ** 2).sum(1)) /
                  np.sqrt((np.abs(z64) ** 2).sum(1))).max())

  e = errors(spec[..., :C].astype(np.float64) + 1j * spec[..., C:])
  e_ref = errors(scipy.fft.fft(
      dh.window_batch(raw_host, 2 * pos[0], L).astype(np.complex64), axis=1))
  u = 2.0 ** -24
  bound = float(np.log2(L) * (2 * u + 4 * u / (1 - 4 * u) * (np.sqrt(2.0) + 2 * u)))
  if not (e <= bound and e <= 4 * e_ref):
    raise SystemExit('error {} against the float64 transform: bound {}, '
                     'single-precision pocketfft {}'.format(e, bound, e_ref))

  # the materialised resident sets, cut by the same kernel
  sets = {}
  for fft in recs:
    full = torch.empty((N, L, 2 * C if fft else C), device=dev)
    all_starts = torch.arange(0, 2 * N, 2, dtype=torch.int32, device=dev)
    for i in range(0, N, B):
      dh.window_batch_device(raw, all_starts[i:i + B], L, fft, *norm[fft],
                             out=full[i:i + B])
    sets[fft] = full
  torch.cuda.synchronize()
  if not torch.equal(sets[False].index_select(0, dev_pos[0]).cpu(),
                     torch.from_numpy(plain)):
    raise SystemExit('index_select of the materialised set differs')

  def select(fft, k):
    return torch.index_select(sets[fft], 0, dev_pos[k], out=out[fft])

  variants = {
      'window_plain': lambda k: window(False, k),
      'window_fft': lambda k: window(True, k),
      'select_plain': lambda k: select(False, k),
      'select_fft': lambda k: select(True, k),
  }
  host = {}
  for fft in recs:
    best = []
    for _ in range(2):
      t0 = time.perf_counter()
      dh.window_batch(raw_host, 2 * pos[0], L, fft, *norm[fft])
      best.append(time.perf_counter() - t0)
    host[fft] = min(best)

  for k in range(args.warmup):
    for fn in variants.values():
      fn(k)
  ms = {name: [] for name in variants}
  for r in range(reps):
    k = args.warmup + r
    for name, fn in variants.items():
      start = torch.cuda.Event(enable_timing=True)
      stop = torch.cuda.Event(enable_timing=True)
      torch.cuda.synchronize()
      start.record()
      for _ in range(inner):
        fn(k)
      stop.record()
      torch.cuda.synchronize()
      ms[name].append(start.elapsed_time(stop) / inner)

  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  window_bytes = 4 * B * L * C
  moved = {'window_plain': 2 * window_bytes, 'window_fft': 3 * window_bytes,
           'select_plain': 2 * window_bytes, 'select_fft': 4 * window_bytes}
  res = {'metric': 'one batch of {} windows ({} rows x {} neurons) into the '
                   'batch buffer: cut out of the resident recording '
                   '(cg_window_batch) against index_select from the '
                   'materialised resident set'.format(B, L, C)}
  for name in variants:
    med, lo, hi = _stats(ms[name])
    res[name + '_ms'] = med
    res[name + '_ms_min'] = lo
    res[name + '_ms_max'] = hi
    res[name + '_mb'] = moved[name] / 1e6
    res[name + '_tb_per_s'] = moved[name] / 1e12 / (med * 1e-3)
  res.update({
      'host_plain_s': host[False],
      'host_fft_s': host[True],
      'resident_recording_mb': 4 * (L + 2 * CFG_SEGMENTS) * C / 1e6,
      'resident_windows_mb': 4 * CFG_SEGMENTS * L * C / 1e6,
      'resident_spectra_mb': 8 * CFG_SEGMENTS * L * C / 1e6,
      'resident_for_segments': CFG_SEGMENTS,
      'timed_set_segments': N,
      'max_error': e,
      'max_error_pocketfft_f32': e_ref,
      'higham_bound': bound,
      'plain_is_the_statement': True,
      'window_plain_faster_than_select': bool(
          res['window_plain_ms'] < res['select_plain_ms']),
      'window_fft_faster_than_select': bool(
          res['window_fft_ms'] < res['select_fft_ms']),
      'reps': reps,
      'inner': inner,
      'warmup': args.warmup,
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
