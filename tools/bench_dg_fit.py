#!/usr/bin/env python
"""Time of the pairwise fit of the dichotomised-Gaussian model
(dataset/generate_dg_data.py) on recordings of 102 and of 512 neurons:
dg.make_recording(C, 20432), 5 151 and 130 816 pairs.

  python tools/bench_dg_fit.py [--reps 30] [--warmup 3] [--host_pairs 66]
      [--json profiles/dg_fit_bench.json]

  fit_c102_ms, fit_c512_ms   dg_fit.gauss_correlation_device
                   (cg_dg_correlation, one launch) on device tensors
  statement_c102_s dg_fit.gauss_correlation (numpy) on the 102-neuron recording
  statement_c512_s_extrapolated   the same per pair, times 130 816 pairs
  scipy_loop_s     the reference's loop (a bisection per pair around scipy's
                   multivariate_normal.cdf) on the first --host_pairs pairs
                   that bisect; scipy_loop_c102_s_extrapolated and
                   scipy_loop_c512_s_extrapolated scale it to all pairs

ms between two stream events around one call, after --warmup calls; the
median of --reps (at least 30) runs, min and max beside it.  Before anything is
timed the device results are held against the numpy statement by the rule of
dg_fit.compare_with_statement (equal status, lambda and iteration count, bit
for bit; a count off by one is excused where the statement's residual at the
earlier stop is within 1e-13 of the tolerance, for at most 1 % of the pairs;
every converged pair has |f| <= tol (1 + 1e-3)): in full at C = 102; at C = 512
on the pairs among the first 64 neurons (a pair's fit depends on nothing but
the pair), the residuals on all pairs.  Clocks are whatever the machine runs
at; no figure here is a pass criterion.  Prints ONE JSON line (and writes it to
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


def _scipy_loop(rates, gamma, cov, pairs, tol=1e-10, maxiters=1000):
  """find_root_bisection as the reference runs it, one pair at a time."""
  from scipy.stats import multivariate_normal
  r32 = rates.astype(np.float32)

  def f(i, j, lam):
    p = multivariate_normal.cdf([gamma[i], gamma[j]], mean=[0., 0.],
                                cov=[[1., lam], [lam, 1.]])
    return p - float(r32[i] * r32[j]) - cov[i, j]

  out = []
  for i, j in pairs:
    lo, hi = -0.99999, 0.99999
    f0, f1 = f(i, j, lo), f(i, j, hi)
    if abs(f0) < tol or abs(f1) < tol or f0 * f1 > tol:
      out.append(0.0)
      continue
    res, it, mid = np.inf, 0, 0.0
    while abs(res) > tol and it < maxiters:
      mid = (lo + hi) / 2
      res = f(i, j, mid)
      if res > 0:
        hi = mid
      elif res < 0:
        lo = mid
      it += 1
    out.append(mid)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--host_pairs', type=int, default=66)
  ap.add_argument('--duration', type=int, default=20432)
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='',
                  help='recorded as is (default: git rev-parse --short HEAD)')
  args = ap.parse_args()
  from calciumgan_amd.data import dg, dg_fit
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  reps = max(args.reps, 30)
  tol = 1e-10

  stats, device_in, results = {}, {}, {}
  for C in (102, 512):
    _, spikes, _ = dg.make_recording(C, args.duration)
    stats[C] = dg_fit.recording_statistics(spikes)
    device_in[C] = tuple(torch.from_numpy(v).to(dev) for v in stats[C])
    results[C] = tuple(t.cpu().numpy() for t in
                       dg_fit.gauss_correlation_device(*device_in[C], tol=tol))

  # the check, and the host's times
  def held(C, n, got):
    rates, gamma, cov = (stats[C][0][:n], stats[C][1][:n], stats[C][2][:n, :n])
    t0 = time.perf_counter()
    want = dg_fit.gauss_correlation(rates, gamma, cov, tol)
    seconds = time.perf_counter() - t0
    report = dg_fit.compare_with_statement(
        rates, gamma, cov, tuple(a[:n, :n] for a in got), want, tol)
    if report['failures'] or report['excused'] > report['pairs'] // 100:
      raise SystemExit('C = {}: the device result differs from the statement: '
                       '{} excused of {}, {}'.format(
                           C, report['excused'], report['pairs'],
                           report['failures'][:5]))
    return report, seconds, want

  report102, statement_s, want102 = held(102, 102, results[102])
  report512, _, _ = held(512, 64, results[512])
  i, j = np.tril_indices(512, -1)
  conv = results[512][1][i, j] == 0
  res = dg_fit.pair_function(*stats[512], i[conv], j[conv],
                             results[512][0][i, j][conv])
  if not np.all(np.abs(res) <= tol * (1 + 1e-3)):
    raise SystemExit('C = 512: a converged pair with residual {}'.format(
        np.abs(res).max()))

  i102, j102 = np.tril_indices(102, -1)
  bisecting = [(a, b) for a, b in zip(i102, j102)
               if want102[2][a, b] > 0][:max(args.host_pairs, 1)]
  t0 = time.perf_counter()
  _scipy_loop(*stats[102], bisecting, tol)
  scipy_s = time.perf_counter() - t0
  per_pair = scipy_s / len(bisecting)

  times = {}
  for C in (102, 512):
    for _ in range(args.warmup):
      dg_fit.gauss_correlation_device(*device_in[C], tol=tol)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
      start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
      start.record()
      dg_fit.gauss_correlation_device(*device_in[C], tol=tol)
      end.record()
      end.synchronize()
      ms.append(start.elapsed_time(end))
    times['fit_c{}_ms'.format(C)] = ms
  try:
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT,
        stderr=subprocess.DEVNULL).decode().strip()
  except Exception:  # noqa: BLE001 -- not a git checkout
    commit = 'unknown'
  out = {'metric': 'latent correlations of the DG fit: dg.make_recording(C, '
                   '{}), C = 102 (5151 pairs) and C = 512 (130816 pairs), tol '
                   '1e-10'.format(args.duration)}
  for name, ms in times.items():
    out[name] = statistics.median(ms)
    out[name + '_min'] = min(ms)
    out[name + '_max'] = max(ms)
  for C in (102, 512):
    k, l = np.tril_indices(C, -1)
    status = results[C][1][k, l]
    out['status_counts_c{}'.format(C)] = [int((status == s).sum())
                                          for s in range(6)]
  out.update({
      'statement_c102_s': statement_s,
      'statement_c512_s_extrapolated': statement_s * 130816 / 5151,
      'scipy_loop_pairs': len(bisecting),
      'scipy_loop_s': scipy_s,
      'scipy_loop_c102_s_extrapolated': per_pair * 5151,
      'scipy_loop_c512_s_extrapolated': per_pair * 130816,
      'excused_c102': report102['excused'],
      'excused_c512_first64': report512['excused'],
      'pairs_checked_c102': report102['pairs'],
      'pairs_checked_c512_first64': report512['pairs'],
      'held_against_statement': True,
      'reps': reps,
      'warmup': args.warmup,
      'n_gpus': 1,
      'gpu': torch.cuda.get_device_name(0),
      'box': socket.gethostname(),
      'commit': commit,
      'conditions': 'one MI355X, one run, clocks not pinned; host figures on '
                    'the same machine\'s CPU, the extrapolated ones scaled by '
                    'the number of pairs',
  })
  line = json.dumps(out)
  if args.json:
    with open(args.json, 'w') as f:
      f.write(line + '\n')
  print(line)


if __name__ == '__main__':
  main()
