"""The shared case table of the trace power-spectrum tests
(tests/test_trace_psd_host.py, tests/test_hip_trace_psd.py): seeded (B, T, C)
float32 trials as read-only numpy arrays with the memory layout the device test
gives them, the float64 reference, and the two bars every case is held to.

The error figure per neuron is e1 = sum_k |P - P64| / sum_k P64 on the
trial-summed totals, P64 the statement wholly in float64 (mean, window and
transform).  Bars:
  (a) e1 <= 2 eps + eps^2 + 3 u, eps = higham_bound(T) + eps_in, u = 2^-24,
      eps_in = u (|m| ||w||_2 + 2 ||y||_2) / ||y||_2 per trace, the largest over
      a neuron's trials: the float32 roundings of the mean, the subtraction and
      the window as a relative 2-norm error of y, the transform's on top, taken
      through |X|^2 = |X64 + d|^2 by Cauchy-Schwarz (sum_k | |X|^2 - |X64|^2 |
      <= 2 ||X64|| ||d|| + ||d||^2), and 3 u for a float32 |X|^2 (two squares
      and a sum; the device forms them in float64)
  (b) the worst e1 <= 4 x the worst e1 of trace_power_spectrum(
      single_precision=True) (single-precision pocketfft), the margin of
      ifft_cases.check_accuracy.
Three results on tones cases are held to (a) only (`BAR_A_ONLY`; their ratio is
still printed and recorded).  Single-precision pocketfft is almost exact on a
pure tone (e1 1.4e-9 .. 4.3e-9 from T = 512 up), so (b) there asks for an error
far below what one float32 rounding of y, or of a stage's twiddle product,
leaves -- while (a) is three orders of magnitude away.  A host build of the
kernel's own pipeline (float32 mean, window and the stages of
csrc/fft_stages.h, contracted; float64 unpacking) gives ratios of 1.69 (T =
128), 1.00 (512), 6.3 (1024), 3.92 (2048), 6.7 (4096) and 16 (8192) on these
tones, and 0.70 .. 1.56 on DG and normal trials at every length.  Measured on
one MI355X (profiles/fft_lengths_parity.txt): 1.00 (128), 1.00 (512), 1.00
(1024), 3.92 (2048), 1.70 (4096), 10.2 (8192, e1 1.74e-8).  So the device's
totals keep both bars on every tones case but the one at 8192, which a correct
kernel need not meet.  The module's numpy statement (float32 y, float64
transform) is 13.7 and 4.7 times pocketfft's at 512 and 1024 (e1 1.9e-8 and
1.1e-8: the rounding of y to float32 alone) and held to (a) only there; at 128,
2048, 4096 and 8192 it is 3.5, 1.05, 0.76 and 1.05 times and keeps both bars.

Shapes are the smallest at which each mechanism of csrc/trace_psd.hip can break,
with G = min(16, 8192 / T) neuron PAIRS per workgroup: one neuron whose partner
is absent, 2 G + 1 neurons (a ragged second group and an odd leftover), every
accepted T -- 32 (an odd log2 T: the radix-2 stage), 64 (none), 128 (the radix-2
stage on a quarter-full image), 512 (the first full image at G = 16: all 8
positions of a lane live), 1024 (G = 8: 16 columns, the column fold of the mean
stops at 16), the report's 2048 and C = 102, 4096 (G = 2: 4 columns), 8192
(G = 1) --, a B of two chunks of trials plus one trial, the chunk plan at its
cap of 64 chunks and just past it (61 chunks of 5), an item count that is a
multiple of 8 below the grid (the renumbered walk of the items), and more
items than one walk of the 1024-workgroup grid."""
import functools
import json
import os
import pickle

import numpy as np

from calciumgan_amd.data import dg
from calciumgan_amd.gan.utils import h5_helper, signals_metrics
from ifft_cases import higham_bound

U = 2.0 ** -24
MAX_GRID = 1024      # csrc/trace_psd.hip: kPsdMaxGrid
TARGET_ITEMS = 512   # kPsdTargetItems
MAX_CHUNKS = 64      # kPsdMaxChunks
MIN_CHUNK = 4        # kPsdMinChunk


def group(T):
  """Neuron pairs per workgroup of csrc/trace_psd.hip."""
  return min(16, 8192 // T)


def plan(B, T, C):
  """(neuron groups, trials per chunk, chunks) of csrc/trace_psd.hip: psd_plan."""
  groups = (C - 1) // (2 * group(T)) + 1
  want = min((TARGET_ITEMS - 1) // groups + 1, MAX_CHUNKS)
  chunk_len = min(max((B - 1) // want + 1, MIN_CHUNK), B)
  return groups, chunk_len, (B - 1) // chunk_len + 1


def _dg(B, T, C, seed):
  return np.asarray(dg.make_dataset(num_neurons=C, sequence_length=T,
                                    num_segments=B, seed=seed)['signals'],
                    dtype=np.float32)


def _normal(B, T, C, seed):
  return np.random.RandomState(seed).standard_normal((B, T, C)).astype(
      np.float32)


def tone_bins(T):
  """Bins of the tones of `_tones`: (trial, neuron) -> bin."""
  return {(0, 0): 1, (0, 1): T // 4 + 1, (1, 0): T // 2 - 1, (1, 1): T // 2}


def _tones(T):
  """Two trials of the two neurons of one pair, each a unit cosine at a bin of
  its own: neuron 0 at 1 and T / 2 - 1, neuron 1 at T / 4 + 1 and T / 2 (a
  swapped unpacking or a wrong digit reversal moves them)."""
  t = np.arange(T)
  x = np.zeros((2, T, 2), np.float32)
  for (b, c), k in tone_bins(T).items():
    x[b, :, c] = np.cos(2 * np.pi * k * t / T)
  return x


# name -> (trials builder, layout[, results held to bar (a) only]); layouts:
# 'contig', 'padded' (channel pitch > C), 'permuted' (stored (B, C, T), viewed
# (B, T, C)); the third entry names the results ('device': cg_trace_psd,
# 'numpy': the module's statement) that the docstring's tones finding takes out
# of bar (b)
_TABLE = {
    't32_c1_dg': (lambda: _dg(1, 32, 1, 1), 'contig'),
    't32_c33_normal': (lambda: _normal(3, 32, 33, 2), 'contig'),
    't32_tones': (lambda: _tones(32), 'contig'),
    't64_c17_dg': (lambda: _dg(2, 64, 17, 3), 'contig'),
    't64_c5_permuted': (lambda: _normal(3, 64, 5, 4), 'permuted'),
    't64_tones': (lambda: _tones(64), 'contig'),
    # chunks of 4 trials: 4 + 4 + 1
    't64_c3_three_chunks': (lambda: _dg(9, 64, 3, 5), 'contig'),
    # one group, 64 chunks of 4 trials, the last of one trial: (1, 4, 64)
    't32_c3_64_chunks': (lambda: _dg(253, 32, 3, 13), 'contig'),
    # past the cap: 61 chunks of 5 trials, the last of one trial: (1, 5, 61)
    't32_c3_chunks_of_5': (lambda: _normal(301, 32, 3, 14), 'contig'),
    't128_c33_normal': (lambda: _normal(3, 128, 33, 15), 'contig'),
    't128_tones': (lambda: _tones(128), 'contig'),
    't256_c5_normal': (lambda: _normal(2, 256, 5, 6), 'contig'),
    't256_c6_padded': (lambda: _dg(2, 256, 6, 7), 'padded'),
    't512_c5_dg': (lambda: _dg(3, 512, 5, 16), 'contig'),
    't512_tones': (lambda: _tones(512), 'contig', 'numpy'),
    # G = 8: 2 G + 1 neurons
    't1024_c17_normal': (lambda: _normal(2, 1024, 17, 17), 'contig'),
    # 8 groups of 16 neurons, one chunk: 8 items, a multiple of 8 below the grid
    't1024_c128_renumbered': (lambda: _normal(2, 1024, 128, 18), 'contig'),
    't1024_tones': (lambda: _tones(1024), 'contig', 'numpy'),
    't2048_c9_dg': (lambda: _dg(3, 2048, 9, 8), 'contig'),
    't2048_c102_dg': (lambda: _dg(1, 2048, 102, 10), 'contig'),
    't2048_tones': (lambda: _tones(2048), 'contig'),
    # G = 2: 2 G + 1 neurons; one neuron whose partner is absent
    't4096_c5_normal': (lambda: _normal(2, 4096, 5, 19), 'contig'),
    't4096_c1_dg': (lambda: _dg(2, 4096, 1, 20), 'contig'),
    't4096_tones': (lambda: _tones(4096), 'contig'),
    't8192_c3_normal': (lambda: _normal(2, 8192, 3, 11), 'contig'),
    't8192_tones': (lambda: _tones(8192), 'contig', 'device'),
    # 1025 groups of 32 neurons, one chunk: 1025 items > 1024 workgroups
    't32_c32769_grid_stride': (lambda: _normal(1, 32, 32 * 1024 + 1, 12),
                               'contig'),
}
CASES = tuple(_TABLE)
# name -> the results of the case that are held to bar (a) only
BAR_A_ONLY = {n: frozenset(_TABLE[n][2].split()) for n in CASES
              if len(_TABLE[n]) > 2}


def items(name):
  """Workgroup items of csrc/trace_psd.hip for the case: groups x chunks."""
  groups, _, chunks = plan(*case(name)[0].shape)
  return groups * chunks


@functools.lru_cache(maxsize=None)
def case(name):
  """(x (B, T, C) float32 read-only, layout)."""
  build, layout = _TABLE[name][:2]
  x = np.ascontiguousarray(build(), dtype=np.float32)
  assert x.ndim == 3
  x.setflags(write=False)
  return x, layout


def float64_totals(x):
  """P64 (T / 2 + 1, C): the statement with a float64 mean, window, product and
  transform."""
  x = np.asarray(x, dtype=np.float64)
  T = x.shape[1]
  w = 0.5 - 0.5 * signals_metrics._cospi(2.0 * np.arange(T) / T)
  y = (x - x.mean(axis=1, keepdims=True)) * w[None, :, None]
  X = np.fft.rfft(y, axis=1)
  return (X.real ** 2 + X.imag ** 2).sum(axis=0)


@functools.lru_cache(maxsize=None)
def reference(name):
  p = float64_totals(case(name)[0])
  p.setflags(write=False)
  return p


def e1(P, P64):
  """(C,) float64: sum_k |P - P64| / sum_k P64, NaN where P64 is all zero -- and
  there P must be exactly zero."""
  P = np.asarray(P, dtype=np.float64)
  assert P.shape == P64.shape, (P.shape, P64.shape)
  norm = P64.sum(axis=0)
  zero = norm == 0
  assert not P[:, zero].any()
  with np.errstate(invalid='ignore', divide='ignore'):
    return np.where(zero, np.nan, np.abs(P - P64).sum(axis=0) / norm)


def input_error(x):
  """(C,) float64: eps_in of the docstring, the largest over the trials."""
  x = np.asarray(x, dtype=np.float32)
  w = signals_metrics.hann_window(x.shape[1])
  m = (x.astype(np.float64).sum(axis=1) / x.shape[1]).astype(np.float32)
  y = signals_metrics._windowed(x, w).astype(np.float64)
  ny = np.sqrt((y * y).sum(axis=1))                      # (B, C)
  nw = np.sqrt((w.astype(np.float64) ** 2).sum())
  with np.errstate(invalid='ignore', divide='ignore'):
    eps = U * (np.abs(m.astype(np.float64)) * nw + 2 * ny) / ny
  return np.where(ny > 0, eps, 0.0).max(axis=0)  # (no trace: nothing to bound)


def derived_bound(x):
  """(C,) float64: bar (a) for the trials x."""
  eps = higham_bound(np.shape(x)[1]) + input_error(x)
  return 2 * eps + eps * eps + 3 * U


@functools.lru_cache(maxsize=None)
def single_precision_e1(name):
  return e1(signals_metrics.trace_power_spectrum(case(name)[0],
                                                 single_precision=True),
            reference(name))


def check_accuracy(P, name, x=None, what='device'):
  """Both bars on (T / 2 + 1, C) totals of the case (or of the trials x, a
  variant of the case's) -- bar (a) alone on a result that BAR_A_ONLY names;
  returns (worst e1, worst e1 of the single-precision
  statement, smallest bound).  CALCIUMGAN_TRACE_PSD_PARITY_OUT=<file>: the line
  printed is appended there (profiles/trace_psd_parity.txt is made from it)."""
  if x is None:
    x, P64, ref = case(name)[0], reference(name), single_precision_e1(name)
  else:
    P64 = float64_totals(x)
    ref = e1(signals_metrics.trace_power_spectrum(x, single_precision=True), P64)
  e = e1(P, P64)
  if np.isnan(e).all():
    return 0.0, 0.0, 0.0
  bound = derived_bound(x)
  worst, worst_ref = float(np.nanmax(e)), float(np.nanmax(ref))
  line = '%-24s %-7s shape %-16s max e1 %.3g  single-precision %.3g  (ratio ' \
      '%.2f)  bound (a) %.3g' % (name, what, 'x'.join(map(str, x.shape)), worst,
                                 worst_ref, worst / worst_ref,
                                 float(np.nanmin(bound)))
  print(line)
  path = os.environ.get('CALCIUMGAN_TRACE_PSD_PARITY_OUT')
  if path:
    with open(path, 'a') as f:
      f.write(line + '\n')
  ok = ~np.isnan(e)
  assert (e[ok] <= bound[ok]).all(), (name, worst, bound[ok].min())
  if what not in BAR_A_ONLY.get(name, ()):
    assert worst <= 4 * worst_ref, (name, worst, worst_ref)
  return worst, worst_ref, float(np.nanmin(bound))


def run_dir(path, T=512, C=6, trials=12):
  """A DG run directory of trials of T frames: the validation cache with its
  spikes, and one generated file holding the traces of another seed with 0.03
  added to every even frame.  Returns (generated file, recorded signals,
  generated signals)."""
  real = dg.make_dataset(num_neurons=C, sequence_length=T, num_segments=trials,
                         seed=21)
  other = dg.make_dataset(num_neurons=C, sequence_length=T, num_segments=trials,
                          seed=22)
  gen_dir = path / 'generated'
  os.makedirs(gen_dir)
  val = str(gen_dir / 'validation.h5')
  sig = np.asarray(real['signals'], dtype=np.float32)
  gen = np.array(other['signals'], dtype=np.float32)
  gen[:, 0::2] += np.float32(0.03)
  h5_helper.write(val, {'signals': sig, 'spikes': real['spikes'].astype(np.int8)})
  fake = str(gen_dir / 'epoch000_signals.h5')
  h5_helper.write(fake, {'signals': gen})
  with open(gen_dir / 'info.pkl', 'wb') as f:
    pickle.dump({0: {'global_step': 1, 'filename': fake}}, f)
  with open(path / 'hparams.json', 'w') as f:
    json.dump(dict(generated_dir=str(gen_dir), validation_cache=val,
                   num_neurons=C, sequence_length=T), f)
  return fake, sig, gen
