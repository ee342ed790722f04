"""CPU test of the butterfly stages the three FFT kernels share
(calciumgan_amd/csrc/fft_stages.h, included unmodified): tests/fft_stages_host.cc
is built with g++ and the address and undefined-behaviour sanitizers into the
test's temporary directory and run as a child process; nothing is preloaded and
the child runs no Python.  No GPU.

`check` holds, for every T in 32 .. 8192 with the kernels' G = min(16, 8192 / T)
and rows_mask = 32 / G - 1: ifft_phys a bijection of [0, T); ifft_row_of_time the
inverse of ifft_time_of_row; bit 1 of a row clear exactly when its bin is below
T / 2 and row 2 holding bin T / 2; psd_low_row listing each such row once; the
mirror-row table of trace_psd.hip inside [0, T); in every stage, the radix-2 one
included, the butterflies' elements inside the image, pairwise disjoint and
covering it (the only reason the stages need no barrier inside them); every
leg's rows of an LDS lane group on distinct bank positions; one-hot bins under
Higham's bound; the schedule walked lane by lane as the kernels' 512 lanes walk
it, with their batches of 4 and of 2 butterflies, leaving the bytes that one
butterfly after the other leaves.  The order of the stages, a lane's walk and
the driver are the header's own, the ones the kernels call.

`ifft` runs the whole schedule one butterfly after the other on float32 spectra
from a file; the result is held to np.fft.ifft in complex128 under
ifft_cases.higham_bound(T) (measured: at most 1.3e-7 against a smallest bound of
2.3e-6)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ifft_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'tests', 'fft_stages_host.cc')
CSRC = os.path.join(ROOT, 'calciumgan_amd', 'csrc')
LENGTHS = (32, 64, 128, 256, 512, 1024, 2048, 4096, 8192)


@pytest.fixture(scope='module')
def program(tmp_path_factory):
  assert shutil.which('g++'), 'the host program needs g++'
  exe = str(tmp_path_factory.mktemp('fft_stages_host') / 'fft_stages_host')
  # (the sanitizers' runtimes linked into the program: it runs whatever else
  # the loader brings in first)
  subprocess.check_call(['g++', '-std=c++17', '-O1', '-g',
                         '-fsanitize=address,undefined',
                         '-fno-sanitize-recover=all', '-static-libasan',
                         '-static-libubsan', '-I', CSRC, SOURCE, '-o', exe])
  return exe


def _run(args):
  return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                        universal_newlines=True)


def test_the_index_functions_and_every_stage_at_every_length(program):
  done = _run([program, 'check'])
  print(done.stdout)
  assert done.returncode == 0, done.stdout
  lines = done.stdout.splitlines()
  assert lines[-1] == 'all checks passed'
  assert [int(l.split()[1]) for l in lines[:-1]] == list(LENGTHS)
  assert [int(l.split()[3]) for l in lines[:-1]] == [
      ifft_cases.group(T) for T in LENGTHS]
  assert [int(l.split()[5]) for l in lines[:-1]] == [
      32 // ifft_cases.group(T) - 1 for T in LENGTHS]


def _spectra(T):
  """(n, T) complex64: ifft_cases.group(T) + 1 traces of normal deviates (a full
  group and a ragged one), then the one-hot bins of ifft_cases._bins as a real 1
  and as an imaginary 1."""
  G = ifft_cases.group(T)
  rng = np.random.RandomState(T)
  z = (rng.standard_normal((G + 1, T)) +
       1j * rng.standard_normal((G + 1, T))).astype(np.complex64)
  bins = ifft_cases._bins(T)                       # (3, T, 4): [re0 re1 | im0 im1]
  hot = np.concatenate([bins[:, :, 0] + 1j * bins[:, :, 2],
                        bins[:, :, 1] + 1j * bins[:, :, 3]]).astype(np.complex64)
  assert hot.shape == (6, T) and (np.abs(hot).sum(axis=1) == 1).all()
  return np.concatenate([z, hot])


@pytest.mark.parametrize('T', LENGTHS)
def test_the_schedule_run_in_order_is_the_inverse_transform(program, tmp_path, T):
  z = _spectra(T)
  n = len(z)
  src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
  z.view(np.float32).reshape(n, T, 2).tofile(src)
  done = _run([program, 'ifft', str(T), str(n), src, dst])
  assert done.returncode == 0, done.stdout
  y = np.fromfile(dst, dtype=np.float32).reshape(n, T, 2)
  y = y[..., 0].astype(np.float64) + 1j * y[..., 1]
  y64 = np.fft.ifft(z.astype(np.complex128), axis=1)
  e = np.sqrt((np.abs(y - y64) ** 2).sum(axis=1) / (np.abs(y64) ** 2).sum(axis=1))
  bound = ifft_cases.higham_bound(T)
  print('T %d: max e %.3g (normal deviates %.3g, one-hot bins %.3g), Higham '
        'bound %.3g' % (T, e.max(), e[:-6].max(), e[-6:].max(), bound))
  assert (e <= bound).all(), (T, e.max(), bound)
