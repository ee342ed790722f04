"""GPU tests of cg_window_batch (csrc/windows.hip: one batch of windows cut out
of the resident recording, optionally as spectra, normalised on the way) on the
cases of window_cases.py -- every case one launch on valid input; the plain
gather held to the numpy statement byte for byte, the FFT to the float64
transform of the float32 windows by the two conditions of
window_cases.check_accuracy -- of its wrapper dataset_helper.window_batch_device,
of RecordingDataset on the device, and of main.py on a recording directory
against main.py on the materialised directory of the same recording.

Measured on one MI355X (max over the traces of each L's cases, e against the
float64 transform, e_ref the same for single-precision pocketfft): DESIGN.md
"Recording datasets"."""
import json
import os

import numpy as np
import pytest
import torch

import main as cli
import oracle as O
import window_cases as WC
from calciumgan_amd import _lib
from calciumgan_amd.data import dg, recording
from calciumgan_amd.gan.utils import dataset_helper, h5_helper

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _raw(name):
  """The case's recording on the device in the case's memory layout: a (T, C)
  view."""
  c = WC.case(name)
  T, C = c['raw'].shape
  t = torch.from_numpy(np.array(c['raw'])).to(DEV)
  lin = c['lin']
  if lin in ('padded', 'padded4'):
    pitch = C + (3 if lin == 'padded' else 4)
    buf = torch.full((T, pitch), float('nan'), device=DEV)
    buf[:, :C] = t
    view = buf[:, :C]
    assert view.stride() == (pitch, 1)
    return view
  if lin == 'transposed':
    view = t.t().contiguous().t()
    assert view.stride() == (1, T)
    return view
  assert lin == 'contig' and t.is_contiguous()
  return t


def _launch(name, raw, fft, sub=None, div=None):
  """The C entry into the case's output layout; returns (y view, whole
  buffer)."""
  c = WC.case(name)
  sub = c['sub'] if sub is None else sub
  div = c['div'] if div is None else div
  starts = torch.from_numpy(np.array(c['starts'])).to(DEV)
  B, L, C = len(c['starts']), c['L'], c['C']
  ch = 2 * C if fft else C
  pitch = ch + {'contig': 0, 'padded': 3, 'padded4': 4}[c['lout']]
  buf = torch.full((B, L, pitch), float('nan'), device=DEV)
  y = buf[:, :, :ch]
  _lib.call('cg_window_batch', raw, raw.shape[0], C, raw.stride(0),
            raw.stride(1), starts, B, L, 1 if fft else 0, sub, div, y,
            y.stride(0), y.stride(1), y.stride(2), _lib.stream())
  torch.cuda.synchronize()
  return y, buf


def _wrapper(name, raw, fft, sub, div):
  c = WC.case(name)
  starts = torch.from_numpy(np.array(c['starts'])).to(DEV)
  dev = dataset_helper.window_batch_device(raw, starts, c['L'], fft=fft, sub=sub,
                                           div=div)
  assert dev.is_cuda and dev.dtype == torch.float32 and dev.is_contiguous()
  return dev.cpu().numpy()


@pytest.mark.parametrize('name', WC.CASES)
def test_the_plain_gather_is_the_statement_byte_for_byte(name):
  c = WC.case(name)
  raw = _raw(name)
  y, buf = _launch(name, raw, False)
  got = y.cpu().numpy()
  want = dataset_helper.window_batch(c['raw'], c['starts'], c['L'], sub=c['sub'],
                                     div=c['div'])
  assert got.shape == want.shape and got.tobytes() == want.tobytes()
  if c['lout'] != 'contig':
    assert bool(torch.isnan(buf[:, :, c['C']:]).all())  # the padding is untouched
  # a second launch gives the same bits
  assert _launch(name, raw, False)[0].cpu().numpy().tobytes() == got.tobytes()
  # the wrapper: a contiguous (B, L, C) device tensor with the same bits
  assert _wrapper(name, raw, False, c['sub'], c['div']).tobytes() == got.tobytes()


@pytest.mark.parametrize('name', WC.FFT_CASES)
def test_the_spectra_against_the_float64_transform(name):
  c = WC.case(name)
  C = c['C']
  raw = _raw(name)
  y, buf = _launch(name, raw, True, sub=0.0, div=1.0)
  got = y.cpu().numpy()
  assert got.shape == (len(c['starts']), c['L'], 2 * C)
  assert not np.isnan(got).any()
  if c['lout'] != 'contig':
    assert bool(torch.isnan(buf[:, :, 2 * C:]).all())
  WC.check_accuracy(got, name)
  if name == 'l256_c4_zero_trace':
    assert not got[:, :, 2].any() and not got[:, :, C + 2].any()
    assert got[:, :, 1].any()
  # determinism: a second launch gives the same bits
  assert _launch(name, raw, True, sub=0.0, div=1.0)[0].cpu().numpy().tobytes() \
      == got.tobytes()
  assert _wrapper(name, raw, True, 0.0, 1.0).tobytes() == got.tobytes()
  if (c['sub'], c['div']) != (0.0, 1.0):
    # normalised: (y0 - sub) / div of the device's own un-normalised output
    norm = _launch(name, raw, True)[0].cpu().numpy()
    want = (got - np.float32(c['sub'])) / np.float32(c['div'])
    assert norm.tobytes() == want.tobytes()
    assert _wrapper(name, raw, True, c['sub'], c['div']).tobytes() == \
        norm.tobytes()


@pytest.mark.parametrize('name', ['l128_c17_normal', 'l512_c17_dg',
                                  'l1024_c17_dg', 'l4096_c3_dg'])
def test_the_f16_library_holds_the_same_kernel(name):
  """The float32 FFT kernel of the other precision build, at the lengths the
  case table gained: under both conditions, and the bf16 build's bits."""
  raw = _raw(name)
  want = _launch(name, raw, True, sub=0.0, div=1.0)[0].cpu().numpy()
  _lib.use('f16')
  try:
    got = _launch(name, raw, True, sub=0.0, div=1.0)[0].cpu().numpy()
  finally:
    _lib.use('bf16')
  WC.check_accuracy(got, name)
  assert got.tobytes() == want.tobytes()


def test_invalid_arguments_are_refused_and_nothing_is_written():
  raw = torch.zeros((200, 3), device=DEV)
  starts = torch.zeros(2, dtype=torch.int32, device=DEV)
  y = torch.full((2, 96, 6), -7.0, device=DEV)
  lib = _lib.load()

  def call(raw=raw, starts=starts, y=y, T=200, C=3, B=2, L=64, fft=0, div=1.0):
    ch = 2 * C if fft else C
    return lib.cg_window_batch(raw, T, C, 3, 1, starts, B, L, fft, 0.0, div, y,
                               L * ch, ch, 1, _lib.stream())

  E = _lib.CG_EINVAL
  for kw in (dict(raw=None), dict(starts=None), dict(y=None), dict(T=0),
             dict(C=0), dict(B=0), dict(B=-2), dict(L=0), dict(div=0.0),
             dict(fft=1, L=96), dict(fft=1, L=16), dict(fft=1, L=16384),
             dict(fft=1, div=0.0)):
    assert call(**kw) == E, kw
  torch.cuda.synchronize()
  assert bool((y == -7.0).all())


def test_a_refused_length_takes_the_host_statement():
  rng = np.random.RandomState(5)
  raw = rng.standard_normal((150, 3)).astype(np.float32)
  starts = np.array([0, 7, 60, -2], np.int32)
  d_raw, d_starts = torch.from_numpy(raw).to(DEV), torch.from_numpy(starts).to(DEV)
  got = dataset_helper.window_batch_device(d_raw, d_starts, 96, fft=True,
                                           sub=-0.5, div=2.5)
  assert got.is_cuda and tuple(got.shape) == (4, 96, 6)
  want = dataset_helper.window_batch(raw, starts, 96, True, -0.5, 2.5)
  assert got.cpu().numpy().tobytes() == want.tobytes()
  # the plain gather takes any length on the device
  got = dataset_helper.window_batch_device(d_raw, d_starts, 96)
  assert got.cpu().numpy().tobytes() == \
      dataset_helper.window_batch(raw, starts, 96).tobytes()
  # into a given any-stride output
  buf = torch.full((4, 96, 5), float('nan'), device=DEV)
  out = dataset_helper.window_batch_device(d_raw, d_starts, 96, out=buf[:, :, :3])
  assert out.data_ptr() == buf.data_ptr()
  assert out.cpu().numpy().tobytes() == got.cpu().numpy().tobytes()
  assert bool(torch.isnan(buf[:, :, 3:]).all())
  # the wrapper refuses host arrays, other dtypes and ranks, a wrong output
  for bad in ((raw, d_starts), (d_raw, starts), (d_raw.double(), d_starts),
              (d_raw, d_starts.long()), (d_raw[0], d_starts)):
    with pytest.raises(ValueError):
      dataset_helper.window_batch_device(bad[0], bad[1], 32)
  with pytest.raises(ValueError):
    dataset_helper.window_batch_device(d_raw, d_starts, 32, out=buf)
  with pytest.raises(ValueError):
    dataset_helper.window_batch_device(d_raw, d_starts, 32, div=0.0)


# -- RecordingDataset on the device -------------------------------------------------
N, L0, C0 = 70, 256, 8


def _dg_recording(fft, device=None, validation_size=6):
  signals, spikes, _ = dg.make_recording(C0, L0 + 2 * N, 1234, 0.05)
  return recording.build(signals, spikes, L0, stride=2, fft=fft,
                         validation_size=validation_size, max_segments=N,
                         device=device)


@pytest.mark.parametrize('fft', [False, True])
def test_recording_dataset_on_the_device(fft):
  rec = _dg_recording(fft, device=DEV if fft else None, validation_size=5)
  assert rec['info']['minmax_by'] == ('device' if fft else 'host')
  sub, div = recording.normalisation(rec['info'])
  ch = 2 * C0 if fft else C0

  def dataset():
    return dataset_helper.RecordingDataset(
        rec['raw'], rec['spikes'], rec['train_starts'], L0, 8, shuffle=True,
        fft=fft, sub=sub, div=div)

  host, dev = dataset(), dataset().to_device(DEV)
  d_raw = torch.from_numpy(rec['raw']).to(DEV)
  gan_buffer = torch.full((8, L0, ch), float('nan'), device=DEV)
  asked = []

  def batch_buffer(n):  # GAN.batch_buffer's contract: full-size batches only
    asked.append(n)
    return gan_buffer if n == 8 else None

  dev.gather_into = batch_buffer
  sizes = []
  for (hs, hk), (ds, dk) in zip(host, dev):
    sizes.append(len(hs))
    assert ds.is_cuda and tuple(ds.shape) == hs.shape
    # the same windows in the same order as the host iterator ...
    assert np.array_equal(np.asarray(dk), np.asarray(hk))
    st = dk.starts
    want = dataset_helper.window_batch_device(
        d_raw, torch.from_numpy(st.astype(np.int32)).to(DEV), L0, fft, sub, div)
    assert torch.equal(ds, want)
    if not fft:
      assert ds.cpu().numpy().tobytes() == hs.tobytes()
    # ... and a full-size batch lands in the bound buffer
    assert (ds.data_ptr() == gan_buffer.data_ptr()) == (len(hs) == 8)
  assert sizes == [8] * 8 + [1] and asked == sizes
  if fft:
    # normalised by the device's own min / max: the whole set lies in [0, 1]
    sig, _ = recording.materialize(rec, device=DEV)
    assert sig.min() == 0.0 and sig.max() == 1.0


def test_gather_into_is_gan_batch_buffer():
  from calciumgan_amd.gan.algorithms import get_algorithm
  from calciumgan_amd.gan.models import get_models
  rec = _dg_recording(False)
  sub, div = recording.normalisation(rec['info'])
  hp = O.make_hparams(L0, C0, 8, m=2)
  hp.verbose = 0
  gen, dis = get_models(hp, None)
  gan = get_algorithm(hp, gen, dis, None)
  ds = dataset_helper.RecordingDataset(
      rec['raw'], rec['spikes'], rec['train_starts'], L0, 8, shuffle=True,
      sub=sub, div=div).to_device(gan.device)
  ds.gather_into = gan.batch_buffer
  signal, spikes = next(iter(ds))
  assert signal.data_ptr() == gan.batch_buffer(8).data_ptr()
  want = dataset_helper.window_batch(rec['raw'], spikes.starts, L0, sub=sub,
                                     div=div)
  assert signal.cpu().numpy().tobytes() == want.tobytes()
  out = gan.train(signal)
  assert np.isfinite(float(out[0])) and np.isfinite(float(out[1]))


# -- main.py on a recording directory (shapes of tests/test_main_e2e.py) ------------
def _scalars(path):
  """Every logged scalar but the timings (elapse, elapse/*, and
  samples_per_sec, which is train_size over an elapsed time)."""
  return [(r['tag'], r['step'], r['value'])
          for r in (json.loads(l) for l in open(path))
          if not r['tag'].startswith('elapse') and r['tag'] != 'samples_per_sec']


def _h5_bytes(path):
  """The bytes of an h5_helper file: of the file, or (without h5py) of every
  chunk file in the directory that stands for it."""
  if os.path.isdir(path):
    return {f: open(os.path.join(path, f), 'rb').read()
            for f in sorted(os.listdir(path))}
  return open(path, 'rb').read()


def _run(input_dir, output_dir):
  a = cli.build_parser().parse_args([
      '--input_dir', input_dir, '--output_dir', output_dir, '--model',
      'calciumgan', '--algorithm', 'wgan-gp', '--batch_size', '8', '--num_units',
      '8', '--m', '2', '--layer_norm', '--epochs', '1', '--save_generated',
      'last', '--spike_metrics', '--verbose', '0'])
  a.global_step = 0
  a.surrogate_ds = False
  cli.main(a)
  return a


def _both_runs(tmp_path, fft):
  device = DEV if fft else None
  rec = _dg_recording(fft, device=device)
  rdir, adir = str(tmp_path / 'rec'), str(tmp_path / 'arrays')
  recording.write(rdir, rec)
  sig, spk = recording.materialize(rec, device=device)
  info = {k: v for k, v in rec['info'].items()
          if k not in ('recording', 'minmax_by')}
  dataset_helper.write_dataset(adir, sig, spk, info, validation_size=6)
  r_out, a_out = str(tmp_path / 'run_rec'), str(tmp_path / 'run_arrays')
  hr, ha = _run(rdir, r_out), _run(adir, a_out)
  assert hr.fft is fft and ha.fft is fft and hr.num_neurons == C0
  assert hr.global_step == ha.global_step == 8
  for sub in ('', 'validation'):
    r = _scalars(os.path.join(r_out, sub, 'scalars.jsonl'))
    a = _scalars(os.path.join(a_out, sub, 'scalars.jsonl'))
    assert r and r == a, sub
  gen = [_h5_bytes(os.path.join(o, 'generated', 'epoch000_signals.h5'))
         for o in (r_out, a_out)]
  assert gen[0] and gen[0] == gen[1]
  return rec, r_out, a_out


def test_main_on_a_recording_directory_is_main_on_its_windows(tmp_path):
  rec, r_out, a_out = _both_runs(tmp_path, False)
  val = [_h5_bytes(os.path.join(o, 'generated', 'validation.h5'))
         for o in (r_out, a_out)]
  assert val[0] and val[0] == val[1]
  va = {t for t, _, _ in _scalars(os.path.join(r_out, 'validation',
                                               'scalars.jsonl'))}
  assert {'spike_metrics/firing_rate_mae', 'signals_metrics/std'} <= va


def test_main_on_an_fft_recording_directory_and_compute_metrics(tmp_path):
  import compute_metrics as cm
  from ifft_cases import higham_bound
  rec, r_out, a_out = _both_runs(tmp_path, True)
  # validation.h5: the exact raw windows here, ifft(fft) of them there
  r_val, a_val = (h5_helper.get(os.path.join(o, 'generated', 'validation.h5'),
                                'signals') for o in (r_out, a_out))
  want = dataset_helper.window_batch(rec['raw'], rec['validation_starts'], L0)
  assert r_val.shape == (6, L0, C0) and r_val.tobytes() == want.tobytes()
  norm = np.sqrt((r_val.astype(np.float64) ** 2).sum(1))
  err = np.sqrt(((a_val.astype(np.float64) - r_val) ** 2).sum(1))
  print('validation.h5: max relative error per trace %.3g, bar %.3g' % (
      (err / norm).max(), 2 * higham_bound(L0)))
  assert (err <= 2 * higham_bound(L0) * norm).all()
  for o in (r_out, a_out):
    spikes = h5_helper.get(os.path.join(o, 'generated', 'validation.h5'), 'spikes')
    assert spikes.shape == (6, L0, C0)
  # compute_metrics.py runs on the recording run's output
  mhp = cm.build_parser().parse_args(['--output_dir', r_out, '--num_processors',
                                      '1', '--verbose', '0'])
  rep = cm.main(mhp)
  assert list(rep) == [0]
  saved = json.load(open(os.path.join(r_out, 'spike_metrics.json')))
  for k in ('firing_rate_kl', 'correlation_kl', 'van_rossum_kl'):
    assert np.isfinite(saved['0'][k]['mean']), (k, saved['0'][k])
