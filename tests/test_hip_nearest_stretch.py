"""GPU tests of cg_nearest_stretch (csrc/nearest_stretch.hip: squared distances
from query trials to every stretch of a recording as a float64 MFMA product
against the recording itself, K split over workgroups, ordered sums and
minima) on the cases of nearest_stretch_cases.py -- every case held to the
direct-form statement by nearest_stretch_cases.check: the derived bar
4 K 2^-53 (|q_n|^2 + W_j), equal bits on integer data --, of its wrappers in
signals_metrics, and of compute_metrics.py --novelty_metrics on both devices.

With NEAREST_STRETCH_PARITY set to a file name, the largest err / bar of every
case is appended to it (profiles/nearest_stretch_parity.txt holds one run on an
MI355X)."""
import os

import numpy as np
import pytest
import torch

import compute_metrics as cm
import nearest_stretch_cases as NC
from calciumgan_amd import _lib
from calciumgan_amd.gan.utils import signals_metrics as sm

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 1024      # elements of the sentinel on either side of a buffer
SENTINEL = -7.0
INT_SENTINEL = -7


def _queries(Q, layout):
  """The queries on the device in the given memory layout: an (N, L, C) view."""
  N, L, C = Q.shape
  t = torch.from_numpy(np.array(Q, dtype=np.float32)).to(DEV)
  if layout == 'padded':
    buf = torch.full((N, L, C + 5), float('nan'), device=DEV)
    buf[:, :, :C] = t
    view = buf[:, :, :C]
    assert view.stride() == (L * (C + 5), C + 5, 1)
    return view
  if layout == 'permuted':
    view = t.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert view.stride() == (C * L, 1, L)
    return view
  assert layout == 'contig' and t.is_contiguous()
  return t


def _recording(R, layout):
  """The recording on the device: a (T_raw, C) view."""
  T, C = R.shape
  t = torch.from_numpy(np.array(R, dtype=np.float32)).to(DEV)
  if layout == 'padded':
    buf = torch.full((T, C + 3), float('nan'), device=DEV)
    buf[:, :C] = t
    view = buf[:, :C]
    assert view.stride() == (C + 3, 1)
    return view
  if layout == 'permuted':
    view = t.t().contiguous().t()
    assert view.stride() == (1, T)
    return view
  assert layout == 'contig' and t.is_contiguous()
  return t


def _guarded(n, dtype=torch.float64, fill=SENTINEL):
  buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=DEV)
  return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, fill=SENTINEL):
  return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def _launch(q, raw, step, exclude=None, exclude_len=0, profile=True):
  """The C entry with sentinel-filled, guarded outputs and workspace; returns
  host (d2 or None, nearest, index)."""
  N, L, C = q.shape
  T_raw = raw.shape[0]
  S = NC.offsets(T_raw, L, step)
  nbytes = _lib.load().cg_nearest_stretch_ws_bytes(N, L, C, T_raw, step)
  assert nbytes == 8 * NC.ws_doubles(N, L, C, T_raw, step)
  dbuf, d2 = _guarded(N * S)
  nbuf, nearest = _guarded(N)
  ibuf, index = _guarded(N, torch.int32, INT_SENTINEL)
  wbuf, ws = _guarded(nbytes // 8)
  ex = None
  if exclude is not None:
    ex = torch.from_numpy(np.array(exclude, dtype=np.int32)).to(DEV)
  _lib.call('cg_nearest_stretch', q, N, L, C, q.stride(0), q.stride(1),
            q.stride(2), raw, T_raw, raw.stride(0), raw.stride(1), step, ex,
            exclude_len, d2 if profile else None, nearest, index, ws,
            _lib.stream())
  torch.cuda.synchronize()
  assert _guards_intact(dbuf) and _guards_intact(nbuf) and _guards_intact(wbuf)
  assert _guards_intact(ibuf, INT_SENTINEL)
  # every element of d2 / nearest / index is written (or d2 not at all)
  assert not bool((nearest == SENTINEL).any())
  assert not bool((index == INT_SENTINEL).any())
  if profile:
    assert not bool((d2 == SENTINEL).any())
  else:
    assert bool((d2 == SENTINEL).all())
  return (d2.view(N, S).cpu().numpy() if profile else None,
          nearest.cpu().numpy(), index.cpu().numpy())


def _case_tensors(name):
  c = NC.case(name)
  return (c, _queries(c['Q'], c['q_layout']), _recording(c['R'], c['r_layout']))


def _record(name, worst):
  path = os.environ.get('NEAREST_STRETCH_PARITY')
  if path:
    with open(path, 'a') as f:
      f.write('%-40s N L C T_raw step = %-24s err / bar %.3e\n' % (
          name, ' '.join(map(str, NC.shape(name))), worst))


@pytest.mark.parametrize('name', NC.CASES)
def test_against_the_statement(name):
  c, q, raw = _case_tensors(name)
  args = (q, raw, c['step'], c['exclude'], c['exclude_len'])
  d2, nearest, index = _launch(*args)
  worst = NC.check(d2, nearest, index, name)
  print(name, 'err / bar', worst)
  _record(name, worst)
  # d2 = NULL: the same nearest / index bits; two calls: the same bits
  _, n2, i2 = _launch(*args, profile=False)
  assert n2.tobytes() == nearest.tobytes() and i2.tobytes() == index.tobytes()
  again = _launch(*args)
  for a, b in zip(again, (d2, nearest, index)):
    assert a.tobytes() == b.tobytes()
  # the wrapper holds the same bits
  dev = sm.nearest_stretch_device(*args, return_profile=True)
  assert all(t.is_cuda and t.is_contiguous() for t in dev)
  assert (dev[0].dtype, dev[1].dtype, dev[2].dtype) == (
      torch.float64, torch.int32, torch.float64)
  for a, b in zip(dev, (nearest, index, d2)):
    assert a.cpu().numpy().tobytes() == b.tobytes()
  pair = sm.nearest_stretch_device(*args)
  assert len(pair) == 2 and pair[0].cpu().numpy().tobytes() == nearest.tobytes()


@pytest.mark.parametrize('name', ['n17_s71_l64_c102_step2', 'exact_unstaged',
                                  'exact_l512_c102_step2'])
def test_the_f16_library_holds_the_same_kernel(name):
  c, q, raw = _case_tensors(name)
  want = _launch(q, raw, c['step'])
  _lib.use('f16')
  try:
    got = _launch(q, raw, c['step'])
  finally:
    _lib.use('bf16')
  for a, b in zip(got, want):
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', ['n17_s64_k15_step2', 'n17_s71_l64_c102_step2',
                                  'n4_s70_l8_c73_step4_unstaged'])
def test_non_finite_samples_spoil_only_their_own_entries(name):
  """A NaN in one query and an Inf in another, a NaN in one row of the
  recording and an Inf in another: the two queries' rows and the offsets whose
  stretch covers either row are NaN (nearest NaN / -1 for the two queries),
  and every other d2 keeps the bits of the clean run."""
  c = NC.case(name)
  N, L, C = c['Q'].shape
  step, T_raw = c['step'], c['R'].shape[0]
  clean = _launch(_queries(c['Q'], 'contig'), _recording(c['R'], 'contig'), step)
  Q, R = np.array(c['Q']), np.array(c['R'])
  Q[1, L // 2, C - 1] = np.nan
  Q[N - 1, 0, 0] = -np.inf
  rows = (L + 3, (NC.offsets(T_raw, L, step) - 1) * step + L - 1)
  R[rows[0], C // 2] = np.nan
  R[rows[1], 0] = np.inf
  d2, nearest, index = _launch(_queries(Q, 'contig'), _recording(R, 'contig'),
                               step)
  s = np.arange(d2.shape[1]) * step
  covered = np.zeros(d2.shape[1], bool)
  for row in rows:
    covered |= (s <= row) & (row < s + L)
  assert 0 < covered.sum() < d2.shape[1]
  spoiled = np.zeros(d2.shape, bool)
  spoiled[[1, N - 1]] = True
  spoiled[:, covered] = True
  assert np.isnan(d2[spoiled]).all()
  assert d2[~spoiled].tobytes() == clean[0][~spoiled].tobytes()
  assert np.isnan(nearest[[1, N - 1]]).all() and (index[[1, N - 1]] == -1).all()
  rest = [n for n in range(N) if n not in (1, N - 1)]
  want = np.where(spoiled, np.inf, clean[0])[rest]
  assert (index[rest] == want.argmin(axis=1)).all()
  assert nearest[rest].tobytes() == want.min(axis=1).tobytes()
  # the statement says the same
  ref = NC.statement(dict(c, Q=Q, R=R))
  assert (np.isnan(ref['d2']) == spoiled).all()
  NC.check(d2, nearest, index, dict(c, Q=Q, R=R), ref=ref)


def test_refused_arguments_return_einval_and_write_nothing():
  lib = _lib.load()
  q = torch.zeros((2, 5, 3), device=DEV)
  raw = torch.zeros((50, 3), device=DEV)
  n = 8 * 1024
  d2 = torch.full((n,), SENTINEL, dtype=torch.float64, device=DEV)
  nearest = torch.full((n,), SENTINEL, dtype=torch.float64, device=DEV)
  index = torch.full((n,), INT_SENTINEL, dtype=torch.int32, device=DEV)
  ws = torch.full((n,), SENTINEL, dtype=torch.float64, device=DEV)

  def call(q=q, raw=raw, nearest=nearest, index=index, ws=ws, N=2, L=5, C=3,
           T_raw=50, step=1, exclude_len=0):
    return lib.cg_nearest_stretch(q, N, L, C, L * C, C, 1, raw, T_raw, C, 1,
                                  step, None, exclude_len, d2, nearest, index,
                                  ws, _lib.stream())

  for kw in (dict(q=None), dict(raw=None), dict(nearest=None), dict(index=None),
             dict(ws=None), dict(N=0), dict(L=0), dict(C=0), dict(step=0),
             dict(N=-1), dict(T_raw=4), dict(exclude_len=-1), dict(N=65536),
             dict(step=(1 << 20) + 1), dict(T_raw=(1 << 31) - 64)):
    assert call(**kw) == _lib.CG_EINVAL, kw
  unaligned = torch.zeros(8 * n + 8, dtype=torch.uint8, device=DEV)[4:]
  assert call(ws=unaligned.data_ptr()) == _lib.CG_EINVAL
  torch.cuda.synchronize()
  for t, fill in ((d2, SENTINEL), (nearest, SENTINEL), (ws, SENTINEL),
                  (index, INT_SENTINEL)):
    assert bool((t == fill).all())
  assert call() == 0
  torch.cuda.synchronize()
  S = 46
  assert not bool((d2[:2 * S] == SENTINEL).any())
  assert bool((d2[2 * S:] == SENTINEL).all())
  assert not bool((nearest[:2] == SENTINEL).any())
  assert bool((nearest[2:] == SENTINEL).all())
  assert bool((index[2:] == INT_SENTINEL).all())
  assert index[:2].tolist() == [0, 0] and nearest[:2].tolist() == [0.0, 0.0]


def test_the_wrappers_with_grouping():
  name = 'exclude_bands_at_both_ends'
  c, q, raw = _case_tensors(name)
  one = sm.nearest_stretch_device(q, raw, c['step'], c['exclude'],
                                  c['exclude_len'])
  NC.check(None, one[0].cpu().numpy(), one[1].cpu().numpy(), name)
  L, C = q.shape[1:]
  for group_bytes in (256 << 20, 4 * L * C * 4, 1):   # one group; of 4 + 2; of 1
    for exclude in (c['exclude'], torch.from_numpy(np.array(c['exclude'])).to(DEV),
                    c['exclude'].tolist()):
      got = sm.nearest_stretch_totals_device(
          q, raw, c['step'], exclude, c['exclude_len'], group_bytes=group_bytes)
      assert got[0].is_cuda and got[0].dtype == torch.float64
      assert got[1].is_cuda and got[1].dtype == torch.int32
      assert got[0].shape == (6,) and got[1].shape == (6,)
      assert got[0].cpu().numpy().tobytes() == one[0].cpu().numpy().tobytes()
      assert torch.equal(got[1], one[1])
  # without exclusion, on a case of two query tiles
  c, q, raw = _case_tensors('n130_s257_k15_step2')
  one = sm.nearest_stretch_device(q, raw, c['step'])
  got = sm.nearest_stretch_totals_device(q, raw, c['step'],
                                         group_bytes=50 * 15 * 4)
  assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1])
  host = torch.from_numpy(np.array(c['Q']))
  for bad in ((host, raw), (q.double(), raw), (q[0], raw), (q, raw[:, :2]),
              (q, raw[:3])):
    with pytest.raises(ValueError):
      sm.nearest_stretch_device(*bad)
  for kw in (dict(step=0), dict(exclude_len=-1), dict(exclude=[1, 2])):
    with pytest.raises(ValueError):
      sm.nearest_stretch_device(q, raw, **kw)


def test_compute_metrics_novelty_flag_on_both_devices(tmp_path):
  """rms = sqrt(nearest / K): a nearest within bar of the host's moves rms by at
  most bar / (2 K rms) (the square root's slope; rms is far from 0 on both
  sides here), and both devices' nearest lie within bar of the statement, so
  the two rms figures are within 2 bar / (2 K rms) of each other -- bar = 4 K
  2^-53 (|q|^2 + W) at its largest over the trials and offsets, computed here
  from the run's own data.  The minima of either side are separated by far more
  than that, so the counts and fractions are equal."""
  reports = {}
  for device in ('cpu', 'gpu'):
    os.makedirs(tmp_path / device)
    fake, rec, gen = NC.run_dir(tmp_path / device, kind='copies')
    hp = cm.build_parser().parse_args(
        ['--output_dir', str(tmp_path / device), '--num_processors', '1',
         '--verbose', '0', '--device', device, '--batch_trials', '5',
         '--novelty_metrics'])
    reports[device] = cm.main(hp)[0]
  cpu, gpu = reports['cpu']['novelty'], reports['gpu']['novelty']
  print('novelty cpu:', cpu)
  print('novelty gpu:', gpu)
  assert set(reports['cpu']) == set(reports['gpu'])
  assert set(cpu) == set(gpu)
  raw, (L, C) = rec['raw'], gen.shape[1:]
  K = L * C
  r64 = raw.astype(np.float64)
  w_max = max((r64[s:s + L] ** 2).sum() for s in range(0, len(raw) - L + 1, 2))
  q_max = max(w_max, (gen.astype(np.float64) ** 2).sum(axis=(1, 2)).max())
  bar = 4 * K * NC.U * (q_max + w_max)
  for side in ('recorded', 'generated'):
    for a, b in zip(cpu['nearest_rms'][side], gpu['nearest_rms'][side]):
      assert a > 0.005 and abs(a - b) <= 2 * bar / (2 * K * min(a, b)), side
  # the ratio of the medians: |a / b - a' / b'| <= (|a - a'| + (a / b) |b - b'|) / b'
  slack = lambda rms: 2 * bar / (2 * K * rms)
  med_r, med_g = cpu['nearest_rms']['recorded'][1], cpu['nearest_rms']['generated'][1]
  assert abs(cpu['nearest_rms_ratio'] - gpu['nearest_rms_ratio']) <= (
      slack(med_g) + cpu['nearest_rms_ratio'] * slack(med_r)) / (
          med_r - slack(med_r))
  for key in ('copied_fraction', 'below_recorded_median', 'distinct_stretches',
              'step', 'offsets', 'num_trials', 'undefined'):
    assert cpu[key] == gpu[key], key
  assert gpu['copied_fraction'] == 1.0 and gpu['num_trials'] == [12, 12]
  # without the flag the device report has no such key
  plain = cm.build_parser().parse_args(
      ['--output_dir', str(tmp_path / 'gpu'), '--num_processors', '1',
       '--verbose', '0', '--device', 'gpu', '--batch_trials', '5'])
  assert not hasattr(plain, 'novelty_metrics')
  assert 'novelty' not in cm.main(plain)[0]
