"""GPU tests of cg_spike_intervals (csrc/spike_intervals.hip: the inter-spike
intervals of packed spike trains, a wave a trial in chunks of 64 words) against
its numpy statement spike_metrics.interval_counts -- equality of integers
throughout -- and of compute_metrics.py --interval_metrics on both devices.

The kernel's paths: one word a trial and two; below, at and past one 64-word
chunk (63, 64, 65) and a third chunk (129), the carry between them; lanes and
chunks empty between two spikes; one trial, fewer than the four waves of a
workgroup and more; the trials split over workgroups with the merge launch.
Every output sits between guard elements and the workspace is poisoned."""
import os

import numpy as np
import pytest
import torch

import compute_metrics as cm
import interval_cases as IC
from calciumgan_amd import _lib
from calciumgan_amd.gan.utils import spike_metrics as sm

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = -7
GUARD = 1024   # elements of SENTINEL on either side of an output
PAD_WORD = 0x55555555   # what the words between the rows hold


def _guarded(n, dtype=torch.int32):
  buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
  return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
  return bool((buf[:GUARD] == SENTINEL).all()) and bool(
      (buf[-GUARD:] == SENTINEL).all())


def _check(got, want):
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape, (got.shape, want.shape)
  diff = got != want
  print('%d of %d elements differ' % (int(diff.sum()), diff.size))
  assert not diff.any(), [(tuple(ix), int(got[tuple(ix)]), int(want[tuple(ix)]))
                          for ix in np.argwhere(diff)[:8]]


def _count(w, trials, max_isi=240, extra=0, poison=0x7f7f7f7f):
  """cg_spike_intervals of host uint32 (C, trials wpt) words with every output
  between guards: (hist, moments, counts) as host arrays."""
  C, W = w.shape
  wpt = W // trials
  stride = W + extra
  t = torch.full((C, stride), PAD_WORD, dtype=torch.int32, device=DEV)
  t[:, :W] = torch.from_numpy(w.view(np.int32).copy()).to(DEV)
  need = _lib.load().cg_spike_intervals_ws_bytes(C, trials, wpt, max_isi)
  assert need >= 16
  # (the workspace's contents do not matter: poison)
  ws = torch.full((need // 4 + 4,), poison, dtype=torch.int32, device=DEV)
  H = max_isi + 1
  hbuf, hist = _guarded(C * H)
  mbuf, moments = _guarded(C * 6, torch.int64)
  cbuf, counts = _guarded(trials * C)
  _lib.call('cg_spike_intervals', t, C, trials, wpt, stride, max_isi, hist,
            moments, counts, ws, _lib.stream())
  torch.cuda.synchronize()
  assert _guards_intact(hbuf) and _guards_intact(mbuf) and _guards_intact(cbuf)
  # the extra words of a row are read by nobody and stay what they were
  assert bool((t[:, W:] == PAD_WORD).all())
  assert torch.equal(t[:, :W].cpu(), torch.from_numpy(w.view(np.int32).copy()))
  return (hist.view(C, H).cpu().numpy(), moments.view(C, 6).cpu().numpy(),
          counts.view(trials, C).cpu().numpy())


def _compare(C, trials, wpt, kind='dense', max_isi=240, extra=0):
  got = _count(IC.words(C, trials, wpt, kind), trials, max_isi, extra)
  for g, w in zip(got, IC.word_counts(C, trials, wpt, kind, max_isi)):
    _check(g, w)
  return got


def _shapes():
  for C in IC.WORD_NEURONS:
    for wpt in IC.WORDS_PER_TRIAL:
      if C == 512 and wpt > 2:
        continue
      yield C, wpt


@pytest.mark.parametrize('shape', list(_shapes()),
                         ids=lambda s: 'x'.join(map(str, s)))
def test_counts_equal_the_statement(shape):
  C, wpt = shape
  # every trial count at the small shapes; the larger ones with seven trials
  for trials in (IC.WORD_TRIALS if C * wpt <= 17 * 129 else [7]):
    _compare(C, trials, wpt, 'dense')
    _compare(C, trials, wpt, 'sparse', extra=5)
    _compare(C, trials, wpt, 'rare', extra=1)


@pytest.mark.parametrize('wpt', [1, 2, 64, 65, 129])
def test_all_ones_all_zeros_and_the_bits_at_the_word_edges(wpt):
  for C, trials in ((1, 1), (3, 7), (17, 2)):
    hist, moments, counts = _compare(C, trials, wpt, 'ones')
    assert (hist[:, 0] == trials * (32 * wpt - 1)).all()
    assert not hist[:, 1:].any()
    assert (counts == 32 * wpt).all()
    for x in _compare(C, trials, wpt, 'zeros', extra=3):
      assert not x.any()
    # bits 0 and 31 of every word: 31 inside a word, 1 across a boundary
    hist, moments, counts = _compare(C, trials, wpt, 'edges')
    assert (hist[:, 30] == trials * wpt).all()
    assert (hist[:, 0] == trials * (wpt - 1)).all()
    assert (hist.sum(1) == trials * (2 * wpt - 1)).all()
    assert (moments[:, 5] == trials * (2 * wpt - 2) * 31).all()


@pytest.mark.parametrize('wpt', [1, 2, 64, 65])
def test_nothing_pairs_across_trials(wpt):
  """The last bit of a trial and the first bit of the next are neighbours in
  memory and one spike each of two trains: no interval."""
  for C, trials in ((1, 2), (3, 7), (17, 6)):
    hist, moments, counts = _compare(C, trials, wpt, 'boundary')
    assert not hist.any() and not moments[:, 1:].any()
    assert (moments[:, 0] == trials).all() and (counts == 1).all()


@pytest.mark.parametrize('wpt,at', [(1, 30), (2, 62), (64, 2046), (65, 2078),
                                    (128, 4094), (129, 4095)])
def test_frame_zero_and_the_last_frame_only(wpt, at):
  """One interval a train that spans every chunk of the trial: 32 wpt - 1
  frames.  4095 at wpt = 128 is the last bin with a length of its own at max_isi
  = 4095; 4127 at wpt = 129 lands in the overflow bin."""
  C, trials = 3, 5
  hist, moments, counts = _compare(C, trials, wpt, 'ends', max_isi=4095)
  I = 32 * wpt - 1
  assert min(I, 4096) - 1 == at
  assert (hist[:, at] == trials).all() and (hist.sum(1) == trials).all()
  assert (moments == [2 * trials, trials, trials * I, trials * I * I, 0, 0]).all()
  assert (counts == 2).all()


@pytest.mark.parametrize('max_isi', IC.MAX_ISIS)
def test_max_isi(max_isi):
  _compare(17, 7, 65, 'dense', max_isi)
  hist, _, _ = _compare(17, 7, 129, 'rare', max_isi, extra=2)
  assert hist.shape == (17, max_isi + 1)
  if max_isi <= 240:
    assert hist[:, max_isi].sum() > 0   # some interval overflows


def test_the_split_path_with_its_merge():
  C, trials, wpt = IC.SPLIT_CASE
  ws = _lib.load().cg_spike_intervals_ws_bytes
  assert ws(C, trials, wpt, 240) > ws(C, 1, wpt, 240)
  _compare(C, trials, wpt, 'dense')
  _compare(C, trials, wpt, 'sparse', extra=1)
  _compare(C, trials, wpt, 'boundary')
  # the report's neurons and frames: ten splits of four trials
  assert ws(102, 40, 64, 240) == 10 * 102 * (241 * 4 + 6 * 8)
  _compare(102, 40, 64, 'rare')


def test_two_calls_give_identical_results():
  for C, trials, wpt in ((102, 7, 65), IC.SPLIT_CASE):
    w = IC.words(C, trials, wpt)
    first = _count(w, trials)
    again = _count(w, trials, poison=-1)
    for a, b in zip(first, again):
      assert a.tobytes() == b.tobytes()
    # the wrapper
    dev = sm.DeviceWords(torch.from_numpy(w.view(np.int32).copy()).to(DEV), C, 1,
                         32 * wpt, trials)
    got = sm.interval_counts_device(dev)
    assert [g.dtype for g in got] == [torch.int32, torch.int64, torch.int32]
    for g, a in zip(got, first):
      assert g.is_cuda
      _check(g.cpu().numpy(), a)


def test_refused_arguments_leave_the_buffers_untouched():
  lib = _lib.load()
  C, trials, wpt, max_isi = 17, 3, 2, 24
  W = trials * wpt
  words = torch.full((C * W + 4,), SENTINEL, dtype=torch.int32, device=DEV)
  out = torch.full((4096,), SENTINEL, dtype=torch.int32, device=DEV)
  mom = torch.full((512,), SENTINEL, dtype=torch.int64, device=DEV)
  ws = torch.full((4096,), SENTINEL, dtype=torch.int32, device=DEV)
  h, cn, m = out[:C * (max_isi + 1)], out[1024:1024 + trials * C], mom[:C * 6]
  st = _lib.stream()

  def count(w=words, C=C, trials=trials, wpt=wpt, stride=W, max_isi=max_isi,
            h=h, m=m, cn=cn, ws=ws):
    return lib.cg_spike_intervals(w, C, trials, wpt, stride, max_isi, h, m, cn,
                                  ws, st)

  for kw in (dict(w=None), dict(ws=None), dict(h=None), dict(m=None),
             dict(cn=None), dict(w=words[1:]), dict(ws=ws[1:]),
             dict(m=mom.view(torch.int32)[1:].data_ptr()), dict(C=0),
             dict(C=4097), dict(trials=0), dict(wpt=0), dict(max_isi=0),
             dict(max_isi=4096), dict(trials=1 << 13, wpt=1 << 13,
                                      stride=1 << 40), dict(stride=W - 1)):
    assert count(**kw) == _lib.CG_EINVAL, kw
  torch.cuda.synchronize()
  for buf in (words, out, mom, ws):
    assert bool((buf == SENTINEL).all())
  x = torch.ones(2, 50, C, dtype=torch.float32, device=DEV)
  with pytest.raises(ValueError):
    sm.interval_counts_device(sm.binary_words_device(x, 12))   # bin != 1
  with pytest.raises(ValueError):
    sm.interval_counts_device(sm.binary_words_device(x, 1), 4096)
  dev = sm.binary_words_device(x, 1)
  with pytest.raises(ValueError):                              # not contiguous
    sm.interval_counts_device(sm.DeviceWords(dev.tensor[:, ::2], C, 1, 50, 1))
  # and the same call, admitted, writes: SENTINEL words are all ones but bits
  # 1 and 2
  assert count() == 0
  torch.cuda.synchronize()
  assert bool((cn == 30 * wpt).all())
  assert bool((m.view(C, 6)[:, 0] == 30 * W).all())


# -- through the wrappers, from float trials ------------------------------------------
def _through_the_wrappers(x, sp, max_isi=240):
  want = sm.interval_counts(sp, max_isi)
  got = sm.interval_counts_device(sm.binary_words_device(x, 1), max_isi)
  for g, w in zip(got, want):
    _check(g.cpu().numpy(), w)
  return want


@pytest.mark.parametrize('T', [50, 2048, 2100])
def test_float_trials_through_the_wrappers(T):
  sp = IC.trains(5, T, 7, 0.05)
  _through_the_wrappers(torch.from_numpy(sp).to(DEV), sp)
  _through_the_wrappers(torch.from_numpy(sp).to(DEV), sp, max_isi=24)
  # batches of trials joined along the words
  x = torch.from_numpy(sp).to(DEV)
  cat = sm.DeviceWords.cat([sm.binary_words_device(x[:2], 1),
                            sm.binary_words_device(x[2:], 1)])
  for g, w in zip(sm.interval_counts_device(cat), sm.interval_counts(sp)):
    _check(g.cpu().numpy(), w)


def test_strided_views_nan_and_minus_zero():
  B, T, C = 2, 50, 17
  sp = IC.trains(B, T, C, 0.5)
  buf = torch.full((B, T, 128), 7.0, dtype=torch.float32, device=DEV)
  buf[:, :, :C] = torch.from_numpy(sp).to(DEV)
  x = buf[:, :, :C]
  assert x.stride() == (T * 128, 128, 1)
  _through_the_wrappers(x, sp)
  sp = np.zeros((1, 24, 3), np.float32)
  sp[0, 1, 0] = np.nan
  sp[0, 5, 0] = 2.0
  sp[0, 2, 1] = -0.0
  sp[0, 13, 1] = -3.5
  hist, moments, counts = _through_the_wrappers(
      torch.from_numpy(sp).to(DEV), sp, max_isi=24)
  assert counts.tolist() == [[2, 1, 0]] and hist[0, 3] == 1


def test_scores_are_the_same_dict_on_both_devices():
  a = IC.gamma_trains(1, shape=(12, 600, 6))
  b = IC.bernoulli_trains(3, shape=(12, 600, 6))
  want = sm.interval_scores(IC.side(a), IC.side(b))

  def device_side(x):
    return sm.interval_counts_device(sm.binary_words_device(
        torch.from_numpy(x.astype(np.float32)).to(DEV), 1))

  got = sm.interval_scores(device_side(a), device_side(b))
  print(want)
  assert IC.same(got, want)
  assert got['num_trials'] == [12, 12]


# -- compute_metrics.py --------------------------------------------------------------
NEW_ENTRY_POINTS = {'cg_binary_words', 'cg_spike_intervals'}


def test_compute_metrics_interval_flag_on_both_devices(tmp_path, monkeypatch):
  called = []
  call = _lib.call

  def recording(name, *args):
    called.append(name)
    return call(name, *args)

  monkeypatch.setattr(_lib, 'call', recording)
  reports, plain = {}, {}
  for device in ('cpu', 'gpu'):
    os.makedirs(tmp_path / device)
    fake, real_spikes, fake_spikes = IC.run_dir(tmp_path / device)
    args = ['--output_dir', str(tmp_path / device), '--num_processors', '1',
            '--verbose', '0', '--device', device, '--batch_trials', '5']
    hp = cm.build_parser().parse_args(args)
    assert not hasattr(hp, 'interval_metrics')
    del called[:]
    plain[device] = cm.main(hp)[0]
    # without the flag none of the new entry points is launched
    assert not NEW_ENTRY_POINTS & set(called), called
    if device == 'gpu':
      assert called
    del called[:]
    reports[device] = cm.main(
        cm.build_parser().parse_args(args + ['--interval_metrics']))[0]
    if device == 'gpu':
      # three sides: three batches of 5, 5, 2 trials and one count each
      assert called.count('cg_binary_words') == 9
      assert called.count('cg_spike_intervals') == 3
    else:
      assert not NEW_ENTRY_POINTS & set(called), called
  cpu, gpu = reports['cpu'], reports['gpu']
  print('intervals cpu:', cpu['intervals'])
  print('intervals gpu:', gpu['intervals'])
  assert IC.same(cpu['intervals'], gpu['intervals'])
  assert IC.same(gpu['intervals'], IC.expected_report(real_spikes, fake_spikes))
  assert not IC.same(gpu['intervals']['generated'], gpu['intervals']['floor'])
  assert gpu['intervals']['floor']['num_trials'] == [12, 12]
  for device in ('cpu', 'gpu'):
    assert 'intervals' not in plain[device]
    rest = {k: v for k, v in reports[device].items()
            if k not in ('intervals', 'elapse')}
    assert IC.same(rest, {k: v for k, v in plain[device].items()
                          if k != 'elapse'})


def test_compute_metrics_gpu_refuses_what_the_packing_kernel_does_not_take(
    tmp_path):
  with pytest.raises(ValueError, match='3 .. 512 neurons'):
    cm.interval_sets_device(
        cm.build_parser().parse_args(['--output_dir', str(tmp_path)]),
        np.zeros((4, 50, 2), np.float32))
