"""GPU tests of cg_binary_words and cg_triplet_counts (csrc/triplets.hip: the
states packed 32 to a word, counted by AND and popcount over tiles of 16
neurons) against their numpy statements spike_metrics.binary_states /
triplet_counts -- equality of integers throughout -- and of compute_metrics.py
--triplet_metrics on both devices.

The kernel's paths: one tile triple (C <= 16), several with a tile of one
neuron (17, 33), the report's 102 and nine tiles (130); W below, at and past
one 64-word chunk; the words split over workgroups with the merge launch (C = 5
against W = 5000, and every C <= 33 at W >= 63); the largest counts (all ones)
and the largest output (C = 512).  Every output sits between guard words."""
import os

import numpy as np
import pytest
import torch

import compute_metrics as cm
import triplet_cases as TC
from calciumgan_amd import _lib
from calciumgan_amd.gan.utils import spike_metrics as sm

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = -7
GUARD = 1024   # elements of SENTINEL on either side of an output


def _guarded(n):
  buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
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


# -- cg_binary_words -----------------------------------------------------------------
def _words_of(x, bin, extra=0):
  """cg_binary_words of a float32 device (B, T, C) view into a guarded buffer
  with `extra` words of row stride past B wpt: uint32 host (C, B wpt)."""
  B, T, C = x.shape
  W = B * -(-(T // bin) // 32)
  stride = W + extra
  buf, out = _guarded(C * stride)
  _lib.call('cg_binary_words', x, B, T, C, x.stride(0), x.stride(1),
            x.stride(2), bin, out, stride, _lib.stream())
  torch.cuda.synchronize()
  assert _guards_intact(buf)
  got = out.view(C, stride).cpu().numpy()
  # nothing but the C x B wpt block is written
  assert (got[:, W:] == SENTINEL).all()
  return np.ascontiguousarray(got[:, :W]).view(np.uint32)


def _check_words(x, sp, bin):
  B, T, C = sp.shape
  nb = T // bin
  states = sm.binary_states(sp, bin)
  want = sm.pack_state_words(states, nb)
  _check(_words_of(x, bin), want)
  _check(_words_of(x, bin, extra=3), want)
  # the wrapper gives the same set
  dev = sm.binary_words_device(x, bin)
  assert (dev.C, dev.bin, dev.nb, dev.trials, len(dev)) == (C, bin, nb, B,
                                                            len(states))
  assert dev.tensor.dtype == torch.int32 and dev.tensor.is_cuda
  assert tuple(dev.tensor.shape) == want.shape
  _check(dev.states(), states)
  return dev, states


@pytest.mark.parametrize('case', TC.TRAINS, ids=lambda s: 'x'.join(map(str, s)))
def test_words_and_counts_of_trains_equal_the_statements(case):
  B, T, C, bin, density = case
  sp = TC.trains(B, T, C, density)
  dev, states = _check_words(torch.from_numpy(sp).to(DEV), sp, bin)
  if density == 1.0:
    assert states.all() and len(states) == B
  # and on through the counts
  want = sm.triplet_counts(states)
  counts, S = sm.triplet_counts_device(dev)
  assert S == len(states)
  for g, w in zip(counts, want):
    assert g.dtype == torch.int32 and g.is_cuda
    _check(g.cpu().numpy(), w)
  # joined sets: the words of the trials side by side
  if B > 1:
    x = torch.from_numpy(sp).to(DEV)
    cat = sm.DeviceWords.cat([sm.binary_words_device(x[:1], bin),
                              sm.binary_words_device(x[1:], bin)])
    assert cat.trials == B and torch.equal(cat.tensor, dev.tensor)


def test_words_read_strided_views_in_place():
  B, T, C, bin = 2, 50, 17, 12
  sp = TC.trains(B, T, C, 0.5)
  buf = torch.full((B, T, 128), 7.0, dtype=torch.float32, device=DEV)
  buf[:, :, :C] = torch.from_numpy(sp).to(DEV)
  x = buf[:, :, :C]
  assert x.stride() == (T * 128, 128, 1)
  _check_words(x, sp, bin)
  rows = torch.from_numpy(np.ascontiguousarray(sp.transpose(0, 2, 1))).to(DEV)
  x = rows.transpose(1, 2)                           # stored (B, C, T)
  assert tuple(x.shape) == (B, T, C) and x.stride() == (C * T, 1, T)
  _check_words(x, sp, bin)
  # reversed in time: a negative stride, which torch does not hold, straight
  # through the C ABI
  flipped = torch.from_numpy(np.ascontiguousarray(sp[:, ::-1])).to(DEV)
  W = B * 1
  wbuf, out = _guarded(C * W)
  last = flipped[:, T - 1:]
  _lib.call('cg_binary_words', last, B, T, C, T * C, -C, 1, bin, out, W,
            _lib.stream())
  torch.cuda.synchronize()
  assert _guards_intact(wbuf)
  _check(out.view(C, W).cpu().numpy().view(np.uint32),
         sm.pack_state_words(sm.binary_states(sp, bin), T // bin))


def test_nan_is_a_spike_and_minus_zero_is_not():
  sp = np.zeros((1, 24, 3), np.float32)
  sp[0, 1, 0] = np.nan
  sp[0, 2, 1] = -0.0
  sp[0, 13, 2] = -3.5
  dev, states = _check_words(torch.from_numpy(sp).to(DEV), sp, 12)
  assert states.tolist() == [[1, 0, 0], [0, 0, 1]]
  assert dev.tensor.cpu().tolist() == [[1], [0], [2]]


# -- cg_triplet_counts ---------------------------------------------------------------
def _count(w, extra=0, poison=0x7f7f7f7f):
  """cg_triplet_counts of host uint32 (C, W) words with every output between
  guards: (singles, pairs, triplets) as host arrays."""
  C, W = w.shape
  stride = W + extra
  t = torch.full((C, stride), 0x55555555, dtype=torch.int32, device=DEV)
  t[:, :W] = torch.from_numpy(w.view(np.int32).copy()).to(DEV)
  need = _lib.load().cg_triplet_counts_ws_bytes(C, W)
  assert need >= 16
  # (the workspace's contents do not matter: poison)
  ws = torch.full((need // 4 + 4,), poison, dtype=torch.int32, device=DEV)
  Tr = C * (C - 1) * (C - 2) // 6
  sbuf, singles = _guarded(C)
  pbuf, pairs = _guarded(C * C)
  tbuf, triplets = _guarded(Tr)
  _lib.call('cg_triplet_counts', t, C, W, stride, singles, pairs, triplets, ws,
            _lib.stream())
  torch.cuda.synchronize()
  assert _guards_intact(sbuf) and _guards_intact(pbuf) and _guards_intact(tbuf)
  return (singles.cpu().numpy(), pairs.view(C, C).cpu().numpy(),
          triplets.cpu().numpy())


def _compare(C, W, kind='dense', extra=0):
  got = _count(TC.words(C, W, kind), extra)
  for g, w in zip(got, TC.word_counts(C, W, kind)):
    _check(g, w)
  return got


@pytest.mark.parametrize('W', TC.WORD_COUNTS)
@pytest.mark.parametrize('C', TC.WORD_NEURONS)
def test_counts_equal_the_statement(C, W):
  _compare(C, W, 'dense')
  _compare(C, W, 'sparse', extra=5)


def test_the_split_path_with_its_merge():
  C, W = TC.SPLIT_CASE
  assert _lib.load().cg_triplet_counts_ws_bytes(C, W) == 40 * 4096 * 4
  _compare(C, W, 'dense')
  _compare(C, W, 'sparse', extra=1)


@pytest.mark.parametrize('shape', [(3, 1), (17, 65), (102, 64), TC.SPLIT_CASE],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_all_ones_and_all_zeros(shape):
  C, W = shape
  singles, pairs, triplets = _compare(C, W, 'ones')
  # the largest counts there are: every state of every word
  assert (singles == 32 * W).all() and (pairs == 32 * W).all()
  assert (triplets == 32 * W).all()
  for x in _compare(C, W, 'zeros'):
    assert not x.any()


def test_the_largest_output():
  C, W = TC.LARGEST_CASE
  assert C == _lib.CONSTANTS['CG_TRIPLET_MAX_C']
  got = _compare(C, W, 'dense')
  assert got[2].shape == (22238720,)


def test_two_calls_give_identical_results():
  for C, W in ((102, 65), TC.SPLIT_CASE):
    w = TC.words(C, W)
    first = _count(w)
    again = _count(w, poison=-1)
    for a, b in zip(first, again):
      assert a.tobytes() == b.tobytes()
    # the wrapper
    dev = sm.DeviceWords(torch.from_numpy(w.view(np.int32).copy()).to(DEV), C, 1,
                         32 * W, 1)
    counts, S = sm.triplet_counts_device(dev)
    assert S == 32 * W
    for g, a in zip(counts, first):
      _check(g.cpu().numpy(), a)


def test_refused_arguments_leave_the_buffers_untouched():
  lib = _lib.load()
  C, W, B, T = 17, 2, 2, 50     # four bins a trial: one word, W = B words
  x = torch.ones(B, T, C, dtype=torch.float32, device=DEV)
  words = torch.full((C * W + 4,), SENTINEL, dtype=torch.int32, device=DEV)
  out = torch.full((4096,), SENTINEL, dtype=torch.int32, device=DEV)
  ws = torch.full((4096,), SENTINEL, dtype=torch.int32, device=DEV)
  s, p, t = out[:C], out[32:32 + C * C], out[512:512 + 680]
  st = _lib.stream()

  def pack(x=x, B=B, T=T, C=C, bin=12, w=words, stride=W):
    return lib.cg_binary_words(x, B, T, C, T * C, C, 1, bin, w, stride, st)

  def count(w=words, C=C, W=W, stride=W, s=s, p=p, t=t, ws=ws):
    return lib.cg_triplet_counts(w, C, W, stride, s, p, t, ws, st)

  for kw in (dict(x=None), dict(w=None), dict(w=words[1:]), dict(B=0),
             dict(T=0), dict(bin=0), dict(bin=51), dict(C=2), dict(C=513),
             dict(stride=1)):
    assert pack(**kw) == _lib.CG_EINVAL, kw
  for kw in (dict(w=None), dict(ws=None), dict(s=None), dict(p=None),
             dict(t=None), dict(w=words[1:]), dict(ws=ws[1:]), dict(C=2),
             dict(C=513), dict(W=0), dict(W=1 << 26), dict(stride=W - 1)):
    assert count(**kw) == _lib.CG_EINVAL, kw
  torch.cuda.synchronize()
  for buf in (words, out, ws):
    assert bool((buf == SENTINEL).all())
  with pytest.raises(ValueError):
    sm.binary_words_device(x[:, :, :2])
  with pytest.raises(ValueError):
    sm.binary_words_device(x, 51)
  # and the same calls, admitted, write
  assert pack() == 0 and count() == 0
  torch.cuda.synchronize()
  assert bool((s == B * 4).all())


def test_scores_are_the_same_dict_on_both_devices():
  a, b = TC.xor_states(1, 1000), TC.xor_states(3, 1000, broken=True)
  want = sm.triplet_scores(TC.side(a), TC.side(b))

  def device_side(x):
    w = torch.from_numpy(sm.pack_state_words(x, len(x)).view(np.int32)).to(DEV)
    counts, S = sm.triplet_counts_device(
        sm.DeviceWords(w, x.shape[1], 1, len(x), 1))
    return counts + (S,)

  got = sm.triplet_scores(device_side(a), device_side(b))
  print(want)
  assert TC.same(got, want)
  assert got['num_states'] == [1000, 1000]


# -- compute_metrics.py --------------------------------------------------------------
NEW_ENTRY_POINTS = {'cg_binary_words', 'cg_triplet_counts'}


def test_compute_metrics_triplet_flag_on_both_devices(tmp_path, monkeypatch):
  called = []
  call = _lib.call

  def recording(name, *args):
    called.append(name)
    return call(name, *args)

  monkeypatch.setattr(_lib, 'call', recording)
  reports, plain = {}, {}
  for device in ('cpu', 'gpu'):
    os.makedirs(tmp_path / device)
    fake, real_spikes, fake_spikes = TC.run_dir(tmp_path / device)
    args = ['--output_dir', str(tmp_path / device), '--num_processors', '1',
            '--verbose', '0', '--device', device, '--batch_trials', '5']
    hp = cm.build_parser().parse_args(args)
    assert not hasattr(hp, 'triplet_metrics')
    del called[:]
    plain[device] = cm.main(hp)[0]
    # without the flag none of the new entry points is launched
    assert not NEW_ENTRY_POINTS & set(called), called
    if device == 'gpu':
      assert called
    del called[:]
    reports[device] = cm.main(
        cm.build_parser().parse_args(args + ['--triplet_metrics']))[0]
    if device == 'gpu':
      # three sides: three batches of 5, 5, 2 trials and one count each
      assert called.count('cg_binary_words') == 9
      assert called.count('cg_triplet_counts') == 3
    else:
      assert not NEW_ENTRY_POINTS & set(called), called
  cpu, gpu = reports['cpu'], reports['gpu']
  print('triplets cpu:', cpu['triplets'])
  print('triplets gpu:', gpu['triplets'])
  assert TC.same(cpu['triplets'], gpu['triplets'])
  assert TC.same(gpu['triplets'], TC.expected_report(real_spikes, fake_spikes))
  assert not TC.same(gpu['triplets']['generated'], gpu['triplets']['floor'])
  assert gpu['triplets']['floor']['num_states'] == [480, 480]
  assert gpu['triplets']['floor']['triplets_observed'][0] > 0.9
  for device in ('cpu', 'gpu'):
    assert 'triplets' not in plain[device]
    rest = {k: v for k, v in reports[device].items()
            if k not in ('triplets', 'elapse')}
    assert TC.same(rest, {k: v for k, v in plain[device].items()
                          if k != 'elapse'})
