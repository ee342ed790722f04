"""Host side of --plot_weights (no GPU): the numpy statements of
cg_tensor_summary (summary_helper.histogram_buckets / variable_statistics) on
the value sets of tests/tensor_summary_cases.py against figures worked out
here, histogram events byte by byte and through a file, the variable-name
table, and Summary.log with and without the flag."""
import json
import math
import os
import struct
from types import SimpleNamespace

import numpy as np
import pytest

import main as cli
import tensor_summary_cases as tc
from calciumgan_amd import _lib
from calciumgan_amd import build as cg_build
from calciumgan_amd import geometry as geo
from calciumgan_amd.gan.utils import summary_helper as sh
from calciumgan_amd.gan.utils import tb_events

K = tc.NUM_BUCKETS


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _python_counts(x, k=K):
  """The statement with Python floats (IEEE double, one rounding per
  operation), value by value."""
  d = [float(v) for v in x]
  mn, mx = min(d), max(d)
  w = (mx - mn) / k
  counts = [0] * k
  for v in d:
    counts[min(int(math.floor((v - mn) / w)), k - 1)] += 1
  return counts


# -- the statements ----------------------------------------------------------
def test_exact_boundaries_one_value_per_bucket_two_in_the_last():
  a = tc.exact_boundaries()
  rows = sh.histogram_buckets(a)
  assert rows.shape == (30, 3) and rows.dtype == np.float64
  left = np.array([j / 16 - 1 for j in range(30)])
  assert np.array_equal(_bits(rows[:, 0]), _bits(left))
  assert np.array_equal(_bits(rows[:, 1]), _bits(left + 1 / 16))  # exact sums
  assert rows[-1, 1] == 0.875
  assert rows[:, 2].tolist() == [1.0] * 29 + [2.0]
  st = sh.variable_statistics(a)
  assert {type(v) for v in st.values()} == {np.float64}
  # an arithmetic progression of 31 terms, step 1/16: variance (31^2 - 1)/12/256
  assert st == dict(mean=-0.0625, stddev=math.sqrt(0.3125), min=-1.0, max=0.875)
  # reversed, and repeated: the same edges, the counts times 133
  assert np.array_equal(sh.histogram_buckets(a[::-1]), rows)
  many = sh.histogram_buckets(np.tile(a, 133))
  assert np.array_equal(many[:, :2], rows[:, :2])
  assert np.array_equal(many[:, 2], rows[:, 2] * 133)


@pytest.mark.parametrize('pair, differing', tc.INEXACT)
def test_inexact_widths_need_the_float64_quotient(pair, differing):
  x = tc.inexact_widths(*pair)
  assert x.shape == (93,) and x.dtype == np.float32
  assert x.min() == np.float32(pair[0]) and x.max() == np.float32(pair[1])
  rows = sh.histogram_buckets(x)
  assert rows[:, 2].tolist() == _python_counts(x)
  assert rows[:, 2].sum() == 93
  assert np.array_equal(np.bincount(tc.statement_index(x), minlength=K),
                        rows[:, 2])
  # a float32 evaluation of the index puts this many values elsewhere: the case
  # fails for a kernel that does not divide in float64
  assert int((tc.float32_index(x) != tc.statement_index(x)).sum()) == differing
  mn, mx = float(x.min()), float(x.max())
  w = (mx - mn) / 30
  assert rows[:, 0].tolist() == [mn + j * w for j in range(30)]
  assert rows[:, 1].tolist() == [mn + j * w for j in range(1, 30)] + [mx]


@pytest.mark.parametrize('n', [1, 5, 257, 70001])
def test_constant_segments_are_one_unit_bucket(n):
  for seg, v in zip(tc.constants(n), (0.0, 1.0, -2.5, 0.0)):
    rows = sh.histogram_buckets(seg)
    assert rows.shape == (1, 3) and rows.dtype == np.float64
    assert rows.tolist() == [[v - 0.5, v + 0.5, float(n)]]
    st = sh.variable_statistics(seg)
    assert (st['mean'], st['stddev'], st['min'], st['max']) == (v, 0.0, v, v)
  # whichever zero is the minimum, the edges carry these bits
  assert np.array_equal(_bits(sh.histogram_buckets(tc.constants(n)[3])[0, :2]),
                        _bits([-0.5, 0.5]))


def test_extreme_magnitudes():
  big = float(tc.F32_MAX)
  rows = sh.histogram_buckets(np.array([big, -big], np.float32))
  w = (big + big) / 30
  assert rows[:, 0].tolist() == [-big + j * w for j in range(30)]
  assert rows[-1, 1] == big and np.isfinite(rows).all()
  assert rows[:, 2].tolist() == [1.0] + [0.0] * 28 + [1.0]
  st = sh.variable_statistics(np.array([big, -big], np.float32))
  assert (st['mean'], st['stddev'], st['min'], st['max']) == (0, big, -big, big)
  tiny = 2.0**-149
  x = np.array([tiny, -tiny, 0.0], np.float32)
  assert x[0] > 0  # (a float32 subnormal, kept)
  rows = sh.histogram_buckets(x)
  assert rows[0, 0] == -tiny and rows[-1, 1] == tiny
  counts = [0.0] * 30
  counts[0] = counts[15] = counts[29] = 1.0
  assert rows[:, 2].tolist() == counts
  st = sh.variable_statistics(x)
  assert st['mean'] == 0 and st['stddev'] == math.sqrt(2 * tiny * tiny / 3)
  # the mixed segments of the case: subnormals fall into the two middle buckets
  for seg in tc.segments('extreme')[:2]:
    rows = sh.histogram_buckets(seg)
    assert rows[:, 2].tolist() == _python_counts(seg)
    assert rows[0, 2] == 1 and rows[-1, 2] == 1
    assert rows[14, 2] + rows[15, 2] == len(seg) - 2


def test_nonfinite_values_and_other_bucket_numbers():
  nan_seg, inf_seg = tc.segments('nonfinite')[1], tc.segments('nonfinite')[3]
  for seg in (nan_seg, inf_seg):
    assert all(np.isnan(v) for v in sh.variable_statistics(seg).values())
    with pytest.raises(ValueError):
      sh.histogram_buckets(seg)
    stats, buckets = tc.statement_rows(seg)
    assert stats[0] == len(seg) and np.isnan(stats[1:7]).all()
    assert not buckets.any()
  assert tc.statement_rows(nan_seg)[0][7] == 1
  assert tc.statement_rows(inf_seg)[0][7] == 2
  x = tc.segments('lengths')[10]
  for k in (1, 2, 7, 512):
    rows = sh.histogram_buckets(x, k)
    assert rows.shape == (k, 3) and rows[:, 2].sum() == len(x)
    assert rows[:, 2].tolist() == _python_counts(x, k)
  for bad in (0, -1):
    with pytest.raises(ValueError):
      sh.histogram_buckets(x, bad)
  with pytest.raises(ValueError):
    sh.histogram_buckets(np.zeros(0, np.float32))


def test_the_cases_are_laid_out_as_described():
  assert tc.CHUNK == int(
      open(os.path.join(cg_build.CSRC, 'summary.hip')).read().split(
          'constexpr int kTsChunk = ')[1].split(';')[0])
  for name in tc.CASES:
    buf, offsets, lengths = tc.case(name)
    assert buf.dtype == np.float32 and not buf.flags.writeable
    inside = np.zeros(len(buf), bool)
    for o, n in zip(offsets, lengths):
      assert 0 <= o and o + n <= len(buf) and n >= 1
      inside[o:o + n] = True
    if name != 'glorot':
      assert np.isnan(buf[~inside]).all() and not inside[0] and not inside[-1]
  assert len(tc.case('forty')[1]) == 40
  odd, aligned = tc.case('lengths'), tc.case('lengths_aligned_first')
  assert odd[2] == aligned[2] == tc.LENGTHS
  assert {tc.CHUNK - 1, tc.CHUNK + 1, 2 * tc.CHUNK + 1, 70001} <= set(tc.LENGTHS)
  for a, b in zip(odd[1], aligned[1]):
    assert (a % 4 == 0) != (b % 4 == 0)
  assert all(o % 4 == 0 for o in tc.case('glorot')[1])
  # the small model of tests/test_main_e2e.py: 24 + 12 variables
  sizes = tc.case('glorot')[2]
  assert len(sizes) == 36
  assert sizes[:4] == (32 * 8 * 32, 8 * 32, 24 * 40 * 32, 40)
  assert sizes[24:26] == (24 * 16 * 8, 8) and sizes[-2:] == (8 * 40, 1)


# -- event files ---------------------------------------------------------------
def _varint(n):
  out = b''
  while True:
    out += bytes([(n & 0x7f) | (0x80 if n > 0x7f else 0)])
    n >>= 7
    if not n:
      return out


def _field(number, payload):
  return _varint(number << 3 | 2) + _varint(len(payload)) + payload


def test_histogram_event_bytes_field_by_field():
  rows = sh.histogram_buckets(tc.exact_boundaries())
  tag = 'plots_generator/01/dense/kernel:0'
  got = tb_events.encode_histogram_event(12.5, 7, tag, rows)
  dims = (_field(2, b'\x08' + _varint(30)) +      # Dim { size = 1: 30 }
          _field(2, b'\x08' + _varint(3)))
  tensor = (b'\x08\x02' +                          # dtype = 1: DT_DOUBLE
            _field(2, dims) +                      # tensor_shape = 2
            _field(4, struct.pack('<90d', *rows.reshape(-1))))
  metadata = _field(1, _field(1, b'histograms'))   # plugin_data { plugin_name }
  value = _field(1, tag.encode()) + _field(8, tensor) + _field(9, metadata)
  want = (b'\x09' + struct.pack('<d', 12.5) +      # wall_time = 1, fixed64
          b'\x10\x07' +                            # step = 2
          _field(5, _field(1, value)))             # summary { value }
  assert got == want
  ev = tb_events.decode_event(got)
  assert set(ev) == {'wall_time', 'step', 'tag', 'histogram'}
  assert ev['tag'] == tag and ev['step'] == 7 and ev['wall_time'] == 12.5
  assert ev['histogram'].dtype == np.float64
  assert np.array_equal(_bits(ev['histogram']), _bits(rows))
  # step 0 is left out, as for a scalar; a single bucket is a (1, 3) tensor
  one = tb_events.encode_histogram_event(1.0, 0, 't', [[-0.5, 0.5, 4.0]])
  assert b'\x10' not in one[:10]
  assert tb_events.decode_event(one)['histogram'].tolist() == [[-0.5, 0.5, 4.0]]
  for bad in (np.zeros((0, 3)), np.zeros(3), np.zeros((4, 2))):
    with pytest.raises(ValueError):
      tb_events.encode_histogram_event(1.0, 0, 't', bad)


def test_scalars_and_histograms_interleaved_through_a_file(tmp_path):
  w = tb_events.EventFileWriter(str(tmp_path))
  rows = [sh.histogram_buckets(seg) for seg in tc.segments('inexact')[:3]]
  w.scalar('loss/generator', 0.25, step=3)
  w.histogram('h/a', rows[0], step=3)
  w.histogram('h/b', np.array([[0.5, 1.5, 9.0]]), step=0)
  w.scalar('elapse', 1.5, step=4)
  w.histogram('h/c', rows[2], step=2**40)
  ev = tb_events.read_events(w.path)
  assert ev[0]['file_version'] == b'brain.Event:2'
  assert [(e.get('tag'), e['step']) for e in ev[1:]] == [
      ('loss/generator', 3), ('h/a', 3), ('h/b', 0), ('elapse', 4),
      ('h/c', 2**40)]
  assert ev[1]['value'] == 0.25 and 'histogram' not in ev[1]
  assert ev[4]['value'] == 1.5 and set(ev[4]) == {'wall_time', 'step', 'tag',
                                                  'value'}
  assert 'value' not in ev[2]
  assert np.array_equal(_bits(ev[2]['histogram']), _bits(rows[0]))
  assert ev[3]['histogram'].tolist() == [[0.5, 1.5, 9.0]]
  assert np.array_equal(_bits(ev[5]['histogram']), _bits(rows[2]))
  # the framing carries its CRCs: a flipped payload byte is caught
  raw = bytearray(open(w.path, 'rb').read())
  raw[-20] ^= 1
  bad = tmp_path / 'corrupt'
  bad.write_bytes(bytes(raw))
  with pytest.raises(IOError):
    tb_events.read_events(str(bad))


# -- names -----------------------------------------------------------------------
def test_variable_names_plain_layer_norm_and_batch_norm():
  plain = geo.generator_variable_names()
  assert plain[:4] == ['dense/kernel:0', 'dense/bias:0',
                       'conv1d_transpose/conv2d_transpose/kernel:0',
                       'conv1d_transpose/conv2d_transpose/bias:0']
  assert plain[4:6] == ['conv1d_transpose_1/conv2d_transpose_1/kernel:0',
                        'conv1d_transpose_1/conv2d_transpose_1/bias:0']
  assert plain[-4:] == ['conv1d_transpose_4/conv2d_transpose_4/kernel:0',
                        'conv1d_transpose_4/conv2d_transpose_4/bias:0',
                        'dense_1/kernel:0', 'dense_1/bias:0']
  assert len(plain) == 14 and len(set(plain)) == 14
  ln = geo.generator_variable_names(layer_norm=True)
  assert len(ln) == 24 and [n for n in ln if 'normalization' not in n] == plain
  assert ln[4:6] == ['layer_normalization/gamma:0', 'layer_normalization/beta:0']
  assert ln[8:10] == ['layer_normalization_1/gamma:0',
                      'layer_normalization_1/beta:0']
  assert ln[20:22] == ['layer_normalization_4/gamma:0',
                       'layer_normalization_4/beta:0']
  bn = geo.generator_variable_names(batch_norm=True)
  assert len(bn) == 34 and [n for n in bn if 'normalization' not in n] == plain
  assert bn[4:8] == ['batch_normalization/gamma:0', 'batch_normalization/beta:0',
                     'batch_normalization/moving_mean:0',
                     'batch_normalization/moving_variance:0']
  assert bn[10:14] == ['batch_normalization_1/' + v + ':0' for v in
                       ('gamma', 'beta', 'moving_mean', 'moving_variance')]
  both = geo.generator_variable_names(layer_norm=True, batch_norm=True)
  assert both[4:10] == bn[4:8] + ln[4:6] and len(both) == 44
  dis = geo.discriminator_variable_names()
  assert dis == ['conv1d/kernel:0', 'conv1d/bias:0', 'conv1d_1/kernel:0',
                 'conv1d_1/bias:0', 'conv1d_2/kernel:0', 'conv1d_2/bias:0',
                 'conv1d_3/kernel:0', 'conv1d_3/bias:0', 'conv1d_4/kernel:0',
                 'conv1d_4/bias:0', 'dense_2/kernel:0', 'dense_2/bias:0']


# -- Summary ---------------------------------------------------------------------
class _Params(object):
  """What Summary.plot_weights uses of nets.FlatParams, over host arrays."""

  def __init__(self, names, arrays, frozen=()):
    self.names, self.arrays, self.frozen = names, arrays, set(frozen)
    self.calls = 0

  def summary_indices(self, trainable_only=True):
    return [i for i in range(len(self.names))
            if not (trainable_only and i in self.frozen)]

  def summaries_host(self, bucket_count=30, trainable_only=True):
    self.calls += 1
    rows = [tc.statement_rows(self.arrays[i], bucket_count)
            for i in self.summary_indices(trainable_only)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def _gan():
  rng = np.random.RandomState(5)
  gen = _Params(['dense/kernel:0', 'dense/bias:0', 'bn/moving_mean:0',
                 'dense_1/kernel:0'],
                [rng.uniform(-1, 1, (4, 9)).astype(np.float32),
                 np.zeros(9, np.float32), np.full(3, 7, np.float32),
                 np.array([1.0, np.nan, 2.0], np.float32)], frozen=[2])
  dis = _Params(['conv1d/kernel:0'], [rng.normal(0, 1, 700).astype(np.float32)])
  model = lambda p: SimpleNamespace(net=SimpleNamespace(params=p))
  return SimpleNamespace(generator=model(gen), discriminator=model(dis),
                         gen_optimizer=SimpleNamespace(),
                         dis_optimizer=SimpleNamespace())


def _log(tmp_path, name, **flags):
  hp = SimpleNamespace(output_dir=str(tmp_path / name), verbose=0, **flags)
  os.makedirs(hp.output_dir)
  summary = sh.Summary(hp)
  gan = _gan()
  summary.log(0.5, -0.25, 0.125, elapse=2.0, gan=gan, step=3, training=True)
  summary.log(0.75, -0.5, None, metrics={'signals_metrics/min': 0.0},
              elapse=1.0, step=3, training=False)
  return hp.output_dir, gan


def _lines(path):
  return [json.loads(l) for l in open(path)]


def test_plot_weights_off_leaves_the_log_as_it_was(tmp_path):
  assert cli.build_parser().parse_args([]).plot_weights is False
  want = [('loss/generator', 0.5), ('loss/discriminator', -0.25),
          ('loss/gradient_penalty', 0.125), ('elapse', 2.0)]
  for name, flags in (('absent', {}), ('off', dict(plot_weights=False))):
    out, gan = _log(tmp_path, name, **flags)
    assert [(r['tag'], r['value']) for r in
            _lines(os.path.join(out, 'scalars.jsonl'))] == want
    assert all(r['step'] == 3 for r in _lines(os.path.join(out, 'scalars.jsonl')))
    assert not os.path.exists(os.path.join(out, 'histograms.jsonl'))
    assert not os.path.exists(os.path.join(out, 'validation',
                                           'histograms.jsonl'))
    ev = tb_events.read_events(_event_file(out))
    assert [e.get('tag') for e in ev[1:]] == [t for t, _ in want]
    assert not any('histogram' in e for e in ev)
    assert gan.generator.net.params.calls == 0


def _event_file(directory):
  files = [f for f in os.listdir(directory) if f.startswith('events.out.')]
  assert len(files) == 1
  return os.path.join(directory, files[0])


def test_plot_weights_writes_scalars_and_histograms_of_trainable_variables(
    tmp_path):
  out, gan = _log(tmp_path, 'on', plot_weights=True)
  gen, dis = gan.generator.net.params, gan.discriminator.net.params
  assert gen.calls == 1 and dis.calls == 1   # one summary per model
  scalars = _lines(os.path.join(out, 'scalars.jsonl'))
  tags = [r['tag'] for r in scalars]
  # (the frozen variable is not counted: dense_1/kernel:0 is number 3)
  names = ['plots_generator/01/dense/kernel:0', 'plots_generator/02/dense/bias:0',
           'plots_generator/03/dense_1/kernel:0',
           'plots_discriminator/01/conv1d/kernel:0']
  assert tags == ['loss/generator', 'loss/discriminator', 'loss/gradient_penalty',
                  'elapse'] + [n + s for n in names for s in
                               ('/0_mean', '/1_stddev', '/2_min', '/3_max')]
  by_tag = {r['tag']: r['value'] for r in scalars}
  for name, values in zip(names, (gen.arrays[0], gen.arrays[1], gen.arrays[3],
                                  dis.arrays[0])):
    st = sh.variable_statistics(values)
    for suffix, key in (('/0_mean', 'mean'), ('/1_stddev', 'stddev'),
                        ('/2_min', 'min'), ('/3_max', 'max')):
      assert np.array_equal(by_tag[name + suffix], float(st[key]),
                            equal_nan=True), (name, suffix)
  assert np.isnan(by_tag[names[2] + '/0_mean'])
  # histograms: every variable but the one with a NaN in it, at the step
  hist = _lines(os.path.join(out, 'histograms.jsonl'))
  assert [h['tag'] for h in hist] == [names[0], names[1], names[3]]
  assert all(h['step'] == 3 for h in hist)
  assert hist[1]['buckets'] == [[-0.5, 0.5, 9.0]]
  assert np.array_equal(np.array(hist[0]['buckets']),
                        sh.histogram_buckets(gen.arrays[0]))
  ev = tb_events.read_events(_event_file(out))
  got = {e['tag']: e['histogram'] for e in ev if 'histogram' in e}
  assert list(got) == [names[0], names[1], names[3]]
  assert np.array_equal(_bits(got[names[3]]),
                        _bits(sh.histogram_buckets(dis.arrays[0])))
  assert got[names[3]][:, 2].sum() == 700
  assert len(ev) == 1 + len(scalars) + len(hist)
  # the validation writer gets none of it
  va = _lines(os.path.join(out, 'validation', 'scalars.jsonl'))
  assert [r['tag'] for r in va] == ['loss/generator', 'loss/discriminator',
                                    'signals_metrics/min', 'elapse']
  assert not os.path.exists(os.path.join(out, 'validation', 'histograms.jsonl'))
  assert not any('histogram' in e for e in tb_events.read_events(
      _event_file(os.path.join(out, 'validation'))))


def test_histogram_and_variable_summary_of_host_arrays(tmp_path):
  hp = SimpleNamespace(output_dir=str(tmp_path / 'h'), verbose=0)
  os.makedirs(hp.output_dir)
  summary = sh.Summary(hp)
  x = tc.segments('lengths')[12]
  summary.histogram('weights', x.reshape(32, 32), step=2)
  summary.variable_summary(x, 'v', step=2, training=False)
  summary.variable_summary(np.array([1.0, np.inf]), 'w', step=2)
  hist = _lines(os.path.join(hp.output_dir, 'histograms.jsonl'))
  assert [h['tag'] for h in hist] == ['weights']
  assert np.array_equal(np.array(hist[0]['buckets']), sh.histogram_buckets(x))
  va = os.path.join(hp.output_dir, 'validation')
  assert [h['tag'] for h in _lines(os.path.join(va, 'histograms.jsonl'))] == ['v']
  assert [r['tag'] for r in _lines(os.path.join(va, 'scalars.jsonl'))] == [
      'v/0_mean', 'v/1_stddev', 'v/2_min', 'v/3_max']
  tr = _lines(os.path.join(hp.output_dir, 'scalars.jsonl'))
  assert [r['tag'] for r in tr] == ['w/0_mean', 'w/1_stddev', 'w/2_min',
                                    'w/3_max']
  assert all(np.isnan(r['value']) for r in tr)
  with pytest.raises(ValueError):
    summary.histogram('bad', np.array([1.0, np.nan]))


# -- the C ABI, as far as a CPU sees it -------------------------------------------
def test_the_entry_points_are_declared_built_and_refuse_bad_arguments():
  assert 'summary.hip' in cg_build.SOURCES
  F, D, V = (_lib._DATA_PTRS[e] for e in ('float', 'double', 'void'))
  LL = _lib._DATA_PTRS['long long']
  import ctypes as C
  assert _lib.SIGNATURES['cg_tensor_summary'] == [
      F, LL, LL, C.c_int, C.c_longlong, C.c_int, D, D, V, C.c_longlong, V]
  assert _lib.SIGNATURES['cg_tensor_summary_ws_bytes'] == [
      C.c_int, C.c_longlong, C.c_int]
  import torch
  t = torch.zeros(3, dtype=torch.int64)
  assert LL.from_param(t[1:]).value == t.data_ptr() + 8
  with pytest.raises(TypeError):
    LL.from_param(torch.zeros(3, dtype=torch.int32))
  cg_build.build(verbose=False)
  for precision in ('bf16', 'f16'):
    lib = _lib.load(precision)
    size = lib.cg_tensor_summary_ws_bytes
    assert size(1, 1, 1) > 0 and size(1, 1, 1) % 8 == 0
    assert size(40, 10**6, 30) >= 41 * 8 + 40 * 30 * 4 + 40 * (10**6 // tc.CHUNK)
    assert size(65535, 2**40, 512) > 2**28 * 40
    for bad in ((0, 1, 30), (-1, 1, 30), (65536, 1, 30), (1, 0, 30), (1, -5, 30),
                (1, 1, 0), (1, 1, 513), (1, 1, -1)):
      assert size(*bad) == -1, bad
    # a NULL pointer or a bad count is refused before anything touches a device
    buf = (C.c_double * 4096)()
    ok = dict(data=buf, off=buf, len=buf, nseg=1, total=1, k=30, stats=buf,
              buckets=buf, ws=buf, ws_bytes=size(1, 1, 30))

    def call(**kw):
      a = dict(ok, **kw)
      return lib.cg_tensor_summary(a['data'], a['off'], a['len'], a['nseg'],
                                   a['total'], a['k'], a['stats'], a['buckets'],
                                   a['ws'], a['ws_bytes'], None)

    for kw in (dict(data=None), dict(off=None), dict(len=None), dict(stats=None),
               dict(buckets=None), dict(ws=None), dict(nseg=0), dict(nseg=65536),
               dict(k=0), dict(k=513), dict(total=0),
               dict(ws_bytes=size(1, 1, 30) - 1),
               dict(ws=C.c_void_p(C.addressof(buf) + 4))):
      assert call(**kw) == _lib.CG_EINVAL, kw
