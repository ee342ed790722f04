"""main.py --plot_weights on the GPU: one epoch on the 70-segment DG set of
tests/test_main_e2e.py, under both algorithms and once with --layer_norm.  Every
trainable variable of both models leaves four scalars and one histogram in the
training event file, equal to the numpy statements on the weights of the epoch's
checkpoint (validation and the checkpoint come after the log and change no
weight); the validation writer gets none of it, and without the flag nothing of
it is written."""
import glob
import json
import math
import os
import pickle

import numpy as np
import pytest

import main as cli
from calciumgan_amd import geometry as geo
from calciumgan_amd.gan.utils import summary_helper as sh
from calciumgan_amd.gan.utils import tb_events
from test_main_e2e import _dataset

pytestmark = pytest.mark.gpu

U = 2.0**-53
SUFFIXES = ('/0_mean', '/1_stddev', '/2_min', '/3_max')


@pytest.fixture(autouse=True)
def _back_to_bf16():
  yield
  from calciumgan_amd import _lib
  _lib.use('bf16')


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _run(tmp_path, *extra):
  out = str(tmp_path / 'run')
  hp = cli.build_parser().parse_args([
      '--input_dir', _dataset(tmp_path), '--output_dir', out, '--model',
      'calciumgan', '--batch_size', '8', '--num_units', '8', '--m', '2',
      '--epochs', '1', '--verbose', '0'] + list(extra))
  hp.global_step = 0
  hp.surrogate_ds = False
  cli.main(hp)
  return out


def _events(directory):
  files = glob.glob(os.path.join(directory, 'events.out.tfevents.*'))
  assert len(files) == 1
  return tb_events.read_events(files[0])


def _lines(path):
  return [json.loads(l) for l in open(path)]


@pytest.mark.parametrize('flags', [('--algorithm', 'wgan-gp'),
                                   ('--algorithm', 'gan'),
                                   ('--algorithm', 'wgan-gp', '--layer_norm')],
                         ids=['wgan-gp', 'gan', 'wgan-gp-layer_norm'])
def test_every_trainable_variable_is_summarised_once_per_epoch(tmp_path, flags):
  out = _run(tmp_path, '--plot_weights', *flags)
  ck = pickle.load(open(os.path.join(out, 'checkpoints', 'epoch-000.pkl'), 'rb'))
  layer_norm = '--layer_norm' in flags
  models = (('plots_generator', geo.generator_variable_names(layer_norm),
             ck['gen_weights']),
            ('plots_discriminator', geo.discriminator_variable_names(),
             ck['dis_weights']))
  assert len(models[0][1]) == len(ck['gen_weights']) == (24 if layer_norm else 14)
  assert len(models[1][1]) == len(ck['dis_weights']) == 12
  events = _events(out)
  scalars = {(e['tag'], e['step']): e['value'] for e in events if 'value' in e}
  hists = [e for e in events if 'histogram' in e]
  doubles = {(r['tag'], r['step']): r['value']
             for r in _lines(os.path.join(out, 'scalars.jsonl'))}
  lines = {(r['tag'], r['step']): np.array(r['buckets'])
           for r in _lines(os.path.join(out, 'histograms.jsonl'))}
  tags = []
  for scope, names, weights in models:
    for i, (name, w) in enumerate(zip(names, weights)):
      tag = '{}/{:02d}/{}'.format(scope, i + 1, name)
      tags.append(tag)
      d = w.astype(np.float64).reshape(-1)
      n = float(d.size)
      # the histogram: one, at step 0, the statement's rows bit for bit
      mine = [e for e in hists if e['tag'] == tag]
      assert len(mine) == 1 and mine[0]['step'] == 0, tag
      rows = mine[0]['histogram']
      assert rows[:, 2].sum() == d.size, tag
      assert np.array_equal(_bits(rows), _bits(sh.histogram_buckets(w))), tag
      assert np.array_equal(_bits(lines[tag, 0]), _bits(rows)), tag
      # the scalars: the event holds the float32 of what scalars.jsonl holds
      for suffix in SUFFIXES:
        assert (tag + suffix, 0) in scalars, tag + suffix
        assert _bits(scalars[tag + suffix, 0]) == _bits(
            np.float32(doubles[tag + suffix, 0])), tag + suffix
      assert doubles[tag + '/2_min', 0] == d.min(), tag
      assert doubles[tag + '/3_max', 0] == d.max(), tag
      # mean = sum / n with |sum - fsum(d)| <= 2 n u sum|d|; the division rounds
      # once there and once here
      mean = doubles[tag + '/0_mean', 0]
      exact = math.fsum(d) / n
      assert abs(mean - exact) <= 2 * U * (math.fsum(np.abs(d)) + abs(exact)), tag
      # stddev = sqrt(sq / n) with sq within 2 (n + 4) u of fsum((d - mean)^2)
      # about the device's own mean: the root halves that, the division and
      # the root round once each
      c = d - mean
      ref = math.sqrt(math.fsum(c * c) / n)
      assert abs(doubles[tag + '/1_stddev', 0] - ref) <= (n + 8) * U * ref, tag
  assert [e['tag'] for e in hists] == tags
  assert sorted(t for t, _ in scalars if t.startswith('plots_')) == sorted(
      t + s for t in tags for s in SUFFIXES)
  assert sorted(t for t, _ in lines) == sorted(tags)
  # the validation writer gets none of these events
  va = _events(os.path.join(out, 'validation'))
  assert len(va) > 1
  assert not any('histogram' in e or e.get('tag', '').startswith('plots_')
                 for e in va)
  assert not os.path.exists(os.path.join(out, 'validation', 'histograms.jsonl'))


def test_without_the_flag_nothing_of_it_is_written(tmp_path):
  out = _run(tmp_path, '--algorithm', 'wgan-gp')
  for directory in (out, os.path.join(out, 'validation')):
    events = _events(directory)
    assert len(events) > 1
    assert not any('histogram' in e for e in events)
    assert not any(e.get('tag', '').startswith('plots_') for e in events)
    assert not os.path.exists(os.path.join(directory, 'histograms.jsonl'))
    assert len(events) == 1 + len(_lines(os.path.join(directory,
                                                      'scalars.jsonl')))
