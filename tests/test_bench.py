"""bench.py's own contract: a plain run times only the headline, --steps sets
the timed steps, and --dump-outputs writes what the last timed step computed,
identically from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Model(object):

  def __init__(self, name, weights):
    self.name = name
    self._weights = weights

  def get_weights(self):
    return [w.copy() for w in self._weights]


class _Gan(object):

  def __init__(self, rng):
    self.generator = _Model('generator', [
        rng.standard_normal((32, 4096)).astype(np.float32),
        rng.standard_normal(7).astype(np.float32)])
    self.discriminator = _Model('discriminator', [
        rng.standard_normal((24, 16, 64)).astype(np.float32)])


def _out():
  from calciumgan_amd.gan.algorithms import wgan_gp as _w
  return (torch.tensor(1.5), torch.tensor(-2.0), torch.tensor(0.25),
          {k: torch.tensor(float(i)) for i, k in enumerate(_w._METRIC_KEYS)})


def _load(path):
  return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_names_dtypes_and_size_cap(tmp_path, monkeypatch):
  import bench
  gan = _Gan(np.random.RandomState(3))
  bench.dump_outputs(str(tmp_path / 'whole'), gan, _out())
  got = _load(str(tmp_path / 'whole'))
  assert sorted(got) == sorted(
      ['gen_loss', 'dis_loss', 'gradient_penalty', 'signals_metrics_min',
       'signals_metrics_max', 'signals_metrics_mean', 'signals_metrics_std',
       'generator_w00', 'generator_w01', 'discriminator_w00'])
  assert all(a.dtype == np.float32 for a in got.values())
  assert float(got['gen_loss']) == 1.5 and float(got['gradient_penalty']) == 0.25
  np.testing.assert_array_equal(got['generator_w00'],
                                gan.generator.get_weights()[0])
  # past the cap: a seeded sample of every array, the same one every time
  limit = 64 << 10
  monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', limit)
  for d in ('a', 'b'):
    bench.dump_outputs(str(tmp_path / d), gan, _out())
  a, b = _load(str(tmp_path / 'a')), _load(str(tmp_path / 'b'))
  assert sum(os.path.getsize(str(tmp_path / 'a' / f))
             for f in os.listdir(str(tmp_path / 'a'))) <= limit
  assert sorted(a) == sorted(got)
  for k in got:
    np.testing.assert_array_equal(a[k], b[k])
  assert float(a['dis_loss']) == -2.0
  w = gan.generator.get_weights()[0].reshape(-1)
  assert 0 < a['generator_w00'].size < w.size
  assert np.isin(a['generator_w00'], w).all()


def _bench(out_dir, steps):
  env = dict(os.environ)
  env.pop('CALCIUMGAN_AUTOTUNE', None)  # the shipped default: static tiles
  env.pop('CALCIUMGAN_TILE_CACHE', None)
  out = subprocess.run(
      [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
       '--steps', str(steps), '--warmup', '2', '--seq_len', '256',
       '--neurons', '16', '--batch', '8', '--dump-outputs', out_dir],
      env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert out.returncode == 0, out.stderr[-2000:]
  lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
  assert len(lines) == 1, out.stdout[-2000:]
  return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_identical_outputs(tmp_path):
  """Two plain runs with the same arguments: the headline fields, no roofline
  or CPU-baseline leg, and bit-identical dumps whose losses are the line's."""
  a = _bench(str(tmp_path / 'a'), 3)
  b = _bench(str(tmp_path / 'b'), 3)
  for rec in (a, b):
    assert rec['steps'] == 3 and rec['warmup'] == 2
    assert rec['ms_per_step'] > 0 and rec['value'] > 0
    assert rec['unit'] == 'samples/s' and rec['higher_is_better'] is True
    assert rec['dtype'] == 'bf16'
    assert rec['roofline'] is None and rec['cpu_baseline'] is None
  da, db = _load(str(tmp_path / 'a')), _load(str(tmp_path / 'b'))
  assert sorted(da) == sorted(db) and 'generator_w00' in da
  for k in da:
    assert da[k].dtype == np.float32
    np.testing.assert_array_equal(da[k], db[k], err_msg=k)
  assert [float(da[k]) for k in ('gen_loss', 'dis_loss', 'gradient_penalty')
         ] == a['final_losses']
