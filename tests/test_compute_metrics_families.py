"""compute_metrics.py with every optional family at once (`cm.REPORTS` and
--victor_purpura), on the run directory of nearest_stretch_cases.run_dir: a
recording of 1500 rows, 12 trials of 256 frames, 24 neurons -- the smallest
fixture on which every family is defined.

The families do not touch each other: the all-flags report holds the eleven
keys in their order, each family's dict is the one of the run with its flag
alone, everything else is the flagless report, and a second `main` on the same
namespace (the kept recorded side of every family at its second use) writes the
same report.  A row of the table reports if and only if its flag was given.

On the device (--batch_trials 5: uneven batches of 5, 5, 2 trials, and of 5, 1
for the halves), with the histograms behind the KL cut on the device and with
CALCIUMGAN_DEVICE_KL=0, the same holds, and the families whose device path is
integer-exact equal the host report: victor_purpura_kl, temporal, states,
triplets, intervals.  spectral and novelty agree with the host to roundings
that tests/test_hip_trace_psd.py and tests/test_hip_nearest_stretch.py derive
and assert; here only their key sets are compared."""
import json

import pytest

import compute_metrics as cm
import nearest_stretch_cases as NC

PLAIN = ['firing_rate_kl', 'correlation_kl', 'van_rossum_heatmap_min',
         'van_rossum_kl']
# flag -> the key it adds, in the order of the keys of spike_metrics.json
FLAGS = {'--victor_purpura': 'victor_purpura_kl',
         '--temporal_metrics': 'temporal', '--spectral_metrics': 'spectral',
         '--novelty_metrics': 'novelty', '--state_metrics': 'states',
         '--triplet_metrics': 'triplets', '--interval_metrics': 'intervals'}
EXACT_ON_DEVICE = ('victor_purpura_kl', 'temporal', 'states', 'triplets',
                   'intervals')
HOST = ('--device', 'cpu', '--num_processors', '1')
DEVICE = ('--device', 'gpu', '--batch_trials', '5')


def _dumps(x):
  return json.dumps(x, sort_keys=True)


def _main(hp):
  """The report of the run's one epoch without `elapse`, the table held to it."""
  report = cm.main(hp)[0]
  del report['elapse']
  for row in cm.REPORTS:
    assert (row.key in report) == getattr(hp, row.flag, False), row.key
  return report


def _report(path, *args):
  hp = cm.build_parser().parse_args(
      ['--output_dir', str(path), '--verbose', '0'] + list(args))
  return hp, _main(hp)


def _check_families(path, device):
  """The three checks of the module docstring; -> (namespace, report) of the
  all-flags run."""
  hp, full = _report(path, *device, *FLAGS)
  assert list(full) == PLAIN + list(FLAGS.values())
  _, plain = _report(path, *device)
  assert list(plain) == PLAIN
  for flag, key in FLAGS.items():
    _, one = _report(path, *device, flag)
    assert list(one) == PLAIN + [key]
    assert _dumps(one.pop(key)) == _dumps(full[key]), key
    assert _dumps(one) == _dumps(plain), key
  again = _main(hp)
  assert list(again) == list(full) and _dumps(again) == _dumps(full)
  return hp, full


@pytest.fixture(scope='module')
def host(tmp_path_factory):
  """(namespace, report) of the all-flags host run, checked."""
  path = tmp_path_factory.mktemp('host')
  NC.run_dir(path)
  return _check_families(path, HOST)


def test_the_families_do_not_touch_each_other_on_the_host(host):
  hp, full = host
  # the table is the flags (all but --victor_purpura, a KL figure) in the order
  # of the report
  assert [('--' + row.flag, row.key) for row in cm.REPORTS] == list(
      FLAGS.items())[1:]
  assert not hasattr(hp, '_recorded_statistics')
  assert not hasattr(hp, '_recorded_statistics_device')
  for key in FLAGS.values():
    assert full[key], key


@pytest.mark.gpu
@pytest.mark.parametrize('device_kl', ['1', '0'])
def test_the_families_do_not_touch_each_other_on_the_device(
    tmp_path, monkeypatch, host, device_kl):
  monkeypatch.setenv('CALCIUMGAN_DEVICE_KL', device_kl)
  NC.run_dir(tmp_path)   # the files of the host run; deconvolved on the device
  hp, full = _check_families(tmp_path, DEVICE)
  assert hasattr(hp, '_recorded_statistics_device') == (device_kl == '1')
  assert hasattr(hp, '_kl_host_fallbacks') == (device_kl == '1')
  assert hasattr(hp, '_recorded_statistics') == (device_kl == '0')
  for key in EXACT_ON_DEVICE:
    assert _dumps(full[key]) == _dumps(host[1][key]), key
  for key in ('spectral', 'novelty'):
    assert _dumps(sorted(full[key])) == _dumps(sorted(host[1][key])), key
