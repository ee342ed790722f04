"""The wave reductions and block folds of the kernel library keep their bits.

tests/golden/reduce_bits.npz holds the raw output bits of every entry point
whose kernel ends in a wave reduction and a fold of the waves' LDS slots,
recorded (tests/make_golden_reduce_bits.py) from the libraries of the commit
before the folds were stated once in cg_common.h (block_fold_put /
block_fold_get), and since the output tails of the MFMA kernels were given
shared helpers also the bits of every cg_swconv tail and cg_wgrad reduction
(groups conv_tails, wgrad_tails), recorded from that change's parent; the
commit's hash is in the file.  The same calls on the same seeded
inputs must give the same bits from this tree's libraries, in both precision
builds: the order of every sum, minimum and maximum is unchanged."""
import os

import numpy as np
import pytest

import make_golden_reduce_bits as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
  return G.load()


@pytest.fixture(scope='module')
def recorded(golden):
  return golden[0]


@pytest.fixture(scope='module')
def computed():
  try:
    return G.compute()
  finally:
    G._lib.use('bf16')


def test_the_fixture_names_its_commit(golden):
  commit = golden[1]
  assert len(commit) == 40 and set(commit) <= set('0123456789abcdef'), commit
  assert os.path.getsize(G.OUT) < 128 * 1024


def test_the_same_cases(recorded, computed):
  assert sorted(recorded) == sorted(computed)
  # every family of the issue's list is there, in both builds where it reads
  # activations
  for pre, family in [('bf16', f) for f in (
      'gp_finalize+critic_loss', 'gp_critic_loss', 'neg_mean', 'gp_loss_scale',
      'rownorm', 'dense1', 'dense1_bce', 'colsum', 'colsum_deferred',
      'signal_metrics', 'spike_stats_error', 'tensor_summary', 'pair_histogram',
      'conv_tails', 'wgrad_tails')
                     ] + [('f16', f) for f in (
                         'gp_loss_scale', 'rownorm', 'dense1', 'dense1_bce', 'colsum',
                         'colsum_deferred', 'conv_tails', 'wgrad_tails')]:
    assert any(k.startswith('{}/{}/'.format(pre, family)) for k in computed), (
        pre, family)


def test_every_output_keeps_its_bits(recorded, computed):
  bad = []
  for name, got in sorted(computed.items()):
    want = recorded[name]
    if got.dtype != want.dtype or got.shape != want.shape or not np.array_equal(
        got, want):
      where = (np.flatnonzero(got != want)[:4].tolist()
               if got.shape == want.shape else 'shape')
      bad.append((name, where))
  assert not bad, '{} of {} outputs differ: {}'.format(len(bad), len(computed),
                                                      bad[:8])
