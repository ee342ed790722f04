#!/usr/bin/env python
"""Post-hoc spike statistics of generated vs recorded signals -- the numbers of
the reference's compute_metrics.py (BASELINE configs[3]: recorded-data pipeline
+ OASIS deconvolution metrics), without its plots:

  deconvolve the generated calcium signals (OASIS AR(1), stored back into the
  generated file as `spikes`)                          compute_metrics.py:35-57
  firing rate per neuron over the trials, KL(recorded || synthetic)    :210-262
  pairwise correlation coefficients per trial, KL                      :306-358
  van Rossum distances between the neurons of a trial, KL; recorded x
  synthetic distance heatmaps for the chosen neurons                   :361-480
  (covariance KL: defined :265-303 but not called by the reference's main; same
  here)

  python compute_metrics.py --output_dir runs/001 [--all_epochs]
      [--device gpu [--batch_trials 128]] [--victor_purpura [--vp_q 1.0]]
      [--temporal_metrics [--max_lag 24]] [--spectral_metrics]
      [--novelty_metrics [--novelty_step 2]]
      [--state_metrics [--state_k 5] [--state_bin 12]]
      [--triplet_metrics [--triplet_bin 12]]
      [--interval_metrics [--max_isi 240]]

--device gpu (not a reference flag) takes the deconvolution, the firing rates,
the per-trial correlations and the van Rossum matrices through the HIP kernels
(csrc/spikes.hip, csrc/van_rossum.hip) in batches of --batch_trials trials: the
spike trains written back are the host's byte for byte, the firing rates equal,
correlations and distances equal to float64 rounding (a value within that of a
histogram edge may change bins in the KL).  The per-trial matrices stay on the
device: cg_pair_histogram (csrc/pair_hist.hip) cuts every pair of upper
triangles into the bins pandas.cut would give them, and only the integer counts
come to the host, where the KL's thirty float32 operations a pair and the
heatmap ordering stay (CALCIUMGAN_DEVICE_KL=0: the matrices come to the host and
pandas cuts them, as before; the same report).  No process pool is created on
that path (--num_processors is ignored): a pool forked after the GPU is open is
not safe.

--victor_purpura (not a reference flag either; absent from the namespace unless
given) adds `victor_purpura_kl`, built exactly as `van_rossum_kl` from the
Victor-Purpura distances (cost --vp_q per second of shift) between the neurons
of a trial: spike_metrics.victor_purpura_distance_frames on the host,
cg_victor_purpura (csrc/victor_purpura.hip) on the device.  The two hold the
same bits, so both devices report the same figure.  Without the flag nothing is
computed or written beyond what was before.

--temporal_metrics [--max_lag 24] (not reference flags, absent from the namespace
unless given) adds `temporal`: spike_metrics.temporal_scores of the generated
file against the validation cache over the first num_samples trials of each --
autocorrelograms, lag-1 covariances, cross-correlograms up to --max_lag frames
and the population-count histogram, the time-axis panels of Spike-GAN's figure
3.  Both come from integer totals: spike_metrics.temporal_totals on the host,
cg_spike_ccg and cg_spike_population_hist (csrc/spike_ccg.hip) on the device in
batches of --batch_trials, the recorded side's kept across epochs; only the
totals come to the host and both devices write the same dict.

--spectral_metrics (not a reference flag, absent from the namespace unless
given) adds `spectral`: signals_metrics.spectral_scores of the generated file's
calcium traces against the validation cache's over the first num_samples trials
of `signals` in each -- the per-neuron power spectrum (mean removed, Hann
window) averaged over trials: log-spectral distance, power ratios in total and
per octave band, the peaks at the periods T / 2, T / 4, ... that stride-2
transposed convolutions leave, and the spectral centroid.  The only figures of
the report that look at the traces before deconvolution.  Both come from
float64 totals: signals_metrics.spectral_totals on the host (a float64
transform), cg_trace_psd (csrc/trace_psd.hip) on the device in batches of
--batch_trials (a float32 transform), the recorded side's kept across epochs.
Unlike `temporal`, the two devices' dicts agree to the rounding of a float32
transform (about 1e-6 dB), not bit for bit.

--novelty_metrics [--novelty_step k] (not reference flags, absent from the
namespace unless given) adds `novelty`: signals_metrics.novelty_scores.  Every
other figure of the report is best for a generator that plays stretches of the
training recording back; this one tells such a copy from a generator that has
learned the distribution.  It needs the run's input_dir (hparams.json) to be a
recording directory (data/recording.py: info['recording']) and raises a
ValueError for anything else.  For the first num_samples trials of `signals` of
the generated file, the squared distance to the nearest stretch of the recording
(raw units, which are the units of the generated files) on the grid of
--novelty_step rows (default: the dataset's stride), no offset excluded; for
num_samples stretches of the recording itself, spread evenly over the grid, the
same with the offsets that overlap the stretch excluded -- computed once and kept
across epochs.  The report holds both as RMS distances per sample, their ratio,
the share of generated trials below the recorded minimum (`copied_fraction`) and
median, and the share of distinct nearest offsets.  signals_metrics.
nearest_stretch(expanded=True) on the host (a float64 matmul against a strided
view of the recording), cg_nearest_stretch (csrc/nearest_stretch.hip: float64
MFMA, the recording's rows staged in LDS, no window materialised) on the device
in batches of --batch_trials with the recording uploaded once.  The two devices
agree to float64 summation rounding, not bit for bit; an index may differ where
two stretches lie that close to each other.

--state_metrics [--state_k 5] [--state_bin 12] (not reference flags, absent from
the namespace unless given) adds `states`: the only figures that ask of single
samples whether each generated one is something the data contains (precision)
and whether everything the data contains is generated (recall, coverage).  The
sample is a population state, the spike counts of all neurons in one bin of
--state_bin frames; the ball of a state reaches to its --state_k-th nearest
other state of its own set (spike_metrics.state_scores).  The recorded trials 0,
2, 4, ... of the first num_samples are the reference set; `generated` scores the
generated trials 1, 3, 5, ... against it and `floor` the recorded trials 1, 3,
5, ...: the figures depend on the set sizes and two draws of one distribution
do not score 1, so each is read beside its floor (computed once, kept across
epochs).  On a recording dataset the validation windows overlap in time, so
the floor there is optimistic.  spike_metrics.state_neighbours on the host,
cg_population_states and cg_state_neighbours (csrc/state_neighbours.hip: the
products on the matrix pipe, the k smallest of every row selected in registers,
no distance matrix in memory) on the device in batches of --batch_trials.  All
distances are exact integers on both, so both devices write the same dict.

--triplet_metrics [--triplet_bin 12] (not reference flags, absent from the
namespace unless given) adds `triplets`: the only figures past the second
order.  A dichotomised-Gaussian twin of a recording matches every rate and every
pairwise covariance by construction; what a generator can have that the twin
cannot is structure beyond pairs, and these figures measure it.  The states are
binary (did the neuron fire in a bin of --triplet_bin frames); kappa_ijk is the
connected third-order correlation of a neuron triplet and the figures compare
it, over all C(C,3) triplets, between the sides (spike_metrics.triplet_scores).
`generated`, `floor` and the trials they are taken from are --state_metrics'.
spike_metrics.triplet_counts on the host; on the device cg_binary_words packs
the states 32 to a word in batches of --batch_trials and cg_triplet_counts
(csrc/triplets.hip: AND and popcount, exact with no bound on the counts) counts
a side in one call.  Only integers come to the host, so both devices write the
same dict.

--interval_metrics [--max_isi 240] (not reference flags, absent from the
namespace unless given) adds `intervals`: the inter-spike-interval histogram of
every neuron (bins of 1 .. --max_isi frames and one overflow bin), its
coefficient of variation and the serial correlation of consecutive intervals,
and across trials the Fano factor of the spike count and the count ("noise")
correlations of neuron pairs (spike_metrics.interval_scores).  The
autocorrelogram of --temporal_metrics stops at --max_lag frames, short of most
intervals; every covariance above is taken within a trial, so a generator whose
trials all carry the expected count passes them.  `generated`, `floor` and the
trials they are taken from are --state_metrics'.  spike_metrics.interval_counts
on the host; on the device cg_binary_words at bin 1 packs the frames 32 to a
word in batches of --batch_trials and cg_spike_intervals
(csrc/spike_intervals.hip) counts a side in one call.  Only integers come to
the host, so both devices write the same dict.

The KL is the reference's: both samples cut into 30 equal-width bins over their
pooled range by pandas.cut, empty bins replaced by 1e-10 (:80-111) -- pandas is
the same library here, so that step is shared, not restated.  Elephant / Neo /
OASIS are absent and un-pinned upstream (PARITY UNPINNED); the statistics come
from gan/utils/spike_metrics.py and csrc/oasis_ar1.c.  Results go to
<output_dir>/spike_metrics.json and, as the reference does, 'elapse/spike_metrics'
to the scalar log.
"""
import argparse
import collections
import json
import multiprocessing
import os
import pickle
import random
from time import time

import numpy as np
import pandas as pd

from calciumgan_amd.gan.utils import (h5_helper, signals_metrics, spike_helper,
                                      spike_metrics, utils)

NUM_BINS = 30  # compute_metrics.py:96
# What an option that is absent from the namespace reads as (`option`; the
# parser's help texts quote these).  --novelty_step falls back to the dataset's
# stride, which `novelty_recording` hands to `option`.
DEFAULTS = dict(
    batch_trials=128,  # --device gpu: trials per launch
    vp_q=1.0,          # --victor_purpura: cost per second of shift
    max_lag=24,        # --temporal_metrics: one second of frames
    state_k=5, state_bin=12,  # --state_metrics (500 ms of frames)
    triplet_bin=12,    # --triplet_metrics (500 ms of frames)
    max_isi=240)       # --interval_metrics (10 s of frames)


def option(hparams, name, default=None):
  """hparams.<name>, or the default of an option that was not given."""
  return getattr(hparams, name, DEFAULTS.get(name, default))


def kept(hparams, name, make):
  """hparams.<name>, made on first use and kept across epochs: the validation
  set and the recording are the same for every epoch."""
  if getattr(hparams, name, None) is None:
    setattr(hparams, name, make())
  return getattr(hparams, name)


def same_frames(filename, frames, recorded_frames):
  """A file whose trials are not as long as the validation cache's is refused."""
  if frames != recorded_frames:
    raise ValueError('{} holds trials of {} frames, the validation cache of {}'
                     .format(filename, frames, recorded_frames))


def kl_divergence(p, q):
  """compute_metrics.py:80-84."""
  p = np.where(p == 0, 1e-10, p)
  q = np.where(q == 0, 1e-10, q)
  return np.sum(p * np.log(p / q))


def pairs_kl_divergence(pairs):
  """compute_metrics.py:87-111: per (recorded, synthetic) pair the KL of their
  histograms over NUM_BINS equal-width bins of the pooled values."""
  kl = np.zeros((len(pairs),), dtype=np.float32)
  for i, (real, fake) in enumerate(pairs):
    real, fake = np.asarray(real), np.asarray(fake)
    pooled = np.concatenate([real, fake])
    bins = np.asarray(pd.cut(pooled, bins=NUM_BINS, labels=np.arange(NUM_BINS)))
    is_real = np.arange(len(pooled)) < len(real)
    real_pdf = np.array([np.sum(bins[is_real] == b) for b in range(NUM_BINS)],
                        dtype=np.float32) / len(real)
    fake_pdf = np.array([np.sum(bins[~is_real] == b) for b in range(NUM_BINS)],
                        dtype=np.float32) / len(fake)
    kl[i] = kl_divergence(real_pdf, fake_pdf)
  return kl


def kl_from_counts(real_counts, fake_counts, n_real, n_fake):
  """The tail of `pairs_kl_divergence` for one pair: from the NUM_BINS integer
  bin counts of either sample and the sample sizes the same float32 it stores
  (counts as float32 divided by the size, then `kl_divergence`)."""
  real_pdf = np.asarray(real_counts).astype(np.float32) / int(n_real)
  fake_pdf = np.asarray(fake_counts).astype(np.float32) / int(n_fake)
  return np.float32(kl_divergence(real_pdf, fake_pdf))


def _spikes(hparams, filename, data_format, neuron=None, trial=None,
            num_trials=None):
  """get_neo_trains (:60-74) up to the Neo conversion: a 2-D {0,1} array in
  `data_format` ('NW' for one neuron over trials, 'CW' for one trial)."""
  assert data_format and (neuron is not None or trial is not None)
  spikes = h5_helper.get(filename, name='spikes', neuron=neuron, trial=trial)
  spikes = utils.set_array_format(np.asarray(spikes), data_format, hparams)
  if num_trials is not None:
    assert data_format[0] == 'N'
    spikes = spikes[:num_trials]
  return spikes.astype(np.float32)


def _deconvolve_neuron(hparams, filename, neuron):
  signals = h5_helper.get(filename, name='signals', neuron=neuron)
  signals = utils.set_array_format(np.asarray(signals), 'NW', hparams)
  return spike_helper.deconvolve_signals(signals, threshold=0.5)


def deconvolve_from_file(hparams, filename):
  """compute_metrics.py:42-57: spikes of every neuron of the generated set,
  stored as int8 NWC beside the signals."""
  if hparams.verbose:
    print('\tDeconvolve {}'.format(filename))
  per_neuron = _map(hparams, _deconvolve_neuron,
                    [(hparams, filename, n) for n in range(hparams.num_neurons)])
  spikes = utils.set_array_format(np.array(per_neuron, dtype=np.int8), 'NWC',
                                  hparams)
  h5_helper.write(filename, {'spikes': spikes})
  return spikes


def firing_rate(hparams, filename, neuron, num_trials=200):
  """:210-232: (recorded, synthetic) firing rates of one neuron, one value per
  trial."""
  real = _spikes(hparams, hparams.validation_cache, 'NW', neuron=neuron,
                 num_trials=num_trials)
  fake = _spikes(hparams, filename, 'NW', neuron=neuron, num_trials=num_trials)
  return (spike_metrics.mean_firing_rate(real),
          spike_metrics.mean_firing_rate(fake))


def _upper(matrix, n):
  return utils.remove_nan(np.asarray(matrix)[np.triu_indices(n, k=1)])


def covariance(hparams, filename, trial):
  """:265-281."""
  n = hparams.num_neurons
  return tuple(_upper(spike_metrics.covariance(_spikes(hparams, f, 'CW',
                                                       trial=trial)), n)
               for f in (hparams.validation_cache, filename))


def correlation_coefficient(hparams, filename, trial):
  """:306-324."""
  n = hparams.num_neurons
  return tuple(
      _upper(spike_metrics.correlation_coefficients(
          _spikes(hparams, f, 'CW', trial=trial)), n)
      for f in (hparams.validation_cache, filename))


def trial_van_rossum(hparams, filename, trial):
  """:415-443: distances between the neurons of one trial, upper triangle."""
  out = []
  for f in (hparams.validation_cache, filename):
    d = spike_metrics.van_rossum_distance(_spikes(hparams, f, 'CW', trial=trial))
    out.append(d[np.triu_indices(len(d), k=1)])
  assert out[0].shape == out[1].shape
  return tuple(out)


def trial_victor_purpura(hparams, filename, trial):
  """`trial_van_rossum` for the Victor-Purpura distances (--victor_purpura)."""
  out = []
  for f in (hparams.validation_cache, filename):
    d = spike_metrics.victor_purpura_distance_frames(
        _spikes(hparams, f, 'CW', trial=trial), q=option(hparams, 'vp_q'))
    out.append(d[np.triu_indices(len(d), k=1)])
  assert out[0].shape == out[1].shape
  return tuple(out)


def sort_heatmap(matrix):
  """:361-386: rows / columns reordered so that the minimum sits top left --
  columns by the row holding the global minimum, then for every column in turn
  the not-yet-used row that is smallest there."""
  matrix = np.asarray(matrix, dtype=np.float32)
  n = len(matrix)
  work = matrix.copy()
  first_row = np.unravel_index(np.argmin(matrix), matrix.shape)[0]
  column_order = np.argsort(matrix[first_row])
  row_order = np.full((n,), -1, dtype=np.int64)
  heatmap = np.full(matrix.shape, np.nan, dtype=np.float32)
  for i in range(n):
    row_order[i] = first_row if i == 0 else np.argsort(work[:, column_order[i]])[0]
    heatmap[i] = matrix[row_order[i]][column_order]
    work[row_order[i], :] = np.inf
  return heatmap, row_order, column_order


def neuron_van_rossum(hparams, filename, neuron, num_trials=50):
  """:389-412: recorded x synthetic distances of one neuron's first trials."""
  real = _spikes(hparams, hparams.validation_cache, 'NW', neuron=neuron,
                 num_trials=num_trials)
  fake = _spikes(hparams, filename, 'NW', neuron=neuron, num_trials=num_trials)
  heatmap, rows, cols = sort_heatmap(
      spike_metrics.van_rossum_distance(real, fake))
  return dict(heatmap=heatmap, xticklabels=rows, yticklabels=cols)


def _map(hparams, fn, args):
  """pool.starmap of the reference (one pool per metric, :45,:240,...)."""
  if getattr(hparams, 'num_processors', 1) > 1 and len(args) > 1:
    with multiprocessing.Pool(hparams.num_processors) as pool:
      return pool.starmap(fn, args)
  return [fn(*a) for a in args]


def _trials(hparams, filename, name='spikes', count=None):
  """The first `count` (num_samples) trials of dataset `name` of `filename` as
  an NWC host array."""
  trials = utils.set_array_format(
      np.asarray(h5_helper.get(filename, name=name)), 'NWC', hparams)
  return trials[:hparams.num_samples if count is None else count]


def _trial_signals(hparams, filename):
  """The first num_samples trials of `signals` of `filename`, float32."""
  return np.asarray(_trials(hparams, filename, 'signals'), dtype=np.float32)


def _print_scores(hparams, scores, labels):
  if hparams.verbose:
    for name, label in labels:
      print('\t{}: {:.04g}'.format(label, scores[name]))
  return scores


def _totals_report(hparams, filename, totals, kept_as, scores, labels):
  """The skeleton of the reports that come from totals over the trials:
  scores(recorded totals, generated totals, T) of `filename` against the
  validation cache; totals(hparams, filename) -> (totals, T), the recorded
  side's kept across epochs as hparams.<kept_as>."""
  real = kept(hparams, kept_as,
              lambda: totals(hparams, hparams.validation_cache))
  fake = totals(hparams, filename)
  same_frames(filename, fake[1], real[1])
  return _print_scores(hparams, scores(real[0], fake[0], real[1]), labels)


def temporal_totals_host(hparams, filename):
  """(spike_metrics.temporal_totals, T) of the trials of `filename`."""
  spikes = _trials(hparams, filename)
  return spike_metrics.temporal_totals(
      spikes, option(hparams, 'max_lag')), spikes.shape[1]


def temporal_report(hparams, filename, totals):
  """--temporal_metrics: spike_metrics.temporal_scores of `filename` against
  the validation cache; totals(hparams, filename) -> ((ccg, hist, trials), T),
  the recorded side's kept across epochs."""
  return _totals_report(
      hparams, filename, totals, '_recorded_temporal_totals',
      spike_metrics.temporal_scores,
      (('autocorrelogram_mae', 'autocorrelogram    MAE'),
       ('lag_covariance_mae', 'lag-1 covariance   MAE'),
       ('lag_covariance_correlation', 'lag-1 covariance     r'),
       ('cross_correlogram_mae', 'cross-correlogram  MAE'),
       ('population_count_js_bits', 'population count    JS')))


def spectral_totals_host(hparams, filename):
  """(signals_metrics.spectral_totals, T) of the trials of `filename`."""
  signals = _trial_signals(hparams, filename)
  return signals_metrics.spectral_totals(signals), signals.shape[1]


def spectral_report(hparams, filename, totals):
  """--spectral_metrics: signals_metrics.spectral_scores of `filename` against
  the validation cache; totals(hparams, filename) -> ((totals, trials), T), the
  recorded side's kept across epochs."""
  return _totals_report(
      hparams, filename, totals, '_recorded_spectral_totals',
      signals_metrics.spectral_scores,
      (('log_spectral_distance_db', 'log-spectral dist.  dB'),
       ('log_spectral_rmse_db', 'log-spectral RMSE   dB'),
       ('total_power_ratio_db', 'total power ratio   dB')))


def novelty_recording(hparams):
  """--novelty_metrics: (raw (T_raw, C) float32, L, step) of the recording the
  run was trained on, in raw units -- the units of the generated files
  (utils.save_fake_signals denormalises, and for an FFT recording the files
  hold traces).  Kept across epochs."""
  def load():
    from calciumgan_amd.data import recording
    input_dir = getattr(hparams, 'input_dir', None)
    info = None
    if input_dir and os.path.exists(os.path.join(input_dir, 'info.pkl')):
      with open(os.path.join(input_dir, 'info.pkl'), 'rb') as f:
        info = pickle.load(f)
    if not (info and info.get('recording') and
            os.path.exists(os.path.join(input_dir, recording.FILENAME))):
      raise ValueError(
          '--novelty_metrics needs the run\'s input_dir to be a recording '
          'directory (info[\'recording\'], {}); {!r} is not one'.format(
              recording.FILENAME, input_dir))
    raw = np.ascontiguousarray(recording.load(input_dir)['raw'],
                               dtype=np.float32)
    step = int(option(hparams, 'novelty_step', info['stride']))
    if step < 1:
      raise ValueError('--novelty_step must be at least 1')
    return raw, int(info['sequence_length']), step

  return kept(hparams, '_novelty_recording', load)


def novelty_nearest_host(hparams, queries, exclude, exclude_len):
  """(nearest, index) of float32 host trials: the expanded form on the host."""
  raw, _, step = novelty_recording(hparams)
  return signals_metrics.nearest_stretch(queries, raw, step, exclude,
                                         exclude_len, expanded=True)


def novelty_report(hparams, filename, nearest):
  """--novelty_metrics: signals_metrics.novelty_scores of the first num_samples
  trials of `filename` against num_samples stretches of the recording itself,
  each with the offsets that overlap it excluded; nearest(hparams, queries,
  exclude, exclude_len) -> (nearest, index), the recorded side's kept across
  epochs."""
  raw, L, step = novelty_recording(hparams)
  C = raw.shape[1]
  S = signals_metrics.stretch_offsets(len(raw), L, step)
  frames, neurons = np.shape(h5_helper.get(filename, name='signals', trial=0))
  if frames != L or neurons != C:
    raise ValueError('{} holds trials of {} frames of {} neurons, the recording '
                     'stretches of {} of {}'.format(filename, frames, neurons,
                                                    L, C))
  fake = _trial_signals(hparams, filename)

  def recorded():
    starts = signals_metrics.recorded_starts(S, hparams.num_samples, step)
    windows = np.lib.stride_tricks.sliding_window_view(raw, L, axis=0)
    queries = windows[starts].transpose(0, 2, 1)   # (n, L, C) views of raw
    return tuple(signals_metrics._host(x)
                 for x in nearest(hparams, queries, starts, L))

  real = kept(hparams, '_recorded_novelty', recorded)
  got = tuple(signals_metrics._host(x) for x in nearest(hparams, fake, None, 0))
  return _print_scores(
      hparams, signals_metrics.novelty_scores(real, got, L, C, step, offsets=S),
      (('nearest_rms_ratio', 'nearest rms    gen / rec'),
       ('copied_fraction', 'copied fraction        '),
       ('distinct_stretches', 'distinct stretches     ')))


def _floor_report(hparams, filename, kept_as, sets, scores, line, names,
                  settings, prepare=lambda ref: (), check_recorded=None,
                  check_generated=None):
  """The skeleton of the reports that read the generated trials beside a floor.
  With ref = sets(hparams, the recorded trials 0, 2, 4, ...), `generated` is
  scores(ref, sets(hparams, the generated trials 1, 3, 5, ...), *prepare(ref))
  and `floor` the same of the recorded trials 1, 3, 5, ...: what two draws of
  the data score at these sizes.  The recorded side (ref, *prepare(ref), floor,
  frames) is kept across epochs as hparams.<kept_as>.  check_recorded and
  check_generated(trials) are the family's own refusals; `line` prints name,
  generated[key], floor[key] of `names`; `settings` joins the returned dict."""
  fake = _trials(hparams, filename)

  def recorded():
    spikes = _trials(hparams, hparams.validation_cache)
    if check_recorded is not None:
      check_recorded(spikes)
    ref = sets(hparams, spikes[0::2])
    more = prepare(ref)
    floor = scores(ref, sets(hparams, spikes[1::2]), *more)
    return (ref,) + more + (floor, spikes.shape[1])

  ref, *more, floor, frames = kept(hparams, kept_as, recorded)
  same_frames(filename, fake.shape[1], frames)
  if check_generated is not None:
    check_generated(fake)
  generated = scores(ref, sets(hparams, fake[1::2]), *more)
  if hparams.verbose:
    for name, key in names:
      print(line.format(name, generated[key], floor[key]))
  return dict(generated=generated, floor=floor, **settings)


def state_sets_host(hparams, spikes):
  """The states of an NWC host array of trials as spike_metrics.state_neighbours
  takes them."""
  return spike_metrics.population_states(spikes, option(hparams, 'state_bin'))


def state_report(hparams, filename, states, neighbours):
  """--state_metrics: `_floor_report` of spike_metrics.state_scores of the
  population states.  states(hparams, trials) -> a set, neighbours the query on
  such sets; the radii of the reference set are kept with it."""
  k = int(option(hparams, 'state_k'))
  return _floor_report(
      hparams, filename, '_recorded_states', states,
      lambda ref, other, rad_ref: spike_metrics.state_scores(
          ref, other, k, neighbours, rad_ref=rad_ref),
      '\tstate {:<9}  gen | floor: {:.04f} | {:.04f}',
      [(name, name) for name in ('precision', 'recall', 'coverage')],
      dict(k=k, bin_frames=int(option(hparams, 'state_bin'))),
      prepare=lambda ref: (spike_metrics.state_radii(ref, k, neighbours),))


def triplet_sets_host(hparams, spikes):
  """(singles, pairs, triplets, S) of an NWC host array of trials: the side
  spike_metrics.triplet_scores takes."""
  states = spike_metrics.binary_states(spikes, option(hparams, 'triplet_bin'))
  return spike_metrics.triplet_counts(states) + (len(states),)


def triplet_report(hparams, filename, sets):
  """--triplet_metrics: `_floor_report` of spike_metrics.triplet_scores of the
  binary states.  sets(hparams, trials) -> a side (singles, pairs, triplets,
  S), host integers."""
  bin = int(option(hparams, 'triplet_bin'))

  def check(spikes):
    if spikes.shape[2] < 3:
      raise ValueError('--triplet_metrics needs three neurons, not {}'.format(
          spikes.shape[2]))
    if spikes.shape[1] < bin:
      raise ValueError('trials of {} frames hold no bin of {}'.format(
          spikes.shape[1], bin))

  return _floor_report(
      hparams, filename, '_recorded_triplets', sets,
      spike_metrics.triplet_scores,
      '\ttriplet cumulant {:<11}  gen | floor: {:.06f} | {:.06f}',
      [(name, 'triplet_cumulant_' + name) for name in ('correlation', 'mae')],
      dict(bin_frames=bin), check_recorded=check)


def interval_sets_host(hparams, spikes):
  """(hist, moments, counts) of an NWC host array of trials: the side
  spike_metrics.interval_scores takes."""
  return spike_metrics.interval_counts(spikes, option(hparams, 'max_isi'))


def interval_report(hparams, filename, sets):
  """--interval_metrics: `_floor_report` of spike_metrics.interval_scores.
  sets(hparams, trials) -> a side (hist, moments, counts), host integers."""
  def check(trials, holder='the validation cache'):
    if len(trials[1::2]) < 2:
      raise ValueError('--interval_metrics needs two trials a side, {} holds {} '
                       'in all'.format(holder, len(trials)))

  return _floor_report(
      hparams, filename, '_recorded_intervals', sets,
      spike_metrics.interval_scores,
      '\tinterval {:<12}  gen | floor: {:.06f} | {:.06f}',
      [(name, name) for name in ('cv_mae', 'isi_js_bits', 'fano_mae')],
      dict(max_isi=int(option(hparams, 'max_isi'))), check_recorded=check,
      check_generated=lambda fake: check(fake, filename))


def host_kl(hparams, filename):
  """name -> callable giving the float32 KL per pair behind each figure of the
  host report (`device_kl` is its counterpart): per neuron the firing rates
  over the trials, per trial the upper triangles of the matrices between its
  neurons, each through a pool of its own."""
  trials = [(hparams, filename, i) for i in range(hparams.num_samples)]
  figures = dict(firing_rate=lambda: pairs_kl_divergence(_map(
      hparams, firing_rate, [(hparams, filename, n, hparams.num_samples)
                             for n in range(hparams.num_neurons)])))
  per_trial = dict(correlation=correlation_coefficient,
                   van_rossum=trial_van_rossum)
  if getattr(hparams, 'victor_purpura', False):
    per_trial['victor_purpura'] = trial_victor_purpura
  for name, fn in per_trial.items():
    figures[name] = lambda fn=fn: pairs_kl_divergence(_map(hparams, fn, trials))
  return figures


def heatmap_minima_host(hparams, filename):
  """The least distance of the heat map of every chosen neuron."""
  heat = _map(hparams, neuron_van_rossum,
              [(hparams, filename, n, 45) for n in hparams.neurons])
  return [np.nanmin(h['heatmap']) for h in heat]


# -- --device gpu ---------------------------------------------------------------
def _device():
  import torch
  return torch.device('cuda', torch.cuda.current_device())


def _batches(hparams, array):
  """float32 device tensors of `batch_trials` trials of an NWC host array."""
  import torch
  step = max(int(option(hparams, 'batch_trials')), 1)
  for i in range(0, len(array), step):
    yield torch.from_numpy(
        np.ascontiguousarray(array[i:i + step], dtype=np.float32)).to(_device())


def deconvolve_from_file_device(hparams, filename):
  """`deconvolve_from_file` through cg_oasis_ar1_batched, a batch of trials per
  launch, scale 1 and offset 0: the float32 signals of the file widened to
  float64 as the host does, so the int8 trains are the host's byte for byte."""
  if hparams.verbose:
    print('\tDeconvolve {}'.format(filename))
  signals = np.asarray(h5_helper.get(filename, name='signals'))
  if signals.dtype != np.float32:
    raise ValueError('--device gpu deconvolves float32 signals; {} holds {}'
                     .format(filename, signals.dtype))
  signals = utils.set_array_format(signals, 'NWC', hparams)
  spikes = np.concatenate([
      spike_helper.deconvolve_signals_device(batch, threshold=0.5).cpu().numpy()
      for batch in _batches(hparams, signals)]).astype(np.int8)
  h5_helper.write(filename, {'spikes': spikes})
  return spikes


def trial_statistics_device(hparams, filename, matrices_on_device=False):
  """Of the first num_samples trials of `filename`, on the device: firing rates
  (n, C) float32 (cg_spike_stats), correlation coefficients and van Rossum
  distances between the trial's neurons (n, C, C) float64 (cg_spike_corrcoef,
  cg_van_rossum), brought to the host; with --victor_purpura the Victor-Purpura
  distances (cg_victor_purpura) as well.  matrices_on_device: the (n, C, C)
  matrices stay device tensors (the firing rates come to the host either way)."""
  import torch
  rates, corr, dist, vp = [], [], [], []
  for batch in _batches(hparams, _trials(hparams, filename)):
    rates.append(spike_metrics.batch_statistics_device(batch)[0].cpu().numpy())
    corr.append(spike_metrics.correlation_coefficients_device(batch))
    dist.append(spike_metrics.van_rossum_distance_device(batch))
    if getattr(hparams, 'victor_purpura', False):
      vp.append(spike_metrics.victor_purpura_distance_device(
          batch, q=option(hparams, 'vp_q')))
    if not matrices_on_device:
      for per_batch in (corr, dist, vp):
        if per_batch:
          per_batch[-1] = per_batch[-1].cpu().numpy()
  join = torch.cat if matrices_on_device else np.concatenate
  stats = dict(rates=np.concatenate(rates), correlation=join(corr),
               van_rossum=join(dist))
  if vp:
    stats['victor_purpura'] = join(vp)
  return stats


def neuron_van_rossum_blocks_device(hparams, filename, neurons, num_trials=45):
  """The recorded x synthetic blocks of `neuron_van_rossum` before sorting, one
  launch for all chosen neurons: their first trials from both files side by side
  as the trains of a (len(neurons), T, 2 num_trials) batch, the cross block
  sliced as the host slices it."""
  import torch
  sides = []
  for f in (hparams.validation_cache, filename):
    # (trials, T, neurons) -> (neurons, T, trials)
    sides.append(_trials(hparams, f, count=num_trials)[:, :, list(neurons)]
                 .transpose(2, 1, 0))
  n_real, n_fake = sides[0].shape[2], sides[1].shape[2]
  batch = torch.from_numpy(np.ascontiguousarray(
      np.concatenate(sides, axis=2), dtype=np.float32)).to(_device())
  dist = spike_metrics.van_rossum_distance_device(batch).cpu().numpy()
  return dist[:, n_real:, :n_fake]


def device_pairs(hparams, filename):
  """The (recorded, synthetic) samples behind the three KL figures, from the
  device statistics: per neuron the firing rates over the trials, per trial the
  upper triangles of the correlation and van Rossum matrices."""
  real = kept(hparams, '_recorded_statistics', lambda: trial_statistics_device(
      hparams, hparams.validation_cache))
  fake = trial_statistics_device(hparams, filename)
  n = hparams.num_neurons
  iu = np.triu_indices(n, k=1)
  trials = range(min(len(real['rates']), len(fake['rates'])))
  pairs = dict(
      firing_rate=[(real['rates'][:, c], fake['rates'][:, c]) for c in range(n)],
      correlation=[(_upper(real['correlation'][i], n),
                    _upper(fake['correlation'][i], n)) for i in trials],
      van_rossum=[(real['van_rossum'][i][iu], fake['van_rossum'][i][iu])
                  for i in trials])
  if 'victor_purpura' in fake:
    pairs['victor_purpura'] = [(real['victor_purpura'][i][iu],
                                fake['victor_purpura'][i][iu]) for i in trials]
  return pairs


def device_kl_enabled():
  """CALCIUMGAN_DEVICE_KL=0: the histograms behind the KL figures are cut on the
  host (`device_pairs`, then `pairs_kl_divergence`), as before cg_pair_histogram."""
  return os.environ.get('CALCIUMGAN_DEVICE_KL', '1') != '0'


def pairs_kl_divergence_device(hparams, real, fake, remove_nan):
  """`pairs_kl_divergence` of the upper triangles of the float64 device matrices
  real[i], fake[i] (n, C, C): the bin counts from cg_pair_histogram in one
  launch, only counts, sizes and status brought to the host, `kl_from_counts`
  there.  remove_nan: the samples are what `_upper` keeps (the correlations),
  so the divisor is the pair's own size; otherwise it is C (C - 1) / 2, as the
  host divides the distances.  A pair whose status is not 0 goes through
  `pairs_kl_divergence` itself, its two triangles fetched for it alone
  (counted in hparams._kl_host_fallbacks)."""
  n = min(len(real), len(fake))
  real, fake = real[:n], fake[:n]
  C = real.shape[1]
  counts, valid, _, status = spike_metrics.pair_histograms_device(
      real, fake, NUM_BINS, return_edges=False)
  counts, valid, status = (t.cpu().numpy() for t in (counts, valid, status))
  full = C * (C - 1) // 2
  iu = np.triu_indices(C, k=1)
  kl = np.zeros((n,), dtype=np.float32)
  for i in range(n):
    if status[i] != 0:
      r, f = real[i].cpu().numpy(), fake[i].cpu().numpy()
      pair = (_upper(r, C), _upper(f, C)) if remove_nan else (r[iu], f[iu])
      hparams._kl_host_fallbacks = getattr(hparams, '_kl_host_fallbacks', 0) + 1
      kl[i] = pairs_kl_divergence([pair])[0]
    else:
      n_real, n_fake = valid[i] if remove_nan else (full, full)
      kl[i] = kl_from_counts(counts[i, 0], counts[i, 1], n_real, n_fake)
  return kl


def device_kl(hparams, filename):
  """name -> callable giving the float32 KL per pair behind each figure of the
  device report.  The matrices of both files stay on the device (the recorded
  side cached across epochs) and are cut there; the firing rates (one pair per
  neuron of float32 values) are cut on the host."""
  real = kept(hparams, '_recorded_statistics_device',
              lambda: trial_statistics_device(
                  hparams, hparams.validation_cache, matrices_on_device=True))
  fake = trial_statistics_device(hparams, filename, matrices_on_device=True)
  hparams._kl_host_fallbacks = getattr(hparams, '_kl_host_fallbacks', 0)
  n = hparams.num_neurons
  figures = dict(firing_rate=lambda: pairs_kl_divergence(
      [(real['rates'][:, c], fake['rates'][:, c]) for c in range(n)]))
  for name in ('correlation', 'van_rossum', 'victor_purpura'):
    if name in fake:
      figures[name] = (lambda name=name: pairs_kl_divergence_device(
          hparams, real[name], fake[name], remove_nan=name == 'correlation'))
  return figures


def heatmap_minima_device(hparams, filename):
  """`heatmap_minima_host` from the blocks of one launch; `sort_heatmap` on the
  host."""
  blocks = neuron_van_rossum_blocks_device(hparams, filename, hparams.neurons, 45)
  return [np.nanmin(sort_heatmap(b)[0]) for b in blocks]


def temporal_totals_device(hparams, filename):
  """`temporal_totals_host` through cg_spike_ccg and cg_spike_population_hist, a
  batch of trials at a time; the int64 totals summed on the device and brought
  to the host once."""
  spikes = _trials(hparams, filename)
  max_lag = option(hparams, 'max_lag')
  ccg = hist = None
  for batch in _batches(hparams, spikes):
    c, h, _ = spike_metrics.temporal_totals_device(batch, max_lag)
    ccg, hist = (c, h) if ccg is None else (ccg + c, hist + h)
  return (ccg.cpu().numpy(), hist.cpu().numpy(), len(spikes)), spikes.shape[1]


def spectral_totals_device(hparams, filename):
  """`spectral_totals_host` through cg_trace_psd, a batch of trials at a time;
  the float64 totals summed on the device in batch order and brought to the
  host once."""
  signals = _trial_signals(hparams, filename)
  totals = None
  for batch in _batches(hparams, signals):
    part, _ = signals_metrics.spectral_totals_device(batch)
    totals = part if totals is None else totals + part
  return (totals.cpu().numpy(), len(signals)), signals.shape[1]


def novelty_nearest_device(hparams, queries, exclude, exclude_len):
  """`novelty_nearest_host` through cg_nearest_stretch, a batch of trials at a
  time against the recording uploaded once; the batches' (nearest, index) are
  joined on the device and brought to the host once."""
  import torch
  raw, _, step = novelty_recording(hparams)
  dev_raw = kept(hparams, '_novelty_recording_device',
                 lambda: torch.from_numpy(raw).to(_device()))
  nearest, index = [], []
  for batch in _batches(hparams, queries):
    done = sum(len(n) for n in nearest)
    part = None if exclude is None else np.asarray(
        exclude[done:done + len(batch)], dtype=np.int32)
    n, at = signals_metrics.nearest_stretch_totals_device(
        batch, dev_raw, step, part, exclude_len)
    nearest.append(n)
    index.append(at)
  return torch.cat(nearest).cpu().numpy(), torch.cat(index).cpu().numpy()


def state_sets_device(hparams, spikes):
  """`state_sets_host` through cg_population_states, a batch of trials at a
  time; the states stay on the device."""
  return spike_metrics.DeviceStates.cat(
      spike_metrics.population_states_device(batch, option(hparams, 'state_bin'))
      for batch in _batches(hparams, spikes))


def _words_device(hparams, spikes, bin):
  """cg_binary_words of an NWC host array, a batch of trials at a time."""
  return spike_metrics.DeviceWords.cat(
      spike_metrics.binary_words_device(batch, bin)
      for batch in _batches(hparams, spikes))


def _host_integers(tensors):
  return tuple(x.cpu().numpy().astype(np.int64) for x in tensors)


def triplet_sets_device(hparams, spikes):
  """`triplet_sets_host` through cg_binary_words, a batch of trials at a time,
  and one cg_triplet_counts of the side; the integers come to the host."""
  counts, S = spike_metrics.triplet_counts_device(
      _words_device(hparams, spikes, option(hparams, 'triplet_bin')))
  return _host_integers(counts) + (S,)


def interval_sets_device(hparams, spikes):
  """`interval_sets_host` through cg_binary_words at bin 1, a batch of trials at
  a time, and one cg_spike_intervals of the side; the integers come to the
  host."""
  C = spikes.shape[2]
  if not 3 <= C <= spike_metrics.TRIPLET_MAX_NEURONS:
    raise ValueError('--interval_metrics --device gpu packs the trains with '
                     'cg_binary_words, which takes 3 .. {} neurons, not {} '
                     '(--device cpu takes any)'.format(
                         spike_metrics.TRIPLET_MAX_NEURONS, C))
  return _host_integers(spike_metrics.interval_counts_device(
      _words_device(hparams, spikes, 1), option(hparams, 'max_isi')))


# -- the report of one epoch --------------------------------------------------------
Report = collections.namedtuple('Report', 'key flag report host device')
# The optional reports in the order of their keys in spike_metrics.json: with
# hparams.<flag>, out[key] = report(hparams, filename, *back ends of the device).
# A new family is a row here, its own functions and its parser lines.
REPORTS = (
    Report('temporal', 'temporal_metrics', temporal_report,
           (temporal_totals_host,), (temporal_totals_device,)),
    Report('spectral', 'spectral_metrics', spectral_report,
           (spectral_totals_host,), (spectral_totals_device,)),
    Report('novelty', 'novelty_metrics', novelty_report,
           (novelty_nearest_host,), (novelty_nearest_device,)),
    Report('states', 'state_metrics', state_report,
           (state_sets_host, spike_metrics.state_neighbours),
           (state_sets_device, spike_metrics.state_neighbours_device)),
    Report('triplets', 'triplet_metrics', triplet_report,
           (triplet_sets_host,), (triplet_sets_device,)),
    Report('intervals', 'interval_metrics', interval_report,
           (interval_sets_host,), (interval_sets_device,)),
)


def compute_epoch_spike_metrics(hparams, filename, epoch, device=False):
  """:483-497 without plot_signals / raster_plots: dict of the statistics.
  device: the statistics from the device; the histograms behind the KL from
  cg_pair_histogram (`device_kl`) unless CALCIUMGAN_DEVICE_KL=0, the KL's
  arithmetic and `sort_heatmap` on the host."""
  if not h5_helper.contains(filename, 'spikes'):
    (deconvolve_from_file_device if device else deconvolve_from_file)(
        hparams, filename)
  if not device:
    figures = host_kl(hparams, filename)
  elif device_kl_enabled():
    figures = device_kl(hparams, filename)
  else:
    pairs = device_pairs(hparams, filename)
    figures = {name: (lambda name=name: pairs_kl_divergence(pairs[name]))
               for name in pairs}
  out = {}

  def kl_figure(name, label):
    kl = figures[name]()
    out[name + '_kl'] = dict(mean=float(np.mean(kl)))
    if hparams.verbose:
      print('\t{:<18} KL mean: {:.04f}'.format(label, np.mean(kl)))
    return kl

  kl = kl_figure('firing_rate', 'firing rate')
  out['firing_rate_kl']['neurons'] = {
      int(n): float(kl[n]) for n in hparams.neurons}
  kl_figure('correlation', 'correlation')
  minima = (heatmap_minima_device if device else heatmap_minima_host)(
      hparams, filename)
  out['van_rossum_heatmap_min'] = {
      int(n): float(m) for n, m in zip(hparams.neurons, minima)}
  kl_figure('van_rossum', 'van Rossum')
  if 'victor_purpura' in figures:
    kl_figure('victor_purpura', 'Victor-Purpura')
  for row in REPORTS:
    if getattr(hparams, row.flag, False):
      out[row.key] = row.report(hparams, filename,
                                *(row.device if device else row.host))
  return out


def main(hparams):
  """compute_metrics.py:500-542."""
  if not os.path.exists(hparams.output_dir):
    print('{} not found'.format(hparams.output_dir))
    exit()
  random.seed(hparams.seed)
  np.random.seed(hparams.seed)
  utils.load_hparams(hparams)
  with open(os.path.join(hparams.generated_dir, 'info.pkl'), 'rb') as f:
    info = pickle.load(f)
  hparams.num_samples = min(
      h5_helper.get_dataset_length(hparams.validation_cache, 'signals'), 1000)
  # neurons / trials the reference picks for its plots; the heatmaps and the
  # per-neuron KL lines follow the same choice
  hparams.neurons = (list(range(hparams.num_neurons))
                     if hparams.num_neuron_plots >= hparams.num_neurons else
                     list(np.random.choice(hparams.num_neurons,
                                           hparams.num_neuron_plots)))
  hparams.trials = list(np.random.choice(hparams.num_samples,
                                         hparams.num_trial_plots))
  epochs = sorted(info.keys())
  if not hparams.all_epochs:  # only the last generated file
    epochs = [epochs[-1]]
  report = {}
  for epoch in epochs:
    start = time()
    if hparams.verbose:
      print('\nCompute metrics for {}'.format(info[epoch]['filename']))
    report[int(epoch)] = compute_epoch_spike_metrics(
        hparams, filename=info[epoch]['filename'], epoch=epoch,
        device=getattr(hparams, 'device', 'cpu') == 'gpu')
    report[int(epoch)]['elapse'] = time() - start
    with open(os.path.join(hparams.output_dir, 'scalars.jsonl'), 'a') as f:
      f.write(json.dumps({'tag': 'elapse/spike_metrics',
                          'value': report[int(epoch)]['elapse'],
                          'step': int(epoch)}) + '\n')
  with open(os.path.join(hparams.output_dir, 'spike_metrics.json'), 'w') as f:
    json.dump(report, f, indent=1)
  return report


def build_parser():
  parser = argparse.ArgumentParser()
  parser.add_argument('--output_dir', default='runs')
  parser.add_argument('--num_processors', default=6, type=int)
  parser.add_argument('--all_epochs', action='store_true')
  parser.add_argument('--num_neuron_plots', default=6, type=int)
  parser.add_argument('--num_trial_plots', default=6, type=int)
  parser.add_argument('--plots_per_row', default=3, type=int)
  parser.add_argument('--dpi', default=120, type=int)
  parser.add_argument('--format', default='pdf', choices=['pdf', 'png'])
  parser.add_argument('--verbose', default=1, type=int)
  parser.add_argument('--seed', default=12, type=int)
  parser.add_argument('--device', default='cpu', choices=['cpu', 'gpu'],
                      help='gpu: deconvolution and statistics on the device')
  parser.add_argument('--batch_trials', default=DEFAULTS['batch_trials'],
                      type=int, help='--device gpu: trials per launch')

  def optional(name, help, **kwargs):
    """Not a reference flag: absent from the namespace unless given, as main.py
    --spike_metrics (a flag reads getattr(hparams, 'victor_purpura', False), a
    value `option(hparams, 'vp_q')`; the help quotes DEFAULTS)."""
    parser.add_argument(name, default=argparse.SUPPRESS,
                        help=help.format(**DEFAULTS), **kwargs)

  def flag(name, help):
    optional(name, help, action='store_true')

  flag('--victor_purpura',
       'also report victor_purpura_kl, the KL of the Victor-Purpura distances '
       'between the neurons of a trial')
  optional('--vp_q', '--victor_purpura: cost per second of shifting a spike '
           '(default {vp_q})', type=float)
  flag('--temporal_metrics',
       'also report `temporal`: autocorrelogram, lagged covariance, '
       'cross-correlogram and population-count figures of the generated '
       'against the recorded trials')
  optional('--max_lag', '--temporal_metrics: largest lag in frames (default '
           '{max_lag}, at most 256)', type=int)
  flag('--spectral_metrics',
       'also report `spectral`: power-spectrum figures of the generated '
       'against the recorded calcium traces')
  flag('--novelty_metrics',
       'also report `novelty`: the distance from every generated trial to the '
       'nearest stretch of the recording the run was trained on (a recording '
       'directory), against the recording\'s distance to itself')
  optional('--novelty_step', '--novelty_metrics: rows between two stretches '
           '(default: the stride of the dataset)', type=int)
  flag('--state_metrics',
       'also report `states`: precision, recall and coverage of the generated '
       'population states against the recorded ones, beside the floor two '
       'halves of the recorded trials score')
  optional('--state_k', '--state_metrics: the ball of a state reaches to its '
           'k-th nearest neighbour (default {state_k}, at most 8)', type=int)
  optional('--state_bin', '--state_metrics: frames per bin of a state (default '
           '{state_bin}, at most 127)', type=int)
  flag('--triplet_metrics',
       'also report `triplets`: the connected third-order correlations of all '
       'neuron triplets, generated against recorded, beside the floor two '
       'halves of the recorded trials score')
  optional('--triplet_bin', '--triplet_metrics: frames per bin of a binary '
           'state (default {triplet_bin})', type=int)
  flag('--interval_metrics',
       'also report `intervals`: inter-spike-interval histogram, CV and serial '
       'correlation, Fano factor and count correlations across trials, '
       'generated against recorded, beside the floor two halves of the '
       'recorded trials score')
  optional('--max_isi', '--interval_metrics: the longest interval with a '
           'histogram bin of its own, in frames (default {max_isi}, at most '
           '4095)', type=int)
  return parser


if __name__ == '__main__':
  main(build_parser().parse_args())
