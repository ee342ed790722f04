"""Scalar and histogram logger with the reference's tags and directories
(gan/utils/summary_helper.py: writers :32-40, Summary.scalar :98-101,
Summary.histogram :104-106, variable_summary / plot_weights :523-557,
Summary.log :559-588, profiler hooks :115-119).

Scalars and histograms go to TensorBoard event files --
<output_dir>/events.out.tfevents.* for training, <output_dir>/validation/...
for validation, the reference's two writer directories, written by tb_events.py
without TensorFlow -- and, for grep-ability, to JSON lines next to them
(scalars.jsonl, histograms.jsonl).  Images and trace plots (matplotlib) are
outside the hot path and not produced.

--plot_weights: once per training epoch, mean / stddev / min / max and a
30-bucket histogram of every trainable variable of both models
(Summary.plot_weights).  The figures of a whole model come from ONE
cg_tensor_summary call over its flat parameter buffer (nets.FlatParams.summaries,
csrc/summary.hip) and one device-to-host copy; histogram_buckets and
variable_statistics below are the numpy statements of that kernel, and the path
a host array takes.

--profile: the reference traces batches 2-6 of the second epoch with the TF
profiler (main.py:45-52).  Here profiler_trace() switches that window to eager
launches with the kernel library's launch profiler on (cg_profile_enable: every
MFMA-kernel launch carries its own begin / end timestamps) and
profiler_export() writes <output_dir>/profiler/mfma_kernels.json: launches,
total and mean duration per kernel family per batch of the window.  For a
whole-process trace run the same command under
`rocprofv3 --kernel-trace --stats -d <output_dir>/profiler -- python3 main.py ...`
(the command line is printed).
"""
import json
import os
import sys

import numpy as np

from . import tb_events

BUCKET_COUNT = 30  # tf.summary.histogram's default `buckets`


def _to_float(v):
  if hasattr(v, 'item'):
    return float(v.item())
  return float(v)


def _float64_vector(values):
  d = np.asarray(values).astype(np.float64).reshape(-1)
  if d.size == 0:
    raise ValueError('an empty array has no statistics')
  return d


def histogram_buckets(values, bucket_count=BUCKET_COUNT):
  """The (k, 3) float64 rows (left edge, right edge, count) of
  tf.summary.histogram (TensorBoard's histogram summary v2, as shipped with TF
  2.1-2.4): values cast to float64, bucket_count equal-width buckets over
  [min, max], the maximum clamped into the last bucket; (1, 3), a bucket of
  unit width, when all values are equal.  Operation by operation what
  cg_tensor_summary computes (include/calciumgan_hip.h):

    w = (mx - mn) / k,  idx(d) = min((long)floor((d - mn) / w), k - 1)
    e[j] = mn + fl(j w) for j < k,  e[k] = mx   (a zero mx taken as +0)

  Every value must be finite."""
  d = _float64_vector(values)
  k = int(bucket_count)
  if k < 1:
    raise ValueError('bucket_count must be positive')
  if not np.isfinite(d).all():
    raise ValueError('histogram_buckets: a NaN or an infinity among the values')
  mn, mx = d.min(), d.max() + 0.0
  span = mx - mn
  if span == 0:
    return np.array([[mn - 0.5, mn + 0.5, np.float64(d.size)]], np.float64)
  w = span / np.float64(k)
  idx = np.minimum(np.floor((d - mn) / w).astype(np.int64), k - 1)
  counts = np.bincount(idx, minlength=k).astype(np.float64)
  left = mn + np.arange(k, dtype=np.float64) * w
  right = np.concatenate([left[1:], [mx]])
  return np.stack([left, right, counts], axis=1)


def variable_statistics(values):
  """dict(mean, stddev, min, max) in float64 (summary_helper.py:526-540): sum
  and centred squares of the values cast to float64, mean = sum / n, stddev =
  sqrt(sum (d - mean)^2 / n).  All four are NaN when a value is NaN or
  infinite, as cg_tensor_summary reports such a segment."""
  d = _float64_vector(values)
  if not np.isfinite(d).all():
    return dict(mean=np.float64('nan'), stddev=np.float64('nan'),
                min=np.float64('nan'), max=np.float64('nan'))
  n = np.float64(d.size)
  mean = d.sum() / n
  c = d - mean
  sq = (c * c).sum()
  return dict(mean=mean, stddev=np.sqrt(sq / n), min=d.min(), max=d.max() + 0.0)


def _device_summary(values, bucket_count=BUCKET_COUNT):
  """(stats row, bucket rows) of a float32 device tensor as host arrays, or
  None for anything else.  A contiguous tensor is read in place, whatever its
  offset into its storage."""
  import torch
  if not (torch.is_tensor(values) and values.is_cuda and
          values.dtype == torch.float32 and values.numel() > 0):
    return None
  from ... import nets
  flat = values.detach().contiguous().view(-1)
  plan = nets.TensorSummary([0], [flat.numel()], flat.device, bucket_count)
  plan.run(flat)
  return plan.host()


def _rows(stats, buckets):
  """A segment's bucket rows as they are written: None with a NaN or an
  infinity in it, the single row when all its values are equal."""
  if stats[7] > 0:
    return None
  return buckets[:1] if stats[1] == stats[2] else buckets


class Summary(object):

  def __init__(self, hparams, policy=None):
    self._hparams = hparams
    self._policy = policy
    self._train_dir = hparams.output_dir
    self._validation_dir = os.path.join(hparams.output_dir, 'validation')
    self._profiler_dir = os.path.join(hparams.output_dir, 'profiler')
    os.makedirs(self._validation_dir, exist_ok=True)
    self._files = {
        True: os.path.join(self._train_dir, 'scalars.jsonl'),
        False: os.path.join(self._validation_dir, 'scalars.jsonl')
    }
    self._writers = {
        True: tb_events.EventFileWriter(self._train_dir),
        False: tb_events.EventFileWriter(self._validation_dir)
    }
    self._histogram_files = {
        True: os.path.join(self._train_dir, 'histograms.jsonl'),
        False: os.path.join(self._validation_dir, 'histograms.jsonl')
    }
    self._profile = None

  def scalar(self, tag, value, step=0, training=True):
    value = _to_float(value)
    self._writers[bool(training)].scalar(tag, value, step=step)
    with open(self._files[bool(training)], 'a') as f:
      f.write(json.dumps({'tag': tag, 'value': value, 'step': int(step)}) + '\n')

  # -- histograms and weight statistics (summary_helper.py:104-106, 523-557) ----
  def _write_histogram(self, tag, buckets, step, training):
    buckets = np.asarray(buckets, np.float64)
    self._writers[bool(training)].histogram(tag, buckets, step=step)
    with open(self._histogram_files[bool(training)], 'a') as f:
      f.write(json.dumps({'tag': tag, 'step': int(step),
                          'buckets': buckets.tolist()}) + '\n')

  def histogram(self, tag, values, step=0, training=True):
    """tf.summary.histogram(tag, values, step).  A float32 device tensor is
    cut into its buckets on the device (cg_tensor_summary) and only the rows
    come to the host; anything else goes through histogram_buckets.  Values
    with a NaN or an infinity among them raise ValueError."""
    got = _device_summary(values)
    if got is None:
      rows = histogram_buckets(values)
    else:
      rows = _rows(got[0][0], got[1][0])
      if rows is None:
        raise ValueError('histogram {}: a NaN or an infinity among the values'
                         .format(tag))
    self._write_histogram(tag, rows, step, training)

  def _write_variable(self, name, stats, rows, step, training):
    """Four scalars and the histogram of one variable; rows None (a NaN or an
    infinity in it): the scalars, NaN, and no histogram."""
    for suffix, key in (('0_mean', 'mean'), ('1_stddev', 'stddev'),
                        ('2_min', 'min'), ('3_max', 'max')):
      self.scalar('{}/{}'.format(name, suffix), stats[key], step=step,
                  training=training)
    if rows is not None:
      self._write_histogram(name, rows, step, training)

  def variable_summary(self, variable, name, step=0, training=True):
    """summary_helper.py:523-541: `name`/0_mean, /1_stddev, /2_min, /3_max and a
    histogram under `name` itself."""
    got = _device_summary(variable)
    if got is None:
      stats = variable_statistics(variable)
      rows = (histogram_buckets(variable)
              if np.isfinite(stats['mean']) else None)
    else:
      s = got[0][0]
      stats = dict(mean=s[4], stddev=s[6], min=s[1], max=s[2])
      rows = _rows(s, got[1][0])
    self._write_variable(name, stats, rows, step, training)

  def plot_weights(self, gan, step=0, training=True):
    """summary_helper.py:543-557: every trainable variable of the generator,
    then of the discriminator, under plots_<model>/<i + 1>/<variable name>.
    One cg_tensor_summary call and one device-to-host copy per model."""
    for model, scope in ((gan.generator, 'plots_generator'),
                         (gan.discriminator, 'plots_discriminator')):
      params = model.net.params
      stats, buckets = params.summaries_host(BUCKET_COUNT, trainable_only=True)
      for i, index in enumerate(params.summary_indices(trainable_only=True)):
        s = stats[i]
        self._write_variable(
            '{}/{:02d}/{}'.format(scope, i + 1, params.names[index]),
            dict(mean=s[4], stddev=s[6], min=s[1], max=s[2]),
            _rows(s, buckets[i]), step, training)

  # -- profiler window (main.py:45-52) ------------------------------------------
  def profiler_trace(self, gan=None, capacity=4096):
    """Start of the profiled window: eager launches with per-launch kernel
    timestamps (a captured graph cannot be instrumented)."""
    from ... import _lib
    if self._hparams.verbose:
      print('profiling window open; for a whole-process kernel trace run:\n'
            '  rocprofv3 --kernel-trace --stats -d {} -- python3 {}'.format(
                self._profiler_dir, ' '.join(
                    a for a in sys.argv if a != '--profile')))
    self._profile = dict(gan=gan, graph=getattr(gan, '_use_graph', None),
                         capacity=capacity)
    if gan is not None:
      gan._use_graph = False
    _lib.check(_lib.load().cg_profile_enable(capacity), 'cg_profile_enable')

  def profiler_export(self):
    """End of the window: durations of the cg_swconv / cg_wgrad launches since
    profiler_trace() -> <output_dir>/profiler/mfma_kernels.json."""
    import ctypes
    from ... import _lib
    if self._profile is None:
      return None
    cap = self._profile['capacity']
    ms = (ctypes.c_float * cap)()
    fam = (ctypes.c_int * cap)()
    n = _lib.load().cg_profile_collect(ms, fam, cap)
    if n < 0:
      raise RuntimeError('cg_profile_collect: HIP error {}'.format(-n))
    gan = self._profile['gan']
    if gan is not None and self._profile['graph'] is not None:
      gan._use_graph = self._profile['graph']
    self._profile = None
    out = {}
    for i in range(n):
      d = out.setdefault(('cg_swconv', 'cg_wgrad')[fam[i]],
                         dict(launches=0, total_ms=0.0))
      d['launches'] += 1
      d['total_ms'] += float(ms[i])
    for d in out.values():
      d['mean_us'] = d['total_ms'] / d['launches'] * 1e3
    os.makedirs(self._profiler_dir, exist_ok=True)
    path = os.path.join(self._profiler_dir, 'mfma_kernels.json')
    with open(path, 'w') as f:
      json.dump(dict(launches_recorded=n, capacity=cap, families=out), f,
                indent=1)
    return path

  def plot_traces(self, *args, **kwargs):
    pass

  def log(self, gen_loss, dis_loss, gradient_penalty, metrics=None, elapse=None,
          gan=None, step=0, training=True):
    """summary_helper.py:559-588 (scalar part)."""
    self.scalar('loss/generator', gen_loss, step=step, training=training)
    self.scalar('loss/discriminator', dis_loss, step=step, training=training)
    if gradient_penalty is not None:
      self.scalar('loss/gradient_penalty', gradient_penalty, step=step,
                  training=training)
    if metrics is not None:
      for tag, value in metrics.items():
        self.scalar(tag, value, step=step, training=training)
    if elapse is not None:
      self.scalar('elapse', elapse, step=step, training=training)
    if gan is not None and getattr(self._hparams, 'plot_weights', False):
      # summary_helper.py:581-582 (main.py passes gan on the training call only)
      self.plot_weights(gan, step=step, training=training)
    if training and gan is not None and getattr(
        gan.gen_optimizer, 'loss_scale', None) is not None:
      # summary_helper.py:77-78,586-588 logs the loss scale under mixed precision
      self.scalar('model/loss_scale', gan.dis_optimizer.loss_scale[0], step=step,
                  training=training)
