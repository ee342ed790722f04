"""Exponential moving average of the generator's weights (--ema_decay).

Yazici et al. 2019 and every ProGAN / StyleGAN descendant: train on the raw
weights, validate / sample / checkpoint from their running average.  The
reference has no such option; the statement is TensorFlow's
tf.train.ExponentialMovingAverage with num_updates:

  decay_t = min(decay, (1 + t) / (10 + t))        t updates applied so far
  shadow -= (shadow - value) * (1 - decay_t)      assign_moving_average

The first half of this module states it in numpy on the host (what the kernel
cg_ema_update is tested against, bit for bit); WeightAverage is the device side
over a nets.FlatParams: one streaming launch per train() over the whole flat
buffer.  Averaging reads the weights and never writes them, so it cannot change
a training trajectory.
"""
import contextlib

import numpy as np


def check_decay(decay):
  """ValueError unless 0 < decay < 1 (NaN included); returns it as a float."""
  d = float(decay)
  if not (0.0 < d < 1.0):
    raise ValueError('ema_decay must lie in (0, 1), got {!r}'.format(decay))
  return d


def decay_at(decay, t):
  """The decay of update number t (0 for the first), float64: the warm-up of
  tf.train.ExponentialMovingAverage(decay, num_updates=t), so that the shadow
  does not carry the random initial weights for thousands of steps."""
  t = float(t)
  return np.float64(min(float(decay), (1.0 + t) / (10.0 + t)))


def one_minus(d):
  """float32(1 - d): subtracted in float64, rounded once."""
  return np.float32(1.0 - np.float64(d))


def update_statement(e, p, om):
  """e - fl(fl(e - p) * om) on float32 arrays, every operation rounded to
  float32 on its own (no fused multiply-add).  e == p and om == 0 leave e
  unchanged bit for bit (finite values); om == 1 does NOT give p exactly (the
  inner difference has rounded); NaN and infinities go where the three
  operations take them."""
  e = np.asarray(e, dtype=np.float32)
  p = np.asarray(p, dtype=np.float32)
  om = np.float32(om)
  with np.errstate(invalid='ignore', over='ignore', under='ignore'):
    d = np.subtract(e, p, dtype=np.float32)
    s = np.multiply(d, om, dtype=np.float32)
    return np.subtract(e, s, dtype=np.float32)


class WeightAverage(object):
  """The shadow of a nets.FlatParams: a clone of its whole flat buffer, so
  BatchNormalization's moving statistics (the frozen entries) are averaged like
  the rest and the alignment padding stays zero (0 - (0 - 0) om)."""

  def __init__(self, params, decay):
    import torch
    self.params = params
    self.decay = check_decay(decay)
    self.shadow = params.data.clone()
    # applied(): the raw weights wait here while the shadow stands in for them
    self._spare = torch.empty_like(params.data)
    self.updates = 0  # host count of the updates applied
    sizes = [int(np.prod(s)) for s in params.shapes]
    self.views = [self.shadow[o:o + n].view(s)
                  for o, n, s in zip(params.offsets, sizes, params.shapes)]

  def update(self):
    """One cg_ema_update launch on the current stream; no host sync."""
    from ... import _lib
    om = one_minus(decay_at(self.decay, self.updates))
    _lib.call('cg_ema_update', self.shadow, self.params.data,
              self.params.numel, float(om), _lib.stream())
    self.updates += 1

  def get_weights(self):
    """The averaged weights, Keras order (as FlatParams.get_weights)."""
    return [v.detach().cpu().numpy().copy() for v in self.views]

  def set_weights(self, weights):
    import torch
    if len(weights) != len(self.views):
      raise ValueError('expected {} arrays, got {}'.format(
          len(self.views), len(weights)))
    for v, w in zip(self.views, weights):
      w = np.asarray(w, dtype=np.float32)
      if tuple(w.shape) != tuple(v.shape):
        raise ValueError('shape mismatch {} vs {}'.format(w.shape, v.shape))
      v.copy_(torch.from_numpy(w))

  @contextlib.contextmanager
  def applied(self, net):
    """Inside: `net` (the net of these params) computes with the averaged
    weights.  CONTENTS are swapped, never pointers: captured hipGraphs hold the
    addresses of params.data and of the packed operands; both stay where they
    are, and packing is deterministic, so after exit every buffer a graph
    reads holds its old bits."""
    from ... import _lib
    _lib.use(net.precision)  # (repack launches in the net's build)
    data = self.params.data
    self._spare.copy_(data)
    data.copy_(self.shadow)
    net.repack()
    try:
      yield self
    finally:
      data.copy_(self._spare)
      net.repack()
