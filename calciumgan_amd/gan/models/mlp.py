"""The reference's MLP generator / discriminator (gan/models/mlp.py:15-77) on
the float32 Dense kernels of csrc/mlp.hip, behind the same object surface as
calciumgan.py's models.

  generator      Dense(L * noise_dim) + act, reshaped to (L, noise_dim);
                 Dense(U), Dense(2U), Dense(3U), each + act + dropout;
                 Dense(C) -> sigmoid when hparams.normalize, else linear
  discriminator  Dense(4U), Dense(3U), Dense(2U), Dense(U), each + act +
                 dropout; Flatten (time-major); Dense(1)

Every layer is a Dense over rows: n * L rows for the per-timestep layers, n rows
for the generator's first Dense and the critic's head.  float32 throughout;
--mixed_precision is refused, and so are --batch_norm / --layer_norm (the
reference's MLP has neither layer: asking for one is an error here, not
ignored).  geometry.validate_hparams' convolution rules do not apply: noise_dim
may be any value >= 1.

Dropout is counter-based: the keep mask of a layer's output is a pure function
of (seed, stream id, element index) -- `dropout_keep_mask` below is its numpy
statement, the kernels agree with it bit for bit -- so no mask is stored.  The
stream id of a launch is  (call << 8) | (model << 4) | layer  with `call` the
1-based count of training-mode calls of that model object (generator: model 0,
discriminator: model 1): every (model call, layer) has its own stream, and two
processes that make the same calls draw the same masks.
"""
import numpy as np
import torch

from ... import _lib
from ... import geometry as geo
from ... import nets
from .calciumgan import _INIT_SEED, _Model, _device
from .registry import register

# the dropout masks' Philox key (main.py:11-12 seeds everything with 1234)
DROPOUT_SEED = 1234
MAX_WIDTH = _lib.CONSTANTS['CG_MLP_MAX_WIDTH']
MAX_FLAT = _lib.CONSTANTS['CG_MLP_MAX_FLAT']
FWD_ACT, FWD_TANGENT, FWD_SIGMOID = (
    _lib.CONSTANTS['CG_MLP_FWD_' + n] for n in ('ACT', 'TANGENT', 'SIGMOID'))
BWD_MASK, BWD_SIGMOID, BWD_NONE = (
    _lib.CONSTANTS['CG_MLP_BWD_' + n] for n in ('MASK', 'SIGMOID', 'NONE'))

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
  """Philox4x32-10 (Salmon et al. 2011, Random123) of counter blocks (..., 4)
  and a key (2,), all uint32 values -> uint32 (..., 4)."""
  c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
  k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
  for _ in range(10):
    p0 = np.uint64(_M0) * c[0]
    p1 = np.uint64(_M1) * c[2]
    c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _U32,
         (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _U32]
    k0 = (k0 + _W0) & 0xFFFFFFFF
    k1 = (k1 + _W1) & 0xFFFFFFFF
  return np.stack(c, axis=-1).astype(np.uint32)


def dropout_threshold(p):
  """floor(p * 2^32): an element is kept iff its 32-bit word is >= this."""
  if not 0.0 <= p < 1.0:
    raise ValueError('dropout rate must be in [0, 1), not {}'.format(p))
  return int(np.floor(np.float64(p) * 4294967296.0))


def dropout_scale(p):
  """float32(1 / (1 - p)): what kept elements are multiplied by."""
  return np.float32(1.0 / (1.0 - np.float64(p)))


def dropout_keep_mask(seed, stream, n, p):
  """The keep mask the kernels apply, as bool (n,): element e takes word e & 3
  of the Philox4x32-10 block with counter (lo(e >> 2), hi(e >> 2), lo(stream),
  hi(stream)) and key (lo(seed), hi(seed)); kept iff word >= floor(p 2^32)."""
  n = int(n)
  thr = dropout_threshold(p)
  if thr == 0:
    return np.ones(n, dtype=bool)
  seed, stream = int(seed) & (2**64 - 1), int(stream) & (2**64 - 1)
  blocks = np.arange((n + 3) // 4, dtype=np.uint64)
  counter = np.stack([
      blocks & _U32, blocks >> np.uint64(32),
      np.full_like(blocks, stream & 0xFFFFFFFF),
      np.full_like(blocks, stream >> 32)], axis=-1)
  words = philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32))
  return words.reshape(-1)[:n] >= np.uint32(thr)


def stream_id(call, model, layer):
  """Stream id of (model call, layer): (call << 8) | (model << 4) | layer."""
  return (int(call) << 8) | (int(model) << 4) | int(layer)


# -- shapes --------------------------------------------------------------------
def _dims(hparams):
  L, C = (int(v) for v in hparams.signal_shape)
  return L, C, int(hparams.noise_dim), int(hparams.num_units)


def generator_shapes(hparams):
  """get_weights() shapes of the generator, Keras order (kernel, bias)."""
  L, C, nd, U = _dims(hparams)
  widths = [(nd, L * nd), (nd, U), (U, 2 * U), (2 * U, 3 * U), (3 * U, C)]
  return [s for cin, cout in widths for s in ((cin, cout), (cout,))]


def discriminator_shapes(hparams):
  """get_weights() shapes of the discriminator, Keras order."""
  L, C, _, U = _dims(hparams)
  widths = [(C, 4 * U), (4 * U, 3 * U), (3 * U, 2 * U), (2 * U, U), (L * U, 1)]
  return [s for cin, cout in widths for s in ((cin, cout), (cout,))]


def _dense_names(first, count):
  """Keras' automatic names of `count` Dense layers, the first one the
  process's `first`-th (restated: TensorFlow is absent, the table is UNPINNED)."""
  names = []
  for i in range(first, first + count):
    layer = 'dense' if i == 0 else 'dense_{}'.format(i)
    names += [layer + '/kernel:0', layer + '/bias:0']
  return names


def validate_hparams(hparams):
  """What this model refuses (ValueError), instead of geometry.validate_hparams'
  convolution rules.  Returns the activation's slope for negative inputs."""
  alpha = geo.activation_alpha(hparams)  # a smooth activation raises
  if getattr(hparams, 'mixed_precision', False):
    raise ValueError('calciumgan_amd: --model mlp is float32 only; drop '
                     '--mixed_precision')
  if getattr(hparams, 'batch_norm', False) or getattr(hparams, 'layer_norm',
                                                      False):
    raise ValueError('calciumgan_amd: --model mlp has no normalisation layers '
                     '(the reference\'s MLP has neither); drop --batch_norm / '
                     '--layer_norm')
  if int(getattr(hparams, 'world_size', 1) or 1) > 1:
    raise ValueError('calciumgan_amd: --model mlp is single process only '
                     '(world_size > 1)')
  if len(tuple(hparams.signal_shape)) != 2:
    raise ValueError('calciumgan_amd: --model mlp takes (L, C) signals')
  L, C, nd, U = _dims(hparams)
  if min(L, C, nd, U) < 1:
    raise ValueError('calciumgan_amd: sequence length, channels, noise_dim and '
                     'num_units must be >= 1')
  if max(4 * U, nd, C) > MAX_WIDTH:
    raise ValueError('calciumgan_amd: --model mlp layer widths must be <= {} '
                     '(4 * num_units, noise_dim, channels)'.format(MAX_WIDTH))
  if max(L * U, L * nd) > MAX_FLAT:
    raise ValueError('calciumgan_amd: sequence_length * num_units and '
                     'sequence_length * noise_dim must be <= {}'.format(MAX_FLAT))
  p = float(getattr(hparams, 'dropout', 0.0))
  if not 0.0 <= p < 1.0:
    raise ValueError('calciumgan_amd: --dropout must be in [0, 1)')
  return alpha


class _Layer(object):
  """One Dense over rows.  per: rows per sample; iw: index of its kernel in
  the parameter views (the bias follows)."""

  def __init__(self, cin, cout, per, alpha, drop, sigmoid=False):
    self.cin, self.cout, self.per = cin, cout, per
    self.alpha, self.drop, self.sigmoid = alpha, drop, sigmoid
    self.fwd_mode = FWD_SIGMOID if sigmoid else FWD_ACT
    self.bwd_mode = (BWD_SIGMOID if sigmoid else
                     BWD_NONE if alpha == 1.0 and not drop else BWD_MASK)


class _Pass(object):
  """Buffers of one model at one batch size n: the stored outputs h_l, the
  masked output gradients dz_l and the input gradient of every layer."""

  def __init__(self, net, n):
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=net.device)
    self.n = n
    self.h = [f32(n * l.per, l.cout) for l in net.layers]
    self.dz = [f32(n * l.per, l.cout) for l in net.layers]
    # dx[l]: gradient of layer l's input == of layer l - 1's output
    self.dx = [f32(n * l.per, l.cin) for l in net.layers]
    self.streams = [0] * len(net.layers)


class MLPNet(object):
  """A chain of Dense layers over one FlatParams buffer."""
  precision = 'bf16'  # (the build the shared float32 entry points are called in)
  batch_norm = layer_norm = False

  def __init__(self, hparams, device, rng, shapes, names, layers, model_id):
    self.alpha = validate_hparams(hparams)
    self.device = device
    self.p = float(getattr(hparams, 'dropout', 0.0))
    self.seed = DROPOUT_SEED
    self.model_id = model_id
    self.L, self.C, self.nd, self.U = _dims(hparams)
    self.layers = layers
    self.params = nets.FlatParams(shapes, device, names=names)
    init = []
    for l in layers:
      init.append(nets.glorot_uniform(rng, (l.cin, l.cout), l.cin, l.cout))
      init.append(np.zeros(l.cout, np.float32))
    self.params.set_weights(init)
    self.calls = 0  # training-mode calls so far: the masks' stream counter
    self._passes = {}
    self._ws = None

  def repack(self):
    """(the float32 kernels read the master weights: nothing to pack)"""

  def W(self, l):
    return self.params.views[2 * l]

  def b(self, l):
    return self.params.views[2 * l + 1]

  def buffers(self, n):
    ps = self._passes.get(n)
    if ps is None:
      if self.device.type != 'cuda':
        raise RuntimeError('calciumgan_amd needs a HIP device (no CPU fallback)')
      ps = self._passes[n] = _Pass(self, n)
    return ps

  def _wgrad_ws(self, elems):
    if self._ws is None or self._ws.numel() < elems:
      self._ws = torch.empty(elems, dtype=torch.float32, device=self.device)
    return self._ws

  # -- the launches ---------------------------------------------------------
  def forward(self, x, n, training, x_pitch=None):
    """x: f32 (n * layers[0].per, layers[0].cin) rows at x_pitch -> the last
    layer's output.  training: dropout with the next call's streams."""
    ps = self.buffers(n)
    p = self.p if training else 0.0
    if training:
      self.calls += 1
    s = _lib.stream()
    src, pitch = x, x_pitch
    for i, l in enumerate(self.layers):
      drop = p if l.drop else 0.0
      sid = stream_id(self.calls, self.model_id, i)
      ps.streams[i] = sid if drop > 0.0 else None
      _lib.call('cg_mlp_dense_fwd', src, l.cin if pitch is None else pitch,
                self.W(i), self.b(i), None, ps.h[i], n * l.per, l.cin, l.cout,
                l.fwd_mode, l.alpha, drop, self.seed, sid, s)
      src, pitch = ps.h[i], None
    ps.p = p
    return ps.h[-1]

  def backward(self, n, dout, need_dx=True):
    """Input-gradient chain from dout (gradient of the last layer's output)
    over the stored h of the last forward at batch size n: leaves dz_l of every
    layer and returns the gradient of the model's input (None without
    need_dx)."""
    ps = self.buffers(n)
    s = _lib.stream()
    dh = dout
    for i in range(len(self.layers) - 1, -1, -1):
      l = self.layers[i]
      dx = ps.dx[i] if (i > 0 or need_dx) else None
      _lib.call('cg_mlp_dense_dgrad', dh, ps.h[i], self.W(i), ps.dz[i], dx,
                n * l.per, l.cin, l.cout, l.bwd_mode, l.alpha,
                ps.p if l.drop else 0.0, s)
      dh = dx
    return dh

  def weight_grads(self, n, x, tails=None, seg=None, coef=(1.0, 0.0, 0.0),
                   bias_seg=None):
    """dW / db of every layer into params.grad from the inputs [x | h_0 | ...]
    and dz_l of the last backward.  tails: per layer the replacement input of
    the samples from 2 * seg on (the tangent chain), seg: samples per segment,
    bias_seg: samples that carry a bias gradient (default all)."""
    ps = self.buffers(n)
    s = _lib.stream()
    gv = self.params.grad_views
    seg = n if seg is None else seg
    bias_seg = n if bias_seg is None else bias_seg
    lib = _lib.load()
    ws = self._wgrad_ws(max(
        lib.cg_mlp_wgrad_ws_elems(n * l.per, l.cin, l.cout)
        for l in self.layers))
    for i, l in enumerate(self.layers):
      src = x if i == 0 else ps.h[i - 1]
      tail = None if tails is None else tails[i]
      _lib.call('cg_mlp_dense_wgrad', src, l.cin, tail, 2 * seg * l.per,
                ps.dz[i], gv[2 * i], gv[2 * i + 1], n * l.per, l.cin, l.cout,
                seg * l.per, coef[0], coef[1], coef[2], bias_seg * l.per, ws, s)


class GeneratorNet(MLPNet):

  def __init__(self, hparams, device, rng):
    alpha = validate_hparams(hparams)
    L, C, nd, U = _dims(hparams)
    layers = [_Layer(nd, L * nd, 1, alpha, False),
              _Layer(nd, U, L, alpha, True),
              _Layer(U, 2 * U, L, alpha, True),
              _Layer(2 * U, 3 * U, L, alpha, True),
              _Layer(3 * U, C, L, 1.0, False, sigmoid=bool(hparams.normalize))]
    super().__init__(hparams, device, rng, generator_shapes(hparams),
                     _dense_names(0, 5), layers, model_id=0)
    self.Cf = C  # (row pitch of the generated batch)


class DiscriminatorNet(MLPNet):

  def __init__(self, hparams, device, rng):
    alpha = validate_hparams(hparams)
    L, C, nd, U = _dims(hparams)
    layers = [_Layer(C, 4 * U, L, alpha, True),
              _Layer(4 * U, 3 * U, L, alpha, True),
              _Layer(3 * U, 2 * U, L, alpha, True),
              _Layer(2 * U, U, L, alpha, True),
              _Layer(L * U, 1, 1, 1.0, False)]
    super().__init__(hparams, device, rng, discriminator_shapes(hparams),
                     _dense_names(5, 5), layers, model_id=1)

  def tangent(self, n, seg, v, out):
    """Push v (seg * L, C) through the masked linear chain of the LAST segment
    of the stored forward at batch size n: out[l] = m(h_l) * (out[l - 1] W_l)
    for the four per-timestep layers."""
    ps = self.buffers(n)
    s = _lib.stream()
    src = v
    for i, l in enumerate(self.layers[:-1]):
      h = ps.h[i][(n - seg) * l.per:]
      _lib.call('cg_mlp_dense_fwd', src, l.cin, self.W(i), None, h, out[i],
                seg * l.per, l.cin, l.cout, FWD_TANGENT, l.alpha,
                ps.p if l.drop else 0.0, 0, 0, s)
      src = out[i]


class _MLPModel(_Model):
  is_mlp = True

  def _input(self, x):
    return torch.as_tensor(x, dtype=torch.float32).to(
        self.net.device).contiguous()


class Generator(_MLPModel):
  name = 'generator'

  def __call__(self, noise, training=False):
    """noise (B, noise_dim) -> (B, L, C) float32 (sigmoid when normalize).
    training=False applies no dropout."""
    net = self.net
    _lib.use(net.precision)
    noise = self._input(noise)
    B = noise.shape[0]
    fake = net.forward(noise, B, training)
    return fake.reshape(B, net.L, net.C).clone()


class Discriminator(_MLPModel):
  name = 'discriminator'

  def __call__(self, signals, training=True):
    """signals (B, L, C) -> (B, 1) float32."""
    net = self.net
    _lib.use(net.precision)
    x = self._input(signals)
    B = x.shape[0]
    out = net.forward(x.reshape(B * net.L, net.C), B, training)
    return out.reshape(B, 1).clone()


def generator(hparams, device=None):
  """mlp.py:15-47.  device: where the parameters live (default: the current
  HIP device; a CPU device gives an object whose weights can be read and set
  but that cannot compute)."""
  rng = np.random.RandomState(_INIT_SEED)
  return Generator(GeneratorNet(hparams, device or _device(), rng))


def discriminator(hparams, device=None):
  """mlp.py:50-77."""
  rng = np.random.RandomState(_INIT_SEED + 1)
  return Discriminator(DiscriminatorNet(hparams, device or _device(), rng))


@register('mlp')
def get_mlp(hparams):
  return generator(hparams), discriminator(hparams)
