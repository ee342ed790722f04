"""Host-side shape logic of the CalciumGAN stack (pure python, CPU-testable).

Restates the shape rules of gan/models/calciumgan.py (generator :22-103,
discriminator :141-192, calculate_noise_shape :15-19) and adds the MI355X
layout decisions: channel pitch, channel-chunk (CK) of the packed MFMA operand
and the tile choice of cg_swconv.
"""
from collections import namedtuple

NUM_CONVS = 5
LDS_BYTES = 160 * 1024
_LDS_B = 3 * 64 * 64 * 2  # smallest (64 x 64) 3-deep LDS-DMA weight ring slot set
_SCRATCH = 4 * 16 * 68 * 4


def round_up(v, m):
  return (v + m - 1) // m * m


def pitch(channels):
  """Channel pitch of a bf16 activation: a multiple of 32, so the 32-channel
  chunk (CK = 32: 16-byte rows, uniform K walk, three workgroups per CU)
  always divides it.  102 -> 128: the 23 % extra (zero) K on the C = 102 layers
  is cheaper than the single-chunk CK = 104 path (1 workgroup per CU, measured
  0.49 vs 0.9 PFLOP/s)."""
  return max(32, round_up(channels, 32))


def calculate_noise_shape(output_shape, noise_dim, num_convolutions, strides):
  """calciumgan.py:15-19."""
  w = output_shape[0] / (strides**num_convolutions)
  if not float(w).is_integer():
    raise ValueError('Conv1D: w {} is not an integer.'.format(w))
  return (int(w), noise_dim)


def same_padding_left(kernel_size, strides):
  """TF 'same' left pad for even input lengths: (k - s) // 2."""
  return max(kernel_size - strides, 0) // 2


def tile_rows(Lu, M, n_tiles_n):
  """Row tile of cg_swconv: 256 when the per-sample length allows it and the
  launch still has >= 256 workgroups, else 64.  Returns (CG_TILE_* value, TM)."""
  def ok(tm):
    return (Lu % tm == 0) if Lu >= tm else (tm % Lu == 0)
  if ok(256) and (M // 256) * n_tiles_n >= 256:
    return 0, 256
  if ok(64):
    return 1, 64
  if ok(256):
    return 0, 256
  raise ValueError(
      'unsupported per-sample length {} (must be a power of two <= 64 or a '
      'multiple of 64)'.format(Lu))


def lds_bytes(CK, stride, taps, Lu, TM, TN=64, mfma_rows=16,
              split_parity=False):
  """Smallest dynamic LDS of a cg_swconv launch (64-deep weight stages)."""
  c8 = CK // 8
  if mfma_rows == 16:
    pitch_a = CK + 8 * ((6 - (c8 & 3)) & 3)  # 16-byte slots == 2 (mod 4)
  else:
    pitch_a = CK + 8                         # odd slot count (4 | c8)
  S = min(Lu, TM)
  nseg = TM // S
  WR = S + taps // stride - 1
  regions = 1 if (split_parity and stride == 2) else stride
  a = max(regions * nseg * WR * pitch_a * 2, _SCRATCH)
  return round_up(a, 16) + _LDS_B * (TN // 64)


CK_TARGET = {1: 32, 2: 32}  # preferred channel chunk per source stride


def channel_chunk(Cx, stride, taps, Lu):
  """Channel chunk of a packed operand: a divisor of the pitch, multiple of 8,
  >= 32, valid for both row tiles the launcher may pick.  Preference: the chunk
  that keeps one workgroup's LDS under half the CU (two resident workgroups
  hide each other's staging): 32.  ValueError where no chunk's windows fit LDS
  even on the 64-row tile."""
  cands = [d for d in range(32, Cx + 1, 8) if Cx % d == 0]
  tgt = CK_TARGET[stride]
  pref = sorted(cands, key=lambda d: (d > tgt, abs(d - tgt)))
  tms = [tm for tm in (256, 64)
         if ((Lu % tm == 0) if Lu >= tm else (tm % Lu == 0))]
  if not tms:
    raise ValueError('unsupported per-sample length {}'.format(Lu))
  for d in pref:
    if all(lds_bytes(d, stride, taps, Lu, tm) <= LDS_BYTES for tm in tms):
      return d
  # fall back to the small tile only
  for d in pref:
    if lds_bytes(d, stride, taps, Lu, 64) <= LDS_BYTES:
      return d
  raise ValueError('no channel chunk fits LDS (Cx={}, taps={})'.format(Cx, taps))


def stride2_launches(hp):
  """(network, layer number, Cx, stride, taps, Lu) of the stride-2 'down' launch
  and the two-phase 'up' launch of every layer of both networks: what
  nets.Stride2Layer asks channel_chunk for."""
  k = hp.kernel_size
  out = []
  for i, lay in enumerate(discriminator_layers(hp)):
    out.append(('discriminator', i + 1, lay.cinp, 2, k, lay.lin // 2))
    out.append(('discriminator', i + 1, lay.coutp, 1, k // 2, lay.lin // 2))
  for i, lay in enumerate(generator_layers(hp)):
    out.append(('generator', i + 1, lay.coutp, 2, k, lay.lout // 2))
    out.append(('generator', i + 1, lay.cinp, 1, k // 2, lay.lout // 2))
  return out


def dense_streams(cp):
  """Channel pitches whose per-timestep Dense runs on the streaming kernels
  (cg_dense_rows / cg_dense_rows_act) instead of an LDS-staged cg_swconv
  launch: W in registers up to 128, one 128-column panel of W in LDS for 256,
  384, 512."""
  return cp <= 128 or cp in (256, 384, 512)


ConvLayer = namedtuple('ConvLayer', 'cin cout lin lout cinp coutp')


def discriminator_layers(hp):
  """Conv1D(k, s, 'same') x5 with filters U..5U (calciumgan.py:145-185)."""
  u = hp.num_units
  filters = [u, 2 * u, 3 * u, 4 * u, 5 * u]
  layers = []
  cin, length = hp.num_channels, hp.signal_shape[0]
  for cout in filters:
    if length % hp.strides:
      raise ValueError('sequence length not divisible by strides**5')
    lout = length // hp.strides
    layers.append(ConvLayer(cin, cout, length, lout, pitch(cin), pitch(cout)))
    cin, length = cout, lout
  return layers


def generator_layers(hp):
  """Conv1DTranspose x5 with filters 5U..2U, C (calciumgan.py:37-87)."""
  u = hp.num_units
  filters = [5 * u, 4 * u, 3 * u, 2 * u, hp.num_channels]
  w, nd = calculate_noise_shape(hp.signal_shape, hp.noise_dim, NUM_CONVS,
                                hp.strides)
  layers = []
  cin, length = nd, w
  for cout in filters:
    lout = length * hp.strides
    layers.append(ConvLayer(cin, cout, length, lout, pitch(cin), pitch(cout)))
    cin, length = cout, lout
  return layers


def _keras_name(base, i):
  """Keras' automatic layer name: `base`, `base_1`, `base_2`, ..."""
  return base if i == 0 else '{}_{}'.format(base, i)


def generator_variable_names(layer_norm=False, batch_norm=False):
  """Names of the generator's variables in get_weights() order, as Keras names
  them when the generator is the first model built after clear_session()
  (calciumgan.py:22-103; the reference's Conv1DTranspose layer wraps a
  Conv2DTranspose).  Restated: TensorFlow is absent, the table is UNPINNED."""
  names = ['dense/kernel:0', 'dense/bias:0']
  for i in range(NUM_CONVS):
    conv = '{}/{}'.format(_keras_name('conv1d_transpose', i),
                          _keras_name('conv2d_transpose', i))
    names += [conv + '/kernel:0', conv + '/bias:0']
    if batch_norm:
      names += ['{}/{}:0'.format(_keras_name('batch_normalization', i), v)
                for v in ('gamma', 'beta', 'moving_mean', 'moving_variance')]
    if layer_norm:
      names += ['{}/{}:0'.format(_keras_name('layer_normalization', i), v)
                for v in ('gamma', 'beta')]
  return names + ['dense_1/kernel:0', 'dense_1/bias:0']


def discriminator_variable_names():
  """The same for the discriminator, built after the generator
  (calciumgan.py:141-192): its Dense is the process's third."""
  names = []
  for i in range(NUM_CONVS):
    names += ['{}/{}:0'.format(_keras_name('conv1d', i), v)
              for v in ('kernel', 'bias')]
  return names + ['dense_2/kernel:0', 'dense_2/bias:0']


# activation_fn (gan/models/utils.py:6-8): 'leakyrelu' -> LeakyReLU() (Keras
# default alpha 0.3), any other name -> layers.Activation(name).  The kernels
# implement the PIECEWISE-LINEAR ones as x -> max(x, alpha x): the fused
# epilogues, the LeakyReLU' masks of every backward chain and -- the reason for
# the restriction -- the hand-derived second backward of the gradient penalty,
# which relies on the activation's second derivative being zero.
PIECEWISE_LINEAR_ALPHA = {'leakyrelu': 0.3, 'relu': 0.0, 'linear': 1.0}


def activation_alpha(hp):
  """Slope for negative inputs of hparams.activation, or ValueError."""
  name = getattr(hp, 'activation', 'leakyrelu')
  if name not in PIECEWISE_LINEAR_ALPHA:
    raise ValueError(
        "calciumgan_amd: activation '{}' is not implemented (piecewise-linear "
        'activations only: {}; a smooth activation adds a second-derivative '
        'term to the gradient penalty that the kernel schedule does not '
        'carry)'.format(name, ', '.join(sorted(PIECEWISE_LINEAR_ALPHA))))
  return PIECEWISE_LINEAR_ALPHA[name]


def validate_hparams(hp):
  """Shapes the HIP path supports; raises ValueError like the reference does
  for a non-integer noise width (calciumgan.py:17-18)."""
  if hp.strides != 2:
    raise ValueError('calciumgan_amd: only strides=2 is implemented in HIP')
  if hp.kernel_size % 2 or hp.kernel_size > 24 or hp.kernel_size < 2:
    raise ValueError('calciumgan_amd: kernel_size must be even and <= 24')
  # the input Dense stores h[0] as rows of noise_dim channels and the first
  # transposed convolution reads (and its input gradient writes) them at the
  # channel pitch of every activation, a multiple of 32: the two must agree
  if hp.noise_dim < 32 or pitch(hp.noise_dim) != hp.noise_dim:
    raise ValueError(
        'calciumgan_amd: noise_dim must be a multiple of 32 (got {}): the '
        'generator reshapes its input Dense to rows of noise_dim channels, '
        'and activations have a channel pitch of 32'.format(hp.noise_dim))
  # (batch_norm: single rank only -- GeneratorNet raises under data parallelism,
  # where the batch statistics would need a cross-rank reduction)
  activation_alpha(hp)  # raises for activations the kernels do not cover
  w, _ = calculate_noise_shape(hp.signal_shape, hp.noise_dim, NUM_CONVS,
                               hp.strides)
  for lay in discriminator_layers(hp):
    lu = lay.lout
    if not ((lu % 64 == 0) or (64 % lu == 0)):
      raise ValueError(
          'calciumgan_amd: layer length {} unsupported (sequence_length/32 must '
          'be a power of two or a multiple of 64)'.format(lu))
  # tf.pad(mode='reflect') needs pad < length: PhaseShuffle on the layer-4
  # output (length L/16) bounds m (calciumgan.py:126-135)
  if hp.m >= hp.signal_shape[0] // 16:
    raise ValueError('phase shuffle m={} too large for sequence length'.format(
        hp.m))
  # the staged windows of every layer's launches must fit LDS with some channel
  # chunk (kernel_size 24 at sequence_length 32: 64 one-row samples per tile,
  # each with a 12-row window in both parities)
  for net, i, cx, stride, taps, lu in stride2_launches(hp):
    try:
      channel_chunk(cx, stride, taps, lu)
    except ValueError as e:
      raise ValueError(
          'calciumgan_amd: kernel_size {} at sequence_length {} unsupported: '
          '{} layer {}, stride {}, rows of {}: {}'.format(
              hp.kernel_size, hp.signal_shape[0], net, i, stride, lu, e))
  return w
