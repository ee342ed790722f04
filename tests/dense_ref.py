"""Float64 statements of the per-timestep Dense entry points of the C ABI
(calciumgan_amd/csrc/dense_rows.hip), written from the comments of
include/calciumgan_hip.h, the error bar of an f32 matrix-core contraction, and
the data recipes the parity tests of tests/test_hip_dense_rows.py run them on.

Everything here is numpy float64 on the host.  tests/test_dense_ref.py ties each
statement to an independent one (torch autograd in float64, the oracle of
oracle/calciumgan_oracle.py) and checks on the CPU that the recipes can tell a
wrong kernel from a right one (the bars are far below what a dropped k-group
changes; the exact sums do need rounding)."""
import numpy as np

import pointwise_ref as R

# What the matrix cores of gfx950 do with subnormal INPUTS of the activation
# type.  "Kept" is taken from the ISA documents; the test
# test_hip_dense_rows.py::test_matrix_cores_keep_subnormal_inputs pins it either
# way -- if it fails with zeros, flip the entry.  The reference takes it as an
# explicit argument.
FLUSH_SUBNORMAL_INPUTS = {False: False, True: False}  # f16 -> flushed?

SIG_RTOL, SIG_ATOL = 2e-6, 1e-6  # the project's bar of the sigmoid epilogue
T_MAX = 8.0  # random pre-activations stay within it (the fast exponential's
             # argument rounding, ~ |t| 2^-24 relative, stays inside SIG_RTOL)


# ---------------------------------------------------------------------------
# statements
# ---------------------------------------------------------------------------
def sigmoid(t):
  with np.errstate(over='ignore'):
    return 1.0 / (1.0 + np.exp(-np.asarray(t, np.float64)))


def min_normal(f16):
  return 2.0**-14 if f16 else 2.0**-126


def flush(x, f16):
  """Subnormals of the activation type -> zero of the same sign."""
  x = np.asarray(x, np.float64)
  return np.where(np.abs(x) < min_normal(f16), np.copysign(0.0, x), x)


def dense_rows(x, W, bias=None, epi=None, flush_subnormal_inputs=False, f16=False):
  """y[r, n] = epi(bias[n] + sum_c x[r, c] W[c, n]); epi None or 'sigmoid'.
  flush_subnormal_inputs: x and W lose their subnormals (of the activation type
  f16 selects) before the products."""
  x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
  if flush_subnormal_inputs:
    x, W = flush(x, f16), flush(W, f16)
  with np.errstate(invalid='ignore', over='ignore'):
    t = x @ W
    if bias is not None:
      t = t + np.asarray(bias, np.float64)[None, :]
  if epi is None:
    return t
  assert epi == 'sigmoid'
  return sigmoid(t)


def dense_rows_interp(x, W, bias, epi, real, alpha, n, B, L, f16):
  """The n critic inputs [real | fake_k | x^_k] of one step, x [n B L][K], real
  [B L][N] (f32 values), alpha [n B] or None.  Three steps: (1) fake = the Dense
  on all n B L rows; (2) x^_k = alpha_k real + (1 - alpha_k) fake_k on the
  UNROUNDED values; (3) each segment rounded to the activation type.
  Returns a list of n dicts with the unrounded 'fake', 'xhat' (None without
  alpha) and the rounded 'real_r', 'fake_r', 'xhat_r', each (B, L, N)."""
  N = np.shape(W)[1]
  fake = dense_rows(x, W, bias, epi).reshape(n, B, L, N)
  real = np.asarray(real, np.float64).reshape(B, L, N)
  out = []
  for k in range(n):
    d = {'fake': fake[k], 'real_r': R.round_act(real, f16),
         'fake_r': R.round_act(fake[k], f16), 'xhat': None, 'xhat_r': None}
    if alpha is not None:
      a = np.asarray(alpha, np.float64)[k * B:(k + 1) * B]
      d['xhat'] = R.interp(real, fake[k], a)
      d['xhat_r'] = R.round_act(d['xhat'], f16)
    out.append(d)
  return out


def dense_rows_act(dz, Wt, f16, flush_subnormal_inputs=False):
  """dh[r, c] = sum_n dz[r, n] Wt[n, c], rounded to the activation type."""
  return R.round_act(dense_rows(dz, Wt, None, None, flush_subnormal_inputs, f16), f16)


def dense_wgrad(x, g):
  """dW[cx, cg] = sum_r x[r, cx] g[r, cg]."""
  return np.asarray(x, np.float64).T @ np.asarray(g, np.float64)


def wgrad_ws_elems(rows, Cx_real, Cg_real):
  """cg_dense_wgrad_ws_elems: one partial dW per row range.  ~512 workgroups for
  up to four 128 x 128 tiles of dW, ~1024 beyond, split over the tiles in
  multiples of 8 ranges (at least 8); a range is whole 32-row stages; the count
  of ranges that hold rows, rounded up to a multiple of 8."""
  ntiles = -(-Cx_real // 128) * -(-Cg_real // 128)
  nsplit = max((512 if ntiles <= 4 else 1024) // ntiles // 8 * 8, 8)
  rps = -(-(-(-rows // nsplit)) // 32) * 32
  nsplit = -(-(-(-rows // rps)) // 8) * 8
  return nsplit * Cx_real * Cg_real


# ---------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------
def acc_bound(x, W, bias=None):
  """Error bar of an f32 matrix-core contraction of K terms (+ bias):
  (K + 1) 2^-23 (sum_c |x[r, c] W[c, n]| + |bias[n]|) -- one rounding of up to one
  ulp per addition, in any order; a truncating adder and any split of K across
  MFMA steps are within it.  Derived, not measured."""
  x, W = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(W, np.float64))
  s = x @ W
  if bias is not None:
    s = s + np.abs(np.asarray(bias, np.float64))[None, :]
  return (x.shape[1] + 1) * 2.0**-23 * s


def sigmoid_bar(acc, s):
  """The sigmoid epilogue: its largest slope (1/4) times the bar of its argument
  plus the project's bar for the epilogue itself."""
  return 0.25 * acc + SIG_RTOL * np.abs(s) + SIG_ATOL


def xhat_err(alpha, real, fake, err_fake):
  """f32_err of the x^ segment: |1 - alpha| err_fake + 3 ulp_f32(|alpha real| +
  |(1 - alpha) fake|) -- the two products and one add, each possibly contracted.
  alpha (B,), real / fake / err_fake (B, L, N)."""
  a = np.asarray(alpha, np.float64).reshape(-1, 1, 1)
  return np.abs(1 - a) * err_fake + 3 * R.ulp_f32(
      np.abs(a * real) + np.abs((1 - a) * fake))


def wgrad_bound(x, g):
  """f32 sum of `rows` products per weight: R.sum_bound over the rows (rows 2^-24
  sum_r |x[r, cx] g[r, cg]|), doubled to the 2^-23 convention of acc_bound."""
  x, g = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(g, np.float64))
  return 2 * x.shape[0] * R.U32 * (x.T @ g)


# ---------------------------------------------------------------------------
# data recipes (numpy only: the CPU tests check them, the GPU tests run them)
# ---------------------------------------------------------------------------
def planted_row_start(f16):
  tiny = R.act_limits(f16)[0]
  return [0.0, -0.0, tiny, -tiny, 1.0, -1.0]


def _tame(x, W, bias):
  """W halved until every pre-activation of the finite rows of x lies within
  T_MAX (a power of two: the recipe's bits keep their pattern)."""
  fin = np.isfinite(x).all(axis=1) & (np.abs(x).max(axis=1) <= 16)
  while np.abs(x[fin] @ W + bias).max() > T_MAX:
    W = W / 2
  return W


def real_recipe(seed, rows, K, N, f16):
  """x = round_act(randn) (rows, K), W = 0.2 randn (K, N) as f32 -- the pack
  rounds it: the statement takes round_act(W) --, bias = f32(0.1 randn).  Every
  row starts with +-0, the smallest subnormal and its negative, +-1.
  Returns x, W (f32 values), round_act(W), bias."""
  rng = np.random.RandomState(seed)
  x = R.round_act(rng.randn(rows, K), f16)
  x[:, :6] = planted_row_start(f16)
  bias = (0.1 * rng.randn(N)).astype(np.float32).astype(np.float64)
  W = _tame(x, 0.2 * rng.randn(K, N), bias)
  W32 = W.astype(np.float32).astype(np.float64)
  return x, W32, R.round_act(W32, f16), bias


ZC = 2  # the all-zero column of W in special_recipe


def special_recipe(seed, rows, K, N, f16):
  """real_recipe plus: channel K - 1 is a switch (0 in every ordinary row, W[K -
  1, n] = +1 / -1 for even / odd n), column ZC of W is all zero and |W[8, :]| <=
  1/2 (the largest finite value times it stays an f32).  Rows (rows >= 16, N >= 4):
    'inf': +inf in channel 7;  'nan': NaN in channel 9;
    'big': the largest finite value in channel 8;
    'sat30' / 'sat100': 30 / -100 in the switch channel, 0 elsewhere: t = +-30 /
    -+100 (+ bias) by column parity.
  They sit in the first, an inner and the last (ragged, clamped) row block.
  Returns x, W (f32 values), round_act(W), bias and the planted row indices."""
  assert rows >= 16 and N >= 4 and K >= 32
  rng = np.random.RandomState(seed)
  x = R.round_act(rng.randn(rows, K), f16)
  x[:, :6] = planted_row_start(f16)
  x[:, K - 1] = 0.0
  bias = (0.1 * rng.randn(N)).astype(np.float32).astype(np.float64)
  W = 0.2 * rng.randn(K, N)
  W[:, ZC] = 0.0
  W[K - 1, :] = 0.0
  W[8] = np.clip(W[8], -0.5, 0.5)
  W = _tame(x, W, bias)
  W[K - 1, :] = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
  W[K - 1, ZC] = 0.0
  rr = {'inf': 1, 'nan': rows // 2, 'big': rows - 1, 'sat30': 3, 'sat100': rows - 2}
  x[rr['inf'], 7] = np.inf
  x[rr['nan'], 9] = np.nan
  x[rr['big'], 8] = R.act_limits(f16)[1]
  for key, v in (('sat30', 30.0), ('sat100', -100.0)):
    x[rr[key]] = 0.0
    x[rr[key], K - 1] = v
  W32 = W.astype(np.float32).astype(np.float64)
  return x, W32, R.round_act(W32, f16), bias, rr


def exact_units(f16):
  """(x unit, W unit): powers of two; a product is a multiple of their product."""
  return 2.0**-3, 2.0**-2


def exact_recipe(seed, rows, K, N, f16):
  """Small integers times a power of two whose sums are exact in f32 and mostly
  NOT representable in the activation type.  Amplitude a with a^2 sqrt(K) / 3 ~
  2^11 (bf16) / 2^13 (fp16) product units: typical sums carry 3 .. 4 bits more than
  the type keeps.  Planted in the last six rows (rows >= 6, N >= 6, K >= 128), with
  x = s sign(W[:, n]) (where W[:, n] is not zero) driving column n to s sum |W[:, n]|:
    columns 0 .. 3 hold sum |W| = T + 1, T + 3, T + 5, T + 7 units (T = 2^8 / 2^11):
    exact ties of the type; columns 4 / 5 are driven beyond +- 1.5 x 65504 (fp16:
    +-inf; bf16: finite).
  Returns x, W (float64, exact in either type), the tie rows' expected values
  and the two overflow positions."""
  assert rows >= 6 and N >= 6 and K >= 128
  rng = np.random.RandomState(seed)
  ux, uw = exact_units(f16)
  a = int(np.sqrt(3 * (2.0**13 if f16 else 2.0**11) / np.sqrt(K)))
  xi = rng.randint(-a, a + 1, (rows, K)).astype(np.float64)
  wi = rng.randint(-a, a + 1, (K, N)).astype(np.float64)
  T = 2**11 if f16 else 2**8
  for j in range(4):  # tie columns: |entries| <= a that add up to T + 2 j + 1
    tgt, col, c = T + 2 * j + 1, np.zeros(K), 0
    while tgt > 0:
      v = min(a, tgt)
      col[c] = v if c % 2 == 0 else -v
      tgt -= v
      c += 1
    assert c <= K
    wi[:, j] = col
  r0 = rows - 6
  for j in range(4):
    # (one unit on the column's support; the random integers stay where W[c, j]
    # is zero, so the row's other columns are ordinary sums)
    on = wi[:, j] != 0
    xi[r0 + j, on] = np.sign(wi[on, j]) * (1 if j % 2 == 0 else -1)
  # overflow rows: s a power of two with s sum |W[:, n]| u > 1.5 x 65504
  for j, sgn in ((4, 1.0), (5, -1.0)):
    s = 2.0**np.ceil(np.log2(1.5 * 65504 / (np.abs(wi[:, j]).sum() * ux * uw)))
    assert s * ux <= 2.0**15
    xi[r0 + j] = sgn * s * np.sign(wi[:, j])
  x, W = xi * ux, wi * uw
  ties = [(r0 + j, j) for j in range(4)]
  over = [(r0 + 4, 4), (r0 + 5, 5)]
  return x, W, ties, over


def wgrad_recipe(seed, rows, Cx_real, Cg_real, f16):
  """x, g = round_act(randn); the first row starts with +-0 and the smallest
  subnormals where there is room."""
  rng = np.random.RandomState(seed)
  x = R.round_act(rng.randn(rows, Cx_real), f16)
  g = R.round_act(rng.randn(rows, Cg_real), f16)
  v = planted_row_start(f16)
  x[0, :min(6, Cx_real)] = v[:min(6, Cx_real)]
  return x, g


def group_signal(x, W):
  """|contribution| of every 8-term k-group to every output: (K / 8, rows, N)."""
  x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
  K = x.shape[1]
  return np.abs(np.stack([x[:, k:k + 8] @ W[k:k + 8] for k in range(0, K, 8)]))
