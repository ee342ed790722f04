"""CPU tests of the float64 statement of cg_swconv (tests/swconv_ref.py): it equals
float64 autograd of the oracle's layers behind O.phase_shuffle -- bit for bit on
the integer data of tests/test_hip_kernels.py --, an f32 evaluation of every real
recipe lies inside its bar, every mutant of the statement moves at least half of
the outputs it touches by 20 bars or more, the exact recipe's sums are exact in
f32 and need rounding, and every admissible dispatch target is among the
collected cases of tests/test_hip_swconv.py."""
import itertools

import numpy as np
import pytest
import torch

import oracle as O
from calciumgan_amd import _lib

import pointwise_ref as R
import swconv_ref as S
import wgrad_ref as W

F64 = torch.float64


def ints(rng, shape, lo=-3, hi=3, scale=1.0):
  return rng.randint(lo, hi + 1, size=shape).astype(np.float64) * scale


def t64(a):
  return torch.tensor(np.asarray(a, np.float64), dtype=F64)


def shuffle_batch(x, shifts, seg):
  return torch.cat([O.phase_shuffle(x[b:b + 1], int(shifts[b // seg]))
                    for b in range(x.shape[0])], 0)


def up_weights(Wk, k):
  """Wl[z][j][c = b][n = a] = W[t0_z - 2 j][a][b], t0_z = ((z + pl) & 1) + k - 2: the tap walk
  of the two output phases of the transposed convolution (nets._transpose_phases)."""
  pl = (k - 2) // 2
  out = []
  for z in (0, 1):
    t0 = ((z + pl) & 1) + k - 2
    out.append(np.stack([Wk[t0 - 2 * j].T for j in range(k // 2)]))
  return np.stack(out)


# ---------------------------------------------------------------------------
# the statement against autograd of the oracle's layers (integer data: equal
# bit for bit, as the references of tests/test_hip_kernels.py are)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('nB,L,Ci,Co,k,seg', [(4, 16, 64, 72, 8, 2), (3, 128, 38, 40, 24, 1)])
def test_stride2_forward_is_conv1d(nB, L, Ci, Co, k, seg):
  rng = np.random.RandomState(1)
  x, Wk, b = ints(rng, (nB, L, Ci)), ints(rng, (k, Ci, Co), -2, 2, 0.5), ints(rng, (Co,), -4, 4)
  shifts = rng.randint(-2, 3, size=-(-nB // seg))
  ref = O.leaky_relu(O.conv1d_same(shuffle_batch(t64(x), shifts, seg), t64(Wk), t64(b), 2))
  G = S.down(nB, L // 2, k, Ci, Co, shifts, seg)
  y, own = S.swconv(G, x, Wk[None], b, S.EPI_LRELU, O.LEAKY_ALPHA)
  assert own.all()
  np.testing.assert_array_equal(y, ref.numpy())


@pytest.mark.parametrize('nB,L,Ci,Co,k', [(4, 16, 64, 72, 8), (2, 64, 16, 40, 24)])
def test_two_phase_launch_is_the_input_gradient(nB, L, Ci, Co, k):
  rng = np.random.RandomState(3)
  Wk, dy = ints(rng, (k, Ci, Co), -2, 2, 0.5), ints(rng, (nB, L // 2, Co))
  x = torch.zeros(nB, L, Ci, dtype=F64, requires_grad=True)
  (O.conv1d_same(x, t64(Wk), None, 2) * t64(dy)).sum().backward()
  G = S.up(nB, L // 2, k, Co, Ci)
  y, own = S.swconv(G, dy, up_weights(Wk, k))
  assert own.all()
  np.testing.assert_array_equal(y, x.grad.numpy())


@pytest.mark.parametrize('B,L,Ci,Co,k', [(3, 16, 32, 102, 24), (2, 4, 32, 6, 8)])
def test_transposed_forward_layernorm_lrelu(B, L, Ci, Co, k):
  rng = np.random.RandomState(4)
  x, Wt, b = ints(rng, (B, L, Ci)), ints(rng, (k, 1, Co, Ci), -2, 2, 0.5), ints(rng, (Co,), -4, 4)
  pre_ref = O.conv1d_transpose_same(t64(x), t64(Wt), t64(b), 2)
  G = S.up(B, L, k, Ci, Co)
  pre, own = S.swconv(G, x, up_weights(Wt[:, 0], k), b)
  np.testing.assert_array_equal(pre, pre_ref.numpy())
  gamma, beta = rng.rand(Co) + 0.5, 0.1 * rng.randn(Co)
  for f16 in (False, True):
    y, h, mean, rstd = S.layernorm(pre / 8, gamma, beta, O.LN_EPS, O.LEAKY_ALPHA, f16)
    yq = t64(R.round_act(pre / 8, f16))
    ref = O.leaky_relu(O.layer_norm(yq, t64(gamma), t64(beta)))
    np.testing.assert_array_equal(y, yq.numpy())
    np.testing.assert_allclose(h, ref.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(mean, yq.mean(-1).numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(rstd, torch.rsqrt(yq.var(-1, unbiased=False) + O.LN_EPS).numpy(),
                               rtol=1e-12)


@pytest.mark.parametrize('B,L,Ci,Co,k', [(2, 64, 32, 40, 24), (3, 8, 64, 38, 8)])
def test_stride2_launch_is_the_transposed_input_gradient(B, L, Ci, Co, k):
  rng = np.random.RandomState(5)
  Wt, dy = ints(rng, (k, 1, Co, Ci), -2, 2, 0.5), ints(rng, (B, 2 * L, Co))
  x = torch.zeros(B, L, Ci, dtype=F64, requires_grad=True)
  (O.conv1d_transpose_same(x, t64(Wt), None, 2) * t64(dy)).sum().backward()
  G = S.down(B, L, k, Co, Ci)
  y, _ = S.swconv(G, dy, Wt[:, 0][None])
  np.testing.assert_array_equal(y, x.grad.numpy())


def test_one_tap_dense_sigmoid():
  rng = np.random.RandomState(6)
  x, Wd, b = ints(rng, (2, 64, 38), -3, 3, 0.25), ints(rng, (38, 102), -2, 2, 0.125), ints(
      rng, (102,), -2, 2, 0.5)
  G = S.dense(2, 64, 38, 102)
  y, _ = S.swconv(G, x, Wd[None, None], b, S.EPI_SIGMOID)
  ref = torch.sigmoid(t64(x) @ t64(Wd) + t64(b))
  np.testing.assert_allclose(y, ref.numpy(), rtol=1e-14)
  lin, _ = S.swconv(G, x, Wd[None, None], b)
  np.testing.assert_array_equal(lin, (t64(x) @ t64(Wd) + t64(b)).numpy())


@pytest.mark.parametrize('side_rows', [2, 4])
def test_out_shifts_and_fixup_are_the_adjoint_of_lrelu_phase_shuffle(side_rows):
  """h -> LeakyReLU -> PhaseShuffle -> stride-2 convolution: the gradient with
  respect to h, from autograd, equals the two-phase launch with out_shifts followed
  by cg_unshuffle_fixup (integer data: the stores round nothing)."""
  rng = np.random.RandomState(7)
  nB, L, Ci, Co, k, alpha = 3, 16, 32, 40, 8, 0.25
  shifts = (2, -2, 0)
  Wk, dy = ints(rng, (k, Ci, Co), -1, 1), ints(rng, (nB, L // 2, Co), -1, 1)
  hv = ints(rng, (nB, L, Ci), -2, 2)
  h = t64(hv).requires_grad_(True)
  s = shuffle_batch(O.leaky_relu(h, alpha), shifts, 1)
  (O.conv1d_same(s, t64(Wk), None, 2) * t64(dy)).sum().backward()
  G = S.up(nB, L // 2, k, Co, Ci)
  Wl = up_weights(Wk, k)
  for f16 in (False, True):
    y, y_own, side, side_own = S.swconv_out_shifts(G, dy, Wl, shifts, 1, side_rows, f16,
                                                   None, S.EPI_MASK, alpha, hv)
    assert np.array_equal(R.round_act(y, f16), y)  # (representable: nothing is rounded)
    for b, sft in enumerate(shifts):
      assert side_own[b].sum() == abs(sft) and y_own[b].sum() == L - abs(sft)
    delta = np.where(y_own[:, :, None], y, -777.0)  # unowned rows: whatever was there
    got = S.unshuffle_fixup(side, hv, delta, shifts, 1, alpha)
    np.testing.assert_array_equal(got, h.grad.numpy())
  # without the mask epilogue the direct rows hold the unmasked gradient
  y0 = S.swconv_out_shifts(G, dy, Wl, shifts, 1, side_rows, False)[0]
  e, _ = S.swconv(G, dy, Wl)
  for b, sft in enumerate(shifts):
    td, r, ts, j = S.out_shift_rows(sft, L)
    np.testing.assert_array_equal(y0[b, r], e[b, td])
    np.testing.assert_array_equal(r, W.shuffle_src(td, sft, L))


# ---------------------------------------------------------------------------
# bars and mutants on the real recipe
# ---------------------------------------------------------------------------
REAL = S.real_geoms()


@pytest.mark.parametrize('G', REAL, ids=S.gid)
@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'f16'])
def test_f32_evaluation_lies_inside_the_bar(G, f16):
  x, Wl, bias = S.real_recipe(G, f16)
  lin = S.linear(G, x, Wl, bias)
  emu = S.linear_f32(G, x, Wl, bias).astype(np.float64)
  bar = S.acc_bound(G, x, Wl, bias)
  assert (np.abs(S.place(G, emu)[0] - S.place(G, lin)[0]) <= bar).all()
  assert K_ok(G)


def K_ok(G):
  return S.K_of(G) <= 24 * 96


def window_touch(G, rows_of_x):
  """Outputs whose window holds one of the flagged rows of the UNSHUFFLED x
  ((nB, Lx) bool), in the geometry of y."""
  ind = np.repeat(rows_of_x[:, :, None].astype(np.float64), G.Cr, axis=2)
  return S.place(G._replace(shifts=None), S.linear(G._replace(shifts=None), ind,
                                                   np.ones(S.wshape(G))))[0] > 0


def moved(y0, y1, bar, touched):
  assert touched.sum() >= 8
  return np.mean(np.abs(y1 - y0)[touched] >= 20 * bar[touched])


@pytest.mark.parametrize('G', REAL, ids=S.gid)
@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'f16'])
def test_statement_mutants_move_half_of_what_they_touch_by_20_bars(G, f16):
  x, Wl, bias = S.real_recipe(G, f16)
  alpha = R.f32(0.3)
  EPI = S.sweep_epi(G)
  y0, _ = S.swconv(G, x, Wl, bias, EPI, alpha)
  lin0 = S.place(G, S.linear(G, x, Wl, bias))[0]
  bar = S.epilogue_bound(S.acc_bound(G, x, Wl, bias), lin0, y0, EPI)
  everything = np.ones(y0.shape, bool)
  # a dropped 32-deep K-step: the middle tap's first 32 channels
  tap = G.taps // 2
  Wd = Wl.copy()
  Wd[:, tap, :32, :] = 0.0
  u = np.arange(G.Lu)
  hit = np.zeros((G.nphase, G.nB, G.Lu, G.N))
  for z in range(G.nphase):
    r = G.stride * u + G.off + z * G.off_step + tap
    hit[z][:, (r >= 0) & (r < G.Lx)] = 1.0
  assert moved(y0, S.swconv(G, x, Wd, bias, EPI, alpha)[0], bar,
               S.place(G, hit)[0] > 0) >= 0.5
  # a tap off by one row
  assert moved(y0, S.swconv(G, x, Wl, bias, EPI, alpha, off_delta=1)[0], bar,
               everything) >= 0.5
  if G.nphase == 2:  # the two phases swapped
    assert moved(y0, S.swconv(G, x, Wl[::-1], bias, EPI, alpha)[0], bar,
                 everything) >= 0.5
  if G.shifts is not None:  # reflected rows read unshuffled
    refl = np.zeros((G.nB, G.Lx), bool)
    for b in range(G.nB):
      refl[b, W.reflected_rows(G.shifts[b // G.seg], G.Lx)] = True
    # (the window is flagged where the SHUFFLED row t is a reflected one; shifts of
    # zero reflect no row: the mutant touches nothing there)
    assert not refl.any() or moved(y0, S.swconv(G, x, Wl, bias, EPI, alpha, plain_reflected=True)[0],
                 bar, window_touch(G, refl)) >= 0.5
  if G.stride == 2:  # the even / odd tap groups of a parity-major operand swapped
    perm = np.arange(G.taps).reshape(-1, 2)[:, ::-1].ravel()
    assert moved(y0, S.swconv(G, x, Wl[:, perm], bias, EPI, alpha)[0], bar,
                 everything) >= 0.5
  # the bias added after the epilogue: wherever the slope applies on either side
  acc = S.place(G, S.linear(G, x, Wl))[0]
  y0 = S.swconv(G, x, Wl, bias, S.EPI_LRELU, alpha)[0]
  bar = S.epilogue_bound(S.acc_bound(G, x, Wl, bias), lin0, y0, S.EPI_LRELU)
  assert moved(y0, S.swconv(G, x, Wl, bias, S.EPI_LRELU, alpha, bias_after=True)[0], bar,
               (acc < 0) | (lin0 < 0)) >= 0.5
  # alpha for mask_src >= 0 instead of > 0: on the elements whose mask is +-0
  rng = np.random.RandomState(5)
  mask = R.round_act(rng.randn(*y0.shape), f16)
  mask[:, :, 0::3], mask[:, :, 1::3] = 0.0, -0.0
  ym = S.swconv(G, x, Wl, bias, S.EPI_MASK, alpha, mask)[0]
  barm = S.epilogue_bound(S.acc_bound(G, x, Wl, bias), lin0, ym, S.EPI_MASK)
  assert moved(ym, S.swconv(G, x, Wl, bias, S.EPI_MASK, alpha, mask, ge=True)[0], barm,
               mask == 0) >= 0.5


def test_exact_only_lists_what_cannot_hold():
  assert all(G not in REAL for G in S.EXACT_ONLY)


# ---------------------------------------------------------------------------
# the exact recipe
# ---------------------------------------------------------------------------
MIN_UNREPRESENTABLE = 0.5  # (sums of >= 1 in units of 2^-9 / 2^-12: at most 1/4 representable;
                           # the smallest shapes hold many sums below 1)


@pytest.mark.parametrize('G', REAL + S.K_MULTI_EXACT_ONLY, ids=S.gid)
@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'f16'])
def test_exact_recipe_is_exact_in_f32_and_needs_rounding(G, f16):
  x, Wl, bias, plants = S.exact_recipe(G, f16)
  assert np.array_equal(R.round_act(x, f16), x) and np.array_equal(R.round_act(Wl, f16), Wl)
  unit = 2.0**-12 if f16 else 2.0**-9
  y, own = S.swconv(G, x, Wl, bias)
  mag = S.place(G, S.linear(G, np.abs(x), np.abs(Wl), np.abs(bias)))[0]
  rest = np.ones(G.N, bool)
  rest[2:4] = False  # the overflow columns: two terms of 2^15 at the plant, else two x
  assert (mag[:, own][:, :, rest] / unit < 2.0**24).all()
  assert np.array_equal(np.round(y / unit), y / unit)
  assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
  # (x 1/4, the exact recipe's slope, keeps every value a multiple of unit / 4 below 2^22 units)
  assert np.mean(R.round_act(y[:, own], f16) != y[:, own]) >= MIN_UNREPRESENTABLE
  lo, hi = (-1, 1)
  for b, t, n, v in plants['ties']:
    assert y[b, t, n] == v
    r = R.round_act(v, f16)
    other = r + np.sign(v - r) * R.ulp_act(v, f16)
    assert r != v and abs(v - r) == abs(other - v)          # an exact tie ...
    assert (r / R.ulp_act(v, f16)) % 2 == 0                  # ... rounded to even
  downs = [R.round_act(v, f16) < v for _, _, _, v in plants['ties']]
  assert sorted(downs) == [False, True]                      # one each way
  for b, t, n, sgn in plants['over']:
    assert y[b, t, n] == sgn * 2.0**16
    assert R.round_act(y[b, t, n], f16) == (sgn * np.inf if f16 else sgn * 2.0**16)


def test_subnormal_recipe_has_one_exact_product_per_output():
  for f16 in (False, True):
    G = S.CLASSIC_DOWN[0]
    x, Wl = S.subnormal_recipe(G, f16)
    tiny, _ = R.act_limits(f16)
    assert (np.abs(x) < D_min_normal(f16)).all() and (np.abs(x) >= tiny).all()
    assert np.array_equal(R.round_act(x, f16), x)
    assert (np.count_nonzero(Wl, axis=(1, 2)) == 1).all()
    y, _ = S.swconv(G, x, Wl)
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y) and (y != 0).mean() > 0.5
    assert not S.swconv(G, S.flush(x, f16), Wl)[0].any()


def D_min_normal(f16):
  return 2.0**-14 if f16 else 2.0**-126


# ---------------------------------------------------------------------------
# every admissible dispatch target is a collected case
# ---------------------------------------------------------------------------
def _key(G, kw):
  uni = (kw.get('CK', 32) // 8) % 4 == 0
  # (the software-pipelined tiles do not consult split_parity)
  sp = kw.get('sp', 0) if kw['tile'] < 9 else 0
  return (kw['tile'], kw.get('ks', 2), G.stride, uni, sp, kw.get('narrow', 0),
          kw.get('epi') == S.EPI_LN)


def test_every_admissible_dispatch_target_is_collected():
  """(tile, stage depth, stride, UNI / non-UNI, split_parity, narrow, LN) over every
  combination cg_swconv_check admits in either build, enumerated here without the
  test file's own list; and the four lean forms on tiles 13 - 15."""
  import test_hip_swconv as T
  geoms = [(S.CLASSIC_DOWN[0], 32), (S.CLASSIC_UP[0], 32), (S.NON_UNI, 40),
           (S.NON_UNI_UP, 40), (S.CLASSIC_DOWN[3], 32), (S.SWP_DOWN, 32),
           (S.SWP_DOWN_NARROW, 32), (S.SWP_UP, 32)] + [(G, 32) for G in S.LN_GEOMS]
  try:
    for build in ('bf16', 'f16'):
      _lib.use(build)
      have = {}
      for p in T.dispatch_cases():
        G, kw, exact_only = p.values
        have.setdefault(_key(G, kw), set()).update(T.recipes_of(G, exact_only))
        assert 'exact' in T.recipes_of(G, exact_only)
        assert 'real' in T.recipes_of(G, exact_only) or G in S.EXACT_ONLY
        assert G in S.EXACT_ONLY or G in REAL, S.gid(G)
      # the classic tiles' further shapes: each on both MFMA shapes, both recipes
      for G in S.CLASSIC_MORE:
        mf = set(T.CLASSIC_MF[p.values[1]['tile']] for p in T.dispatch_cases()
                 if p.values[0] == G and T.recipes_of(*p.values[::2]) == ('real', 'exact'))
        assert mf == {16, 32}, S.gid(G)
      # Lu = the tile's rows and twice that on every classic tile, the tile's rows on
      # every software-pipelined one
      for tile in T.CLASSIC + T.SWP:
        rows = T.rows_of_tile(tile)
        lus = set(p.values[0].Lu for p in T.dispatch_cases() if p.values[1]['tile'] == tile)
        assert rows in lus and (tile in T.SWP or 2 * rows in lus), tile
      lean = set((p.values[2]['tile'], p.values[0]) for p in T.lean_cases())
      assert lean == set(itertools.product(T.LEAN, ('lrelu', 'mask', 'maskshift', 'lrelussq')))
      n = 0
      for (G, CK), tile, ks, sp, pm, nar, ln in itertools.product(
          geoms, range(16), (2, 4), (0, 1), (0, 1), (0, 1), (0, 1)):
        if tile >= 9 and ks == 4:
          continue  # (the software-pipelined tiles have one stage depth)
        if G.stride == 1 and (sp or pm or nar):
          continue  # (stride 2 only: the fields are not consulted)
        if nar and not (G.Cx - 32 < G.Cr <= G.Cx - 24 and G.Cx >= 64):
          continue  # (no operand of this geometry is packed narrow)
        kw = dict(tile=tile, ks=ks, sp=sp, pmajor=pm, narrow=nar, CK=CK,
                  epi=S.EPI_LN if ln else S.EPI_LRELU)
        if T.admits(T.desc_of(G, **kw)):
          n += 1
          assert have.get(_key(G, kw)) == {'real', 'exact'}, (build, S.gid(G), kw)
      assert n > 100
  finally:
    _lib.use('bf16')


def test_tap_sweep_is_collected_at_every_kernel_size():
  """The dispatch key above does not hold the tap count.  Per kernel size of
  swconv_ref.TAP_SWEEP, in either build: tiles 0, 1, 2 at both stage depths and tile 4
  run the stride-2 launch, the narrow one (6 taps and up) and the two phases; the
  three-chunk geometry runs on tiles 1 and 4; split-parity staging on tile 1 is
  collected exactly where a parity's K groups fill whole stages (k a multiple of 4
  at 2 K-steps per stage, of 8 at 4), plain and narrow; the LayerNorm tiles run k = 6
  and 22.  Nothing the check refuses drops a case of this list silently."""
  import test_hip_swconv as T
  try:
    for build in ('bf16', 'f16'):
      _lib.use(build)
      got = set()
      for p in T.dispatch_cases():
        G, kw, exact_only = p.values
        got.add((G, kw['tile'], kw.get('ks', 2), kw.get('sp', 0), kw.get('narrow', 0),
                 kw['epi'] == S.EPI_LN))
      for k in S.TAP_SWEEP:
        for tile, ks in T.SWEEP_TILES:
          assert (S.K_DOWN[k], tile, ks, 0, 0, False) in got, (build, k, tile, ks)
          assert (S.K_UP[k], tile, ks, 0, 0, False) in got, (build, k, tile, ks)
          if k >= 6:
            assert (S.K_DOWN_NARROW[k], tile, ks, 0, 1, False) in got, (build, k, tile, ks)
        for tile, ks in ((1, 2), (1, 4), (4, 2)):
          assert (S.K_DOWN_MULTI[k], tile, ks, 0, 0, False) in got, (build, k, tile, ks)
        for ks in (2, 4):
          whole = k % (2 * ks) == 0
          assert ((S.K_DOWN[k], 1, ks, 1, 0, False) in got) == whole, (build, k, ks)
          if k >= 6:
            assert ((S.K_DOWN_NARROW[k], 1, ks, 1, 1, False) in got) == whole, (build, k, ks)
      for k in (6, 22):
        for tile in T.LN_CLASSIC:
          for ks in (2, 4):
            assert (S.K_UP_LN[k], tile, ks, 0, 0, True) in got, (build, k, tile, ks)
      # the geometries reach what the sweep is for
      assert all(S.K_UP[k].off_step == (0 if k % 4 == 2 else 1) for k in S.TAP_SWEEP)
      assert any((4 * S.K_UP[k].taps) % 16 for k in S.TAP_SWEEP)
  finally:
    _lib.use('bf16')
