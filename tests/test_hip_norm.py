"""Float64 parity of the normalisation family of calciumgan_amd/csrc/pointwise.hip
in both precision builds: cg_ln_lrelu_fwd (ln_fwd_kernel, ln_fwd8_kernel<2..8>),
cg_ln_lrelu_bwd (ln_bwd_kernel and the ordered finish), cg_bn_stats, cg_bn_apply,
cg_bn_bwd and cg_unshuffle_mask, at the smallest shapes that reach each path.

Every case is one entry-point call on valid input, compared with the float64
statement of tests/norm_ref.py (tied to autograd in tests/test_norm_ref.py, which
also caps every bar below the old tests' tolerances).  Inputs are random reals
rounded to the type the kernel reads, with planted +-0, the smallest subnormal,
a large value, a constant row / column (variance exactly 0) and zeros of both
signs in h where the mask is decided.  Channels [C, Cp) of every activation input
of the LN and BN entries are NaN (they mask by c < C); cg_unshuffle_mask does not
mask: its padding is zero and must come out as +0.  Every output is over-allocated
and pre-filled with a sentinel: guard rows and guard elements must still hold it,
channels [C, Cp) of a stored activation must be +0.  The workspace starts as NaN.
Bars: bit-equal, or one activation ulp plus the derived f32 bar, or sum_bound plus
per-term bars (norm_ref) -- never a measured number.

Row counts sit around the block of each path, blk = 4 * rpw * rows_per_slot, computed
here from the same rule as the host code.

Out of scope: the kMaxParts and workspace caps of bn_rows_per_block need more than
8M rows (2048 blocks of 4096 rows); they are not reached here.  Where a row count
would make the float64 reference slow, C is reduced and the pitch and the row
count -- which select the path -- are kept."""
import numpy as np
import pytest
import torch

from calciumgan_amd import _lib

import hip_utils as H
import norm_ref as N
import pointwise_ref as R
import test_hip_pointwise as P
from test_hip_pointwise import precision, _back_to_bf16  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

U = R.U32
EINVAL = _lib.CG_EINVAL
GUARD = 3                 # guard rows behind every activation output
G32 = 5                   # guard elements behind every f32 output
A32 = R.f32(0.3)
EPS = R.f32(1e-3)
MOM = R.f32(0.99)
NAN = float('nan')


# ---------------------------------------------------------------------------
# the host code's launch rules
# ---------------------------------------------------------------------------
def lanes_per_row(Cp):
  lpr = 1
  while lpr * 8 < Cp:
    lpr *= 2
  return lpr


def rows_per_slot_for(rows, rpw, lo, hi):
  want = rows // (rpw * 8192)
  rps = lo
  while rps * 2 <= want and rps * 2 <= hi:
    rps *= 2
  return rps


def is_fwd8(Cp):
  """The pitches cg_ln_lrelu_fwd routes to ln_fwd8_kernel (CALCIUMGAN_LN_POW2 unset)."""
  return lanes_per_row(Cp) * 8 != Cp and Cp >= 64


def fwd_rule(Cp):
  """(rpw, lo, hi) of the forward kernel a pitch goes to."""
  return (8, 2, 8) if is_fwd8(Cp) else (64 // lanes_per_row(Cp), 4, 8)


def bwd_rule(Cp, ws):
  return (64 // lanes_per_row(Cp),) + ((4, 16) if ws else (16, 64))


def blk_of(rule, rows):
  rpw, lo, hi = rule
  return 4 * rpw * rows_per_slot_for(rows, rpw, lo, hi)


def row_counts(rule):
  """1, one short of a block, one past it, three blocks and five rows -- at the minimum
  rows_per_slot, which every one of them keeps (asserted)."""
  blk = 4 * rule[0] * rule[1]
  out = [1, blk - 1, blk + 1, 3 * blk + 5]
  assert all(blk_of(rule, r) == blk for r in out)
  return out


# ---------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------
def pitched(x, Cp, f16, pad=NAN):
  """(rows, C) float64 values of the activation type -> device (rows, Cp), channels
  [C, Cp) = pad."""
  rows, C = x.shape
  out = torch.full((rows, Cp), pad, dtype=R.act_dtype(f16), device=H.DEV)
  out[:, :C] = P.dev_act(x, f16)
  return out


def vec32(x, guard=NAN):
  """f32 input vector followed by G32 elements the kernel must not read into a result."""
  return P.dev32(np.r_[np.asarray(x, np.float64), np.full(G32, guard)])


def out_act(rows, Cp, f16):
  return P.sent_act((rows + GUARD, Cp), f16)


def out32(n, zero=False):
  t = P.sent32(n + G32)
  if zero:
    t[:n] = 0.0
  return t


def check_act(out, rows, C, want, f16, err, what='', zero_sign=True):
  """Rows [0, rows) x channels [0, C) within one ulp + err of round_act(want); channels
  [C, Cp) +0; the guard rows untouched.  zero_sign False: where the float64 result is an
  exact zero because terms CANCEL (do - dbeta / R with one row), not because a factor is
  +-0, no sign is prescribed -- the sign of such a zero depends on the order of the sums --
  and the stored value is held to the bar alone."""
  assert P.is_sentinel(out[rows:]), what + ': guard rows'
  if out.shape[1] > C:
    assert int(out[:rows, C:].view(torch.int16).count_nonzero()) == 0, what + ': padding'
  if zero_sign:
    P.assert_act(out[:rows, :C], want, f16, err)
    return
  g, r = P.host(out[:rows, :C]), R.round_act(want, f16)
  fin = np.isfinite(r)
  assert np.array_equal(g[~fin], r[~fin]), what
  bad = np.argwhere(fin & ~(np.abs(g - np.where(fin, r, 0.0)) <= R.ulp_act(r, f16) + err))
  assert bad.size == 0, (what, bad[:5], g[tuple(bad[0])], r[tuple(bad[0])])


def check32(out, n, want, bar, what=''):
  assert P.is_sentinel(out[n:]), what + ': guard elements'
  P.assert_f32(out[:n], want, bar, what)


# ---------------------------------------------------------------------------
# cg_ln_lrelu_fwd
# ---------------------------------------------------------------------------
POW2 = [(5, 8), (16, 16), (30, 32), (64, 64), (102, 128), (256, 256), (500, 512)]
IDLE = [(20, 24), (33, 40), (56, 56)]
FWD8 = [(65, 72), (192, 192), (224, 224), (300, 320), (384, 384), (400, 416),
        (450, 456), (504, 504)]
LN_FWD_CASES = [(C, Cp, rows) for C, Cp in POW2 + IDLE + FWD8
                for rows in row_counts(fwd_rule(Cp))]


def test_ln_dispatch_of_the_listed_pitches():
  import os
  assert 'CALCIUMGAN_LN_POW2' not in os.environ
  assert sorted((Cp // 8 + 7) // 8 for _, Cp in FWD8) == [2, 3, 4, 5, 6, 7, 8, 8]
  for _, Cp in FWD8:
    assert is_fwd8(Cp)
  for _, Cp in POW2:
    assert lanes_per_row(Cp) * 8 == Cp
  for _, Cp in IDLE:
    assert lanes_per_row(Cp) * 8 > Cp and not is_fwd8(Cp)
  # both a full multiple of 64 and pitches that leave groups of the last pass empty
  assert any(Cp % 64 == 0 for _, Cp in FWD8) and any(Cp % 64 for _, Cp in FWD8)


def ln_fwd_launch(yd, gd, bd, rows, C, Cp, f16, stats=True):
  h = out_act(rows, Cp, f16)
  mean, rstd = (out32(rows), out32(rows)) if stats else (None, None)
  _lib.call('cg_ln_lrelu_fwd', H.p(yd), H.p(gd), H.p(bd), H.p(h), H.p(mean), H.p(rstd),
            rows, C, Cp, EPS, A32, H.stream())
  H.sync()
  return h, mean, rstd


def ln_fwd_check(y, gamma, beta, h, mean, rstd, C, f16, r0=0):
  """Rows [r0, r0 + len(y)) of the outputs against the statement."""
  n = y.shape[0]
  f = N.ln_fwd(y, gamma, beta, EPS, A32, f16)
  P.assert_f32(mean[r0:r0 + n], f['mean'], f['e_mean'], 'mean')
  P.assert_f32(rstd[r0:r0 + n], f['rstd'], f['e_rstd'], 'rstd')
  P.assert_act(h[r0:r0 + n, :C], f['h'], f16, f['e_h'])


@pytest.mark.parametrize('C,Cp,rows', LN_FWD_CASES)
def test_ln_fwd(C, Cp, rows, precision):
  f16 = precision
  y, gamma, beta, _ = N.ln_recipe(1000 + Cp + rows, rows, C, f16)
  yd, gd, bd = pitched(y, Cp, f16), vec32(gamma), vec32(beta)
  h, mean, rstd = ln_fwd_launch(yd, gd, bd, rows, C, Cp, f16)
  f = N.ln_fwd(y, gamma, beta, EPS, A32, f16)
  check32(mean, rows, f['mean'], f['e_mean'], 'mean')
  check32(rstd, rows, f['rstd'], f['e_rstd'], 'rstd')
  check_act(h, rows, C, f['h'], f16, f['e_h'], 'h')
  if rows > 1:  # the constant row: the data's variance is exactly 0
    assert f['rstd'][1] == 1.0 / np.sqrt(EPS)
  # without the statistics: the same bits of h
  h2, _, _ = ln_fwd_launch(yd, gd, bd, rows, C, Cp, f16, stats=False)
  assert torch.equal(P.bits(h2), P.bits(h))


@pytest.mark.parametrize('C,Cp', [(500, 512), (65, 72)])
def test_ln_fwd_rows_past_the_doubling_of_rows_per_slot(C, Cp, precision):
  f16 = precision
  rule = fwd_rule(Cp)
  rpw, lo, hi = rule
  rows = 2 * lo * rpw * 8192 + 3
  assert rows_per_slot_for(rows, *rule) == 2 * lo
  assert rows_per_slot_for(rows - 4, *rule) == lo
  rng = np.random.RandomState(Cp)
  gamma = (rng.rand(C) + 0.5).astype(np.float32).astype(np.float64)
  beta = (0.1 * rng.randn(C)).astype(np.float32).astype(np.float64)
  yd = torch.full((rows, Cp), NAN, dtype=R.act_dtype(f16), device=H.DEV)
  yd[:, :C] = (torch.randn(rows, C, device=H.DEV,
                           generator=torch.Generator(H.DEV).manual_seed(Cp)) * 2 +
               0.5).to(R.act_dtype(f16))
  h, mean, rstd = ln_fwd_launch(yd, vec32(gamma), vec32(beta), rows, C, Cp, f16)
  assert P.is_sentinel(h[rows:]) and P.is_sentinel(mean[rows:]) and P.is_sentinel(rstd[rows:])
  if Cp > C:
    assert int(h[:rows, C:].view(torch.int16).count_nonzero()) == 0
  # the reference in row chunks
  step = 8192
  for r0 in range(0, rows, step):
    y = P.host(yd[r0:r0 + step, :C])
    ln_fwd_check(y, gamma, beta, h, mean, rstd, C, f16, r0)


# ---------------------------------------------------------------------------
# cg_ln_lrelu_bwd
# ---------------------------------------------------------------------------
LN_BWD_PITCHES = [(5, 8), (30, 32), (33, 40), (102, 128), (300, 320), (500, 512)]
LN_BWD_CASES = [(C, Cp, rows) for C, Cp in LN_BWD_PITCHES
                for rows in row_counts(bwd_rule(Cp, True))]


def ln_bwd_inputs(C, Cp, rows, f16, given, seed):
  """given 'fwd': h, mean, rstd are the kernel-forward's outputs (zeros then planted in
  h); 'any': arbitrary f32 statistics, an rstd that is not 1 / sqrt(var + eps) of the data,
  and an h of its own."""
  y, gamma, beta, dh = N.ln_recipe(seed, rows, C, f16, big=False)
  if given == 'fwd':
    hd, md, rd = ln_fwd_launch(pitched(y, Cp, f16), vec32(gamma), vec32(beta), rows, C, Cp,
                               f16)
    h, mean, rstd = P.host(hd[:rows, :C]), P.host(md[:rows]), P.host(rd[:rows])
  else:
    rng = np.random.RandomState(seed + 1)
    h = R.round_act(rng.randn(rows, C), f16)
    mean = (0.5 * rng.randn(rows)).astype(np.float32).astype(np.float64)
    rstd = rng.uniform(0.3, 2.0, rows).astype(np.float32).astype(np.float64)
  N.plant_mask_zeros(h, dh)
  return y, gamma, dh, h, mean, rstd


def ln_bwd_run(y, gamma, dh, h, mean, rstd, C, Cp, f16, forms):
  """The entry point in each of `forms` = (ws, dbias) against the statement; the ordered
  form twice (bit for bit).  Returns the number of blocks of the ws form."""
  rows = y.shape[0]
  ref = N.ln_bwd(dh, h, y, mean, rstd, gamma, A32)
  dev = [pitched(a, Cp, f16) for a in (dh, h, y)]
  md, rd, gd = vec32(mean), vec32(rstd), vec32(gamma)
  for use_ws, use_dbias in forms:
    runs = []
    for _ in range(2 if use_ws else 1):
      ws = H.reduce_ws() if use_ws else None
      dy = out_act(rows, Cp, f16)
      dg, db = out32(C, not use_ws), out32(C, not use_ws)
      dbias = out32(C, not use_ws) if use_dbias else None
      _lib.call('cg_ln_lrelu_bwd', H.p(dev[0]), H.p(dev[1]), H.p(dev[2]), H.p(md), H.p(rd),
                H.p(gd), H.p(dy), H.p(dg), H.p(db), H.p(dbias), rows, C, Cp, A32, H.p(ws),
                H.stream())
      H.sync()
      runs.append((dy, dg, db) + ((dbias,) if use_dbias else ()))
    what = 'ws={} dbias={}'.format(use_ws, use_dbias)
    if use_ws:
      for a, b in zip(*runs):
        assert torch.equal(P.bits(a), P.bits(b)), what + ': repeat'
    check_act(dy, rows, C, ref['dy'], f16, ref['e_dy'], what + ' dy')
    check32(dg, C, ref['dgamma'], ref['e_dgamma'], what + ' dgamma')
    check32(db, C, ref['dbeta'], ref['e_dbeta'], what + ' dbeta')
    if use_dbias:  # the column sums of the dy this very launch stored
      want, bar = N.dbias(P.host(dy[:rows, :C]))
      check32(dbias, C, want, bar, what + ' dbias')


ALL_FORMS = [(True, True), (True, False), (False, True), (False, False)]


@pytest.mark.parametrize('given', ['fwd', 'any'])
@pytest.mark.parametrize('C,Cp,rows', LN_BWD_CASES)
def test_ln_bwd(C, Cp, rows, given, precision):
  f16 = precision
  args = ln_bwd_inputs(C, Cp, rows, f16, given, 2000 + Cp + rows)
  ln_bwd_run(*args, C, Cp, f16, ALL_FORMS)


@pytest.mark.parametrize('C,Cp', [(5, 8), (300, 320)])
def test_ln_bwd_rows_around_the_block_of_the_atomics_form(C, Cp, precision):
  """ws == NULL runs longer blocks (rows_per_slot from 16): its own block boundaries."""
  f16 = precision
  rule = bwd_rule(Cp, False)
  for rows in row_counts(rule)[1:3]:
    args = ln_bwd_inputs(C, Cp, rows, f16, 'any', 2500 + Cp + rows)
    ln_bwd_run(*args, C, Cp, f16, [(False, True)])


@pytest.mark.parametrize('nblocks', [16, 17, 113, 129])
def test_ln_bwd_block_counts_of_the_ordered_finish(nblocks, precision):
  """finish_cols_kernel adds partial rows j, j + 16, ... per wave, eight at a time while r +
  112 < nparts: 16 blocks (one row per wave), 17 (a second row for wave 0), 113 (the last
  count the unrolled loop does not enter), 129 (one unrolled pass and a tail)."""
  f16 = precision
  C, Cp = 500, 512
  rule = bwd_rule(Cp, True)
  rows = (nblocks - 1) * 16 + 1
  assert blk_of(rule, rows) == 16 and -(-rows // 16) == nblocks
  args = ln_bwd_inputs(C, Cp, rows, f16, 'any', 3000 + nblocks)
  ln_bwd_run(*args, C, Cp, f16, [(True, True)])


def test_ln_bwd_more_blocks_than_partial_rows(precision):
  """rows = 16 * 2048 + 1 at Cp = 512: 2049 blocks at the minimum rows_per_slot, more than
  kMaxParts = 2048 partial rows -- the doubling loop of cg_ln_lrelu_bwd runs.  C = 12: the
  pitch and the row count select the path, the float64 reference stays small."""
  f16 = precision
  C, Cp, rows = 12, 512, 16 * 2048 + 1
  rule = bwd_rule(Cp, True)
  assert -(-rows // blk_of(rule, rows)) == 2049 and -(-(rows - 1) // blk_of(rule, rows - 1)) == 2048
  args = ln_bwd_inputs(C, Cp, rows, f16, 'any', 3100)
  ln_bwd_run(*args, C, Cp, f16, [(True, True)])


# ---------------------------------------------------------------------------
# BatchNormalization
# ---------------------------------------------------------------------------
BN_PITCHES = [(5, 8), (30, 32), (102, 128), (300, 320), (2040, 2048)]
BN_ROWS = [1, 2, 255, 257]
MANY = 256 * 113 + 1   # 114 blocks: both loops of the finishing kernels
# (C reduced to at most 30 at the large row counts: see the module's docstring)
BN_CASES = ([(C, Cp, rows) for C, Cp in BN_PITCHES for rows in BN_ROWS] +
            [(min(C, 30), Cp, MANY) for C, Cp in BN_PITCHES] +
            [(30, 32, 262144 + 3)])


def test_bn_launch_geometry_of_the_listed_shapes():
  assert N.bn_row_lanes(320) == 6 and 256 - 6 * 40 == 16   # 16 idle threads
  assert N.bn_row_lanes(2048) == 1 and N.bn_row_lanes(8) == 256
  assert N.bn_rows_per_block(MANY) == 256 and -(-MANY // 256) == 114
  assert N.bn_rows_per_block(262144 + 3) == 512 and N.bn_rows_per_block(262143) == 256


def bn_col(x, C):
  return P.host(x[:C])


@pytest.mark.parametrize('C,Cp,rows', BN_CASES)
def test_bn_stats_apply_bwd(C, Cp, rows, precision):
  f16 = precision
  y, gamma, beta, dout = N.bn_recipe(4000 + Cp + rows % 1000, rows, C, f16)
  rl = N.bn_row_lanes(Cp)
  yd = pitched(y, Cp, f16)
  rng = np.random.RandomState(Cp + rows % 1000)
  mm0 = rng.randn(C).astype(np.float32).astype(np.float64)
  mv0 = rng.uniform(0.5, 2.0, C).astype(np.float32).astype(np.float64)
  s = N.bn_stats(y, MOM, mm0, mv0, rlanes=rl)
  # statistics: with the moving pair, without it (the same bits), and again
  got = []
  for moving in (True, False, True):
    mean, var = out32(C), out32(C)
    mm, mv = (vec32(mm0, P.SENT32), vec32(mv0, P.SENT32)) if moving else (None, None)
    _lib.call('cg_bn_stats', H.p(yd), rows, C, Cp, H.p(mean), H.p(var), H.p(mm), H.p(mv),
              MOM, H.p(H.reduce_ws()), H.stream())
    H.sync()
    check32(mean, C, s['mean'], s['e_mean'], 'mean')
    check32(var, C, s['var'], s['e_var'], 'var')
    if moving:
      check32(mm, C, s['mm'], s['e_mm'], 'moving_mean')
      check32(mv, C, s['mv'], s['e_mv'], 'moving_var')
    got.append((mean, var))
  for other in got[1:]:
    assert torch.equal(P.bits(got[0][0]), P.bits(other[0]))
    assert torch.equal(P.bits(got[0][1]), P.bits(other[1]))
  assert s['var'][C - 1] == 0 and float(var[C - 1]) >= 0   # the constant column
  mean32, var32 = bn_col(mean, C), bn_col(var, C)
  md, vd, gd, bd = vec32(mean32), vec32(var32), vec32(gamma), vec32(beta)
  # apply: no activation, LeakyReLU, and the moving statistics (inference)
  hd = None
  for alpha, (m_, v_) in ((1.0, (mean32, var32)), (A32, (mean32, var32)),
                          (A32, (s['mm'].astype(np.float32).astype(np.float64),
                                 np.abs(s['mv']).astype(np.float32).astype(np.float64)))):
    out, m_d, v_d = out_act(rows, Cp, f16), vec32(m_), vec32(v_)
    _lib.call('cg_bn_apply', H.p(yd), H.p(m_d), H.p(v_d), H.p(gd), H.p(bd), H.p(out), rows, C,
              Cp, EPS, alpha, H.stream())
    H.sync()
    want, bar = N.bn_apply(y, m_, v_, gamma, beta, EPS, alpha)
    check_act(out, rows, C, want, f16, bar, 'apply alpha={}'.format(alpha))
    if alpha != 1.0 and hd is None:
      hd = out
  # backward: act = 0 (h = NULL) and act = 1 (the stored h, zeros of both signs planted)
  h = P.host(hd[:rows, :C])
  N.plant_mask_zeros(h, dout)
  dd, hp = pitched(dout, Cp, f16), pitched(h, Cp, f16)
  ws = H.reduce_ws()
  for act in (0, 1):
    alpha = A32 if act else 1.0
    runs = []
    for _ in range(2):
      dy, dg, db = out_act(rows, Cp, f16), out32(C), out32(C)
      _lib.call('cg_bn_bwd', H.p(dd), H.p(hp) if act else None, H.p(yd), H.p(md), H.p(vd),
                H.p(gd), H.p(dy), H.p(dg), H.p(db), rows, C, Cp, EPS, alpha, act, H.p(ws),
                H.stream())
      H.sync()
      runs.append((dy, dg, db))
    for a, b in zip(*runs):
      assert torch.equal(P.bits(a), P.bits(b)), 'act={}: repeat'.format(act)
    what = 'bwd act={} '.format(act)
    pure = N.bn_bwd(dout, h, y, mean32, var32, gamma, EPS, alpha, act)
    check32(dg, C, pure['dgamma'], pure['e_dgamma'], what + 'dgamma')
    check32(db, C, pure['dbeta'], pure['e_dbeta'], what + 'dbeta')
    own = N.bn_bwd(dout, h, y, mean32, var32, gamma, EPS, alpha, act,
                   dgamma=bn_col(dg, C), dbeta=bn_col(db, C))
    check_act(dy, rows, C, own['dy'], f16, own['e_dy'], what + 'dy (own sums)', False)
    check_act(dy, rows, C, pure['dy'], f16, pure['e_dy'], what + 'dy (float64 chain)', False)


@pytest.mark.parametrize('rows,C,Cp,centre,spread', [(257, 102, 128, 50.0, 1.0),
                                                     (MANY, 30, 32, -200.0, 2.0),
                                                     (255, 300, 320, 50.0, 0.5)])
def test_bn_stats_of_off_centre_channels(rows, C, Cp, centre, spread, precision):
  """|mean| / std of 50 to 100 (the old test's recipe) against the derived bar -- which
  tests/test_norm_ref.py holds below that test's rtol of 1e-4 on the variance."""
  f16 = precision
  y = N.off_centre_recipe(14, rows, C, centre, spread, f16)
  s = N.bn_stats(y, MOM, rlanes=N.bn_row_lanes(Cp))
  mean, var, yd = out32(C), out32(C), pitched(y, Cp, f16)
  _lib.call('cg_bn_stats', H.p(yd), rows, C, Cp, H.p(mean), H.p(var), None, None, MOM,
            H.p(H.reduce_ws()), H.stream())
  H.sync()
  check32(mean, C, s['mean'], s['e_mean'], 'mean')
  check32(var, C, s['var'], s['e_var'], 'var')


# ---------------------------------------------------------------------------
# cg_unshuffle_mask
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('seg', [1, 2])
@pytest.mark.parametrize('Cp', [8, 40, 128])
@pytest.mark.parametrize('w', [2, 8, 64])
def test_unshuffle_mask(w, Cp, seg, precision):
  f16 = precision
  nB, C = 11, Cp - 3
  assert nB % seg or seg == 1
  e, h, shifts = N.unshuffle_recipe(5000 + w + Cp + seg, nB, w, C, seg, f16)
  assert {0, 1, -1, w - 1, -(w - 1)} <= set(int(v) for v in shifts)
  null = (w, Cp, seg) == (8, 40, 1)   # one case passes shifts = NULL
  ed = pitched(e.reshape(nB * w, C), Cp, f16, 0.0)
  hd = pitched(h.reshape(nB * w, C), Cp, f16, 0.0)
  sh = None if null else torch.tensor(np.r_[shifts, [7777] * G32].astype(np.int32),
                                      device=H.DEV)
  delta = out_act(nB * w, Cp, f16)
  _lib.call('cg_unshuffle_mask', H.p(ed), H.p(hd), H.p(delta), H.p(sh), nB, w, Cp, seg, A32,
            H.stream())
  H.sync()
  want, exact = N.unshuffle_mask(e, h, None if null else shifts, seg, A32)
  want, exact = want.reshape(nB * w, C), exact.reshape(nB * w, C)
  assert P.is_sentinel(delta[nB * w:])
  assert int(delta[:nB * w, C:].view(torch.int16).count_nonzero()) == 0   # +0
  got = P.host(delta[:nB * w, :C])
  r = R.round_act(want, f16)
  # nothing rounds in f32: the store's rounding is the only one -- bit for bit, ties to even
  assert np.array_equal(got[exact], r[exact])
  assert np.array_equal(np.signbit(got[exact]), np.signbit(r[exact]))
  # the sum or the product rounded in f32 first (two roundings at most)
  bar = R.ulp_act(r, f16) + 2 * U * np.abs(want)
  assert (np.abs(got - r)[~exact] <= bar[~exact]).all()
  if not null and w > 2:
    a, b = N.tie_values(f16)
    assert (want[:, 2] == a + b).any()


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_refusals(precision):
  """CG_EINVAL before any launch: every output still holds its sentinel."""
  f16 = precision
  lib = _lib.load()
  rows, Cmax = 4, 2056
  act = lambda: torch.zeros(rows, Cmax, dtype=R.act_dtype(f16), device=H.DEV)
  y, dh, h = act(), act(), act()
  v = lambda: torch.ones(Cmax, device=H.DEV)
  gam, bet, mean, var, rmean, rrstd = v(), v(), v(), v(), v(), v()
  ws = H.reduce_ws()
  outs = dict(o=P.sent_act((rows, Cmax), f16), a=P.sent32(Cmax), b=P.sent32(Cmax),
              c=P.sent32(Cmax), d=P.sent32(Cmax))
  p, st = H.p, H.stream()
  o, a, b, c, d = (outs[k] for k in 'oabcd')
  bad_shapes = [(rows, 5, 12), (rows, 16, 8), (0, 8, 8)]   # Cp % 8, C > Cp, rows = 0
  for r_, C, Cp in bad_shapes + [(rows, 500, 520)]:
    assert lib.cg_ln_lrelu_fwd(p(y), p(gam), p(bet), p(o), p(a), p(b), r_, C, Cp, EPS, A32,
                               st) == EINVAL
    for w_ in (ws, None):
      assert lib.cg_ln_lrelu_bwd(p(dh), p(h), p(y), p(rmean), p(rrstd), p(gam), p(o), p(a),
                                 p(b), p(c), r_, C, Cp, A32, p(w_), st) == EINVAL

  def stats(yy=y, m=a, v_=b, mm=c, mv=d, w_=ws, r_=rows, C=8, Cp=8):
    return lib.cg_bn_stats(p(yy), r_, C, Cp, p(m), p(v_), p(mm), p(mv), MOM, p(w_), st)

  def apply(yy=y, m=mean, v_=var, g=gam, be=bet, out=o, r_=rows, C=8, Cp=8):
    return lib.cg_bn_apply(p(yy), p(m), p(v_), p(g), p(be), p(out), r_, C, Cp, EPS, A32, st)

  def bwd(do=dh, hh=h, yy=y, m=mean, v_=var, g=gam, dy=o, dg=a, db=b, w_=ws, r_=rows, C=8,
          Cp=8, act_=1):
    return lib.cg_bn_bwd(p(do), p(hh), p(yy), p(m), p(v_), p(g), p(dy), p(dg), p(db), r_, C,
                         Cp, EPS, A32, act_, p(w_), st)

  for r_, C, Cp in bad_shapes:
    assert stats(r_=r_, C=C, Cp=Cp) == EINVAL
    assert apply(r_=r_, C=C, Cp=Cp) == EINVAL
    assert bwd(r_=r_, C=C, Cp=Cp) == EINVAL
  assert stats(C=2050, Cp=2056) == EINVAL and bwd(C=2050, Cp=2056) == EINVAL
  for k in ('yy', 'm', 'v_', 'w_'):
    assert stats(**{k: None}) == EINVAL
  assert stats(mm=None) == EINVAL and stats(mv=None) == EINVAL   # one of the pair
  for k in ('yy', 'm', 'v_', 'g', 'be', 'out'):
    assert apply(**{k: None}) == EINVAL
  for k in ('do', 'yy', 'm', 'v_', 'g', 'dy', 'dg', 'db', 'w_'):
    assert bwd(**{k: None}) == EINVAL
  assert bwd(hh=None, act_=1) == EINVAL
  sh = torch.zeros(4, dtype=torch.int32, device=H.DEV)
  for nB, w, Cp, seg in ((2, 2, 12, 1), (0, 2, 8, 1), (2, 0, 8, 1), (2, 2, 8, 0)):
    assert lib.cg_unshuffle_mask(p(y), p(h), p(o), p(sh), nB, w, Cp, seg, A32, st) == EINVAL
  H.sync()
  for t in outs.values():
    assert P.is_sentinel(t)
