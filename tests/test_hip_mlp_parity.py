"""Elementwise float64 parity of the entry points of calciumgan_amd/csrc/mlp.hip
-- cg_mlp_dense_fwd and cg_mlp_dense_dgrad in their three modes,
cg_mlp_dense_wgrad, cg_mlp_interp, cg_mlp_gp_loss -- at the extents they admit.

Every comparison is ONE launch against the float64 statement of
tests/mlp_ref.py (tied to autograd and to mlp_oracle in tests/test_mlp_ref.py)
on its recipes: `exact` (integer operands: the device must give the statement's
values, a dropped, doubled or misplaced term changes an integer -- this is what
guards the flat extents), `real` (rounded normals under per-element bars derived
from the operation counts, never measured) and `special` (infinities, NaN,
zeros, subnormals, saturation).  Every output and workspace is a slice of a
larger buffer with sentinels in front and behind, starts as NaN and must be
fully written; every launch runs twice and must give the same bits.  The
entries are float32 in both precision builds: the exact cases run under each."""
import functools

import numpy as np
import pytest
import torch

import mlp_ref as M
from calciumgan_amd import _lib

pytestmark = pytest.mark.gpu

SEED = 1234
STREAM = M.mlp.stream_id(3, 1, 2)
GUARD = 8
SENT = 12345.0
ALPHA, P = 0.3, 0.5  # of the real recipe

ids = lambda shapes: ['{}x{}to{}'.format(*s) for s in shapes]
ALL = M.DENSE_SMALL + M.DENSE_WIDE + M.DENSE_FLAT


@pytest.fixture(autouse=True)
def _back_to_bf16():
  _lib.use('bf16')
  yield
  _lib.use('bf16')


@pytest.fixture(params=['bf16', 'f16'])
def build(request):
  _lib.use(request.param)
  return request.param


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class Out(object):
  """n floats of NaN handed over as a slice, sentinels in front and behind."""

  def __init__(self, n):
    self.n = n
    self.buf = torch.full((n + 2 * GUARD,), SENT, device='cuda')
    self.t = self.buf[GUARD:GUARD + n]
    self.t.fill_(float('nan'))

  def get(self, written=True):
    torch.cuda.synchronize()
    a = self.buf.cpu().numpy()
    assert (a[:GUARD] == SENT).all() and (a[GUARD + self.n:] == SENT).all(), 'sentinel'
    a = a[GUARD:GUARD + self.n]
    if written:
      return a
    assert np.isnan(a).all(), 'written where nothing is due'
    return None


def twice(run):
  """Two launches on fresh buffers: the same bits."""
  a, b = run(), run()
  for u, v in zip(a, b):
    assert np.array_equal(bits(u), bits(v)), 'not repeatable'
  return a


def fully_written(a, want):
  """No NaN of the fill is left where the statement has none."""
  assert not (np.isnan(a) & ~np.isnan(np.asarray(want))).any(), 'unwritten'


def check_exact(name, got, want):
  fully_written(got, want)
  assert M.same_values(got, want), name


def check_real(name, got, want, bar):
  fully_written(got, want)
  f = M.used(got, want, bar)
  print('USED {:<40} {:.3f}'.format(name, f))
  assert f <= 1.0, name
  return f


@functools.lru_cache(maxsize=8)
def keep_of(rows, N, p):
  return M.keep_mask(SEED, STREAM, rows, N, p) if p > 0 else None


def run_fwd(x, W, b, mode, alpha, p, rows, K, N, h_mask=None, pitch=None):
  """One cg_mlp_dense_fwd.  pitch: x rows at that pitch, NaN in the padding.
  h_mask is handed over as the last row block of a buffer three times its size
  (the x^ segment of a stored h), the rest NaN."""
  if pitch is not None:
    xp = np.full((rows, pitch), np.nan, np.float32)
    xp[:, :K] = x
    x = xp
  xd, Wd = dev(x), dev(W)
  bd = None if b is None else dev(b)
  hm = None
  if h_mask is not None:
    big = np.full((3 * rows, N), np.nan, np.float32)
    big[2 * rows:] = h_mask
    hm = dev(big)[2 * rows:]

  def run():
    out = Out(rows * N)
    _lib.call('cg_mlp_dense_fwd', xd, K if pitch is None else pitch, Wd, bd, hm,
              out.t, rows, K, N, mode, alpha, p, SEED, STREAM, _lib.stream())
    return [out.get().reshape(rows, N)]

  return twice(run)[0]


def run_dgrad(dh, h, W, mode, alpha, p, rows, Cin, Cout, want_dx=True):
  dhd, Wd = dev(dh), dev(W)
  hd = None if h is None else dev(h)

  def run():
    dz, dx = Out(rows * Cout), Out(rows * Cin)
    _lib.call('cg_mlp_dense_dgrad', dhd, hd, Wd, dz.t, dx.t if want_dx else None,
              rows, Cin, Cout, mode, alpha, p, _lib.stream())
    dxa = dx.get(written=want_dx)
    return [dz.get().reshape(rows, Cout)] + (
        [dxa.reshape(rows, Cin)] if want_dx else [])

  return twice(run)


def stored(rows, N, p, exact):
  """The stored h (known signs under the keep mask) and sigmoid output."""
  keep = keep_of(rows, N, p)
  k1 = np.ones((rows, N), bool) if keep is None else keep
  return M.planted_h(11, k1, exact), M.planted_y(12, rows, N, exact)


# ---------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('p', M.EXACT_P)
@pytest.mark.parametrize('rows,K,N', ALL, ids=ids(ALL))
def test_forward_exact(rows, K, N, p, build):
  d = M.exact_dense(7, rows, K, N)
  a = M.EXACT_ALPHA
  keep = keep_of(rows, N, p)
  got = run_fwd(d['x'], d['W'], d['b'], M.FWD_ACT, a, p, rows, K, N)
  check_exact('act', got, M.dense_fwd(d['x'], d['W'], d['b'], M.FWD_ACT, a, p, keep))
  # the dropout positions are the statement's; dropped elements are +0
  assert (bits(got)[~keep] == 0).all()
  h, _ = stored(rows, N, p, True)
  got = run_fwd(d['t'], d['W'], None, M.FWD_TANGENT, a, p, rows, K, N, h_mask=h)
  check_exact('tangent', got,
              M.dense_fwd(d['t'], d['W'], None, M.FWD_TANGENT, a, p, h_mask=h))
  if p == 0.5:  # no bias, no dropout: act(x W) alone
    got = run_fwd(d['x'], d['W'], None, M.FWD_ACT, a, 0.0, rows, K, N)
    check_exact('act, no bias', got, M.dense_fwd(d['x'], d['W'], None, M.FWD_ACT, a))


@pytest.mark.parametrize('rows,K,N', ALL, ids=ids(ALL))
def test_forward_real(rows, K, N):
  d = M.real_dense(9, rows, K, N)
  tag = ' {}x{}->{}'.format(rows, K, N)
  keep = keep_of(rows, N, P)
  h, _ = stored(rows, N, P, False)
  for name, x, b, mode, kw in (
      ('fwd act', d['x'], d['b'], M.FWD_ACT, dict(keep=keep)),
      ('fwd sigmoid', d['x'], d['b'], M.FWD_SIGMOID, {}),
      ('fwd tangent', d['t'], None, M.FWD_TANGENT, dict(h_mask=h))):
    got = run_fwd(x, d['W'], b, mode, ALPHA, P, rows, K, N, h_mask=kw.get('h_mask'))
    check_real(name + tag, got, M.dense_fwd(x, d['W'], b, mode, ALPHA, P, **kw),
               M.fwd_bar(x, d['W'], b, mode, ALPHA, P, **kw))
    if mode == M.FWD_ACT:
      assert (bits(got)[~keep] == 0).all()


def test_forward_reads_x_through_its_pitch():
  rows, K, N = M.SPECIAL_SHAPE
  d = M.exact_dense(8, rows, K, N)
  got = run_fwd(d['x'], d['W'], d['b'], M.FWD_ACT, M.EXACT_ALPHA, 0.5, rows, K, N,
                pitch=K + 5)
  check_exact('pitch', got, M.dense_fwd(d['x'], d['W'], d['b'], M.FWD_ACT,
                                        M.EXACT_ALPHA, 0.5, keep_of(rows, N, 0.5)))


# ---------------------------------------------------------------------------
# input gradient: the layer is (Cin, Cout) = (K, N), so the kernel adds over N
# and walks K in column tiles -- the flat shapes arrive transposed
# ---------------------------------------------------------------------------
MODES = [('mask', M.BWD_MASK), ('sigmoid', M.BWD_SIGMOID), ('none', M.BWD_NONE)]


def _aux(mode, rows, N, p, exact):
  h, y = stored(rows, N, p, exact)
  return {M.BWD_MASK: h, M.BWD_SIGMOID: y, M.BWD_NONE: None}[mode]


@pytest.mark.parametrize('p', M.EXACT_P)
@pytest.mark.parametrize('rows,K,N', ALL, ids=ids(ALL))
def test_input_gradient_exact(rows, K, N, p, build):
  d = M.exact_dense(7, rows, K, N)
  for name, mode in MODES:
    aux = _aux(mode, rows, N, p, True)
    dz, dx = run_dgrad(d['dh'], aux, d['W'], mode, M.EXACT_ALPHA, p, rows, K, N)
    wz, wx = M.dense_dgrad(d['dh'], aux, d['W'], mode, M.EXACT_ALPHA, p)
    check_exact('dz ' + name, dz, wz)
    check_exact('dx ' + name, dx, wx)
    if mode == M.BWD_NONE:
      assert np.array_equal(bits(dz), bits(d['dh']))


@pytest.mark.parametrize('rows,K,N', ALL, ids=ids(ALL))
def test_input_gradient_real(rows, K, N):
  d = M.real_dense(9, rows, K, N)
  for name, mode in MODES:
    aux = _aux(mode, rows, N, P, False)
    dz, dx = run_dgrad(d['dh'], aux, d['W'], mode, ALPHA, P, rows, K, N)
    wz, wx = M.dense_dgrad(d['dh'], aux, d['W'], mode, ALPHA, P)
    ez, ex = M.dgrad_bars(d['dh'], aux, d['W'], mode, ALPHA, P)
    tag = ' {} {}x{}->{}'.format(name, rows, K, N)
    check_real('dgrad dz' + tag, dz, wz, ez)
    check_real('dgrad dx' + tag, dx, wx, ex)


@pytest.mark.parametrize('rows,K,N', [(33, 33, 65), (3, 5, 65536)])
def test_input_gradient_without_dx(rows, K, N):
  d = M.exact_dense(7, rows, K, N)
  h, _ = stored(rows, N, 0.5, True)
  dz, = run_dgrad(d['dh'], h, d['W'], M.BWD_MASK, M.EXACT_ALPHA, 0.5, rows, K, N,
                  want_dx=False)
  check_exact('dz only', dz, M.dense_dgrad(d['dh'], h, d['W'], M.BWD_MASK,
                                           M.EXACT_ALPHA, 0.5)[0])


# ---------------------------------------------------------------------------
# weight and bias gradient
# ---------------------------------------------------------------------------
WG = M.WGRAD_CASES


def run_wgrad(case, d, kw):
  """One cg_mlp_dense_wgrad: (dW, db or None, ws[:used]).  The rows of x that
  the tail replaces are NaN, and so is the padding of a pitch."""
  rows, Cin, Cout = case['rows'], case['Cin'], case['Cout']
  pitch = case.get('pitch', Cin)
  xp = np.full((rows, pitch), np.nan, np.float32)
  xp[:, :Cin] = d['x']
  if d['tail'] is not None:
    xp[kw['tail_row0']:] = np.nan
  xd, dzd = dev(xp), dev(d['dz'])
  td = None if d['tail'] is None else dev(d['tail'])
  plan = M.wgrad_plan(rows, kw['seg_rows'], Cin, Cout)
  elems = _lib.load().cg_mlp_wgrad_ws_elems(rows, Cin, Cout)
  assert elems == plan['bound'] >= plan['used']
  c = kw['coef']

  def run():
    dW, db, ws = Out(Cin * Cout), Out(Cout), Out(elems)
    _lib.call('cg_mlp_dense_wgrad', xd, pitch, td,
              kw['tail_row0'] if td is not None else 0, dzd, dW.t,
              None if case.get('no_db') else db.t, rows, Cin, Cout,
              kw['seg_rows'], c[0], c[1], c[2], kw['bias_rows'], ws.t,
              _lib.stream())
    w = ws.get()
    assert not np.isnan(w[:plan['used']]).any(), 'a planned slice is unwritten'
    assert np.isnan(w[plan['used']:]).all(), 'ws written past the plan'
    res = [dW.get().reshape(Cin, Cout), w[:plan['used']]]
    dba = db.get(written=not case.get('no_db'))  # db = NULL: left unwritten
    return res if dba is None else res + [dba]

  r = twice(run)
  return r[0], (r[2] if len(r) > 2 else None), r[1]


@pytest.mark.parametrize('case', WG, ids=[c['id'] for c in WG])
def test_weight_gradient_exact(case, build):
  d, kw = M.wgrad_case(case, exact=True)
  dW, db, ws = run_wgrad(case, d, kw)
  W64, b64, _ = M.dense_wgrad(d['x'], d['tail'], **kw)
  check_exact('dW', dW, W64)
  if db is not None:
    check_exact('db', db, b64)
  # the slices of ws: every chunk's own sums, zeros where it holds no rows
  Cin, Cout = case['Cin'], case['Cout']
  plan = M.wgrad_plan(case['rows'], kw['seg_rows'], Cin, Cout)
  xe = M.wgrad_x(d['x'], d['tail'], kw['tail_row0']).astype(np.float64)
  dz = d['dz'].astype(np.float64)
  for slot, _, r0, r1 in plan['chunks']:
    sl = ws[slot * plan['slice']:(slot + 1) * plan['slice']]
    assert np.array_equal(sl[:Cin * Cout].reshape(Cin, Cout), xe[r0:r1].T @ dz[r0:r1])
    assert np.array_equal(sl[Cin * Cout:],
                          dz[r0:max(r0, min(r1, kw['bias_rows']))].sum(axis=0))
  if case.get('cancel'):
    # c0 S0 + c1 S1 with S0 == S1, c0 == -c1: exactly +0, so db is +0 in every
    # column and dW is the third segment's contribution alone
    s2 = 2 * kw['seg_rows']
    assert (bits(db) == 0).all()
    assert M.same_values(dW, M.R.f32(kw['coef'][2]) * (xe[s2:].T @ dz[s2:]))


@pytest.mark.parametrize('case', WG, ids=[c['id'] for c in WG])
def test_weight_gradient_real(case):
  d, kw = M.wgrad_case(case, exact=False)
  dW, db, _ = run_wgrad(case, d, kw)
  W64, b64, _ = M.dense_wgrad(d['x'], d['tail'], **kw)
  eW, eb = M.wgrad_bars(d['x'], d['tail'], **kw)
  check_real('wgrad dW ' + case['id'], dW, W64, eW)
  if db is not None:
    check_real('wgrad db ' + case['id'], db, b64, eb)


# ---------------------------------------------------------------------------
# interp and gp_loss
# ---------------------------------------------------------------------------
def run_interp(d, B, n):
  r, f, a = dev(d['real']), dev(d['fake']), dev(d['alpha'])

  def run():
    out = Out(3 * B * n)
    _lib.call('cg_mlp_interp', r, f, a, out.t, B, n, _lib.stream())
    return [out.get().reshape(3, B, n)]

  got = twice(run)[0]
  assert np.array_equal(bits(got[0]), bits(d['real']))
  assert np.array_equal(bits(got[1]), bits(d['fake']))
  return got


def run_gp_loss(d, B, n, penalty):
  g, do = dev(d['g']), dev(d['d_out'])
  names = ('norm', 'gp', 'coef', 'v', 'loss')

  def run(want_v=True):
    outs = [Out(k) for k in (B, 1, B, B * n, 2)]
    _lib.call('cg_mlp_gp_loss', g, do, outs[0].t, outs[1].t, outs[2].t,
              outs[3].t if want_v else None, outs[4].t, B, n, penalty,
              _lib.stream())
    return [o.get(written=want_v or i != 3) for i, o in enumerate(outs)]

  got = twice(run)
  bare = run(want_v=False)  # v = NULL: v stays unwritten, the rest is the same
  for i in (0, 1, 2, 4):
    assert np.array_equal(bits(got[i]), bits(bare[i]))
  r = dict(zip(names, got))
  r['v'] = r['v'].reshape(B, n)
  return r


@pytest.mark.parametrize('B,n', [(1, 1), (1, 12), (256, 1), (256, 12), (2, 65536)])
def test_small_steps_exact(B, n, build):
  d = M.interp_data(3, B, n, True)
  check_exact('interp', run_interp(d, B, n), M.interp(**d))
  d = M.gp_data(4, B, n, True)
  got = run_gp_loss(d, B, n, M.EXACT_PENALTY)
  want = M.gp_loss(d['g'], d['d_out'], M.EXACT_PENALTY)
  for name in ('norm', 'gp', 'loss'):
    check_exact(name, got[name], want[name])
  # coef: one correctly rounded quotient (exact but for the rows of norm 5); 0
  # at norm 1; v from the stored coef, one rounded product
  assert np.array_equal(got['coef'], want['coef'].astype(np.float32))
  assert (got['coef'][want['norm'] == 1] == 0).all()
  assert np.array_equal(got['v'], M.v_of(got['coef'], d['g']).astype(np.float32))


@pytest.mark.parametrize('B,n', [(1, 1), (1, 12), (256, 12), (257, 1), (257, 12),
                                 (3, 65536)])
def test_small_steps_real(B, n):
  tag = ' B{} n{}'.format(B, n)
  d = M.interp_data(3, B, n, False)
  check_real('interp' + tag, run_interp(d, B, n), M.interp(**d), M.interp_bar(**d))
  d = M.gp_data(4, B, n, False)
  got = run_gp_loss(d, B, n, 10.0)
  want = M.gp_loss(d['g'], d['d_out'], 10.0)
  bars = M.gp_loss_bars(d['g'], d['d_out'], 10.0)
  for name in ('norm', 'gp', 'coef', 'loss'):
    check_real('gp_loss ' + name + tag, got[name], want[name], bars[name])
  v = M.v_of(got['coef'], d['g'])
  check_real('gp_loss v' + tag, got['v'], v, bars['v_from_coef'](v))


# ---------------------------------------------------------------------------
# special values
# ---------------------------------------------------------------------------
def check_special(name, got, want, bar):
  assert M.same_classes(got, want), name + ': non-finite classes'
  check_real(name, got, want, bar)


def test_special_values_forward():
  rows, K, N = M.SPECIAL_SHAPE
  S = M.SP
  d = M.special_dense(21, rows, K, N)
  x, W, b = d['x'], d['W'], d['b']
  fin = np.isfinite(x).all(axis=1)
  keep = keep_of(rows, N, P)
  for alpha in (ALPHA, 0.0):
    got = run_fwd(x, W, b, M.FWD_ACT, alpha, P, rows, K, N)
    want = M.dense_fwd(x, W, b, M.FWD_ACT, alpha, P, keep)
    check_special('special act alpha {}'.format(alpha), got, want,
                  M.fwd_bar(x, W, b, M.FWD_ACT, alpha, P, keep))
    assert (bits(got)[~keep] == 0).all()  # dropped: +0, in the inf and NaN rows too
    if alpha == 0.0:
      # a kept, clearly negative pre-activation is stored as -0
      z = M.preact(x, W, b)
      neg = keep & fin[:, None] & (z < -M.dense_sum_bar(x, W, b, 1))
      assert neg.any() and (bits(got)[neg] == np.int32(-2**31)).all()
  # the product of a subnormal and a normal is kept, not flushed
  got = run_fwd(x, W, b, M.FWD_ACT, 1.0, 0.0, rows, K, N)
  want = M.dense_fwd(x, W, b, M.FWD_ACT, 1.0)
  check_special('special act identity', got, want, M.fwd_bar(x, W, b, M.FWD_ACT, 1.0))
  assert got[S['sub_row'], S['sub_col']] != 0
  got = run_fwd(x, W, b, M.FWD_SIGMOID, 0.0, 0.0, rows, K, N)
  check_special('special sigmoid', got, M.dense_fwd(x, W, b, M.FWD_SIGMOID),
                M.fwd_bar(x, W, b, M.FWD_SIGMOID))
  # saturation: exactly 1 at +100, exactly +0 at -100
  assert (bits(got)[fin, S['hi_col']] == bits(np.float32(1.0))).all()
  assert (bits(got)[fin, S['lo_col']] == 0).all()


def test_special_values_masked_backward():
  """Inf, NaN and zero rows of dh, and the rule at a stored zero: a kept
  position whose h is +0 or -0 counts as dropped, its dz is 0."""
  rows, K, N = M.SPECIAL_SHAPE
  d = M.special_dense(21, rows, K, N)
  keep = keep_of(rows, N, P)
  h = M.planted_h(11, keep, False)
  zr, zc = np.nonzero(keep[5:7])  # two kept positions of ordinary rows
  plus, minus = (5 + zr[0], zc[0]), (5 + zr[-1], zc[-1])
  assert plus != minus
  h[plus], h[minus] = 0.0, -0.0
  for alpha in (ALPHA, 0.0):
    dz, dx = run_dgrad(d['dh'], h, d['W'], M.BWD_MASK, alpha, P, rows, K, N)
    wz, wx = M.dense_dgrad(d['dh'], h, d['W'], M.BWD_MASK, alpha, P)
    ez, ex = M.dgrad_bars(d['dh'], h, d['W'], M.BWD_MASK, alpha, P)
    check_special('special dz alpha {}'.format(alpha), dz, wz, ez)
    check_special('special dx alpha {}'.format(alpha), dx, wx, ex)
    assert dz[plus] == 0 and dz[minus] == 0
    assert (dz[~keep & np.isfinite(d['dh'])] == 0).all()
