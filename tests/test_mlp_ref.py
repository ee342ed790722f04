"""Host tests of tests/mlp_ref.py: the float64 statements of csrc/mlp.hip's
entry points against independent ones (float64 torch autograd, the hand-written
schedule of mlp_oracle), the restated launch plan of the weight gradient, and
the recipes' power to tell a wrong kernel from a right one -- a float32 numpy
evaluation stays inside every bar (and equals float64 under the exact recipe),
each planted fault does not."""
import numpy as np
import pytest
import torch

import mlp_oracle as MO
import mlp_ref as M
from test_mlp_host import make_hparams

SEED = 1234
STREAM = M.mlp.stream_id(3, 1, 2)
# (rows, K, N): every pairing of a tile edge and one past it; width 1024 on the
# narrow side; the flat sides of the generator's first Dense and of the head
SMALL = M.DENSE_SMALL
WIDE = M.DENSE_WIDE
FLAT = M.DENSE_FLAT
ids = lambda shapes: ['{}x{}to{}'.format(*s) for s in shapes]


def _keep(rows, N, p):
  return M.keep_mask(SEED, STREAM, rows, N, p) if p > 0 else None


# ---------------------------------------------------------------------------
# statements against autograd and the oracle's schedule
# ---------------------------------------------------------------------------
def _t64(a, grad=False):
  return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def _close(a, b, what):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), what


@pytest.mark.parametrize('rows,K,N', [(5, 7, 9), (33, 33, 65)])
def test_dense_statements_agree_with_autograd(rows, K, N):
  d = M.real_dense(3, rows, K, N)
  alpha, p = 0.25, 0.5
  keep, s = _keep(rows, N, p), M.scale_of(p)
  x, W, b = _t64(d['x'], True), _t64(d['W'], True), _t64(d['b'], True)
  z = x @ W + b
  assert float(z.detach().abs().min()) > 1e-9  # LeakyReLU away from 0
  h = torch.nn.functional.leaky_relu(z, alpha) * _t64(keep) * s
  _close(M.dense_fwd(d['x'], d['W'], d['b'], M.FWD_ACT, alpha, p, keep), h.detach(),
         'act')
  dx, dW, db = torch.autograd.grad(h, (x, W, b), _t64(d['dh']))
  h64 = h.detach().numpy()
  dz, dxs = M.dense_dgrad(d['dh'], h64, d['W'], M.BWD_MASK, alpha, p)
  _close(dxs, dx, 'dx')
  dWs, dbs, _ = M.dense_wgrad(d['x'], None, 0, dz, rows, (1.0, 0.0, 0.0), rows)
  _close(dWs, dW, 'dW')
  _close(dbs, db, 'db')
  # the tangent mode is the forward's directional derivative
  f = lambda v: torch.nn.functional.leaky_relu(v @ W.detach() + b.detach(),
                                               alpha) * _t64(keep) * s
  _, jv = torch.autograd.functional.jvp(f, x.detach(), _t64(d['t']))
  _close(M.dense_fwd(d['t'], d['W'], None, M.FWD_TANGENT, alpha, p, h_mask=h64),
         jv, 'tangent')
  # sigmoid and its backward from the stored output
  y = torch.sigmoid(x @ W + b)
  _close(M.dense_fwd(d['x'], d['W'], d['b'], M.FWD_SIGMOID), y.detach(), 'sigmoid')
  dx, = torch.autograd.grad(y, x, _t64(d['dh']))
  _close(M.dense_dgrad(d['dh'], y.detach().numpy(), d['W'], M.BWD_SIGMOID)[1], dx,
         'sigmoid dx')
  dz, dxs = M.dense_dgrad(d['dh'], None, d['W'], M.BWD_NONE)
  assert np.array_equal(dz, d['dh'].astype(np.float64))
  _close(dxs, d['dh'].astype(np.float64) @ d['W'].astype(np.float64).T, 'none dx')


def test_statements_run_the_oracles_critic_schedule():
  """interp, the forward, the input-gradient chain, gp_loss, the tangent chain
  and the weight gradient with coefficients (-1/B, 1/B, 1), a tail and bias_rows
  = 2 seg, chained as the device chains them, give
  mlp_oracle.hand_critic_grads' loss, penalty and all ten gradients."""
  B, L, C, U = 4, 3, 2, 4
  hp = make_hparams(L=L, C=C, noise_dim=4, num_units=U, dropout=0.5)
  hp.alpha = 0.25  # (a float32: the statements take scalars at their f32 value)
  rng = np.random.RandomState(0)
  w = [rng.standard_normal(s) * 0.5 for s in M.mlp.discriminator_shapes(hp)]
  real, fake = rng.uniform(0, 1, (B, L, C)), rng.uniform(0, 1, (B, L, C))
  a = rng.uniform(0, 1, B)
  widths = [4 * U, 3 * U, 2 * U, U]
  masks = [rng.uniform(size=(3 * B, L, n)) > 0.5 for n in widths]
  loss, gp, grads = MO.hand_critic_grads(w, real, fake, a, masks, hp)

  alpha, p, lam = hp.alpha, hp.dropout, hp.gradient_penalty
  x0 = M.interp(real.reshape(B, -1), fake.reshape(B, -1), a).reshape(3 * B * L, C)
  xs = [x0]
  for l in range(4):
    xs.append(M.dense_fwd(xs[-1], w[2 * l], w[2 * l + 1], M.FWD_ACT, alpha, p,
                          masks[l].reshape(3 * B * L, -1)))
  flat = xs[4].reshape(3 * B, L * U)
  d_out = M.dense_fwd(flat, w[8], w[9], M.FWD_ACT, 1.0)  # act = identity
  dz = [None] * 5
  dz[4], dh = M.dense_dgrad(np.ones((3 * B, 1)), None, w[8], M.BWD_NONE)
  dh = dh.reshape(3 * B * L, U)
  for l in range(3, -1, -1):
    dz[l], dh = M.dense_dgrad(dh, xs[l + 1], w[2 * l], M.BWD_MASK, alpha, p)
  r = M.gp_loss(dh[2 * B * L:].reshape(B, L * C), d_out[:, 0], lam)
  tang = [r['v'].reshape(B * L, C)]
  for l in range(4):
    tang.append(M.dense_fwd(tang[-1], w[2 * l], None, M.FWD_TANGENT, alpha, p,
                            h_mask=xs[l + 1][2 * B * L:]))
  _close(r['loss'][0], loss, 'loss')
  _close(r['gp'][0], gp, 'gp')
  for l in range(5):
    per = 1 if l == 4 else L
    x = flat if l == 4 else xs[l]
    t = tang[4].reshape(B, L * U) if l == 4 else tang[l]
    dW, db, _ = M.dense_wgrad(x, t, 2 * B * per, dz[l], B * per,
                              (-1.0 / B, 1.0 / B, 1.0), 2 * B * per)
    _close(dW, grads[2 * l], 'dW{}'.format(l))
    _close(db, grads[2 * l + 1].reshape(-1), 'db{}'.format(l))


def test_small_step_statements_agree_with_autograd():
  d = M.gp_data(5, 6, 12, exact=False)
  g = _t64(d['g'], True)
  norm = g.norm(dim=1)
  gp = ((norm - 1)**2).mean()
  v, = torch.autograd.grad(10.0 * gp, g)
  r = M.gp_loss(d['g'], d['d_out'], 10.0)
  _close(r['norm'], norm.detach(), 'norm')
  _close(r['gp'][0], gp.detach(), 'gp')
  _close(r['v'], v, 'v')
  do = d['d_out'].astype(np.float64)
  _close(r['loss'], [-do[:6].mean() + do[6:12].mean() + 10.0 * float(gp.detach()),
                     -do[6:12].mean()], 'loss')


# ---------------------------------------------------------------------------
# the launch plan
# ---------------------------------------------------------------------------
def _check_plan(rows, seg_rows):
  plan = M.wgrad_plan(rows, seg_rows)
  segs = M.segments(rows, seg_rows)
  assert plan['nseg'] * plan['cps'] * plan['slice'] == plan['used'] <= plan['bound']
  assert plan['chunk_rows'] % 16 == 0 and plan['chunk_rows'] >= 64
  assert -(-rows // plan['chunk_rows']) <= 64
  assert [c[0] for c in plan['chunks']] == list(range(plan['nseg'] * plan['cps']))
  owner = np.full(rows, -1)
  for slot, k, r0, r1 in plan['chunks']:
    s, e = segs[k]
    assert s <= r0 <= r1 <= e and r1 - r0 <= plan['chunk_rows']
    assert (owner[r0:r1] == -1).all()  # covered once
    owner[r0:r1] = k
  want = np.minimum(np.arange(rows) // seg_rows, 2)
  assert np.array_equal(owner, want)  # every row, in its own segment


def test_plan_chunks_lie_in_one_segment_and_cover_it_once():
  for rows in (1, 2, 3, 17, 63, 64, 65, 128, 129, 200, 1000):
    for seg_rows in range(1, rows + 1):
      _check_plan(rows, seg_rows)
  for rows in (4096, 4097, 5000):
    for seg_rows in range(1, rows + 1):
      _check_plan(rows, seg_rows)
  assert M.wgrad_chunk_rows(4096) == 64 and M.wgrad_chunk_rows(4097) == 80
  # the cases of the GPU file reach what they are meant to
  p = M.wgrad_plan(4097, 1366)
  assert p['chunk_rows'] == 80 and 1366 % 80 == 6 and 1366 % 16 != 0
  p = M.wgrad_plan(4097, 2000)  # a third segment of 97 rows: empty chunks
  assert sum(1 for c in p['chunks'] if c[1] == 2 and c[2] == c[3]) == p['cps'] - 2
  p = M.wgrad_plan(4097, 1000)  # a third segment longer than seg_rows
  assert p['cps'] == -(-2097 // 80)


# ---------------------------------------------------------------------------
# the exact recipe: f32 numpy == f64 numpy
# ---------------------------------------------------------------------------
def _dense_outputs(d, rows, K, N, alpha, p, exact, dt, x=None, W=None, b=None,
                   flip=None):
  """Every Dense statement on one recipe: dict name -> result.  flip = (r, c):
  the stored h / h_mask has the wrong sign there (a planted fault)."""
  x = d['x'] if x is None else x
  W = d['W'] if W is None else W
  b = d['b'] if b is None else b
  keep = _keep(rows, N, p)
  k1 = np.ones((rows, N), bool) if keep is None else keep
  h = M.planted_h(11, k1, exact)
  if flip is not None:
    h = h.copy()
    h[flip] = -h[flip]
  y = M.planted_y(12, rows, N, exact)
  out = dict(act=M.dense_fwd(x, W, b, M.FWD_ACT, alpha, p, keep, dt=dt),
             sigmoid=M.dense_fwd(x, W, b, M.FWD_SIGMOID, dt=dt),
             tangent=M.dense_fwd(x, W, None, M.FWD_TANGENT, alpha, p, h_mask=h, dt=dt))
  # the input gradient's layer is (Cin, Cout) = (K, N): dh (rows, N), W (K, N)
  for name, mode, aux in (('mask', M.BWD_MASK, h), ('sig', M.BWD_SIGMOID, y),
                          ('none', M.BWD_NONE, None)):
    out['dz_' + name], out['dx_' + name] = M.dense_dgrad(d['dh'], aux, W, mode,
                                                         alpha, p, dt=dt)
  return out


def _dense_bars(d, rows, K, N, alpha, p, exact):
  keep = _keep(rows, N, p)
  k1 = np.ones((rows, N), bool) if keep is None else keep
  h, y = M.planted_h(11, k1, exact), M.planted_y(12, rows, N, exact)
  bars = dict(act=M.fwd_bar(d['x'], d['W'], d['b'], M.FWD_ACT, alpha, p, keep),
              sigmoid=M.fwd_bar(d['x'], d['W'], d['b'], M.FWD_SIGMOID),
              tangent=M.fwd_bar(d['x'], d['W'], None, M.FWD_TANGENT, alpha, p,
                                h_mask=h))
  for name, mode, aux in (('mask', M.BWD_MASK, h), ('sig', M.BWD_SIGMOID, y),
                          ('none', M.BWD_NONE, None)):
    bars['dz_' + name], bars['dx_' + name] = M.dgrad_bars(d['dh'], aux, d['W'],
                                                          mode, alpha, p)
  return bars


@pytest.mark.parametrize('p', M.EXACT_P)
@pytest.mark.parametrize('rows,K,N', SMALL + WIDE + FLAT, ids=ids(SMALL + WIDE + FLAT))
def test_exact_recipe_is_exact_in_float32(rows, K, N, p):
  d = M.exact_dense(7, rows, K, N)
  o64 = _dense_outputs(d, rows, K, N, M.EXACT_ALPHA, p, True, np.float64)
  o32 = _dense_outputs(d, rows, K, N, M.EXACT_ALPHA, p, True, np.float32)
  for name in o64:
    if name == 'sigmoid':
      continue  # (exp: the exact recipe has no sigmoid forward)
    assert o32[name].dtype == np.float32
    assert M.same_values(o32[name], o64[name]), name


WG = M.WGRAD_CASES


@pytest.mark.parametrize('case', WG, ids=[c['id'] for c in WG])
def test_exact_weight_gradient_is_exact_in_float32(case):
  d, kw = M.wgrad_case(case, exact=True)
  W64, b64, _ = M.dense_wgrad(d['x'], d['tail'], dt=np.float64, **kw)
  W32, b32, _ = M.dense_wgrad(d['x'], d['tail'], dt=np.float32, **kw)
  assert M.same_values(W32, W64) and M.same_values(b32, b64)


@pytest.mark.parametrize('B,n', [(1, 1), (256, 12), (256, 4096)])
def test_exact_small_steps_are_exact_in_float32(B, n):
  d = M.interp_data(3, B, n, True)
  assert M.same_values(M.interp(dt=np.float32, **d), M.interp(**d))
  d = M.gp_data(4, B, n, True)
  r64 = M.gp_loss(d['g'], d['d_out'], M.EXACT_PENALTY)
  r32 = M.gp_loss(d['g'], d['d_out'], M.EXACT_PENALTY, dt=np.float32)
  norm = r64['norm']
  assert set(np.unique(norm)) <= {1.0, 2.0, 4.0, 5.0} and (norm == 1).any()
  assert (r64['coef'][norm == 1] == 0).all()
  for name in ('norm', 'gp', 'loss'):
    assert M.same_values(r32[name], r64[name]), name
  # coef of the norm-5 rows is 64 / (5 B): ONE correctly rounded quotient, so the
  # float32 evaluation is the rounded statement; v is stated from the stored coef
  c32 = r64['coef'].astype(np.float32)
  assert np.array_equal(r32['coef'], c32)
  assert M.same_values(c32[norm != 5], r64['coef'][norm != 5])
  assert np.array_equal(r32['v'], M.v_of(c32, d['g']).astype(np.float32))


# ---------------------------------------------------------------------------
# the real recipe: f32 numpy inside the bars, planted faults outside
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('rows,K,N', SMALL + WIDE + FLAT, ids=ids(SMALL + WIDE + FLAT))
def test_float32_numpy_stays_inside_the_bars(rows, K, N):
  d = M.real_dense(9, rows, K, N)
  alpha, p = 0.3, 0.5
  o64 = _dense_outputs(d, rows, K, N, alpha, p, False, np.float64)
  o32 = _dense_outputs(d, rows, K, N, alpha, p, False, np.float32)
  bars = _dense_bars(d, rows, K, N, alpha, p, False)
  for name in sorted(o64):
    f = M.used(o32[name], o64[name], bars[name])
    print('USED host {:<8} {}x{}->{}  {:.3f}'.format(name, rows, K, N, f))
    assert f <= 1.0, name


@pytest.mark.parametrize('case', WG, ids=[c['id'] for c in WG])
def test_float32_weight_gradient_stays_inside_the_bars(case):
  d, kw = M.wgrad_case(case, exact=False)
  W64, b64, _ = M.dense_wgrad(d['x'], d['tail'], **kw)
  W32, b32, _ = M.dense_wgrad(d['x'], d['tail'], dt=np.float32, **kw)
  eW, eb = M.wgrad_bars(d['x'], d['tail'], **kw)
  fW, fb = M.used(W32, W64, eW), M.used(b32, b64, eb)
  print('USED host wgrad {}  dW {:.3f} db {:.3f}'.format(case['id'], fW, fb))
  assert fW <= 1.0 and fb <= 1.0


@pytest.mark.parametrize('B,n', [(1, 1), (256, 12), (257, 12), (3, 4096)])
def test_float32_small_steps_stay_inside_the_bars(B, n):
  d = M.interp_data(3, B, n, False)
  f = M.used(M.interp(dt=np.float32, **d), M.interp(**d), M.interp_bar(**d))
  d = M.gp_data(4, B, n, False)
  r64 = M.gp_loss(d['g'], d['d_out'], 10.0)
  r32 = M.gp_loss(d['g'], d['d_out'], 10.0, dt=np.float32)
  bars = M.gp_loss_bars(d['g'], d['d_out'], 10.0)
  fs = {k: M.used(r32[k], r64[k], bars[k]) for k in ('norm', 'gp', 'coef', 'loss')}
  v = M.v_of(r32['coef'], d['g'])
  fs['v'] = M.used(r32['v'], v, bars['v_from_coef'](v))
  print('USED host interp {:.3f} gp_loss {}'.format(f, fs))
  assert f <= 1.0 and max(fs.values()) <= 1.0


def _dense_faults(d, rows, K, N, alpha, p, exact):
  """name -> (outputs that must change, the faulty outputs)."""
  o = lambda **kw: _dense_outputs(d, rows, K, N, alpha, p, exact, np.float64, **kw)
  good = o()
  # the wrong-sign slope is planted where the stored h is kept and the
  # gradient that meets it is largest
  keep = _keep(rows, N, p)
  k1 = np.ones((rows, N), bool) if keep is None else keep
  z = np.abs(M.preact(d['x'], d['W'])) * np.abs(d['dh']) * k1
  flip = np.unravel_index(np.argmax(z), z.shape)
  xk, Wk = M.fault_dropped_k(d['x'], d['W'])
  # the dropped term of the input gradient is its last k: the last COLUMN of W
  Wc = np.array(d['W'])
  Wc[:, -1] = 0
  j = int(np.argmax(np.abs(d['b']) * k1.any(axis=0)))  # (a column that is kept)
  return good, {
      'dropped k (forward)': (['act', 'sigmoid', 'tangent'], o(x=xk, W=Wk)),
      'dropped k (dgrad)': (['dx_mask', 'dx_sig', 'dx_none'], o(W=Wc)),
      'skipped bias column': (['act', 'sigmoid'], o(b=M.fault_bias_column(d['b'], j))),
      'slope of the wrong sign': (['tangent', 'dz_mask', 'dx_mask'], o(flip=flip)),
  }


@pytest.mark.parametrize('rows,K,N', SMALL + WIDE, ids=ids(SMALL + WIDE))
def test_bars_reject_planted_dense_faults(rows, K, N):
  """(Not at the flat shapes: at K = 65536 the bar is 0.4 % of sum |a| |b| and says
  nothing about one term -- bit equality under the exact recipe guards those,
  see the next test.)"""
  d = M.real_dense(9, rows, K, N)
  alpha, p = 0.3, 0.5
  bars = _dense_bars(d, rows, K, N, alpha, p, False)
  good, faults = _dense_faults(d, rows, K, N, alpha, p, False)
  for what, (names, bad) in faults.items():
    for name in names:
      assert M.rejected(bad[name], good[name], bars[name]), (what, name)


@pytest.mark.parametrize('rows,K,N', SMALL + WIDE + FLAT, ids=ids(SMALL + WIDE + FLAT))
def test_bit_equality_rejects_planted_dense_faults(rows, K, N):
  d = M.exact_dense(7, rows, K, N)
  good, faults = _dense_faults(d, rows, K, N, M.EXACT_ALPHA, 0.5, True)
  for what, (names, bad) in faults.items():
    for name in names:
      if name != 'sigmoid':
        assert M.rejected(bad[name], good[name]), (what, name)


def _wgrad_faults(d, kw):
  """A tail row taken from x; the last row of segment 0 counted in segment 1."""
  rows = d['x'].shape[0]
  out = {}
  if d['tail'] is not None:
    t = np.array(d['tail'])
    i = int(np.argmax(np.abs(t - d['x'][kw['tail_row0']:]).sum(axis=1)))
    t[i] = d['x'][kw['tail_row0'] + i]
    out['tail row from x'] = M.dense_wgrad(d['x'], t, **kw)
  if rows > kw['seg_rows']:
    seg = np.minimum(np.arange(rows) // kw['seg_rows'], 2)
    seg[kw['seg_rows'] - 1] = 1
    out['row in the neighbouring segment'] = M.dense_wgrad(d['x'], d['tail'],
                                                           row_seg=seg, **kw)
  return out


@pytest.mark.parametrize('exact', [False, True], ids=['real', 'exact'])
@pytest.mark.parametrize('case', WG, ids=[c['id'] for c in WG])
def test_planted_weight_gradient_faults_are_rejected(case, exact):
  d, kw = M.wgrad_case(case, exact)
  W64, b64, _ = M.dense_wgrad(d['x'], d['tail'], **kw)
  eW, eb = (None, None) if exact else M.wgrad_bars(d['x'], d['tail'], **kw)
  for what, (Wf, bf, _) in _wgrad_faults(d, kw).items():
    assert M.rejected(Wf, W64, eW), what
    if what.startswith('row') and kw['bias_rows'] >= kw['seg_rows']:
      assert M.rejected(bf, b64, eb), what


# ---------------------------------------------------------------------------
# the special recipe
# ---------------------------------------------------------------------------
def test_special_recipe_plants_what_it_says():
  rows, K, N = M.SPECIAL_SHAPE
  d = M.special_dense(21, rows, K, N)
  S = M.SP
  z = M.preact(d['x'], d['W'], d['b'])
  fin = np.isfinite(d['x']).all(axis=1)
  assert (~fin).sum() == 2
  assert (z[fin][:, S['hi_col']] > 89).all() and (z[fin][:, S['lo_col']] < -89).all()
  s = M.dense_fwd(d['x'], d['W'], d['b'], M.FWD_SIGMOID)
  assert (s[fin][:, S['hi_col']] == 1).all()  # 1 + e^-89 is 1 in float64 as well
  # +inf times a column of W: an infinity of W's sign, NaN at the zero column
  zi = z[S['inf_row']]
  w = d['W'][S['inf_k']].astype(np.float64)
  assert np.array_equal(np.isnan(zi), w == 0) and np.isnan(zi[S['zero_col']])
  assert np.array_equal(zi[w != 0], np.sign(w[w != 0]) * np.inf)
  assert np.isnan(z[S['nan_row']]).all()
  assert np.isfinite(z[fin]).all()  # nothing leaks out of the two rows
  assert np.array_equal(z[S['zero_row']], d['b'].astype(np.float64))
  v = z[S['sub_row'], S['sub_col']]
  assert 0 < abs(v) < 2.0**-126
  # alpha = 0: every clearly negative pre-activation is stored as -0
  h = M.dense_fwd(d['x'], d['W'], d['b'], M.FWD_ACT, 0.0)
  neg = fin[:, None] & (z < 0)
  assert neg.any() and (h[neg] == 0).all() and np.signbit(h[neg]).all()
  # the documented rule at a stored zero of either sign: the mask is 0
  assert np.array_equal(M.slope_mask(np.float32([0.0, -0.0, 2.0, -2.0]), 0.25, 0.5),
                        [0.0, 0.0, 2.0, 0.5])
