"""Generate tests/golden/reduce_bits.npz (run on a GPU from the repo root:
``python tests/make_golden_reduce_bits.py <commit>``): the raw output bits of
every entry point whose kernel ends in a wave reduction and a fold of the
waves' LDS slots, recorded from the libraries of ONE commit (named inside the
file) so that a later commit which restates those folds can be held to the same
bits (tests/test_hip_reduce_bits.py).  Data only.  The groups conv_tails and
wgrad_tails hold, per launch, the SHA-256 words of all output buffers of the MFMA
kernels' tails (cg_swconv in every dispatch target and epilogue form, cg_wgrad
and cg_wgrad_batched with partials), built with the tests' own case builders.

Only the C ABI (through calciumgan_amd._lib) and seeded numpy inputs are used,
and only paths whose result does not depend on the arrival order of atomics: a
workspace given, or a single block.  CALCIUMGAN_HIP_LIB / CALCIUMGAN_HIP_LIB_F16
select the libraries.  Entry points that read activations run in both builds
(keys 'bf16/...' and 'f16/...'), the others in the bf16 build alone.  An output
is stored as its int16 / int32 / int64 view; one of more than 256 elements
(seeds of the head kernels, scaled rows, the vectors of the larger batches) as the
four int64 words of its SHA-256.
"""
import hashlib
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from calciumgan_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'reduce_bits.npz')
DEV = 'cuda'
VIEW = {2: torch.int16, 4: torch.int32, 8: torch.int64}
ALPHA = 0.3


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def act(a, f16):
  return dev(np.asarray(a, np.float32)).to(torch.float16 if f16 else torch.bfloat16)


def f32(*shape, fill=0.0):
  return torch.full(shape, fill, dtype=torch.float32, device=DEV)


def bits(t):
  a = t.detach().contiguous().cpu()
  a = a.view(VIEW[a.element_size()]).numpy().reshape(-1)
  if a.size > 256:
    a = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.int64).copy()
  return a


def call(name, *args):
  _lib.call(name, *(args + (_lib.stream(),)))


_WS = {}


def reduce_ws():
  """The ordered reductions' workspace, NaN in every slot nobody writes."""
  if 'ws' not in _WS:
    _WS['ws'] = torch.empty(_lib.load().cg_reduce_ws_elems(), dtype=torch.float32,
                            device=DEV)
  _WS['ws'].fill_(float('nan'))
  return _WS['ws']


# ---------------------------------------------------------------------------
# single-block tails of the WGAN-GP step
# ---------------------------------------------------------------------------
def tails(out, f16):
  """cg_gp_finalize / cg_critic_loss / cg_gp_critic_loss / cg_neg_mean do not
  read activations (bf16 build only); cg_gp_loss_scale does when it has rows
  to scale."""
  for B in (1, 63, 256, 257, 600):
    rng = np.random.RandomState(100 + B)
    norm = (0.25 + rng.rand(B) * 2.0).astype(np.float32)
    d_out = rng.randn(2 * B).astype(np.float32)
    dd = dev(d_out)
    if not f16:
      for squared in (0, 1):
        tag = 'B{}/sq{}'.format(B, squared)
        src = norm * norm if squared else norm
        n1, gp1, c1, l1 = dev(src), f32(1), f32(B), f32(2)
        call('cg_gp_finalize', n1, gp1, c1, B, 10.0, squared)
        call('cg_critic_loss', dd, gp1, 10.0, l1, B)
        for k, t in (('norm', n1), ('gp', gp1), ('coef', c1), ('loss', l1)):
          out['bf16/gp_finalize+critic_loss/{}/{}'.format(tag, k)] = bits(t)
        n2, gp2, c2, l2 = dev(src), f32(1), f32(B), f32(2)
        call('cg_gp_critic_loss', n2, gp2, c2, dd, l2, B, 10.0, squared, 0.75)
        for k, t in (('norm', n2), ('gp', gp2), ('coef', c2), ('loss', l2)):
          out['bf16/gp_critic_loss/{}/{}'.format(tag, k)] = bits(t)
      nm = f32(1)
      call('cg_neg_mean', dd, nm, B)
      out['bf16/neg_mean/B{}'.format(B)] = bits(nm)
    for P in (1, 3):
      ssq = dev((0.05 + rng.rand(B, P)).astype(np.float32))
      for n in (0, 8, 2056):
        if f16 and n == 0:
          continue  # no activations read: the bf16 build's case
        g = act(rng.randn(B, n), f16) if n else None
        dst = torch.zeros_like(g) if n else None
        nrm, gp, coef, loss = f32(B), f32(1), f32(B), f32(2)
        call('cg_gp_loss_scale', ssq, P, nrm, gp, coef, dd, loss, B, 10.0, 0.75,
             g, dst, n)
        tag = '{}/gp_loss_scale/B{}/P{}/n{}'.format('f16' if f16 else 'bf16', B, P, n)
        for k, t in (('norm', nrm), ('gp', gp), ('coef', coef), ('loss', loss)):
          out['{}/{}'.format(tag, k)] = bits(t)
        if n:
          out[tag + '/dst'] = bits(dst)


def rownorm(out, f16):
  pre = 'f16' if f16 else 'bf16'
  B = 3
  for n in (8, 8 * 256, 8 * 256 * 2 + 8):
    rng = np.random.RandomState(200 + n)
    g = act(rng.randn(B, n), f16)
    norm = f32(B, fill=12345.0)
    call('cg_rownorm', g, norm, B, n, reduce_ws())
    out['{}/rownorm/ws/n{}'.format(pre, n)] = bits(norm)
    if n == 8:  # one block per sample onto a zeroed output
      norm = f32(B)
      call('cg_rownorm', g, norm, B, n, None)
      out['{}/rownorm/atomic/n{}'.format(pre, n)] = bits(norm)


# ---------------------------------------------------------------------------
# the discriminator head
# ---------------------------------------------------------------------------
def _head(rng, nB, Lt, C, Cp, f16):
  h = np.zeros((nB, Lt, Cp), np.float32)
  h[:, :, :C] = rng.randn(nB, Lt, C)
  w = rng.randn(Lt * C).astype(np.float32)
  return act(h, f16), dev(w), dev(np.float32([0.25]))


def head(out, f16):
  """(Lt, C, Cp, nB, seg): the smallest case of test_dense1_fwd_bwd's HEAD list
  for dense1_fwd_kernel<256> and the one of fewest rows for <1024> (F = Lt Cp >=
  8192); BCE_SHAPES' first shape of each width, with seeds (the row kept in LDS)
  and without (kRow = 1): all four dense1_bce_kernel instantiations, each
  followed by dense1_bce_finish."""
  pre = 'f16' if f16 else 'bf16'
  for Lt, C, Cp, nB, seg in ((8, 6, 8, 1, 1), (256, 320, 320, 4, 2)):
    rng = np.random.RandomState(300 + Lt)
    h, w, b = _head(rng, nB, Lt, C, Cp, f16)
    tag = '{}/dense1/Lt{}C{}'.format(pre, Lt, C)
    o = f32(nB, fill=12345.0)
    call('cg_dense1_fwd', h, w, b, o, nB, Lt, C, Cp)
    out[tag + '/fwd/out'] = bits(o)
    nseg = (nB + seg - 1) // seg
    coef = dev(rng.randn(nseg).astype(np.float32))
    o, delta = f32(nB, fill=12345.0), torch.zeros_like(h)
    call('cg_dense1_fwd_bwd', h, w, b, o, coef, delta, nB, Lt, C, Cp, seg, ALPHA)
    out[tag + '/fwd_bwd/out'] = bits(o)
    out[tag + '/fwd_bwd/delta'] = bits(delta)
  for Lt, C, Cp in ((1, 8, 8), (256, 32, 32)):
    for B in (2, 257):
      if B == 257 and Lt != 1:
        continue  # (the finish's second pass over b: the small shape is enough)
      rng = np.random.RandomState(400 + Lt + B)
      h, w, b = _head(rng, 2 * B, Lt, C, Cp, f16)
      for seeds in (True, False):
        tag = '{}/dense1_bce/Lt{}C{}B{}/{}'.format(pre, Lt, C, B,
                                                   'seeds' if seeds else 'validate')
        o, cd, cg, loss = f32(2 * B), f32(2 * B), f32(B), f32(2, fill=12345.0)
        dd = torch.zeros_like(h) if seeds else None
        dg = torch.zeros_like(h[:B]) if seeds else None
        call('cg_dense1_bce', h, w, b, o, cd, cg, dd, dg, loss, None, None, B, Lt,
             C, Cp, ALPHA, reduce_ws())
        for k, t in (('out', o), ('coef_d', cd), ('coef_g', cg), ('loss', loss)):
          out['{}/{}'.format(tag, k)] = bits(t)
        if seeds:
          out[tag + '/delta_d'] = bits(dd)
          out[tag + '/delta_g'] = bits(dg)


# ---------------------------------------------------------------------------
# finishing launches
# ---------------------------------------------------------------------------
def colsum(out, f16):
  """256 rows per block at these sizes: 1, 17 and 129 partial rows (129 crosses
  finish_cols' eight-deep unrolled loop)."""
  pre = 'f16' if f16 else 'bf16'
  cases = []
  for rows in (200, 4100, 32800):
    for C in (1, 65):
      Cp = (C + 7) // 8 * 8
      rng = np.random.RandomState(500 + rows + C)
      cases.append((rows, C, Cp, act(rng.randn(rows, Cp), f16)))
  for rows, C, Cp, x in cases:
    o = f32(Cp, fill=12345.0)
    call('cg_colsum', x, o, rows, C, Cp, reduce_ws())
    out['{}/colsum/rows{}C{}'.format(pre, rows, C)] = bits(o)
  # the batched kernel: two queued reductions of different widths, so that the
  # blocks past the narrower one's columns take its early exit
  lib = _lib.load()
  ws = reduce_ws()
  (r0, C0, Cp0, x0), (r1, C1, Cp1, x1) = cases[2], cases[5]
  o0, o1 = f32(Cp0, fill=12345.0), f32(Cp1, fill=12345.0)
  half = ws.numel() // 2
  assert lib.cg_finish_defer(1) == 0
  try:
    call('cg_colsum', x0, o0, r0, C0, Cp0, ws[:half])
    call('cg_colsum', x1, o1, r1, C1, Cp1, ws[half:])
  finally:
    rc = lib.cg_finish_flush(_lib.stream())
  assert rc == 0
  out['{}/colsum_deferred/rows{}C{}'.format(pre, r0, C0)] = bits(o0)
  out['{}/colsum_deferred/rows{}C{}'.format(pre, r1, C1)] = bits(o1)


def signal_metrics(out):
  for rows in (1, 1025):  # C = 1: 1024 rows per block; C = 102: 64
    for C in (1, 102):
      rng = np.random.RandomState(600 + rows + C)
      real = dev(rng.rand(rows, C).astype(np.float32))
      fake = dev(rng.rand(rows, C + 2).astype(np.float32))
      o = f32(4, fill=12345.0)
      call('cg_signal_metrics', real, fake, o, rows, C, C, C + 2, -0.5, 3.0,
           reduce_ws())
      out['bf16/signal_metrics/rows{}C{}'.format(rows, C)] = bits(o)


# ---------------------------------------------------------------------------
# the metric kernels
# ---------------------------------------------------------------------------
def spike_stats_error(out):
  lib = _lib.load()
  for n_fr, n_cov in ((1, 1), (2049, 5), (5, 2049)):
    rng = np.random.RandomState(700 + n_fr)
    a, b = (dev(rng.rand(n_fr).astype(np.float32)) for _ in range(2))
    c, d = (dev(rng.randn(n_cov).astype(np.float32)) for _ in range(2))
    ws = f32(lib.cg_spike_stats_error_ws_elems(n_fr, n_cov), fill=float('nan'))
    o = f32(4, fill=12345.0)
    call('cg_spike_stats_error', a, b, n_fr, c, d, n_cov, o, ws)
    out['bf16/spike_stats_error/fr{}cov{}'.format(n_fr, n_cov)] = bits(o)


def tensor_summary(out):
  """Segments of one tile less one element, one tile and one tile plus one
  element; the 4096-element one starts on an unaligned float; -0, +0, a NaN and
  an infinity."""
  lib = _lib.load()
  lengths = [1, 4095, 4096, 4097, 5, 5]
  offsets = [0, 4, 4099, 8196, 12296, 12304]
  rng = np.random.RandomState(800)
  data = rng.randn(12312).astype(np.float32)
  data[4:6] = [-0.0, 0.0]
  data[12298] = np.nan
  data[12305] = np.inf
  x = dev(data)
  off = torch.tensor(offsets, dtype=torch.int64, device=DEV)
  ln = torch.tensor(lengths, dtype=torch.int64, device=DEV)
  nseg, total = len(lengths), sum(lengths)
  for k in (1, 30):
    nbytes = lib.cg_tensor_summary_ws_bytes(nseg, total, k)
    ws = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=DEV)
    stats = torch.zeros(nseg, 8, dtype=torch.float64, device=DEV)
    buckets = torch.zeros(nseg, k, 3, dtype=torch.float64, device=DEV)
    call('cg_tensor_summary', x, off, ln, nseg, total, k, stats, buckets, ws,
         ws.numel() * 8)
    out['bf16/tensor_summary/k{}/stats'.format(k)] = bits(stats)
    out['bf16/tensor_summary/k{}/buckets'.format(k)] = bits(buckets)


def pair_histogram(out):
  """Pair 0 plain, pair 1 all NaN on one side, pair 2 constant, pair 3 with an
  infinity."""
  P = 4
  for C in (2, 65, 130):
    rng = np.random.RandomState(900 + C)
    a, b = rng.randn(P, C, C), rng.randn(P, C, C)
    a[0, 0, C - 1] = np.nan
    a[1] = np.nan
    a[2], b[2] = 1.5, 1.5
    b[3, 0, 1] = np.inf
    da, db = dev(a), dev(b)
    for N in (1, 30, 256):
      counts = torch.full((P, 2, N), -1, dtype=torch.int32, device=DEV)
      valid = torch.full((P, 2), -1, dtype=torch.int32, device=DEV)
      edges = torch.full((P, N + 1), -1.0, dtype=torch.float64, device=DEV)
      status = torch.full((P,), -1, dtype=torch.int32, device=DEV)
      call('cg_pair_histogram', da, C * C, C, 1, db, C * C, C, 1, P, C, N, counts,
           valid, edges, status)
      tag = 'bf16/pair_histogram/C{}N{}'.format(C, N)
      for k, t in (('counts', counts), ('valid', valid), ('edges', edges),
                   ('status', status)):
        out['{}/{}'.format(tag, k)] = bits(t)


# ---------------------------------------------------------------------------
# the output tails of the MFMA kernels
# ---------------------------------------------------------------------------
def launch_bits(*tensors):
  """One entry per launch: the SHA-256 words of all its output buffers, guards
  and sentinels included (a store outside the owned rows changes it too)."""
  h = hashlib.sha256()
  for t in tensors:
    if t is not None:
      a = t.detach().contiguous().cpu()
      h.update(a.view(VIEW[a.element_size()]).numpy().tobytes())
  return np.frombuffer(h.digest(), np.int64).copy()


def conv_tails(out, f16):
  """cg_swconv with the case builders of tests/test_hip_swconv.py and
  tests/test_unshuffle_folded.py (the inputs whose float64 parity those tests
  establish), the `real` recipe, deterministic forms only: every dispatch
  target at one stage depth, the lean epilogues, the test_epilogues grid, the
  per-sample scale, the ordered and the deferred penalty norm, out_shifts with
  a side buffer and folded, the forward-only LayerNorm."""
  import swconv_ref as S
  import test_hip_swconv as T
  import test_unshuffle_folded as F
  lib = _lib.load()
  pre = '{}/conv_tails/'.format('f16' if f16 else 'bf16')

  def run(name, G, sigmoid=False, **kw):
    L = T.Launch(G, T.case(G, f16, 'real', sigmoid), f16, 'real', sigmoid, **kw)
    assert L.run() == 0, name
    assert pre + name not in out, name
    out[pre + name] = launch_bits(L.y, L.h, L.mean, L.rstd, L.ws, L.ssq, L.ssq_ws,
                                  L.side)

  # (the kernel-size sweep of the classic tiles was added after the fixture was
  # recorded; it reaches no tail the cases below do not)
  sweep = set(S.sweep_geoms())
  for p in T.dispatch_cases():
    G, kw, _ = p.values
    if kw.get('ks', 2) != 2 or G in sweep:
      continue  # (the stage depth does not reach the epilogue)
    if kw['epi'] == S.EPI_LN:
      run('dispatch/' + p.id, G, ln=T.ln_params(G) + (True,), **kw)
    else:
      run('dispatch/' + p.id, G, mask='inplace' if kw.get('ksplit') else None, **kw)
  was = lib.cg_debug_lean_epilogue(1)
  try:
    for p in T.lean_cases():
      form, G, kw = p.values
      if form == 'maskshift':
        run(p.id, G, out_shifts=((2, -1, 0), 1, 2), **kw)
      else:
        run(p.id, G, ssq='ordered' if form == 'lrelussq' else None, **kw)
  finally:
    lib.cg_debug_lean_epilogue(was)
  for tile, tkw in T.FEATURE_TILES:
    for epi in (S.EPI_NONE, S.EPI_LRELU, S.EPI_MASK, S.EPI_SIGMOID):
      for out_f32 in (0, 1):
        for bias in (True, False):
          run('epilogues/t{}-epi{}-f32{}-bias{}'.format(tile, epi, out_f32, int(bias)),
              S.EPI_GEOM, epi == S.EPI_SIGMOID, bias=bias, tile=tile, epi=epi,
              out_f32=out_f32, **tkw)
  for tile in (9, 12, 13):
    for epi in (S.EPI_NONE, S.EPI_LRELU, S.EPI_MASK):
      run('row_scale/t{}-epi{}'.format(tile, epi), S.SWP_DOWN,
          row_scale=np.array([-1.5, 0.0, 2.0**-20]), tile=tile, pmajor=1, epi=epi)
  for tile in (2, 6, 12, 13):
    rows = _lib.tile_shape(tile)[0]
    for Lu, out_f32 in ((rows, 1), (2 * rows, 0)):
      for form in ('ordered', 'defer'):
        run('rowsumsq/t{}-Lu{}-{}'.format(tile, Lu, form), S.SSQ_GEOMS[Lu], tile=tile,
            out_f32=out_f32, ssq=form)
  for tile, side_rows in ((1, 2), (6, 3), (12, 2), (13, 5)):
    for epi in (S.EPI_NONE, S.EPI_MASK):
      run('out_shifts/t{}-side{}-epi{}'.format(tile, side_rows, epi), S.SWP_UP,
          out_shifts=((2, -2, 0), 1, side_rows), tile=tile, epi=epi)
  # folded: |shift| = 1 .. 3 of both signs ('small'), the largest admitted, +-15
  # ('m15'), and the zero tail of a second column tile ('n102')
  for p in F.PARAMS:
    if p.id.split('-')[0] in ('small', 'm15', 'n102'):
      G, osh, oseg, side_rows, Cy, tile = p.values
      pr = F.Pair(G, T.case(G, f16, 'real'), f16, 'real', osh, oseg, side_rows, Cy, tile,
                  T.ALPHA)
      out[pre + 'folded/' + p.id] = launch_bits(pr.launch(folded=True))
  for tile in (6, 12):
    G = S.LN_GEOMS[0]
    run('ln_forward_only/t{}'.format(tile), G, ln=T.ln_params(G) + (False,), tile=tile,
        epi=S.EPI_LN)


def wgrad_tails(out, f16):
  """cg_wgrad with partials and `store` (one split, a few, and enough that
  several threads share an element's splits; real channel counts short of
  their pitches; 12 and 20 taps) and cg_wgrad_batched in the split and the
  flex form, with the case builders of tests/test_hip_wgrad.py."""
  import test_hip_wgrad as T
  import wgrad_ref as W
  lib = _lib.load()
  pre = '{}/wgrad_tails/'.format('f16' if f16 else 'bf16')

  def make(G, **kw):
    c = T.case(G, f16, 'real')
    return T.Launch(G, c['x'], c['g'], f16, **kw)

  def record(name, L):
    assert pre + name not in out, name
    out[pre + name] = launch_bits(L.dw, L.db, L.ws)

  def run(name, G, **kw):
    L = make(G, **kw)
    assert L.run() == 0, name
    record(name, L)

  run('join/direct1', W.JOIN, join='direct', nsplit=1, bias_rows=576)
  for nsplit in (2, 3, 9, 17):  # the reduce kernel's zc = 1, 1, 2, 4
    run('join/store{}'.format(nsplit), W.JOIN, join='store', nsplit=nsplit, bias_rows=576)
  for taps, gi in ((12, 1), (20, 0), (20, 1)):
    G = W.instantiation_geoms(taps)[gi]
    run('taps{}-g{}'.format(taps, gi), G, join='store', nsplit=2,
        bias_rows=W.rows_of(G) // 2)
  for Cx, Cxp, Cg, Cgp in W.CHANNELS[2:4]:
    run('channels/{}x{}'.format(Cx, Cg), W.channel_geom(Cx, Cg), join='store', nsplit=3,
        bias_rows=128, Cxp=Cxp, Cgp=Cgp)
  run('bias_ring/rows100', W.BIAS_RING, join='store', nsplit=2, bias_rows=100)
  for bias_rows in (20, 36):
    run('bias_nseg/rows{}'.format(bias_rows), W.BIAS_NSEG, join='store', nsplit=2,
        bias_rows=bias_rows)
  batches = [
      ('batch', lambda: [make(G, join='store', bias_rows=128) for G in W.BATCH]),
      ('join', lambda: [make(W.JOIN, join='store', nsplit=n, bias_rows=576)
                        for n in (9, 17)]),
      ('bias_ring', lambda: [make(W.BIAS_RING, join='store', nsplit=2, bias_rows=r)
                             for r in (128, 32)]),
      ('bias_nseg', lambda: [make(W.BIAS_NSEG, join='store', nsplit=2, bias_rows=r)
                             for r in (20, 36)])]
  for mode, form in ((0, 'split'), (2, 'flex')):
    was = lib.cg_debug_wgrad_flex(mode)
    try:
      for name, mk in batches:
        Ls = mk()
        assert T.run_batched(Ls) == 0, (form, name)
        for i, L in enumerate(Ls):
          record('batched-{}/{}/{}'.format(form, name, i), L)
    finally:
      lib.cg_debug_wgrad_flex(was)


def compute():
  """name -> integer array, from the libraries _lib resolves."""
  out = {}
  for precision in ('bf16', 'f16'):
    _lib.use(precision)
    f16 = precision == 'f16'
    tails(out, f16)
    rownorm(out, f16)
    head(out, f16)
    colsum(out, f16)
    conv_tails(out, f16)
    wgrad_tails(out, f16)
  _lib.use('bf16')
  signal_metrics(out)
  spike_stats_error(out)
  tensor_summary(out)
  pair_histogram(out)
  torch.cuda.synchronize()
  return out


def save(dest, arrays, commit):
  """One npz of five arrays -- the names, each output's length and item size,
  all values as one int64 vector (a member per output would be mostly zip
  headers), the commit -- with a fixed timestamp on every member: two runs that
  agree in every output agree byte for byte."""
  names = sorted(arrays)
  packed = {
      'names': np.frombuffer('\n'.join(names).encode(), np.uint8),
      'sizes': np.array([arrays[n].size for n in names], np.int64),
      'itemsizes': np.array([arrays[n].itemsize for n in names], np.int64),
      'values': np.concatenate([arrays[n].astype(np.int64) for n in names]),
      'commit': np.frombuffer(commit.encode(), np.uint8)}
  with zipfile.ZipFile(dest, 'w', zipfile.ZIP_DEFLATED) as z:
    for name in sorted(packed):
      info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type = zipfile.ZIP_DEFLATED
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.ascontiguousarray(packed[name]),
                                allow_pickle=False)
      z.writestr(info, buf.getvalue())


def load(path=None):
  """-> (name -> integer array as compute() gives it, commit)."""
  with np.load(path or OUT) as z:
    names = bytes(z['names']).decode().split('\n')
    ends = np.cumsum(z['sizes'])
    kind = {2: np.int16, 4: np.int32, 8: np.int64}
    arrays = {n: z['values'][e - s:e].astype(kind[int(i)])
              for n, s, i, e in zip(names, z['sizes'], z['itemsizes'], ends)}
    return arrays, bytes(z['commit']).decode()


def main():
  commit = sys.argv[1] if len(sys.argv) > 1 else 'unknown'
  dest = sys.argv[2] if len(sys.argv) > 2 else OUT
  out = compute()
  save(dest, out, commit)
  print('wrote {} ({} outputs, {} bytes) from {} and {}'.format(
      dest, len(out), os.path.getsize(dest), _lib.LIB_PATH, _lib.LIB_PATH_F16))


if __name__ == '__main__':
  main()
