"""Inputs shared by tests/test_pair_hist_host.py and tests/test_hip_pair_hist.py:
named (real, fake) pairs of float64 (P, C, C) matrices, the smallest shapes at
which cg_pair_histogram (csrc/pair_hist.hip) can go wrong.  No matrix is
symmetric, so a lower-triangle or transposed read shows.  The arrays are shared
and read-only; two of them are views with other strides than a packed array's."""
import functools

import numpy as np

NUM_BINS = 30

CASES = ('one_value', 'c3', 'c17_strided', 'c102', 'on_edges', 'ties',
         'nan_rows', 'scales', 'degenerate')


def _from_triangles(P, C, tri_a, tri_b, seed):
  """Matrices whose upper triangles (np.triu_indices order) hold the given
  values; diagonal and lower triangle hold values far outside them."""
  rng = np.random.RandomState(seed)
  iu = np.triu_indices(C, k=1)
  out = []
  for tri in (tri_a, tri_b):
    m = 1e3 + rng.normal(size=(P, C, C))
    for p in range(P):
      m[p][iu] = tri[p]
    out.append(m)
  return out


def _on_edges(seed, lo, hi, C=12):
  """2 x 66 values: the 31 np.linspace edges of [lo, hi] and their nextafter
  neighbours on both sides, clipped to the range, then values drawn inside it;
  dealt to the two sides at random."""
  rng = np.random.RandomState(seed)
  e = np.linspace(lo, hi, NUM_BINS + 1)
  v = np.concatenate([e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf)])
  v = np.clip(v, lo, hi)
  n = C * (C - 1)
  assert len(v) <= n
  v = np.concatenate([v, rng.uniform(lo, hi, size=n - len(v))])
  v = v[rng.permutation(n)]
  return v[:n // 2], v[n // 2:]


@functools.lru_cache(maxsize=None)
def case(name):
  """name -> (real, fake), float64 (P, C, C) each."""
  rng = np.random.RandomState(1000 + CASES.index(name))
  if name == 'one_value':
    a, b = _from_triangles(3, 2, [[0.3], [2.5], [0.0]], [[1.7], [2.5], [0.0]], 1)
  elif name == 'c3':
    a, b = rng.normal(size=(3, 3, 3)), rng.normal(size=(3, 3, 3))
  elif name == 'c17_strided':
    buf = rng.normal(size=(2, 20, 24))
    a = buf[:, 2:19, 5:22]                      # a slice of a larger buffer
    b = rng.normal(size=(17, 2, 17)).transpose(1, 2, 0)   # permuted strides
    assert a.shape == b.shape == (2, 17, 17)
    assert a.strides == (3840, 192, 8) and b.strides == (136, 8, 272)
  elif name == 'c102':
    a, b = rng.normal(size=(2, 102, 102)), rng.normal(size=(2, 102, 102))
  elif name == 'on_edges':
    s0, s1 = _on_edges(5, 0.0, 1.0), _on_edges(6, -3.7, 12.9)
    a, b = _from_triangles(2, 12, [s0[0], s1[0]], [s0[1], s1[1]], 2)
  elif name == 'ties':
    a = np.round(rng.normal(size=(2, 17, 17)), 1)
    b = np.round(rng.normal(size=(2, 17, 17)), 1)
  elif name == 'nan_rows':
    a, b = rng.normal(size=(3, 7, 7)), rng.normal(size=(3, 7, 7))
    for m, p, silent in ((a, 0, (2, 5)), (b, 1, (0,)), (a, 1, (6,))):
      for c in silent:       # what np.corrcoef gives a silent train
        m[p, c, :] = np.nan
        m[p, :, c] = np.nan
    a[2] = np.nan            # a side without a value
  elif name == 'scales':
    scale = np.array([1e-9, 1.0, 1e6])[:, None, None]
    a, b = rng.normal(size=(3, 9, 9)) * scale, rng.normal(size=(3, 9, 9)) * scale
    assert (a < 0).any() and (b < 0).any()
  elif name == 'degenerate':
    one, nxt = 1.0, np.nextafter(1.0, 2.0)
    a, b = _from_triangles(2, 3, [[0.5, np.inf, 2.0], [one, nxt, one]],
                           [[0.1, 0.2, 0.3], [nxt, one, nxt]], 3)
  else:
    raise KeyError(name)
  for m in (a, b):
    assert m.dtype == np.float64
    (m if m.base is None else m.base).setflags(write=False)
    m.setflags(write=False)
  return a, b


def triangles(a, b, p):
  """The two samples of pair p as compute_metrics._upper forms them."""
  iu = np.triu_indices(a.shape[1], k=1)
  out = []
  for m in (a, b):
    s = np.asarray(m[p])[iu]
    out.append(s[~np.isnan(s)])
  return out


def to_device(x, device):
  """A float64 device tensor with the shape, strides and contents of the numpy
  array x (its whole base buffer is copied, then viewed as x views it)."""
  import torch
  base = x if x.base is None else x.base
  assert base.flags['C_CONTIGUOUS'] and base.dtype == np.float64
  offset = (x.__array_interface__['data'][0] -
            base.__array_interface__['data'][0]) // 8
  flat = torch.from_numpy(base.copy().reshape(-1)).to(device)
  return torch.as_strided(flat, x.shape, tuple(s // 8 for s in x.strides),
                          int(offset))
