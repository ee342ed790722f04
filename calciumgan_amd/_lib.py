"""ctypes binding of the C ABI in include/calciumgan_hip.h, derived from that
header at import: its prototypes, descriptor structs and CG_* constants are
written down nowhere else in Python.

The HIP library is the ONLY compute path of this package: if it is missing or
fails to load, every op raises (there is no CPU / eager fallback).
"""
import ctypes as C
import os
import re

# torch before the library is loaded: its wheel bundles a HIP runtime, and the
# library must bind to THAT copy -- loaded before torch, it pulled in
# /opt/rocm's libamdhip64 and the process ended up with two runtimes (first
# launch: hipErrorNoDevice)
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.normpath(
    os.path.join(_HERE, '..', 'include', 'calciumgan_hip.h'))
# CALCIUMGAN_HIP_LIB points at another build of the same C ABI (development)
LIB_PATH = os.environ.get('CALCIUMGAN_HIP_LIB') or os.path.join(
    _HERE, 'csrc', 'libcalciumgan_hip.so')
# the same sources with fp16 activations: the reference's mixed_float16 mode
LIB_PATH_F16 = os.environ.get('CALCIUMGAN_HIP_LIB_F16') or os.path.join(
    _HERE, 'csrc', 'libcalciumgan_hip_f16.so')
# CG_TILE_*: value -> (rows, cols, mfma rows)
TILES = {0: (256, 64, 16), 1: (64, 64, 16), 2: (128, 64, 16),
         3: (256, 64, 32), 4: (128, 64, 32), 5: (256, 128, 32),
         6: (128, 128, 32), 7: (256, 128, 16),
         8: (128, 128, 16)}
# CG_TILE_SWP_*: value -> (rows, cols); swconv_swp.hip, two waves per SIMD
SWP_TILES = {9: (512, 64), 10: (256, 64), 11: (256, 128), 12: (128, 128),
             13: (128, 64), 14: (256, 64), 15: (128, 128)}


def tile_shape(tile):
  """(rows, cols) of any CG_TILE_* value."""
  return TILES[tile][:2] if tile in TILES else SWP_TILES[tile]


class HipLibraryError(RuntimeError):
  pass


class DataPtr(C.c_void_p):
  """Argtype of a `[const] void|float|double|int|long long *` parameter.  Takes
  a torch tensor as its data_ptr() once its dtype matches the element type
  (int64 for `long long*`; `void*`
  takes any; device and contiguity are the caller's business: several entry
  points take host buffers), None as NULL, and whatever c_void_p itself takes:
  ctypes arrays, byref(...), pointer instances, ints."""


def _data_ptr(ctype, dtype):
  # (closed-over names, not class attributes: this runs once per pointer
  # argument of every launch)
  tensor, address, other = torch.Tensor, C.c_void_p, C.c_void_p.from_param

  def from_param(cls, obj):
    if not isinstance(obj, tensor):
      return other(obj)
    if dtype is not None and obj.dtype is not dtype:
      raise TypeError('a {} parameter takes a {} tensor, not {}'.format(
          ctype, dtype, obj.dtype))
    return address(obj.data_ptr())

  return type('DataPtr_' + ctype[:-1].replace(' ', '_'), (DataPtr,), {
      'ctype': ctype, 'dtype': dtype, 'from_param': classmethod(from_param)})


_SCALARS = {'int': C.c_int, 'long long': C.c_longlong, 'float': C.c_float,
            'double': C.c_double}
_DATA_PTRS = {'void': _data_ptr('void*', None),
              'float': _data_ptr('float*', torch.float32),
              'double': _data_ptr('double*', torch.float64),
              'int': _data_ptr('int*', torch.int32),
              'long long': _data_ptr('long long*', torch.int64)}


def _unknown(decl):
  raise HipLibraryError('calciumgan_amd: no ctypes binding for this '
                        'declaration of {}: "{}"'.format(
                            HEADER, ' '.join(decl.split())))


def _declarator(text, structs, decl, field=False):
  """(ctypes type, name) of one `type name`; `decl` is what an error quotes."""
  *tokens, name = text.replace('*', ' * ').split() or ['']
  if tokens[:1] == ['const']:
    tokens = tokens[1:]
  spelled = ' '.join(tokens)
  if not re.fullmatch(r'[A-Za-z_]\w*', name):
    _unknown(decl)
  if spelled in _SCALARS:
    return _SCALARS[spelled], name
  if spelled == 'void * const *':  # a host table of device pointers
    return C.POINTER(C.c_void_p), name
  if spelled[:-2] in structs and spelled.endswith(' *'):
    return C.POINTER(structs[spelled[:-2]]), name
  if spelled[:-2] in _DATA_PTRS and spelled.endswith(' *'):
    # (a struct field is assigned an address, never a tensor)
    return (C.c_void_p if field else _DATA_PTRS[spelled[:-2]]), name
  _unknown(decl)


def parse_header(text):
  """(constants, structs, prototypes) of a header written like
  calciumgan_hip.h: `#define CG_NAME integer`, `typedef struct cg_x_desc {...}
  cg_x_desc;` and `int|long long cg_name(...);`.  name -> int, name ->
  ctypes.Structure, name -> (argtypes, restype).  Anything else raises."""
  text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
  text = re.sub(r'#\s*ifdef\s+__cplusplus\b.*?#\s*endif', ' ', text, flags=re.S)
  constants, structs, protos = {}, {}, {}
  for line in re.findall(r'^[ \t]*#[ \t]*define[ \t]+CG_.*$', text, re.M):
    m = re.fullmatch(r'\s*#\s*define\s+(CG_\w+)\s+(-?\d+)\s*', line)
    if not m:
      _unknown(line)
    constants[m.group(1)] = int(m.group(2))
  text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)

  def struct(m):
    tag, body, name = m.groups()
    fields = []
    for decl in filter(str.strip, body.split(';')):
      first, *more = decl.split(',')  # `int nB, Lx, Cx;`
      ctype, fname = _declarator(first, structs, decl, field=True)
      for other in more:
        if not re.fullmatch(r'\s*[A-Za-z_]\w*\s*', other):
          _unknown(decl)
      fields += [(n.strip(), ctype) for n in [fname] + more]
    if tag != name or not fields:
      _unknown(m.group(0))
    cls = ''.join(w.title() for w in name.split('_')[1:])  # cg_conv_desc: ConvDesc
    structs[name] = type(cls, (C.Structure,), {
        '_fields_': fields, '__doc__': 'struct {}.'.format(name)})
    return ' '

  text = re.sub(r'typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;', struct,
                text)
  for decl in filter(str.strip, text.split(';')):
    m = re.fullmatch(r'\s*(int|long\s+long)\s+(\w+)\s*\(([^()]*)\)\s*', decl)
    if not m:
      _unknown(decl)
    params = [] if m.group(3).strip() == 'void' else m.group(3).split(',')
    protos[m.group(2)] = ([_declarator(p, structs, decl)[0] for p in params],
                          _SCALARS[' '.join(m.group(1).split())])
  return constants, structs, protos


def _read_header():
  try:
    with open(HEADER) as f:
      return f.read()
  except OSError as e:
    raise HipLibraryError('calciumgan_amd: cannot read the C header {}: {}'
                          .format(HEADER, e))


CONSTANTS, STRUCTS, _PROTOS = parse_header(_read_header())
CG_EINVAL, CG_ABI_VERSION = CONSTANTS['CG_EINVAL'], CONSTANTS['CG_ABI_VERSION']
EPI_NONE, EPI_LRELU, EPI_MASK, EPI_SIGMOID, EPI_LN_LRELU = (
    CONSTANTS['CG_EPI_' + n]
    for n in ('NONE', 'LRELU', 'MASK', 'SIGMOID', 'LN_LRELU'))
DTYPE_BF16, DTYPE_F16 = CONSTANTS['CG_DTYPE_BF16'], CONSTANTS['CG_DTYPE_F16']
# in the order of cg_struct_size(which)
ConvDesc, PackDesc, WgradDesc = (
    STRUCTS[n] for n in ('cg_conv_desc', 'cg_pack_desc', 'cg_wgrad_desc'))
SIGNATURES = {name: argtypes for name, (argtypes, _) in _PROTOS.items()}

_libs = {}       # precision -> ctypes handle
_active = 'bf16'  # precision of the library `call` / `load()` address


def use(precision):
  """Select the build every later `call` / `load()` goes to: 'bf16' (default)
  or 'f16' (mixed_float16).  The two builds keep separate kernels and tuning
  tables; objects created under one precision must be driven under it (the
  algorithm object checks)."""
  global _active
  if precision not in ('bf16', 'f16'):
    raise ValueError("precision must be 'bf16' or 'f16'")
  load(precision)
  _active = precision


def active():
  return _active


def load(precision=None):
  """Load (once per precision) and return the ctypes handle.  Raises
  HipLibraryError when the library has not been built -- there is deliberately
  no fallback path."""
  precision = precision or _active
  if precision in _libs:
    return _libs[precision]
  path = LIB_PATH_F16 if precision == 'f16' else LIB_PATH
  if not os.path.exists(path):
    raise HipLibraryError(
        'calciumgan_amd: {} not found. Build it with `python -m '
        'calciumgan_amd.build` (hipcc --offload-arch=gfx950); there is no '
        'CPU fallback.'.format(path))
  try:
    lib = C.CDLL(path)
  except OSError as e:
    raise HipLibraryError('calciumgan_amd: cannot load {}: {}'.format(path, e))
  for name, (argtypes, restype) in _PROTOS.items():
    fn = getattr(lib, name)  # AttributeError if the symbol is missing
    fn.argtypes = argtypes
    fn.restype = restype
  if lib.cg_abi_version() != CG_ABI_VERSION:
    raise HipLibraryError(
        'calciumgan_amd: ABI version {} in the header, {} in {} -- stale build '
        'or binding (rebuild with `python -m calciumgan_amd.build`)'.format(
            CG_ABI_VERSION, lib.cg_abi_version(), path))
  # the structs as parsed from the header must match the ones the compiler laid out
  for which, cls in enumerate((ConvDesc, PackDesc, WgradDesc)):
    if lib.cg_struct_size(which) != C.sizeof(cls):
      raise HipLibraryError(
          'calciumgan_amd: {} is {} bytes here, {} in {} -- stale build or '
          'binding (rebuild with `python -m calciumgan_amd.build`)'.format(
              cls.__name__, C.sizeof(cls), lib.cg_struct_size(which), path))
  want = DTYPE_F16 if precision == 'f16' else DTYPE_BF16
  if lib.cg_act_dtype() != want:
    raise HipLibraryError(
        'calciumgan_amd: {} computes with dtype {} (wanted {})'.format(
            path, lib.cg_act_dtype(), want))
  _libs[precision] = lib
  return lib


def check(rc, what):
  if rc != 0:
    if rc == CG_EINVAL:
      raise ValueError('{}: unsupported shape/arguments (CG_EINVAL)'.format(what))
    raise RuntimeError('{}: HIP error {}'.format(what, rc))


def call(name, *args):
  """Invoke an int-returning entry point of the active build and raise on a
  non-zero code."""
  try:
    rc = getattr(load(), name)(*args)
  except C.ArgumentError as e:  # "argument 3: TypeError: a float* parameter..."
    raise TypeError('{}: {}'.format(name, e)) from None
  check(rc, name)


def workspace(query, device, *args, least=0):
  """The workspace an entry point asks for: a uint8 tensor on `device` of the
  bytes its size query `query`(*args) returns (so numel() is the size to hand
  to the entry point), of `least` bytes where that is more, None for no bytes
  at all.  A shape the entry point refuses (the query's -1) is a ValueError."""
  need = getattr(load(), query)(*args)
  if need < 0:
    raise ValueError('{}: unsupported shape {}'.format(query, args))
  size = max(need, least)
  return torch.empty(size, dtype=torch.uint8, device=device) if size else None


def stream():
  """The current torch stream as the `void* stream` argument."""
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)
