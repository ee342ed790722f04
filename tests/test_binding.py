"""The ctypes binding that calciumgan_amd/_lib.py derives from
include/calciumgan_hip.h: the header reader on small texts, the struct layouts
against the host C compiler, and the tensor marshalling of the data-pointer
argtypes (CPU tensors: nothing here needs a device)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from calciumgan_amd import _lib
from calciumgan_amd import build as cg_build

VOID, FLOAT, DOUBLE, INT = (_lib._DATA_PTRS[e]
                            for e in ('void', 'float', 'double', 'int'))


def test_prototype_over_three_lines_with_inline_comments():
  consts, structs, protos = _lib.parse_header('''
      #define CG_EINVAL 100001
      #define CG_EPI_NONE 0     /* y = acc (+bias) */
      long long cg_f(const void* y_pre /*act [rows][Cp], a, b*/,
                     const float* gamma, // int not_a_param,
                     double* out /*[rows] or NULL*/, long long rows, int C,
                     float eps, double g, const int* shifts, void* stream);
      ''')
  assert consts == {'CG_EINVAL': 100001, 'CG_EPI_NONE': 0}
  assert structs == {}
  assert protos == {'cg_f': ([VOID, FLOAT, DOUBLE, C.c_longlong, C.c_int,
                              C.c_float, C.c_double, INT, VOID], C.c_longlong)}


def test_void_parameter_list_is_empty():
  protos = _lib.parse_header('int cg_abi_version(void);\n'
                             'long  long cg_elems( void );')[2]
  assert protos == {'cg_abi_version': ([], C.c_int),
                    'cg_elems': ([], C.c_longlong)}


def test_comma_declared_fields_and_struct_pointer():
  _, structs, protos = _lib.parse_header('''
      typedef struct cg_toy_desc {
        const void* x;   /* bf16; not a field: int ghost; */
        float* dw;
        int nB, Lx, Cx, seg_size;
        long long s_tap, s_c;
        float alpha;
        double g;
      } cg_toy_desc;
      int cg_toy(const cg_toy_desc* d, void* stream);
      ''')
  toy = structs['cg_toy_desc']
  assert toy.__name__ == 'ToyDesc' and issubclass(toy, C.Structure)
  assert toy._fields_ == [
      ('x', C.c_void_p), ('dw', C.c_void_p), ('nB', C.c_int), ('Lx', C.c_int),
      ('Cx', C.c_int), ('seg_size', C.c_int), ('s_tap', C.c_longlong),
      ('s_c', C.c_longlong), ('alpha', C.c_float), ('g', C.c_double)]
  argtypes, restype = protos['cg_toy']
  assert argtypes[0]._type_ is toy and argtypes[1] is VOID and restype is C.c_int
  d = toy()
  d.x, d._keep = 0x1000, [1]  # an address in a field, a Python attribute beside
  assert d.x == 0x1000 and d._keep == [1]


def test_pointer_table_parameter():
  protos = _lib.parse_header('int cg_t(void* const* x0, int n);')[2]
  assert protos['cg_t'][0] == [C.POINTER(C.c_void_p), C.c_int]


def test_prototype_inside_a_comment_is_ignored():
  protos = _lib.parse_header('''
      /* int cg_block(unsigned n);
       *   blocks = cg_pack_plan_build(descs, n, NULL, 0);   (sizing pass) */
      // int cg_line(size_t n);
      int cg_real(int n);
      ''')[2]
  assert list(protos) == ['cg_real']


@pytest.mark.parametrize('text, named', [
    ('int cg_ok(int a);\nint cg_u(const float* x, unsigned n);', 'cg_u'),
    ('int cg_s(size_t bytes, void* stream);', 'cg_s'),
    ('int cg_p(const cg_other_desc* d);', 'cg_p'),
    ('int cg_cb(int (*fn)(int), int n);', 'cg_cb'),
    ('typedef struct cg_a_desc { struct { int a; } in; int b; } cg_a_desc;',
     'cg_a_desc'),
    ('typedef struct cg_b_desc { unsigned n; } cg_b_desc;', 'unsigned n'),
    ('float cg_r(int n);', 'cg_r'),
    ('int cg_unnamed(int, float);', 'cg_unnamed'),
    ('#define CG_MASK (1 << 3)', 'CG_MASK'),
])
def test_what_the_reader_does_not_understand_raises(text, named):
  with pytest.raises(_lib.HipLibraryError) as e:
    _lib.parse_header(text)
  assert named in str(e.value)


def test_missing_header_names_the_path(monkeypatch):
  monkeypatch.setattr(_lib, 'HEADER', '/nonexistent/calciumgan_hip.h')
  with pytest.raises(_lib.HipLibraryError) as e:
    _lib._read_header()
  assert '/nonexistent/calciumgan_hip.h' in str(e.value)


def test_the_real_header_is_bound_whole():
  text = open(_lib.HEADER).read()
  assert _lib.CG_ABI_VERSION == int(
      re.search(r'#define CG_ABI_VERSION (\d+)', text).group(1))
  assert [s.__name__ for s in (_lib.ConvDesc, _lib.PackDesc, _lib.WgradDesc)
         ] == ['ConvDesc', 'PackDesc', 'WgradDesc']
  assert sorted(_lib.STRUCTS) == ['cg_conv_desc', 'cg_pack_desc',
                                  'cg_wgrad_desc']
  assert _lib.SIGNATURES['cg_swconv'][0]._type_ is _lib.ConvDesc
  assert _lib.SIGNATURES['cg_adam'][:5] == [FLOAT, FLOAT, FLOAT, FLOAT,
                                            C.c_longlong]
  assert _lib.SIGNATURES['cg_pair_histogram'][-5:] == [INT, INT, DOUBLE, INT,
                                                       VOID]


def test_struct_layouts_match_the_c_compiler(tmp_path):
  """sizeof and every offsetof, as the host C compiler lays the real header
  out, against the ctypes classes read from the same header."""
  lines = ['#include <stdio.h>', '#include "calciumgan_hip.h"',
           'int main(void) {']
  for name, cls in _lib.STRUCTS.items():
    lines.append('  printf("{0} %zu\\n", sizeof({0}));'.format(name))
    for field, _ in cls._fields_:
      lines.append('  printf("{0}.{1} %zu %zu\\n", offsetof({0}, {1}), '
                   'sizeof((({0}*)0)->{1}));'.format(name, field))
  lines += ['  return 0;', '}']
  src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
  src.write_text('\n'.join(lines) + '\n')
  subprocess.check_call(['gcc', '-I', os.path.dirname(_lib.HEADER), '-o',
                         str(exe), str(src)])
  got = subprocess.check_output([str(exe)]).decode().split('\n')
  want = []
  for name, cls in _lib.STRUCTS.items():
    want.append('{} {}'.format(name, C.sizeof(cls)))
    for field, ctype in cls._fields_:
      want.append('{}.{} {} {}'.format(name, field, getattr(cls, field).offset,
                                       C.sizeof(ctype)))
  assert got == want + ['']
  assert len(want) == 3 + 50 + 14 + 24


_TENSORS = [(FLOAT, torch.float32), (DOUBLE, torch.float64), (INT, torch.int32)]


def test_tensor_goes_into_the_matching_typed_pointer():
  for ptr, dtype in _TENSORS:
    t = torch.zeros(5, dtype=dtype)
    assert ptr.from_param(t).value == t.data_ptr()
    assert ptr.from_param(t[2:]).value == t.data_ptr() + 2 * t.element_size()


def test_tensor_of_another_dtype_raises():
  for ptr, own in _TENSORS:
    for dtype in (torch.float32, torch.float64, torch.int32, torch.bfloat16,
                  torch.float16, torch.int64):
      if dtype is own:
        continue
      with pytest.raises(TypeError) as e:
        ptr.from_param(torch.zeros(3, dtype=dtype))
      assert ptr.ctype in str(e.value) and str(own) in str(e.value)
      assert str(dtype) in str(e.value)


def test_void_pointer_takes_any_dtype():
  for dtype in (torch.float32, torch.float64, torch.int32, torch.bfloat16,
                torch.float16, torch.uint8):
    t = torch.zeros(4, dtype=dtype)
    assert VOID.from_param(t).value == t.data_ptr()


def test_none_arrays_byref_and_ints_pass_as_c_void_p_takes_them():
  """Through a real foreign call, so that the converted value is what arrives:
  memmove(dst, src, n) declared with the data-pointer argtypes."""
  libc = C.CDLL(None)
  move = libc.memmove
  move.restype = C.c_void_p
  for ptr in (VOID, FLOAT, INT):
    assert ptr.from_param(None) is None  # ctypes passes NULL
    move.argtypes = [ptr, ptr, C.c_size_t]
    assert move(None, None, 0) is None
    src, dst = (C.c_float * 3)(1.0, 2.0, 3.0), (C.c_float * 3)()
    assert move(dst, src, 12) == C.addressof(dst) and list(dst) == [1, 2, 3]
    one, got = C.c_int(7), C.c_int()
    move(C.byref(got), C.byref(one), 4)
    assert got.value == 7
    move(C.addressof(got), C.addressof(src), 4)  # plain ints
    assert got.value == C.c_int.from_buffer(src).value
    move(C.c_void_p(C.addressof(got)), C.pointer(one), 4)
    assert got.value == 7
  t = torch.arange(3, dtype=torch.float32)
  move.argtypes = [FLOAT, FLOAT, C.c_size_t]
  move(dst, t, 12)
  assert list(dst) == [0, 1, 2]
  with pytest.raises(C.ArgumentError) as e:
    move(dst, t.double(), 12)
  assert 'float*' in str(e.value) and 'torch.float64' in str(e.value)
  with pytest.raises(C.ArgumentError):
    move(dst, 3.5, 4)  # (c_void_p takes no float either)


def test_call_names_the_entry_point_of_a_dtype_mismatch():
  cg_build.build(verbose=False)
  with pytest.raises(TypeError) as e:
    _lib.call('cg_neg_mean', torch.zeros(4, dtype=torch.bfloat16),
              torch.zeros(1), 4, None)
  for part in ('cg_neg_mean', 'argument 1', 'float*', 'torch.bfloat16'):
    assert part in str(e.value)


def test_load_refuses_a_library_of_another_abi_version(monkeypatch):
  cg_build.build(verbose=False)
  version = _lib.load().cg_abi_version()
  monkeypatch.setattr(_lib, '_libs', {})
  monkeypatch.setattr(_lib, 'CG_ABI_VERSION', version + 1)
  with pytest.raises(_lib.HipLibraryError) as e:
    _lib.load()
  assert 'stale build or binding' in str(e.value)
  assert str(version) in str(e.value) and str(version + 1) in str(e.value)
  monkeypatch.setattr(_lib, 'CG_ABI_VERSION', version)
  assert _lib.load().cg_abi_version() == version
