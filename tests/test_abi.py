"""The binding is derived from include/cpn_hip.h (celldetection_amd/_header.py, _lib.py): the parser on literal snippets, and the
real header against a crude count of its own, the symbols of the built library, the compiler's struct layout and literal values.
Nothing here needs a GPU.  An ABI bump is typed by hand in two places: the header and the version test below."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint8, c_uint32, c_uint64, c_void_p

import pytest

import celldetection_amd as cda
from celldetection_amd import _header, _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'cpn_hip.h')
STRUCTS = {'cpn_tensor_desc': _lib.TensorDesc, 'cpn_op_desc': _lib.OpDesc, 'CpnObjectiveArgs': _lib.ObjectiveArgs,
           'CpnOptimTensor': _lib.OptimTensor}

SNIPPET = '''
#ifndef CPN_SNIPPET_H
#define CPN_SNIPPET_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define CPN_HOST  /* an empty macro: no constant */
#define CPN_ANSWER 42
#define CPN_E_BAD (-7)  // negative, in parentheses
#define CPN_NEG -3
#define CPN_MASK 0x10
enum { CPN_A = 0, CPN_B = 5, CPN_C, CPN_D = 2 };
typedef struct {
    int32_t src0, src1, res;  /* three fields of one declaration */
    float scale;
    int64_t offset;
} cpn_small;
typedef struct CpnArgs {
    const float *scores, *locations;
    void *p;
    double w;
    uint8_t flag;
} CpnArgs;
typedef struct cpn_plan cpn_plan;
const char *cpn_last_error(void);
void cpn_plan_destroy(cpn_plan *plan);
int cpn_plan_create(cpn_plan **plan, const cpn_small *ops, int32_t n, const void *weights,
                    size_t weight_bytes,
                    const float *bias);
int64_t cpn_bytes(int64_t n, double x, float y, uint32_t a, uint8_t b);
int cpn_refine(float *contours /* in/out [P,S,2], a comma */, const CpnArgs *args, int32_t info[5], int64_t more[]);
int cpn_probe(CPN_HOST unsigned long long *out15, int reset, unsigned long long ticks);
int cpn_run(cpn_plan *plan, float *const *outputs, CPN_HOST int32_t *h, const CPN_HOST int64_t *offsets, int32_t *device);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_parser_reads_every_shape_the_header_uses():
    h = _header.parse(SNIPPET)
    assert h.constants == dict(CPN_ANSWER=42, CPN_E_BAD=-7, CPN_NEG=-3, CPN_MASK=16, CPN_A=0, CPN_B=5, CPN_C=6, CPN_D=2)
    small, args = h.structs['cpn_small'], h.structs['CpnArgs']
    assert list(h.structs) == ['cpn_small', 'CpnArgs'] and issubclass(small, ctypes.Structure)
    assert small._fields_ == [('src0', c_int32), ('src1', c_int32), ('res', c_int32), ('scale', c_float), ('offset', c_int64)]
    assert args._fields_ == [('scores', c_void_p), ('locations', c_void_p), ('p', c_void_p), ('w', c_double), ('flag', c_uint8)]
    assert list(h.prototypes) == ['cpn_last_error', 'cpn_plan_destroy', 'cpn_plan_create', 'cpn_bytes', 'cpn_refine', 'cpn_probe',
                                  'cpn_run']
    assert h.prototypes['cpn_last_error'] == (c_char_p, [])
    assert h.prototypes['cpn_plan_destroy'] == (None, [c_void_p])
    assert h.prototypes['cpn_plan_create'] == (c_int32, [POINTER(c_void_p), POINTER(small), c_int32, c_void_p, c_size_t, c_void_p])
    assert h.prototypes['cpn_bytes'] == (c_int64, [c_int64, c_double, c_float, c_uint32, c_uint8])
    assert h.prototypes['cpn_refine'] == (c_int32, [c_void_p, POINTER(args), POINTER(c_int32), POINTER(c_int64)])
    assert h.prototypes['cpn_probe'] == (c_int32, [POINTER(c_uint64), c_int32, c_uint64])
    assert h.prototypes['cpn_run'] == (c_int32, [c_void_p, POINTER(c_void_p), POINTER(c_int32), POINTER(c_int64), c_void_p])
    assert ctypes.c_int is c_int32 and ctypes.c_ulonglong is c_uint64  # (what the hand-written table called them)


@pytest.mark.parametrize('text, named', [
    ('int cpn_x(int32_t a, floaty *b);', ('cpn_x', 'parameter 2', 'floaty')),  # an unknown type
    ('int cpn_x(int32_t a, struct foo *b);', ('cpn_x', 'parameter 2')),
    ('long cpn_x(int32_t a);', ('cpn_x', 'long')),  # an unknown return type
    ('int cpn_x(int32_t a, char *b);', ('cpn_x', 'parameter 2')),  # a type without a ctypes counterpart here
    ('int cpn_x(int32_t a, float ***b);', ('cpn_x', 'parameter 2')),
    ('int cpn_x(int32_t a;\nint cpn_y(void);', ('cpn_x',)),  # unbalanced: must not vanish
    ('int cpn_y(void);\nint cpn_x(int32_t a, float *b)', ('cpn_x',)),  # no closing ';'
    ('int cpn_x(int (*callback)(int));', ('cpn_x',)),
    ('int cpn_x(void);\nint cpn_x(void);', ('cpn_x',)),  # declared twice
    ('typedef struct { int32_t a; floaty b; } cpn_s;', ('cpn_s', 'floaty')),
    ('typedef struct { int32_t a; int32_t; } cpn_s;', ('cpn_s',)),
    ('#define CPN_X 1.5', ('CPN_X', '1.5')),
    ('#define CPN_X (1 << 4)', ('CPN_X',)),
    ('#define CPN_X 3 \\\n', ('CPN_X',)),
    ('enum { CPN_A = 0, CPN_B = CPN_A + 1 };', ('CPN_B',)),
    ('static int x = 3;', ('static int x',)),  # a statement of no known kind
])
def test_parser_raises_naming_what_it_cannot_read(text, named):
    with pytest.raises(ValueError) as e:
        _header.parse(text)
    for word in named:
        assert word in str(e.value), (word, str(e.value))


def test_every_prototype_of_the_header_is_parsed():
    """A deliberately crude count of its own: the ``cpn_name(`` of the comment-stripped header inside a text that ends in ';'."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', open(HEADER).read(), flags=re.S)
    crude = [name for piece in text.split(';')[:-1] for name in re.findall(r'\b(cpn_\w+)\s*\(', piece)]
    h = _header.header()
    assert len(crude) == len(h.prototypes) == len(_lib.EXPORTED_SYMBOLS) == len(set(crude)) >= 146
    assert tuple(crude) == tuple(h.prototypes) == _lib.EXPORTED_SYMBOLS  # in header order
    assert h is _header.header()  # parsed once per process
    assert sorted(STRUCTS) == sorted(h.structs) and all(h.structs[name] is cls for name, cls in STRUCTS.items())
    lib = _lib.load()
    for name, (restype, argtypes) in h.prototypes.items():
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes, name
    # the one marker for host memory: on scalar pointers only, and every array parameter is host memory without it
    marked = re.findall(r'CPN_HOST\s+([^,)]*)', text.replace('#define CPN_HOST', ''))
    assert marked and all(re.fullmatch(r'(const )?(u?int\d+_t|float|double|unsigned long long) \*\w+', m.strip()) for m in marked)


def test_library_exports_exactly_what_the_header_declares():
    nm = shutil.which('nm')
    if nm is None:
        pytest.skip('nm (binutils) is not installed: the dynamic symbols of the library cannot be listed')
    out = subprocess.run([nm, '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith('cpn_')}
    declared = set(_header.header().prototypes)
    assert exported - declared == set(), 'exported by the library, missing from include/cpn_hip.h'
    assert declared - exported == set(), 'declared by include/cpn_hip.h, defined by no unit'


def test_struct_layouts_are_the_compilers(tmp_path):
    """sizeof and every offsetof of the four structs as the C++ compiler lays them out = the ctypes classes = the numpy record."""
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "cpn_hip.h"', 'int main() {']
    for name, cls in STRUCTS.items():
        lines.append(f'    std::printf("{name} sizeof %zu\\n", sizeof({name}));')
        lines += [f'    std::printf("{name} {f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    src, exe = tmp_path / 'layout.cpp', str(tmp_path / 'layout')
    src.write_text('\n'.join(lines + ['    return 0;', '}', '']))
    subprocess.check_call([build._hipcc(), '-x', 'c++', '-std=c++17', '-I' + os.path.dirname(HEADER), str(src), '-o', exe])
    got = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        name, field, value = line.split()
        got.setdefault(name, {})[field] = int(value)
    for name, cls in STRUCTS.items():
        want = dict(sizeof=ctypes.sizeof(cls), **{f: getattr(cls, f).offset for f, _ in cls._fields_})
        assert got[name] == want and len(want) == len(cls._fields_) + 1, name
    rec = cda.optim._RECORD
    assert dict(sizeof=rec.itemsize, **{f: rec.fields[f][1] for f in rec.names}) == got['CpnOptimTensor']
    assert rec.itemsize == _lib.OPTIM_TENSOR_BYTES == 80 and rec.names == tuple(f for f, _ in _lib.OptimTensor._fields_)
    assert [rec.fields[f][0].str for f in rec.names] == ['<u8'] * 4 + ['<i8', '<i4', '<i4'] + ['<f4'] * 8
    assert ctypes.sizeof(_lib.TensorDesc) == 12 and _lib.OpDesc.weight_offset.offset == 64 and _lib.ObjectiveArgs.w_fourier.offset == 168


def test_version_of_header_binding_and_library():
    text = open(HEADER).read()
    assert int(re.search(r'#define\s+CPN_ABI_VERSION\s+(\d+)', text).group(1)) == _lib.ABI_VERSION == _lib.load().cpn_abi_version() == 22


def test_constants_have_the_headers_values():
    """Plain literals per family: a parser that read garbage would not pass by agreeing with itself."""
    assert (_lib.OP_INPUT, _lib.OP_CONV, _lib.OP_ACT) == (0, 1, 9) and (_lib.ACT_NONE, _lib.ACT_TANH_SCALED, _lib.ACT_SOFTPLUS) == (0, 3, 12)
    assert (_lib.E_INVALID, _lib.E_UNSUPPORTED, _lib.E_WORKSPACE, _lib.E_INTERNAL) == (-1, -2, -3, -4)
    assert (_lib.SUBPIXEL_NONE, _lib.SUBPIXEL_SCATTER, _lib.SUBPIXEL_BL_FRAME) == (0, 4, 7)
    assert (_lib.PRECISION_BF16, _lib.PRECISION_F32, _lib.PRECISION_FP8) == (0, 1, 2)
    assert (_lib.OUT_SCORES, _lib.OUT_UNCERTAINTY, _lib.NUM_OUTPUTS) == (0, 4, 5)
    assert _lib.PROP_CODES['orientation'] == 14 and _lib.PROP_NAMES[0] == 'label' and len(_lib.PROP_NAMES) == _lib.PROP_COUNT == 18
    assert _lib.PROP_CODES['equivalent_diameter_area'] == 6 and 'count' not in _lib.PROP_NAMES
    assert _lib.SHAPE_NAMES[-1] == 'solidity' and _lib.SHAPE_CODES['euler_number'] == 4 and len(_lib.SHAPE_NAMES) == _lib.SHAPE_COUNT == 7
    assert (_lib.PROPS_U8, _lib.PROPS_I16, _lib.PROPS_I32) == (0, 1, 2)
    assert _lib.CONV_MODE_NAMES == {0: 'PW', 1: 'S1', 2: 'S2', 3: 'BL', 6: 'N', 7: 'S1F', 8: 'BR', 10: 'S1Q'}
    assert (_lib.OPTIM_CHUNK, _lib.OPTIM_FLAG_SCALAR) == (8192, 1) and (_lib.CONV_TRAIN_F32, _lib.CONV_TRAIN_BF16) == (0, 1)
    assert (_lib.DIST_L1, _lib.DIST_L2, _lib.DIST_C) == (1, 2, 3) == (cda.targets.DIST_L1, cda.targets.DIST_L2, cda.targets.DIST_C)
    assert (_lib.OBJECTIVE_MAX_ITERATIONS, _lib.OBJECTIVE_META_WORDS, _lib.OBJECTIVE_FLAG_CLASS_RANGE) == (64, 2, 4)
    assert _lib.COMPONENTS_MODES == dict(equal=0, nonzero=1) and _lib.CONV_PACK_MODES == dict(forward=0, dgrad=1)
    assert cda.flat_labels.MAX_STEPS == cda.targets.MAX_STEPS == 8 and cda.fourier.CHUNK == 256 and cda.fourier.MAX_ORDER == 64
    assert cda.label_contours.TILE == cda.overlay.TILE == 32
    assert not hasattr(_lib, 'HOST') and not hasattr(_lib, 'HIP_H')  # macros without a value define nothing


def test_bind_refuses_a_missing_library_and_a_missing_header(tmp_path, monkeypatch):
    with pytest.raises(RuntimeError, match='not found'):
        _lib.bind(str(tmp_path / 'libnone.so'))
    assert _lib.bind(_lib.LIB_PATH).cpn_abi_version() == _lib.ABI_VERSION  # a second handle, typed like load()'s
    monkeypatch.setattr(_header, '_header', None)
    monkeypatch.setattr(_header, 'HEADER_PATH', str(tmp_path / 'cpn_hip.h'))
    with pytest.raises(RuntimeError, match=re.escape(str(tmp_path / 'cpn_hip.h'))):
        _header.header()
