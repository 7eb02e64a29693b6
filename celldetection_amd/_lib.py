"""ctypes binding of libcpn_hip.so (the C ABI declared in include/cpn_hip.h).  Every signature, struct and constant here is read
from that header (_header.py); this module adds only what the header does not state.

The product path has NO CPU fallback: if the HIP library is missing or does not export the expected symbols,
importing the binding raises, and every op raises ``RuntimeError`` on failure with ``cpn_last_error()``.
"""
import ctypes
import os
from ctypes import c_int32, c_void_p

from ._header import header

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CPN_HIP_LIB') or os.path.join(HERE, 'libcpn_hip.so')  # env: kernel A/B tuning only

_h = header()
# every CPN_X of the header (integer #defines and enumerators) is X here: ABI_VERSION, E_*, OP_*, ACT_*, SUBPIXEL_*, OUT_*, ...
globals().update((name[len('CPN_'):], value) for name, value in _h.constants.items())


def _names(prefix):
    """Lower-cased suffixes of the header's CPN_<prefix>* constants in value order, without COUNT."""
    found = sorted((v, k[len(prefix):].lower()) for k, v in _h.constants.items() if k.startswith(prefix) and k != prefix + 'COUNT')
    return tuple(name for _, name in found)


# conv kernel modes (CPN_CONV_MODE_*) as cpn_conv2d_kernel_info reports them
CONV_MODE_NAMES = {v: k[len('CPN_CONV_MODE_'):] for k, v in _h.constants.items() if k.startswith('CPN_CONV_MODE_')}
# region properties (CPN_PROP_*) and shape properties (CPN_SHAPE_*), in code order
PROP_NAMES, SHAPE_NAMES = _names('CPN_PROP_'), _names('CPN_SHAPE_')
PROP_CODES = {name: code for code, name in enumerate(PROP_NAMES)}
SHAPE_CODES = {name: code for code, name in enumerate(SHAPE_NAMES)}
COMPONENTS_MODES = {'equal': COMPONENTS_EQUAL, 'nonzero': COMPONENTS_NONZERO}
CONV_PACK_MODES = {'forward': CONV_PACK_FORWARD, 'dgrad': CONV_PACK_DGRAD}
CONV_TRAIN_F32, CONV_TRAIN_BF16 = 0, 1  # the `dtype` arguments of the training calls: the header states the codes in prose, no macro

TensorDesc, OpDesc = _h.structs['cpn_tensor_desc'], _h.structs['cpn_op_desc']
ObjectiveArgs, OptimTensor = _h.structs['CpnObjectiveArgs'], _h.structs['CpnOptimTensor']
OPTIM_TENSOR_BYTES = ctypes.sizeof(OptimTensor)

EXPORTED_SYMBOLS = tuple(_h.prototypes)  # every function the header declares, in its order

_lib = None


def bind(path):
    """Loads the library at ``path`` and types every function the header declares; raises RuntimeError (never falls back) when
    the file or a symbol is missing or its ABI version is not the header's."""
    if not os.path.isfile(path):
        raise RuntimeError(f'{path} not found: build the HIP extension first '
                           f'(python -m celldetection_amd.build); there is no CPU fallback.')
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in _h.prototypes.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f'{path} does not export {name}; rebuild it.') from e
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.cpn_abi_version() != ABI_VERSION:
        raise RuntimeError(f'{path} ABI version {lib.cpn_abi_version()} != expected {ABI_VERSION}; rebuild it.')
    return lib


def load():
    """libcpn_hip.so, bound once per process."""
    global _lib
    if _lib is None:
        _lib = bind(LIB_PATH)
    return _lib


def check(rc, what=''):
    if rc != 0:
        msg = load().cpn_last_error()
        raise RuntimeError(f'libcpn_hip {what} failed (code {rc}): {msg.decode() if msg else "?"}')


def stream_ptr():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device/host pointer of a tensor (None -> NULL)."""
    return c_void_p(0 if t is None else t.data_ptr())


def conv_kernel_info(op, precision, n, hin, win, c0_stride, c1_stride=0, res_stride=0, dst_stride=0):
    """The kernel cpn_conv2d (PRECISION_BF16; a CONV_BRIDGE descriptor: cpn_conv_bridge) or cpn_conv2d_fp8 (PRECISION_FP8)
    would launch for this descriptor, these channel strides and this input size -> (mode name, TH, BN, WM, WN): the
    instantiation conv_igemm_kernel<TH, BN, WM, WN, mode>.  Host arithmetic only: needs no GPU.  Raises like the launch
    itself for a call it rejects."""
    info = (c_int32 * 5)()
    check(load().cpn_conv2d_kernel_info(op, precision, c0_stride, c1_stride, res_stride, dst_stride, n, hin, win, info),
          'conv2d_kernel_info')
    return (CONV_MODE_NAMES[info[0]],) + tuple(info[1:])
