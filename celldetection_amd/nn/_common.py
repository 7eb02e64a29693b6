"""What every family of the package shares: the dtype table, the channels-last operand every kernel reads, the descriptor and the
launch of a dense ``cpn_conv2d``, and the one caller of the weight-gradient entry points."""
import ctypes

import torch

from .. import _lib

_DTYPES = {torch.float32: _lib.CONV_TRAIN_F32, torch.bfloat16: _lib.CONV_TRAIN_BF16}


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _dt(t):
    return 0 if t is None else _DTYPES[t.dtype]


def _nhwc(t, dtype=None):
    """[N, C, H, W] -> a detached tensor whose memory is NHWC from a 16-byte aligned address, as the kernels' 16-byte loads need:
    no copy for an aligned channels-last tensor of that dtype; a view into the middle of a buffer is cloned."""
    t = t.detach().to(dtype or t.dtype).contiguous(memory_format=torch.channels_last)
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.preserve_format)


def _conv_desc(cin, cout, k, bias):
    """cpn_op_desc of a plain dense conv: one source, act none, weights at offset 0."""
    d = _lib.OpDesc()
    d.op, d.src0, d.src1, d.res, d.dst = _lib.OP_CONV, 0, -1, -1, 1
    d.c0_used = d.cin_b = cin
    d.cout_b = d.cout_real = cout
    d.kh = d.kw = k
    d.stride, d.pad, d.bundles = 1, k // 2, 1
    d.weight_offset, d.bias_offset = 0, (0 if bias else -1)
    d.act, d.out_index, d.mult_offset = _lib.ACT_NONE, -1, -1
    d.fuse_weight_offset = d.fuse_bias_offset = -1
    return d


def _run_conv(src, packed, bias, cin, cout, k, res=None, stride=1):
    """cpn_conv2d on a bf16 tensor whose memory is NHWC -> bf16 [N, cout, Hout, Wout] in channels_last.  ``res``: a bf16 NHWC tensor
    of the output's shape added to the fp32 sum before the one rounding; ``stride`` 2: the pointwise conv (k = 1) only."""
    n, _, h, w = src.shape
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    out = torch.empty((n, cout, ho, wo), dtype=torch.bfloat16, device=src.device, memory_format=torch.channels_last)
    if out.numel() == 0:
        return out
    d = _conv_desc(cin, cout, k, bias is not None)
    res_stride = 0
    if stride != 1:
        assert k == 1, (k, stride)
        d.stride = stride
    if res is not None:
        assert tuple(res.shape) == tuple(out.shape) and res.dtype == torch.bfloat16, (tuple(res.shape), res.dtype)
        d.res, res_stride = 2, cout
    _lib.check(_lib.load().cpn_conv2d(ctypes.byref(d), _lib.ptr(src), cin, _lib.ptr(None), 0, _lib.ptr(res), res_stride, _lib.ptr(out),
                                      cout, n, h, w, _lib.ptr(packed), _lib.ptr(bias), _lib.stream_ptr()), 'conv2d')
    return out


# ---- the weight-gradient entry points.  ``cpn_<family>_wgrad``, ``cpn_<family>_wgrad_workspace_bytes`` and
# ``cpn_<family>_wgrad_info`` (family: conv, grouped_conv, cat_conv, resized_conv, stem) take one geometry (the integers between
# the operands and the results) and share their tails by design: the launch ends in (dw, dw_dtype, db, db_dtype, workspace,
# nbytes, stream), the query in nothing, the info in an int32[5].

def _weight_grad_info(family, *geometry):
    """-> dict(slabs, slab_rows, steps, reduce_chain, bias_chain) of ``cpn_<family>_wgrad_info``; raises like the launch for a
    geometry it rejects."""
    info = (ctypes.c_int32 * 5)()
    _lib.check(getattr(_lib.load(), f'cpn_{family}_wgrad_info')(*geometry, info), f'{family}_wgrad_info')
    return dict(zip(('slabs', 'slab_rows', 'steps', 'reduce_chain', 'bias_chain'), (int(v) for v in info)))


def _grad_dtypes(dtype, bias_dtype):
    """-> (dtype, bias_dtype) of dW and db, ``bias_dtype`` None being ``dtype``; both must be float32 or bfloat16."""
    bias_dtype = dtype if bias_dtype is None else bias_dtype
    if dtype not in _DTYPES or bias_dtype not in _DTYPES:
        raise NotImplementedError(f'dtype {dtype} / {bias_dtype}: gradients are float32 or bfloat16')
    return dtype, bias_dtype


def _weight_grad(family, geometry, operands, dw_shape, device, weight, bias, dtypes, fill, no_pixels=False, launch_geometry=None):
    """The call behind every ``*_weight_grad`` -> (dW | None, db | None), None where not asked for.  ``dtypes``: what
    ``_grad_dtypes`` returned where the public function checks them.  ``fill`` (``torch.zeros`` | ``torch.empty``) allocates dW ``dw_shape`` and db
    ``[dw_shape[0]]``; with ``no_pixels`` (an empty input) they are returned as they are and nothing is launched.  ``operands``: a
    function -> the device tensors in front of the geometry, called only when something is launched.  A query that returns no size
    asks ``cpn_<family>_wgrad_info`` to raise the reason.  ``launch_geometry``: where the launch takes other integers than the query."""
    dtype, bias_dtype = dtypes
    dw = fill(tuple(dw_shape), dtype=dtype, device=device) if weight else None
    db = fill((dw_shape[0],), dtype=bias_dtype, device=device) if bias else None
    if no_pixels or not (weight or bias):
        return dw, db
    tensors = operands()
    lib = _lib.load()
    nbytes = int(getattr(lib, f'cpn_{family}_wgrad_workspace_bytes')(*geometry))
    if nbytes <= 0:
        _lib.check(getattr(lib, f'cpn_{family}_wgrad_info')(*geometry, (ctypes.c_int32 * 5)()), f'{family}_wgrad')
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    launch = getattr(lib, f'cpn_{family}_wgrad')
    _lib.check(launch(*(_lib.ptr(t) for t in tensors), *(launch_geometry or geometry), _lib.ptr(dw), _DTYPES[dtype], _lib.ptr(db),
                      _DTYPES[bias_dtype], _lib.ptr(ws), nbytes, _lib.stream_ptr()), f'{family}_wgrad')
    return dw, db
