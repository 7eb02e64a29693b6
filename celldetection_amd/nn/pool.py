"""The max-pool in front of ``layer1`` and of the U-Net encoders ("Trainable stem and max-pool" of include/cpn_hip.h,
csrc/pool_train.hip, csrc/pool_adjoint.h; the family is described with the stem's, in stem.py): ``max_pool2d`` stores one ``uint8``
tap index per output element and saves nothing else; its backward is a gather in a fixed order (no atomics, no scatter)."""
import torch

from .. import _lib
from ..ops import _need_cuda
from ._common import _DTYPES, _nhwc, _pair

POOL_GEOMETRIES = ((3, 2, 1), (2, 2, 0))


def _pool_unsupported(kernel_size, stride, padding, dilation=1, ceil_mode=False, return_indices=False):
    """The first argument the trainable max-pool does not run, as a sentence, or None."""
    if _pair(dilation) != (1, 1):
        return f'dilation {dilation}: dilation 1 only'
    if ceil_mode:
        return 'ceil_mode True: floor mode only'
    if return_indices:
        return 'return_indices True: the tap index stays inside the function'
    k, s, p = _pair(kernel_size), _pair(kernel_size if stride is None else stride), _pair(padding)
    if k[0] != k[1] or s[0] != s[1] or p[0] != p[1] or (k[0], s[0], p[0]) not in POOL_GEOMETRIES:
        return f'kernel_size {kernel_size}, stride {stride}, padding {padding}: (kernel_size, stride, padding) in {POOL_GEOMETRIES} only'
    return None


class _MaxPool2dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s, pad):
        n, c, h, w = (int(v) for v in x.shape)
        ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
        xs = _nhwc(x)
        y = torch.empty((n, c, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        index = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device)
        _lib.check(_lib.load().cpn_maxpool2d_indexed(_lib.ptr(xs), _DTYPES[x.dtype], n, h, w, c, k, s, pad, _lib.ptr(y), _lib.ptr(index),
                                                     _lib.stream_ptr()), 'maxpool2d_indexed')
        ctx.save_for_backward(index)  # one byte per output element; neither x nor y
        ctx.geometry, ctx.size, ctx.dtype = (k, s, pad), (n, c, h, w), x.dtype
        return y

    @staticmethod
    def backward(ctx, grad_output):
        index, = ctx.saved_tensors
        n, c, h, w = ctx.size
        k, s, pad = ctx.geometry
        gs = _nhwc(grad_output, ctx.dtype)
        dx = torch.empty((n, c, h, w), dtype=ctx.dtype, device=gs.device, memory_format=torch.channels_last)
        _lib.check(_lib.load().cpn_maxpool2d_backward(_lib.ptr(gs), _lib.ptr(index), _DTYPES[ctx.dtype], n, h, w, c, k, s, pad,
                                                      _lib.ptr(dx), _lib.stream_ptr()), 'maxpool2d_backward')
        return dx, None, None, None


def max_pool2d(x, kernel_size, stride=None, padding=0, dilation=1, ceil_mode=False, return_indices=False):
    """``torch.nn.functional.max_pool2d`` for ``(kernel_size, stride, padding)`` = (3, 2, 1) or (2, 2, 0) on a 4-D float32 or
    bfloat16 input with ``C`` a positive multiple of 8 -> the output in ``x``'s dtype and ``torch.channels_last``, with torch's tie
    rule (the first maximum of a window in raster order takes the gradient).  Saves one ``uint8`` per output element.  Inputs are
    finite: NaN is outside the contract."""
    why = _pool_unsupported(kernel_size, stride, padding, dilation, ceil_mode, return_indices)
    if why is not None:
        raise NotImplementedError(why)
    if x.dim() != 4:
        raise NotImplementedError(f'input of {x.dim()} dimensions: the trainable max-pool takes a 4-D [N, C, H, W] input')
    if x.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {x.dtype}: the trainable max-pool takes float32 or bfloat16 activations')
    n, c, h, w = (int(v) for v in x.shape)
    if c < 8 or c % 8:
        raise NotImplementedError(f'input of {c} channels (C % 8 != 0): the trainable max-pool needs a positive multiple of 8')
    k, pad = _pair(kernel_size)[0], _pair(padding)[0]
    s = k if stride is None else _pair(stride)[0]
    if n < 1 or h + 2 * pad < k or w + 2 * pad < k:
        raise ValueError(f'input of size {tuple(x.shape)}: the output of a {k}x{k} pool would be empty')
    _need_cuda(x)
    return _MaxPool2dFunction.apply(x, k, s, pad)


class MaxPool2d(torch.nn.MaxPool2d):
    """``torch.nn.MaxPool2d`` with torch's constructor arguments whose forward is ``max_pool2d``; an argument outside the supported
    family raises ``NotImplementedError`` naming it."""

    def __init__(self, kernel_size, stride=None, padding=0, dilation=1, return_indices=False, ceil_mode=False):
        why = _pool_unsupported(kernel_size, stride, padding, dilation, ceil_mode, return_indices)
        if why is not None:
            raise NotImplementedError(why)
        super().__init__(kernel_size, stride, padding, dilation, return_indices, ceil_mode)

    def forward(self, x):
        return max_pool2d(x, self.kernel_size, self.stride, self.padding)


def _pool_why_not(pool):
    if type(pool) is not torch.nn.MaxPool2d:
        return f'a subclass of torch.nn.MaxPool2d ({type(pool).__name__}): its forward may differ'
    return _pool_unsupported(pool.kernel_size, pool.stride, pool.padding, pool.dilation, pool.ceil_mode, pool.return_indices)
