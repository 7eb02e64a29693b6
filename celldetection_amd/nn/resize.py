"""The bilinear resize behind the heads ("Trainable bilinear resize" of include/cpn_hip.h, csrc/bilinear_train.hip,
csrc/bilinear_adjoint.h)

The reference's ``CPNCore`` enlarges the refinement features to the input's size in front of the refinement head
(``refinement_full_res``) and every head map that is smaller than the input (``_equal_size``, ``models/cpn.py:109-115, 277-279``).
``resized_conv2d`` runs the first as one autograd function on the low-resolution features: the conv's loader blends (MODE_BL of
the inference path), the weight gradient blends while it stages, the input gradient goes through the adjoint of the resize as a
gather, ``bilinear_resize_backward``; the resized tensor -- the largest activation of the net -- is neither written nor saved.
``bilinear_resize`` is the resize on its own, for activations and for the fp32 head maps; it saves nothing but the sizes.
``CPNCore`` / ``convert_cpn_core_`` put both where the reference's core has ``F.interpolate``.  Known limits: the gradient at the
input's size (``T``) is written and read once, before it is summed; the training forward is not decomposed into sub-pixel phases; upward resizes,
``'bilinear'`` and k in {3, 5, 7} only.
"""
import ctypes

import torch

from .. import _lib
from ..ops import _need_cuda
from ._common import _DTYPES, _conv_desc, _grad_dtypes, _nhwc, _pair, _run_conv, _weight_grad, _weight_grad_info
from .conv import Conv2d, _unsupported, _why_not, conv2d, pack_weight

RESIZED_KERNEL_SIZES = (3, 5, 7)


def _resize_sizes(what, shape, size):
    """(N, C, h, w) and (H, W) of an upward resize, or NotImplementedError naming the argument."""
    n, c, h, w = (int(v) for v in shape)
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise NotImplementedError(f'size {size!r}: {what} takes a pair (H, W)') from None
    if n < 1 or h < 1 or w < 1:
        raise NotImplementedError(f'input of shape {tuple(shape)}: {what} needs at least one pixel')
    if H < h or W < w:
        raise NotImplementedError(f'size {(H, W)} for an input of {h} x {w} pixels: {what} resizes upwards only')
    return (n, c, h, w), (H, W)


def _planes(t):
    """Whether ``t`` belongs to the plane family: fp32 whose memory is NCHW.  A tensor whose memory is NCHW and NHWC at once (one
    pixel, or one channel) belongs to it unless ``C % 8 == 0``."""
    return t.dtype == torch.float32 and t.is_contiguous() and \
        not (int(t.shape[1]) % 8 == 0 and t.is_contiguous(memory_format=torch.channels_last))


def _check_resize(what, x, size):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise NotImplementedError(f'input of {getattr(x, "dim", lambda: None)()} dimensions: {what} takes a 4-D [N, C, H, W] input')
    if x.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {x.dtype}: {what} takes float32 or bfloat16 activations')
    shape, size = _resize_sizes(what, x.shape, size)
    if not _planes(x) and (shape[1] < 8 or shape[1] % 8):
        raise NotImplementedError(f'input of {shape[1]} channels (C % 8 != 0) that is not float32 in contiguous NCHW: {what} needs a '
                                  f'positive multiple of 8 for activations; float32 NCHW planes take any C')
    return shape, size


def _resize_forward(x, size, planes):
    (n, c, h, w), (H, W) = (int(v) for v in x.shape), size
    lib = _lib.load()
    if planes:
        xs = x.detach()
        out = torch.empty((n, c, H, W), dtype=torch.float32, device=x.device)
        _lib.check(lib.cpn_resize_bilinear_f32(_lib.ptr(xs), _lib.ptr(out), n * c, h, w, H, W, _lib.stream_ptr()), 'resize_bilinear_f32')
        return out
    xs = _nhwc(x, torch.bfloat16)
    out = torch.empty((n, c, H, W), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    _lib.check(lib.cpn_resize_bilinear(_lib.ptr(xs), _lib.ptr(out), n, h, w, H, W, c, _lib.stream_ptr()), 'resize_bilinear')
    return out


def bilinear_resize_backward(t, size):
    """The adjoint of ``F.interpolate(x, size=t.shape[2:], mode='bilinear', align_corners=False)`` for ``x`` of ``size`` = (h, w), as a
    gather: every source pixel adds ``weight_y * weight_x * t`` over the output pixels that read it, in fp32, in ascending row-major
    order, the coefficient formed first, no fma, no atomics (bit-identical from run to run).  Two families, as ``bilinear_resize``:
    float32 ``t`` in contiguous NCHW, any ``C`` -> float32 NCHW (the sum as it is); any other float32 or bfloat16 ``t`` with ``C`` a
    positive multiple of 8 is rounded to bf16 on the way in -> bf16 ``[N, C, h, w]`` in ``torch.channels_last``, rounded once.
    1 <= h <= H, 1 <= w <= W.  Known limit: one lane walks a pixel's whole footprint, 4 x 4 at the exact x2 (5 next to the border); any ratio is
    correct, but a tiny ``size`` under a large ``t`` leaves a few lanes reading the whole image."""
    what = 'the bilinear resize adjoint'
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise NotImplementedError(f'input of {getattr(t, "dim", lambda: None)()} dimensions: {what} takes a 4-D [N, C, H, W] input')
    if t.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {t.dtype}: {what} takes float32 or bfloat16 activations')
    n, c, H, W = (int(v) for v in t.shape)
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise NotImplementedError(f'size {size!r}: {what} takes a pair (h, w)') from None
    if h < 1 or w < 1 or h > H or w > W or n < 1:
        raise NotImplementedError(f'size {(h, w)} for an input of shape {tuple(t.shape)}: {what} needs 1 <= h <= H and 1 <= w <= W and '
                                  f'at least one image')
    if not _planes(t) and (c < 8 or c % 8):
        raise NotImplementedError(f'input of {c} channels (C % 8 != 0) that is not float32 in contiguous NCHW: {what} needs a positive '
                                  f'multiple of 8 for activations; float32 NCHW planes take any C')
    _need_cuda(t)
    return _bilinear_sum(t, (h, w), _planes(t))


def _bilinear_sum(t, size, planes):
    """``cpn_bilinear_sum_f32`` on fp32 NCHW planes, ``cpn_bilinear_sum`` on bf16 NHWC activations (arguments checked by the caller)."""
    n, c, H, W = (int(v) for v in t.shape)
    h, w = size
    lib = _lib.load()
    if planes:
        ts = t.detach().float().contiguous()
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=t.device)
        if c > 0:
            _lib.check(lib.cpn_bilinear_sum_f32(_lib.ptr(ts), n * c, H, W, _lib.ptr(out), h, w, _lib.stream_ptr()), 'bilinear_sum_f32')
        return out
    ts = _nhwc(t, torch.bfloat16)
    out = torch.empty((n, c, h, w), dtype=torch.bfloat16, device=ts.device, memory_format=torch.channels_last)
    _lib.check(lib.cpn_bilinear_sum(_lib.ptr(ts), n, H, W, c, _lib.ptr(out), h, w, _lib.stream_ptr()), 'bilinear_sum')
    return out


class _BilinearResizeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size):
        ctx.low, ctx.planes, ctx.dtype = (int(x.shape[2]), int(x.shape[3])), _planes(x), x.dtype  # nothing but the sizes is kept
        return _resize_forward(x, size, ctx.planes)

    @staticmethod
    def backward(ctx, grad_output):
        return _bilinear_sum(grad_output, ctx.low, ctx.planes).to(ctx.dtype), None


def bilinear_resize(x, size):
    """``F.interpolate(x, size, mode='bilinear', align_corners=False)`` as one autograd function, for 1 <= h <= H and 1 <= w <= W
    (``size`` equal to the input's: ``x`` itself).  Two families: float32 ``x`` in contiguous NCHW, any ``C`` -- the head maps --
    -> float32 NCHW (``cpn_resize_bilinear_f32``, torch's operation order); any other float32 or bfloat16 ``x`` with ``C`` a positive
    multiple of 8 is rounded to bf16 -> bf16 in ``torch.channels_last`` (``cpn_resize_bilinear``: the blend in fp32, one rounding).
    The gradient is ``bilinear_resize_backward`` in ``x``'s dtype.  Saved for backward: nothing but the sizes."""
    shape, size = _check_resize('the bilinear resize', x, size)
    _need_cuda(x)
    if size == shape[2:]:
        return x
    return _BilinearResizeFunction.apply(x, size)


def _resized_channels(cin, cout, k):
    """Raises NotImplementedError naming the argument the resized conv does not run."""
    if k not in RESIZED_KERNEL_SIZES:
        raise NotImplementedError(f'kernel_size {k}: the resized conv runs square odd kernels {RESIZED_KERNEL_SIZES} only')
    if cin < 32 or cin % 32:
        raise NotImplementedError(f'in_channels {cin}: the resized conv needs a positive multiple of 32')
    if cout < 32 or cout % 32:
        raise NotImplementedError(f'out_channels {cout}: the resized conv needs a positive multiple of 32')


def _check_resized(x, weight, bias, size):
    """Raises for a call ``resized_conv2d`` does not run -> ((N, Cin, h, w), (H, W), Cout, k)."""
    what = 'the resized conv'
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise NotImplementedError(f'input of {getattr(x, "dim", lambda: None)()} dimensions: {what} takes a 4-D [N, C, h, w] input')
    if weight.dim() != 4:
        raise NotImplementedError(f'weight of {weight.dim()} dimensions: {what} needs [Cout, Cin, k, k]')
    if weight.shape[2] != weight.shape[3]:
        raise NotImplementedError(f'kernel_size {tuple(weight.shape[2:])}: {what} runs square kernels only')
    if weight.dtype not in _DTYPES:
        raise NotImplementedError(f'weight dtype {weight.dtype}: {what} takes float32 or bfloat16 parameters')
    if x.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {x.dtype}: {what} takes float32 or bfloat16 activations')
    cout, cin, k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
    _resized_channels(cin, cout, k)
    if int(x.shape[1]) != cin:
        raise ValueError(f'input has {int(x.shape[1])} channels, weight expects {cin}')
    shape, size = _resize_sizes(what, x.shape, size)
    if bias is not None and (bias.dim() != 1 or int(bias.shape[0]) != cout or bias.dtype not in _DTYPES):
        raise NotImplementedError(f'bias {tuple(bias.shape)} {bias.dtype}: {what} takes a float32 or bfloat16 [{cout}] bias')
    _need_cuda(x, weight, bias)
    return shape, size, cout, k


def _resized_desc(cin, cout, k, bias):
    """cpn_op_desc of the resized conv: the lone source read through the loader's bilinear map (MODE_BL)."""
    d = _conv_desc(cin, cout, k, bias)
    d.up0 = 2
    return d


def _run_resized_conv(xs, packed, bias, cin, cout, k, size):
    """xs: bf16 NHWC memory [N, cin, h, w] -> bf16 [N, cout, H, W] in channels_last: ``cpn_conv2d_sized`` with ``up0 = 2``."""
    n, _, h, w = (int(v) for v in xs.shape)
    H, W = size
    out = torch.empty((n, cout, H, W), dtype=torch.bfloat16, device=xs.device, memory_format=torch.channels_last)
    d = _resized_desc(cin, cout, k, bias is not None)
    stored = (ctypes.c_int32 * 6)(h, w, H, W, H, W)
    _lib.check(_lib.load().cpn_conv2d_sized(ctypes.byref(d), _lib.ptr(xs), cin, _lib.ptr(None), 0, _lib.ptr(None), 0, _lib.ptr(out), cout,
                                            n, H, W, stored, _lib.ptr(packed), _lib.ptr(bias), _lib.stream_ptr()), 'resized_conv2d')
    return out


def resized_weight_grad_info(n, h, w, cin, low_size, cout, k, slab_rows=0):
    """What ``resized_conv2d_weight_grad`` would run for ``n`` gradients of ``h`` x ``w`` and inputs of ``low_size`` -> dict(slabs,
    slab_rows, steps (MFMA steps per slab), reduce_chain, bias_chain).  Host arithmetic only: needs no GPU.  Raises like the launch
    for a call it rejects."""
    return _weight_grad_info('resized_conv', n, h, w, cin, int(low_size[0]), int(low_size[1]), cout, k, slab_rows)


def resized_conv2d_weight_grad(x, grad_output, kernel_size, slab_rows=0, weight=True, bias=True, dtype=torch.float32, bias_dtype=None):
    """(x [N, Cin, h, w], grad_output [N, Cout, H, W]) -> (dW [Cout, Cin, k, k] | None, db [Cout] | None): the gradients
    ``resized_conv2d`` returns for its weight and bias, as fp32 sums over the bf16-rounded operands of the virtual resized tensor --
    blended in fp32 from the bf16 ``x`` and rounded to bf16 while it is staged -- rounded once to ``dtype`` / ``bias_dtype``.
    ``slab_rows``: image rows per slab of the reduction (0: chosen by the library)."""
    _need_cuda(x, grad_output)
    k = int(kernel_size)
    n, cin, h, w = (int(v) for v in x.shape)
    cout, H, W = int(grad_output.shape[1]), int(grad_output.shape[2]), int(grad_output.shape[3])
    _resized_channels(cin, cout, k)
    dtypes = _grad_dtypes(dtype, bias_dtype)
    assert int(grad_output.shape[0]) == n, (tuple(grad_output.shape), tuple(x.shape))
    return _weight_grad('resized_conv', (n, H, W, cin, h, w, cout, k, slab_rows),
                        lambda: (_nhwc(x, torch.bfloat16), _nhwc(grad_output, torch.bfloat16)),
                        (cout, cin, k, k), x.device, weight, bias, dtypes, torch.empty)


class _ResizedConv2dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, size):
        cout, cin, k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        xs = _nhwc(x, torch.bfloat16)
        b32 = None if bias is None else bias.detach().float().contiguous()
        out = _run_resized_conv(xs, pack_weight(weight, 'forward'), b32, cin, cout, k, size)
        ctx.save_for_backward(xs, weight)  # x at its own low resolution: nothing of size's extent
        ctx.x_dtype = x.dtype
        ctx.bias_dtype = None if bias is None else bias.dtype
        return out

    @staticmethod
    def backward(ctx, grad_output):
        xs, weight = ctx.saved_tensors
        cout, cin, k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and ctx.bias_dtype is not None
        gs = _nhwc(grad_output, torch.bfloat16)
        dx = dw = db = None
        if need_x:  # T = the dgrad conv at size, then the adjoint of the resize
            t = _run_conv(gs, pack_weight(weight, 'dgrad'), None, cout, cin, k)
            dx = bilinear_resize_backward(t, xs.shape[2:]).to(ctx.x_dtype)
        if need_w or need_b:
            dw, db = resized_conv2d_weight_grad(xs, gs, k, weight=need_w, bias=need_b, dtype=weight.dtype,
                                                bias_dtype=ctx.bias_dtype or weight.dtype)
        return dx, dw, db, None


def resized_conv2d(x, weight, bias=None, size=None):
    """``F.conv2d(F.interpolate(x, size, mode='bilinear', align_corners=False), weight, bias, padding=k // 2)`` as one autograd
    function that never writes the resized tensor, with gradients for ``x``, ``weight`` and ``bias`` as autograd asks for them -> bf16
    ``[N, Cout, H, W]`` in ``torch.channels_last``.

    ``x`` ``[N, Cin, h, w]``, ``size`` = (H, W) with h <= H and w <= W at any ratio (equal sizes, or ``size=None``: ``conv2d``),
    ``weight`` ``[Cout, Cin, k, k]`` with k in {3, 5, 7}, ``Cin`` and ``Cout`` positive multiples of 32, stride 1, zero padding
    ``k // 2``, float32 or bfloat16 inputs and parameters on the GPU.  Anything else raises ``NotImplementedError`` naming the
    argument; there is no fallback.

    Arithmetic: ``x`` is rounded to bf16, the blend is fp32 and is rounded to bf16 before it enters the MFMA, in the forward's loader
    and in the weight gradient's staging alike; sums are fp32; every stored value is rounded once.  The input gradient is the dgrad
    conv at ``size`` followed by ``bilinear_resize_backward``; a gradient that is not asked for is not computed.  Saved for backward:
    the bf16 ``x`` at its low resolution and ``weight``."""
    if size is None:
        return conv2d(x, weight, bias)
    shape, size, cout, k = _check_resized(x, weight, bias, size)
    if size == shape[2:]:
        return conv2d(x, weight, bias)
    return _ResizedConv2dFunction.apply(x, weight, bias, size)


def _resized_unsupported(kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels, transposed=False):
    """The first argument the resized conv does not run, as a sentence, or None."""
    why = _unsupported(kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels, transposed)
    if why is None and _pair(kernel_size)[0] not in RESIZED_KERNEL_SIZES:
        why = f'kernel_size {kernel_size}: square odd kernels {RESIZED_KERNEL_SIZES} only behind a resize'
    return why


class ResizedConv2d(Conv2d):
    """``Conv2d`` (torch's constructor arguments and parameter names: ``state_dict``s interchange) at the head of a ReadOut block that
    sits behind a bilinear resize: ``forward(x, size)`` is ``resized_conv2d``, ``forward(x)`` the plain ``conv2d``, so the module
    keeps working inside a stock ``Sequential``.  k in {3, 5, 7}; an argument outside the supported family raises
    ``NotImplementedError`` naming it."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=None, dilation=1, groups=1, bias=True,
                 padding_mode='zeros', device=None, dtype=None):
        ks = _pair(kernel_size)
        pad = ks[0] // 2 if padding is None else padding
        why = _resized_unsupported(kernel_size, stride, pad, dilation, groups, padding_mode, in_channels, out_channels)
        if why is not None:
            raise NotImplementedError(why)
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device, dtype)

    def forward(self, x, size=None, fork=False):
        if size is None:
            return super().forward(x, fork)
        if fork:
            raise NotImplementedError('fork True with a size: the resized conv has no second output')
        return resized_conv2d(x, self.weight, self.bias, size)


def _resized_why_not(conv):
    """Why a conv cannot become a ``ResizedConv2d`` (stock, or a ``Conv2d`` of this library), or None."""
    if isinstance(conv, ResizedConv2d):
        return None
    if type(conv) is not Conv2d:
        why = _why_not(conv)
        if why is not None:
            return why
    return _resized_unsupported(conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.padding_mode,
                                conv.in_channels, conv.out_channels, conv.transposed)
