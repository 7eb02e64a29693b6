"""The grouped 3x3 conv of a ResNeXt bottleneck block ("Trainable grouped convolution" of include/cpn_hip.h,
csrc/grouped_conv_train.hip, csrc/grouped_conv.h)

``conv2`` of every block of a ResNeXt encoder: C -> C channels in groups of ``C / groups`` in {4, 8, 16, 32, 64}, 3x3, padding 1,
stride 1 or 2.  It runs as ``C / bw`` block-diagonal dense convs ("bundles") of bw = 32 | 64 channels, the geometry of
``pack._bundle_geometry``: forward and input gradient are ``cpn_conv2d`` on records packed on the device every step, the weight
gradient computes the diagonal 32 x 32 fragments only.  Stride 2 goes through zero-dilation: ``dZ[2i][2j] = dY[i][j]``, then the
stride-1 input and weight gradients of ``dZ`` are those of the strided conv.  Known limit: that does 4 x the minimal work of the
three strided convs of an encoder and holds one more tensor of ``x``'s size.  ``groups = 1`` with ``C`` = 32 or 64 is the
one-bundle edge of the family and runs through ``grouped_conv2d``; ``GroupedConv2d`` and ``convert_grouped_conv2d_`` take
``groups > 1`` only (dense convs are ``Conv2d``'s).

The strided 1x1 shortcut conv of a stage entry lives here as well, because it shares the stride-2 machinery: ``strided_conv1x1`` /
``StridedConv1x1`` scatter their input gradient with ``grouped_dilate`` and take their weight gradient on ``subsample2d(x)``.
"""
import ctypes

import torch

from .. import _lib
from ..ops import _need_cuda
from ._common import _DTYPES, _conv_desc, _grad_dtypes, _nhwc, _pair, _run_conv, _weight_grad, _weight_grad_info
from .conv import _check_weight, conv2d_weight_grad, pack_weight

GROUP_WIDTHS = (4, 8, 16, 32, 64)


def _grouped_channels(in_channels, out_channels, groups):
    """The first channel argument the grouped conv does not run, as a sentence, or None."""
    if groups < 1 or in_channels % groups or out_channels % groups:
        return f'groups {groups}: must divide in_channels {in_channels} and out_channels {out_channels}'
    if in_channels != out_channels:
        return f'out_channels {out_channels}: the grouped conv needs out_channels == in_channels ({in_channels})'
    cig = in_channels // groups
    if cig not in GROUP_WIDTHS:
        return f'groups {groups}: in_channels / groups = {cig}, the grouped conv runs {GROUP_WIDTHS} channels per group only'
    bw = 64 if cig == 64 else 32
    if in_channels < bw or in_channels % bw:
        return f'in_channels {in_channels}: the grouped conv needs a positive multiple of {bw} for {cig} channels per group'
    return None


def _grouped_unsupported(kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels, transposed=False):
    """The first argument ``GroupedConv2d`` does not run, as a sentence, or None."""
    if transposed:
        return 'transposed convs are not run'
    if groups <= 1:
        return f'groups {groups}: grouped convs only (groups > 1)'
    if _pair(kernel_size) != (3, 3):
        return f'kernel_size {kernel_size}: 3x3 only'
    if _pair(stride) not in ((1, 1), (2, 2)):
        return f'stride {stride}: stride 1 or 2 only'
    if _pair(dilation) != (1, 1):
        return f'dilation {dilation}: dilation 1 only'
    if padding != 'same' and (isinstance(padding, str) or _pair(padding) != (1, 1)):
        return f'padding {padding!r}: 1 zero on every side only'
    if padding == 'same' and _pair(stride) != (1, 1):
        return f"padding 'same': stride 1 only"
    if padding_mode != 'zeros':
        return f"padding_mode '{padding_mode}': zeros only"
    return _grouped_channels(in_channels, out_channels, groups)


def _check_grouped(weight, stride, groups):
    """Raises NotImplementedError naming the argument the kernels do not run -> (C, channels per group, stride)."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise NotImplementedError(f'kernel_size / weight {tuple(weight.shape)}: the grouped conv runs [C, C / groups, 3, 3] weights only')
    if weight.dtype not in _DTYPES:
        raise NotImplementedError(f'weight dtype {weight.dtype}: the grouped conv takes float32 or bfloat16 parameters')
    c = int(weight.shape[0])
    cig, stride = _grouped_args(int(weight.shape[1]) * groups if isinstance(groups, int) else 0, c, stride, groups)
    return c, cig, stride


def _grouped_args(in_channels, out_channels, stride, groups):
    """Raises NotImplementedError naming the argument the kernels do not run -> (channels per group, stride)."""
    if not isinstance(groups, int) or groups < 1:
        raise NotImplementedError(f'groups {groups!r}: a positive int')
    if _pair(stride) not in ((1, 1), (2, 2)):
        raise NotImplementedError(f'stride {stride}: the grouped conv runs stride 1 or 2 only')
    why = _grouped_channels(in_channels, out_channels, groups)
    if why is not None:
        raise NotImplementedError(why)
    return in_channels // groups, _pair(stride)[0]


def _grouped_desc(c, cig, stride, bias):
    """cpn_op_desc of the grouped conv as C / bw block-diagonal dense convs of bw -> bw channels (pack._bundle_geometry)."""
    bw = 64 if cig == 64 else 32
    d = _conv_desc(bw, bw, 3, bias)
    d.c0_used, d.cout_real, d.bundles, d.stride = c, c, c // bw, stride
    return d


def grouped_pack_weight(weight, groups, mode='forward'):
    """weight [C, C / groups, 3, 3] (float32 | bfloat16, on the GPU) -> the bf16 records ``cpn_conv2d`` reads for the C / bw
    block-diagonal convs, packed on the device: [bundle, (bw / 32) 9 items (+ one zero item when odd), bw, 32]; ``'dgrad'``: the taps
    flipped and the channel roles swapped inside each group.  Entries across two groups of a bundle are exact zeros."""
    _need_cuda(weight)
    c, cig, _ = _check_grouped(weight, 1, groups)
    w = weight.detach().contiguous()
    bw = 64 if cig == 64 else 32
    items = bw // 32 * 9
    packed = torch.empty((c // bw, items + items % 2, bw, 32), dtype=torch.bfloat16, device=w.device)
    _lib.check(_lib.load().cpn_grouped_conv_pack(_lib.ptr(w), _DTYPES[w.dtype], c, cig, _lib.CONV_PACK_MODES[mode], _lib.ptr(packed),
                                                 _lib.stream_ptr()), 'grouped_conv_pack')
    return packed


def _run_grouped(src, packed, bias, c, cig, stride):
    """cpn_conv2d on a bf16 tensor whose memory is NHWC -> bf16 [N, C, Hout, Wout] in channels_last."""
    n, _, h, w = src.shape
    out = torch.empty((n, c, (h - 1) // stride + 1, (w - 1) // stride + 1), dtype=torch.bfloat16, device=src.device,
                      memory_format=torch.channels_last)
    if out.numel() == 0:
        return out
    d = _grouped_desc(c, cig, stride, bias is not None)
    _lib.check(_lib.load().cpn_conv2d(ctypes.byref(d), _lib.ptr(src), c, _lib.ptr(None), 0, _lib.ptr(None), 0, _lib.ptr(out), c,
                                      n, h, w, _lib.ptr(packed), _lib.ptr(bias), _lib.stream_ptr()), 'grouped_conv2d')
    return out


def grouped_dilate(grad_output, size):
    """The stride-2 gradient at the input's size: grad_output [N, C, Hout, Wout] -> bf16 dZ [N, C, H, W] in ``torch.channels_last``
    with ``dZ[..., 2i, 2j] = grad_output[..., i, j]`` and exact zeros elsewhere; ``size`` = (H, W) with Hout = (H - 1) // 2 + 1."""
    _need_cuda(grad_output)
    h, w = (int(v) for v in size)
    n, c, ho, wo = (int(v) for v in grad_output.shape)
    if c < 32 or c % 32:
        raise NotImplementedError(f'grad_output of {c} channels: the grouped conv needs a positive multiple of 32')
    if h < 1 or w < 1 or (ho, wo) != ((h - 1) // 2 + 1, (w - 1) // 2 + 1):
        raise ValueError(f'grad_output {ho} x {wo} is not the stride-2 output of a {h} x {w} input')
    gs = _nhwc(grad_output, torch.bfloat16)
    dz = torch.empty((n, c, h, w), dtype=torch.bfloat16, device=gs.device, memory_format=torch.channels_last)
    if dz.numel():
        _lib.check(_lib.load().cpn_grouped_conv_dilate(_lib.ptr(gs), n, h, w, c, _lib.ptr(dz), _lib.stream_ptr()), 'grouped_conv_dilate')
    return dz


def grouped_weight_grad_info(n, h, w, channels, groups, stride=1, slab_rows=0):
    """What ``grouped_conv2d_weight_grad`` would run on ``n`` inputs of ``h`` x ``w`` -> dict(slabs, slab_rows, steps (MFMA steps per
    slab), reduce_chain, bias_chain).  Host arithmetic only: needs no GPU.  Raises like the launch for a call it rejects."""
    cig = channels // groups if groups > 0 and channels % groups == 0 else 0
    return _weight_grad_info('grouped_conv', n, h, w, channels, cig, stride, slab_rows)


def grouped_conv2d_weight_grad(x, grad_output, groups, stride=1, slab_rows=0, weight=True, bias=True, dtype=torch.float32,
                               bias_dtype=None, dilated=None):
    """(x [N, C, H, W], grad_output [N, C, Hout, Wout]) -> (dW [C, C / groups, 3, 3] | None, db [C] | None): the gradients
    ``grouped_conv2d`` returns for its weight and bias, as fp32 sums over the bf16-rounded operands rounded once to ``dtype`` /
    ``bias_dtype``.  ``slab_rows``: image rows per slab of the reduction (0: chosen by the library); ``dilated``: stride 2, the
    result of ``grouped_dilate(grad_output, (H, W))`` when the caller has it already.  An empty input: zeros."""
    _need_cuda(x, grad_output)
    n, c, h, w = (int(v) for v in x.shape)
    dtypes = _grad_dtypes(dtype, bias_dtype)
    cig, stride = _grouped_args(c, int(grad_output.shape[1]), stride, groups)
    want = (n, c, (h - 1) // stride + 1, (w - 1) // stride + 1)
    assert tuple(grad_output.shape) == want, (tuple(grad_output.shape), want)

    def operands():  # (x, the gradient at the input's size -- stride 2: dilated first --, the gradient itself for the bias)
        xs, gs = _nhwc(x, torch.bfloat16), _nhwc(grad_output, torch.bfloat16)
        dz = gs
        if stride == 2 and weight:
            dz = grouped_dilate(gs, (h, w)) if dilated is None else dilated
        return xs, dz, gs

    return _weight_grad('grouped_conv', (n, h, w, c, cig, stride, slab_rows), operands, (c, cig, 3, 3), x.device, weight, bias, dtypes,
                        torch.zeros, no_pixels=n * h * w == 0)


class _GroupedConv2dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, groups):
        c, cig = int(weight.shape[0]), int(weight.shape[1])
        xs = _nhwc(x, torch.bfloat16)
        b32 = None if bias is None else bias.detach().float().contiguous()
        out = _run_grouped(xs, grouped_pack_weight(weight, groups, 'forward'), b32, c, cig, stride)
        ctx.save_for_backward(xs, weight)
        ctx.x_dtype, ctx.stride, ctx.groups = x.dtype, stride, groups
        ctx.bias_dtype = None if bias is None else bias.dtype
        return out

    @staticmethod
    def backward(ctx, grad_output):
        xs, weight = ctx.saved_tensors
        c, cig = int(weight.shape[0]), int(weight.shape[1])
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and ctx.bias_dtype is not None
        gs = _nhwc(grad_output, torch.bfloat16)
        dz = gs  # the gradient at the input's size: stride 2 by zero-dilation, shared by the input and the weight gradient
        if ctx.stride == 2 and (need_x or need_w):
            dz = grouped_dilate(gs, xs.shape[2:])
        dx = dw = db = None
        if need_x:  # the stride-1 conv of dz with the flipped, channel-swapped weights
            dx = _run_grouped(dz, grouped_pack_weight(weight, ctx.groups, 'dgrad'), None, c, cig, 1).to(ctx.x_dtype)
        if need_w or need_b:
            dw, db = grouped_conv2d_weight_grad(xs, gs, ctx.groups, ctx.stride, weight=need_w, bias=need_b, dtype=weight.dtype,
                                                bias_dtype=ctx.bias_dtype or weight.dtype, dilated=dz)
        return dx, dw, db, None, None


def grouped_conv2d(x, weight, bias=None, stride=1, groups=1):
    """``torch.nn.functional.conv2d(x, weight, bias, stride, padding=1, groups=groups)`` for a 3x3 ``weight`` ``[C, C / groups, 3, 3]``
    of the supported family (module docstring), with gradients for ``x``, ``weight`` and ``bias`` as autograd asks for them -> bf16
    ``[N, C, (H - 1) // stride + 1, (W - 1) // stride + 1]`` in ``torch.channels_last``.  Anything unsupported raises
    ``NotImplementedError`` naming the argument; there is no fallback."""
    if x.dim() != 4:
        raise NotImplementedError(f'input of {x.dim()} dimensions: the grouped conv takes a 4-D [N, C, H, W] input')
    c, cig, stride = _check_grouped(weight, stride, groups)
    if x.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {x.dtype}: the grouped conv takes float32 or bfloat16 activations')
    if int(x.shape[1]) != c:
        raise ValueError(f'input has {int(x.shape[1])} channels, weight expects {c}')
    if bias is not None and (bias.dim() != 1 or int(bias.shape[0]) != c or bias.dtype not in _DTYPES):
        raise NotImplementedError(f'bias {tuple(bias.shape)} {bias.dtype}: the grouped conv takes a float32 or bfloat16 [{c}] bias')
    _need_cuda(x, weight, bias)
    return _GroupedConv2dFunction.apply(x, weight, bias, stride, groups)


class GroupedConv2d(torch.nn.Conv2d):
    """``torch.nn.Conv2d`` with torch's constructor arguments and parameter names (``weight``, ``bias``: ``state_dict``s
    interchange) whose forward is ``grouped_conv2d``.  ``kernel_size`` is 3 and ``padding`` defaults to 1; an argument outside the
    supported family raises ``NotImplementedError`` naming it."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=32, bias=True,
                 padding_mode='zeros', device=None, dtype=None):
        why = _grouped_unsupported(kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels)
        if why is not None:
            raise NotImplementedError(why)
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device, dtype)

    def forward(self, x):
        return grouped_conv2d(x, self.weight, self.bias, self.stride, self.groups)


def _grouped_why_not(conv):
    if type(conv) is not torch.nn.Conv2d:
        return f'a subclass of torch.nn.Conv2d ({type(conv).__name__}): its forward may differ'
    if conv.weight.dtype not in _DTYPES:
        return f'weight dtype {conv.weight.dtype}: float32 or bfloat16 only'
    return _grouped_unsupported(conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.padding_mode,
                                conv.in_channels, conv.out_channels, conv.transposed)


def subsample2d(x, stride=2):
    """x [N, C, H, W] -> bf16 ``x[..., ::2, ::2]`` in ``torch.channels_last`` by one 16-byte-per-lane gather (``C`` a positive
    multiple of 8): the operand of the strided shortcut's weight gradient."""
    if x.dim() != 4:
        raise NotImplementedError(f'input of {x.dim()} dimensions: the subsample takes a 4-D [N, C, H, W] input')
    n, c, h, w = (int(v) for v in x.shape)
    if c < 8 or c % 8:
        raise NotImplementedError(f'input of {c} channels: the subsample needs a positive multiple of 8')
    if stride != 2:
        raise NotImplementedError(f'stride {stride}: the subsample runs stride 2 only')
    _need_cuda(x)
    xs = _nhwc(x, torch.bfloat16)
    out = torch.empty((n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=torch.bfloat16, device=xs.device, memory_format=torch.channels_last)
    if out.numel():
        _lib.check(_lib.load().cpn_subsample2d(_lib.ptr(xs), n, h, w, c, 2, _lib.ptr(out), _lib.stream_ptr()), 'subsample2d')
    return out


def _check_strided(weight, stride):
    """Raises NotImplementedError naming the argument the strided shortcut does not run."""
    _check_weight(weight)
    if int(weight.shape[2]) != 1:
        raise NotImplementedError(f'kernel_size {int(weight.shape[2])}: the strided shortcut conv is 1x1')
    if _pair(stride) != (2, 2):
        raise NotImplementedError(f'stride {stride}: the strided shortcut conv runs stride 2 only')


class _StridedConv1x1Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        cout, cin = int(weight.shape[0]), int(weight.shape[1])
        xs = _nhwc(x, torch.bfloat16)
        b32 = None if bias is None else bias.detach().float().contiguous()
        out = _run_conv(xs, pack_weight(weight, 'forward'), b32, cin, cout, 1, stride=2)  # the pointwise tile gathers its outputs
        ctx.save_for_backward(xs, weight)
        ctx.x_dtype = x.dtype
        ctx.bias_dtype = None if bias is None else bias.dtype
        return out

    @staticmethod
    def backward(ctx, grad_output):
        xs, weight = ctx.saved_tensors
        cout, cin = int(weight.shape[0]), int(weight.shape[1])
        need_x, need_w, need_b = ctx.needs_input_grad
        need_b = need_b and ctx.bias_dtype is not None
        gs = _nhwc(grad_output, torch.bfloat16)
        dx = dw = db = None
        if need_x:  # the stride-1 dgrad conv at the small size, then the scatter onto the even grid of the input's size
            small = _run_conv(gs, pack_weight(weight, 'dgrad'), None, cout, cin, 1)
            dx = grouped_dilate(small, xs.shape[2:]).to(ctx.x_dtype)
        if need_w or need_b:  # dW(x, dy) = dW_dense(x[::2, ::2], dy); the gather runs only when dW is asked for
            sub = subsample2d(xs) if need_w else torch.empty((xs.shape[0], cin) + tuple(gs.shape[2:]), dtype=torch.bfloat16,
                                                             device=xs.device, memory_format=torch.channels_last)
            dw, db = conv2d_weight_grad(sub, gs, 1, weight=need_w, bias=need_b, dtype=weight.dtype,
                                        bias_dtype=ctx.bias_dtype or weight.dtype)
        return dx, dw, db


def strided_conv1x1(x, weight, bias=None, stride=2):
    """``torch.nn.functional.conv2d(x, weight, bias, stride=2)`` for a 1x1 ``weight`` ``[Cout, Cin, 1, 1]``, ``Cin`` and ``Cout``
    multiples of 32: the shortcut conv at a stage entry of the encoder, with gradients for ``x``, ``weight`` and ``bias`` as autograd
    asks for them -> bf16 ``[N, Cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1]`` in ``torch.channels_last``.  Arithmetic and layout are
    ``conv2d``'s.  The forward reads ``x`` itself (no gathered copy); the input gradient is the 1x1 dgrad conv of ``grad_output`` at
    the small size scattered onto the even grid (exact zeros elsewhere); the weight gradient is ``conv2d_weight_grad`` on
    ``subsample2d(x)``.  Anything else raises ``NotImplementedError`` naming the argument; there is no fallback."""
    if x.dim() != 4:
        raise NotImplementedError(f'input of {x.dim()} dimensions: the strided shortcut conv takes a 4-D [N, C, H, W] input')
    _check_strided(weight, stride)
    if x.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {x.dtype}: the strided shortcut conv takes float32 or bfloat16 activations')
    if int(x.shape[1]) != int(weight.shape[1]):
        raise ValueError(f'input has {int(x.shape[1])} channels, weight expects {int(weight.shape[1])}')
    if bias is not None and (bias.dim() != 1 or bias.shape[0] != weight.shape[0] or bias.dtype not in _DTYPES):
        raise NotImplementedError(f'bias {tuple(bias.shape)} {bias.dtype}: the strided shortcut conv takes a float32 or bfloat16 '
                                  f'[Cout] bias')
    _need_cuda(x, weight, bias)
    if x.shape[0] * x.shape[2] * x.shape[3] == 0:
        raise NotImplementedError(f'input of shape {tuple(x.shape)}: the strided shortcut conv needs at least one pixel')
    return _StridedConv1x1Function.apply(x, weight, bias)


def _strided_unsupported(kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels, transposed=False):
    """The first argument ``StridedConv1x1`` does not run, as a sentence, or None."""
    if transposed:
        return 'transposed convs are not run'
    if _pair(kernel_size) != (1, 1):
        return f'kernel_size {kernel_size}: 1x1 only'
    if _pair(stride) != (2, 2):
        return f'stride {stride}: stride 2 only'
    if groups != 1:
        return f'groups {groups}: dense convs only'
    if _pair(dilation) != (1, 1):
        return f'dilation {dilation}: dilation 1 only'
    if padding != 'valid' and (isinstance(padding, str) or _pair(padding) != (0, 0)):
        return f'padding {padding!r}: no padding only'
    if padding_mode != 'zeros':
        return f"padding_mode '{padding_mode}': zeros only"
    if in_channels < 32 or in_channels % 32:
        return f'in_channels {in_channels}: multiples of 32 only'
    if out_channels < 32 or out_channels % 32:
        return f'out_channels {out_channels}: multiples of 32 only'
    return None


class StridedConv1x1(torch.nn.Conv2d):
    """``torch.nn.Conv2d(cin, cout, 1, stride=2)`` with torch's constructor arguments and parameter names (``weight``, ``bias``:
    ``state_dict``s interchange) whose forward is ``strided_conv1x1``.  An argument outside the supported family raises
    ``NotImplementedError`` naming it."""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=2, padding=0, dilation=1, groups=1, bias=True,
                 padding_mode='zeros', device=None, dtype=None):
        why = _strided_unsupported(kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels)
        if why is not None:
            raise NotImplementedError(why)
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device, dtype)

    def forward(self, x):
        return strided_conv1x1(x, self.weight, self.bias)


def _strided_why_not(conv):
    if type(conv) is not torch.nn.Conv2d:
        return f'a subclass of torch.nn.Conv2d ({type(conv).__name__}): its forward may differ'
    if conv.weight.dtype not in _DTYPES:
        return f'weight dtype {conv.weight.dtype}: float32 or bfloat16 only'
    return _strided_unsupported(conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.padding_mode,
                                conv.in_channels, conv.out_channels, conv.transposed)
