"""The first conv of a U-Net decoder level: nearest resize + concat + conv ("Trainable concat convolution" of
include/cpn_hip.h, csrc/cat_conv_train.hip, csrc/nearest_adjoint.h)

Every level of the reference decoder runs its block on ``cat((lateral, interpolate(top, size=lateral.shape[2:])), 1)``.  Stock torch
writes the resized and the concatenated tensor and saves the latter; ``cat_conv2d`` reads both sources in the conv's loader and in
the weight gradient's staging, and saves the lateral and the low-resolution top only.  The input gradient is two dgrad convs
(one per source, each run only when asked for); the top's goes through the adjoint of the resize, ``nearest_resize_backward``.
``UNetDecoder`` also applies the level's 1x1 ``inner`` conv BEFORE the resize (per pixel the same bits, at the low resolution).
Known limits: the top's gradient at the lateral's size (``T``) is written and read once, before it is summed (no footprint sum in
the dgrad epilogue, no 4x4 stride-2 adjoint for the exact x2); the forward is not decomposed into sub-pixel phases.
"""
import ctypes

import torch

from .. import _lib
from ..ops import _need_cuda
from ._common import _DTYPES, _conv_desc, _grad_dtypes, _nhwc, _pair, _run_conv, _weight_grad, _weight_grad_info
from .conv import _unsupported, conv2d, pack_weight

CAT_KERNEL_SIZES = (1, 3, 5, 7)


def _cat_channels(c0, c1, cout, k):
    """Raises NotImplementedError naming the argument the concat conv does not run (``c0`` None: the bridge level)."""
    if k not in CAT_KERNEL_SIZES:
        raise NotImplementedError(f'kernel_size {k}: the concat conv runs square odd kernels {CAT_KERNEL_SIZES} only')
    if c0 is not None and (c0 < 32 or c0 % 32):
        raise NotImplementedError(f'lateral of {c0} channels: the concat conv needs a positive multiple of 32')
    if c1 < 32 or c1 % 32:
        raise NotImplementedError(f'top of {c1} channels: the concat conv needs a positive multiple of 32')
    if cout < 32 or cout % 32:
        raise NotImplementedError(f'out_channels {cout}: the concat conv needs a positive multiple of 32')


def _check_cat(lateral, top, weight, bias):
    """Raises for a call ``cat_conv2d`` does not run -> (N, C0 (0: bridge), C1, Cout, k, H, W, h, w)."""
    if not isinstance(top, torch.Tensor) or top.dim() != 4:
        raise NotImplementedError(f'top of {getattr(top, "dim", lambda: None)()} dimensions: the concat conv takes a 4-D [N, C1, h, w] top')
    if lateral is not None and (not isinstance(lateral, torch.Tensor) or lateral.dim() != 4):
        raise NotImplementedError(f'lateral of {getattr(lateral, "dim", lambda: None)()} dimensions: the concat conv takes a 4-D '
                                  f'[N, C0, H, W] lateral or None')
    if weight.dim() != 4:
        raise NotImplementedError(f'weight of {weight.dim()} dimensions: the concat conv needs [Cout, C0 + C1, k, k]')
    if weight.shape[2] != weight.shape[3]:
        raise NotImplementedError(f'kernel_size {tuple(weight.shape[2:])}: the concat conv runs square kernels only')
    if weight.dtype not in _DTYPES:
        raise NotImplementedError(f'weight dtype {weight.dtype}: the concat conv takes float32 or bfloat16 parameters')
    for name, t in (('top', top), ('lateral', lateral)):
        if t is not None and t.dtype not in _DTYPES:
            raise NotImplementedError(f'{name} dtype {t.dtype}: the concat conv takes float32 or bfloat16 activations')
    n, c1, h, w = (int(v) for v in top.shape)
    cout, cin, k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
    c0 = None if lateral is None else int(lateral.shape[1])
    _cat_channels(c0, c1, cout, k)
    if (c0 or 0) + c1 != cin:
        raise ValueError(f'lateral and top have {c0 or 0} + {c1} channels, weight expects {cin}')
    if lateral is None:
        H, W = 2 * h, 2 * w
    else:
        H, W = int(lateral.shape[2]), int(lateral.shape[3])
        if int(lateral.shape[0]) != n:
            raise ValueError(f'lateral holds {int(lateral.shape[0])} images, top {n}')
        if h > H or w > W:
            raise NotImplementedError(f'top of {h} x {w} pixels is larger than the lateral of {H} x {W}: the concat conv resizes upwards '
                                      f'only')
    if n * h * w == 0 or n * H * W == 0:
        raise NotImplementedError(f'top of shape {tuple(top.shape)}' + (f', lateral of shape {tuple(lateral.shape)}' if lateral is not None
                                                                          else '') + ': the concat conv needs at least one pixel')
    if bias is not None and (bias.dim() != 1 or int(bias.shape[0]) != cout or bias.dtype not in _DTYPES):
        raise NotImplementedError(f'bias {tuple(bias.shape)} {bias.dtype}: the concat conv takes a float32 or bfloat16 [{cout}] bias')
    _need_cuda(lateral, top, weight, bias)
    return n, c0 or 0, c1, cout, k, H, W, h, w


def _cat_desc(c0, c1, cout, k, bias):
    """cpn_op_desc of the concat conv: the lateral plain, the top resized by the loader; without a lateral the lone source resized."""
    d = _conv_desc(c0 + c1, cout, k, bias)
    if c0:
        d.src1, d.up1, d.c0_used = 2, 1, c0
    else:
        d.up0 = 1
    return d


def _run_cat_conv(ls, ts, packed, bias, c0, c1, cout, k, size):
    """ls: bf16 NHWC memory [N, C0, H, W] or None, ts: [N, C1, h, w] -> bf16 [N, cout, H, W] in channels_last: ``cpn_conv2d_sized``
    on the two sources (``cpn_conv2d`` on the lone resized source of the bridge level)."""
    n, _, h, w = (int(v) for v in ts.shape)
    H, W = size
    out = torch.empty((n, cout, H, W), dtype=torch.bfloat16, device=ts.device, memory_format=torch.channels_last)
    d = _cat_desc(c0, c1, cout, k, bias is not None)
    lib = _lib.load()
    if ls is None:
        assert (H, W) == (2 * h, 2 * w), (H, W, h, w)
        _lib.check(lib.cpn_conv2d(ctypes.byref(d), _lib.ptr(ts), c1, _lib.ptr(None), 0, _lib.ptr(None), 0, _lib.ptr(out), cout, n, H, W,
                                  _lib.ptr(packed), _lib.ptr(bias), _lib.stream_ptr()), 'cat_conv2d')
    else:
        stored = (ctypes.c_int32 * 6)(H, W, h, w, H, W)
        _lib.check(lib.cpn_conv2d_sized(ctypes.byref(d), _lib.ptr(ls), c0, _lib.ptr(ts), c1, _lib.ptr(None), 0, _lib.ptr(out), cout, n,
                                        H, W, stored, _lib.ptr(packed), _lib.ptr(bias), _lib.stream_ptr()), 'cat_conv2d')
    return out


def cat_weight_grad_info(n, h, w, c0, c1, top_size, cout, k, slab_rows=0):
    """What ``cat_conv2d_weight_grad`` would run on ``n`` laterals of ``h`` x ``w`` (``c0`` = 0: the bridge level) and tops of
    ``top_size`` -> dict(slabs, slab_rows, steps (MFMA steps per slab), reduce_chain, bias_chain).  Host arithmetic only: needs no GPU.
    Raises like the launch for a call it rejects."""
    return _weight_grad_info('cat_conv', n, h, w, c0, c1, int(top_size[0]), int(top_size[1]), cout, k, slab_rows)


def cat_conv2d_weight_grad(lateral, top, grad_output, kernel_size, slab_rows=0, weight=True, bias=True, dtype=torch.float32,
                           bias_dtype=None):
    """(lateral [N, C0, H, W] | None, top [N, C1, h, w], grad_output [N, Cout, H, W]) -> (dW [Cout, C0 + C1, k, k] | None, db [Cout] |
    None): the gradients ``cat_conv2d`` returns for its weight and bias, as fp32 sums over the bf16-rounded operands of the virtual
    concat rounded once to ``dtype`` / ``bias_dtype``.  ``slab_rows``: image rows per slab of the reduction (0: chosen by the library)."""
    _need_cuda(lateral, top, grad_output)
    k = int(kernel_size)
    n, c1, h1, w1 = (int(v) for v in top.shape)
    c0 = 0 if lateral is None else int(lateral.shape[1])
    cout, h, w = int(grad_output.shape[1]), int(grad_output.shape[2]), int(grad_output.shape[3])
    _cat_channels(None if lateral is None else c0, c1, cout, k)
    dtypes = _grad_dtypes(dtype, bias_dtype)
    assert int(grad_output.shape[0]) == n and (lateral is None or tuple(lateral.shape) == (n, c0, h, w)) and \
        (lateral is not None or (h, w) == (2 * h1, 2 * w1)), (tuple(grad_output.shape), tuple(top.shape))
    return _weight_grad('cat_conv', (n, h, w, c0, c1, h1, w1, cout, k, slab_rows),
                        lambda: (None if lateral is None else _nhwc(lateral, torch.bfloat16), _nhwc(top, torch.bfloat16),
                                 _nhwc(grad_output, torch.bfloat16)),
                        (cout, c0 + c1, k, k), top.device, weight, bias, dtypes, torch.empty)


def nearest_resize_backward(t, size):
    """The adjoint of ``F.interpolate(x, size=t.shape[2:], mode='nearest')`` for ``x`` of ``size`` = (h, w): t [N, C, H, W] -> bf16
    [N, C, h, w] in ``torch.channels_last``, every pixel the sum of ``t`` over the pixels that read it (fp32 adds in ascending
    row-major order, one rounding; exact zeros where none does).  ``t`` is rounded to bf16 on the way in; ``C`` a positive multiple
    of 8, 1 <= h <= H, 1 <= w <= W.  Known limit: one lane walks a pixel's whole footprint, which suits the 2 x 2 footprints of a
    decoder; any ratio is correct, but a tiny ``size`` under a large ``t`` leaves a few lanes reading the whole image."""
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise NotImplementedError(f'input of {getattr(t, "dim", lambda: None)()} dimensions: the resize adjoint takes a 4-D [N, C, H, W] input')
    if t.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {t.dtype}: the resize adjoint takes float32 or bfloat16 activations')
    n, c, H, W = (int(v) for v in t.shape)
    h, w = (int(v) for v in size)
    if c < 8 or c % 8:
        raise NotImplementedError(f'input of {c} channels: the resize adjoint needs a positive multiple of 8')
    if h < 1 or w < 1 or h > H or w > W or n < 1:
        raise NotImplementedError(f'size {(h, w)} for an input of shape {tuple(t.shape)}: the resize adjoint needs 1 <= h <= H and '
                                  f'1 <= w <= W and at least one image')
    _need_cuda(t)
    ts = _nhwc(t, torch.bfloat16)
    out = torch.empty((n, c, h, w), dtype=torch.bfloat16, device=ts.device, memory_format=torch.channels_last)
    _lib.check(_lib.load().cpn_nearest_sum(_lib.ptr(ts), n, H, W, c, _lib.ptr(out), h, w, _lib.stream_ptr()), 'nearest_sum')
    return out


class _CatConv2dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lateral, top, weight, bias):
        cout, k = int(weight.shape[0]), int(weight.shape[2])
        c1 = int(top.shape[1])
        c0 = int(weight.shape[1]) - c1
        ls = None if lateral is None else _nhwc(lateral, torch.bfloat16)
        ts = _nhwc(top, torch.bfloat16)
        size = (2 * int(top.shape[2]), 2 * int(top.shape[3])) if lateral is None else (int(lateral.shape[2]), int(lateral.shape[3]))
        b32 = None if bias is None else bias.detach().float().contiguous()
        out = _run_cat_conv(ls, ts, pack_weight(weight, 'forward'), b32, c0, c1, cout, k, size)
        ctx.save_for_backward(ls, ts, weight)  # the lateral and the top at its own low resolution: nothing of the concat's size
        ctx.lateral_dtype = None if lateral is None else lateral.dtype
        ctx.top_dtype = top.dtype
        ctx.bias_dtype = None if bias is None else bias.dtype
        return out

    @staticmethod
    def backward(ctx, grad_output):
        ls, ts, weight = ctx.saved_tensors
        cout, k = int(weight.shape[0]), int(weight.shape[2])
        c1 = int(ts.shape[1])
        c0 = int(weight.shape[1]) - c1
        need_l, need_t, need_w, need_b = ctx.needs_input_grad
        need_l = need_l and ls is not None
        need_b = need_b and ctx.bias_dtype is not None
        gs = _nhwc(grad_output, torch.bfloat16)
        dl = dt = dw = db = None
        if need_l:  # dcat[:, :C0]: the dgrad conv on the lateral's part of the weights, written directly
            dl = _run_conv(gs, pack_weight(weight.detach()[:, :c0], 'dgrad'), None, cout, c0, k).to(ctx.lateral_dtype)
        if need_t:  # T = dcat[:, C0:] at the lateral's size, then the footprint sums (the identity resize: T itself)
            t = _run_conv(gs, pack_weight(weight.detach()[:, c0:], 'dgrad'), None, cout, c1, k)
            dt = (t if t.shape[2:] == ts.shape[2:] else nearest_resize_backward(t, ts.shape[2:])).to(ctx.top_dtype)
        if need_w or need_b:
            dw, db = cat_conv2d_weight_grad(ls, ts, gs, k, weight=need_w, bias=need_b, dtype=weight.dtype,
                                            bias_dtype=ctx.bias_dtype or weight.dtype)
        return dl, dt, dw, db


def cat_conv2d(lateral, top, weight, bias=None):
    """``F.conv2d(torch.cat((lateral, F.interpolate(top, size=lateral.shape[2:], mode='nearest')), 1), weight, bias, padding=k // 2)``
    -- the lateral first -- as one autograd function that never writes the resized or the concatenated tensor, with gradients for
    ``lateral``, ``top``, ``weight`` and ``bias`` as autograd asks for them -> bf16 ``[N, Cout, H, W]`` in ``torch.channels_last``.

    ``lateral`` ``[N, C0, H, W]``, ``top`` ``[N, C1, h, w]`` with 1 <= h <= H and 1 <= w <= W at any ratio (equal sizes: no resize),
    ``weight`` ``[Cout, C0 + C1, k, k]``; ``lateral=None`` is the bridge level: the only source is ``top`` resized by exactly 2
    (``scale_factor=2``) -> ``[N, Cout, 2h, 2w]``.  The family is ``conv2d``'s: ``C0``, ``C1`` and ``Cout`` positive multiples of 32,
    a square odd ``k`` in {1, 3, 5, 7}, stride 1, zero padding ``k // 2``, float32 or bfloat16 inputs and parameters on the GPU.
    Anything else raises ``NotImplementedError`` naming the argument; there is no fallback.

    Arithmetic is ``conv2d``'s.  The lateral's gradient is written by its own dgrad conv; the top's is the dgrad conv at the lateral's
    size followed by ``nearest_resize_backward``, whose index map is the forward loader's own, so the two are exact adjoints at every
    size; a conv whose gradient is not asked for is not run.  Saved for backward: the bf16 lateral, the bf16 top at its low
    resolution and ``weight``."""
    _check_cat(lateral, top, weight, bias)
    return _CatConv2dFunction.apply(lateral, top, weight, bias)


_ONE_INPUT = object()  # CatConv2d.forward(x): the concatenated tensor itself


class CatConv2d(torch.nn.Conv2d):
    """``torch.nn.Conv2d`` with torch's constructor arguments and parameter names (``in_channels`` = C0 + C1; ``state_dict``s
    interchange) at the head of a decoder level: ``forward(lateral, top)`` is ``cat_conv2d``, ``forward(None, top)`` the bridge level,
    and ``forward(x)`` with the one concatenated tensor is ``conv2d(x)``, so the module keeps working inside a stock ``Sequential``.
    ``padding`` defaults to ``kernel_size // 2``; an argument outside the supported family raises ``NotImplementedError`` naming it."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=None, dilation=1, groups=1, bias=True,
                 padding_mode='zeros', device=None, dtype=None):
        ks = _pair(kernel_size)
        padding = ks[0] // 2 if padding is None else padding
        why = _unsupported(kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels)
        if why is not None:
            raise NotImplementedError(why)
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device, dtype)

    def forward(self, lateral, top=_ONE_INPUT):
        if top is _ONE_INPUT:
            return conv2d(lateral, self.weight, self.bias)
        return cat_conv2d(lateral, top, self.weight, self.bias)
