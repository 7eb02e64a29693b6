"""Trainable convolution on the MI355X: ``conv2d`` (one ``torch.autograd.Function``), the ``nn.Conv2d`` drop-in ``Conv2d`` and
``convert_conv2d_``, which replaces the eligible convs of a torch module in place.

A training step of the reference model under PyTorch-ROCm spends >= 99.9 % of its FLOPs in convolutions; the four 7x7 ReadOut
convs and the UNet decoder convs (93 % of them) are dense stride-1 convs whose channel counts are multiples of 32.  For that family
forward, input gradient and weight gradient run in this library's HIP kernels (the rule is the "Trainable convolution" section of
include/cpn_hip.h):

* forward: ``cpn_conv2d`` (csrc/conv_igemm.hip) on weights packed on the device every step;
* input gradient: for stride 1 and ``padding = k // 2`` again such a conv, of ``grad_output``, with the taps flipped and the channel
  roles swapped -- the same kernel on the dgrad pack;
* weight gradient: the bf16 MFMA kernel of csrc/conv_train.hip, which reduces over pixels in slabs and adds the slabs' fp32 partial
  sums in a fixed order (no floating-point atomics: bit-identical from run to run); the bias gradient comes from a small kernel
  of its own.

Supported: ``groups = 1``, ``stride = 1``, ``dilation = 1``, a square odd ``k`` in {1, 3, 5, 7}, ``padding = k // 2`` with zeros,
``Cin`` and ``Cout`` multiples of 32, a 4-D input on the GPU.  Everything else raises ``NotImplementedError`` naming the argument;
there is no CPU fallback.  ``convert_conv2d_`` leaves every other conv and says why: the grouped 3x3 convs of the encoder are the
business of ``grouped_conv2d``, the final 1x1 convs of the heads (1 / 2 / 20 output channels) of ``dropout_conv1x1``, both below.
The stem (a 7x7 stride-2 conv from at most 4 channels) is ``stem_conv2d``'s, at the end of this module.

Arithmetic: activations and weights are rounded to bf16 (round to nearest even), products accumulate in fp32, the forward output
and the input gradient are stored as bf16, the weight and bias gradients are fp32 sums rounded once to the parameter's dtype.  ``x``
may be bf16 or fp32 (rounded to bf16 on the way in, as autocast would); the output is bf16 in ``torch.channels_last``.  A
channels-last ``[N, C, H, W]`` tensor is NHWC in memory, the layout of ``cpn_conv2d``: no layout copy is made for such inputs, any
other layout is made channels-last first.

The ``BatchNorm2d`` and ``ReLU`` behind those convs run here as well: ``batch_norm`` (one ``torch.autograd.Function`` with an
optional fused ReLU), the ``nn.BatchNorm2d`` drop-in ``BatchNorm2d`` and ``convert_batchnorm2d_`` (second half of this module; the
rule is the "Trainable batch normalisation" section of include/cpn_hip.h).

The tail of a ReadOut head, ``Dropout2d -> Conv 1x1`` to 1 / 2 / 20 channels, runs here too: ``dropout_conv1x1`` (one
``torch.autograd.Function``: three passes over the head's largest activation instead of stock's seven, and only ``x`` saved), the
``nn.Conv2d`` drop-in ``DropoutConv1x1`` and ``convert_readout_tail_`` (third part of this module; the rule is the "Trainable
ReadOut tail" section of include/cpn_hip.h).  After the three converts a ReadOut head runs conv -> norm -> ReLU -> dropout -> 1x1
without leaving the library; the bilinear resize behind the heads stays stock.

The grouped 3x3 ``conv2`` of the ResNeXt encoder's bottleneck blocks, at stride 1 and 2, runs here as well: ``grouped_conv2d`` (one
``torch.autograd.Function``), the ``nn.Conv2d`` drop-in ``GroupedConv2d`` and ``convert_grouped_conv2d_`` (fourth part of this
module; the rule is the "Trainable grouped convolution" section of include/cpn_hip.h).  The 1x1 ``conv1`` / ``conv3`` around it are
dense stride-1 convs that ``convert_conv2d_`` takes.

The whole bottleneck block runs here: ``Bottleneck`` and ``convert_bottleneck_`` (last part of this module; the rule is the
"Trainable bottleneck block" section of include/cpn_hip.h) put the convs and norms above together with the norm's residual tail
(``batch_norm(..., residual=)``: ``relu(bn3(h) + identity)`` in one pass), the strided 1x1 shortcut of a stage entry
(``strided_conv1x1``) and the block-input gradient in the epilogue of ``conv1``'s input-gradient conv (``conv2d_fork``).  Known limit:
at a stage entry the shortcut's norm and the tail are two kernels (``relu(bn3(h) + bn_d(h_d))`` is not one pass).

The decoder's nearest resize + concat run here too: ``cat_conv2d`` (one ``torch.autograd.Function``: the conv reads the lateral and
the low-resolution top through the loader's own nearest map, the weight gradient gathers the same way, the top's gradient goes
through the exact adjoint of the resize, ``nearest_resize_backward``; neither the resized nor the concatenated tensor is written or
saved), the ``nn.Conv2d`` drop-in ``CatConv2d``, the decoder ``UNetDecoder``, which also runs the level's 1x1 ``inner`` conv before
the resize instead of after it, and ``convert_unet_decoder_`` (the part after the bottleneck; the rule is the "Trainable concat
convolution" section of include/cpn_hip.h).  After it a decoder level runs conv -> norm -> ReLU -> conv -> norm -> ReLU on
``(lateral, top)`` without a stock op.  Known limits: the top's gradient at the lateral's size is written once before it is summed
(no footprint sum in the dgrad epilogue, no 4x4 stride-2 adjoint for the exact x2); the forward is not decomposed into sub-pixel
phases.

The stem and the max-pool in front of ``layer1`` run here as well: ``stem_conv2d`` (one ``torch.autograd.Function``: the 7x7 stride-2
conv from at most 4 channels on the inference stem's padded 4-channel layout, forward without ReLU, an MFMA weight gradient, no
input gradient: the image needs none), the ``nn.Conv2d`` drop-in ``StemConv2d``, ``convert_stem_conv2d_``; ``max_pool2d`` for
(3, 2, 1) and (2, 2, 0) (one ``uint8`` tap index per output element saved, the gradient a gather in a fixed order), the drop-in
``MaxPool2d`` and ``convert_maxpool2d_`` (last part of this module; the rule is the "Trainable stem and max-pool" section of
include/cpn_hip.h).  After ``convert_conv2d_``, ``convert_batchnorm2d_``, ``convert_grouped_conv2d_``, ``convert_bottleneck_`` and
these two, in any order, an encoder runs without a stock operation.  Known limits: batch-norm statistics are not folded into the
stem's epilogue; the pool is not fused into the norm's apply; the sum of the pool's gradient and a lateral's stays autograd's add;
7x7 / stride 2 only (not the 3x3 first conv of the ``U22`` encoders); the bilinear resize behind the heads stays stock;
``cda.models.*`` stay inference-only.

That resize runs here too, as the last part of this module: ``bilinear_resize`` (one ``torch.autograd.Function`` that saves nothing
but the sizes; its gradient, ``bilinear_resize_backward``, is the adjoint of the resize as a gather, for bf16 activations and for
the fp32 head maps), ``resized_conv2d`` (resize + conv of the refinement head as one function that never writes the enlarged
tensor: the forward's loader blends, the weight gradient blends while it stages, only the low-resolution input is saved), the
drop-in ``ResizedConv2d``, and ``CPNCore`` / ``convert_cpn_core_``, which put both where the reference's core calls
``F.interpolate`` (the rule is the "Trainable bilinear resize" section of include/cpn_hip.h).  After all converts a training step
of the reference model has no stock resize between the image and the head maps.  Known limits: the gradient at the input's size is
written once before it is summed; the training forward is not decomposed into sub-pixel phases; upward bilinear resizes and k in
{3, 5, 7} only.
"""
import ctypes

import torch

from . import _lib
from .ops import _need_cuda

__all__ = ['conv2d', 'Conv2d', 'convert_conv2d_', 'is_supported', 'pack_weight', 'conv2d_weight_grad', 'weight_grad_info',
           'batch_norm', 'batch_norm_forward', 'batch_norm_info', 'BatchNorm2d', 'convert_batchnorm2d_',
           'dropout_conv1x1', 'dropout_conv1x1_backward', 'readout_tail_info', 'DropoutConv1x1', 'convert_readout_tail_',
           'grouped_conv2d', 'GroupedConv2d', 'convert_grouped_conv2d_', 'grouped_weight_grad_info', 'grouped_conv2d_weight_grad',
           'grouped_pack_weight', 'grouped_dilate',
           'conv2d_fork', 'strided_conv1x1', 'StridedConv1x1', 'subsample2d', 'Bottleneck', 'convert_bottleneck_',
           'cat_conv2d', 'CatConv2d', 'cat_conv2d_weight_grad', 'cat_weight_grad_info', 'nearest_resize_backward', 'UNetDecoder',
           'convert_unet_decoder_',
           'stem_conv2d', 'StemConv2d', 'convert_stem_conv2d_', 'stem_pack_weight', 'stem_weight_grad', 'stem_weight_grad_info',
           'max_pool2d', 'MaxPool2d', 'convert_maxpool2d_',
           'bilinear_resize', 'bilinear_resize_backward', 'resized_conv2d', 'ResizedConv2d', 'resized_conv2d_weight_grad',
           'resized_weight_grad_info', 'CPNCore', 'convert_cpn_core_']

KERNEL_SIZES = (1, 3, 5, 7)
_DTYPES = {torch.float32: _lib.CONV_TRAIN_F32, torch.bfloat16: _lib.CONV_TRAIN_BF16}


def _check_channels(cin, cout, k):
    """Raises NotImplementedError naming the argument the kernels do not run."""
    if k not in KERNEL_SIZES:
        raise NotImplementedError(f'kernel_size {k}: the trainable conv runs square odd kernels {KERNEL_SIZES} only')
    if cin < 32 or cin % 32:
        raise NotImplementedError(f'in_channels {cin}: the trainable conv needs a positive multiple of 32')
    if cout < 32 or cout % 32:
        raise NotImplementedError(f'out_channels {cout}: the trainable conv needs a positive multiple of 32')


def _check_weight(weight):
    if weight.dim() != 4:
        raise NotImplementedError(f'weight of {weight.dim()} dimensions: the trainable conv needs [Cout, Cin, k, k]')
    if weight.shape[2] != weight.shape[3]:
        raise NotImplementedError(f'kernel_size {tuple(weight.shape[2:])}: the trainable conv runs square kernels only')
    if weight.dtype not in _DTYPES:
        raise NotImplementedError(f'weight dtype {weight.dtype}: the trainable conv takes float32 or bfloat16 parameters')
    _check_channels(int(weight.shape[1]), int(weight.shape[0]), int(weight.shape[2]))


def _nhwc_bf16(t):
    """[N, C, H, W] -> bf16 whose memory is NHWC (no copy for a channels-last bf16 tensor)."""
    return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


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


def pack_weight(weight, mode='forward'):
    """weight [Cout, Cin, k, k] (float32 | bfloat16, on the GPU) -> the bf16 records ``cpn_conv2d`` reads, packed on the device:
    ``'forward'``: [(Cin / 32) k k items (+ one zero item when odd)][Cout][32]; ``'dgrad'``: [(Cout / 32) k k items (+ one)][Cin][32]
    with tap (k - 1 - ky, k - 1 - kx) and the channel roles swapped."""
    _need_cuda(weight)
    _check_weight(weight)
    w = weight.detach().contiguous()
    cout, cin, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
    reduced, outc = (cout, cin) if mode == 'dgrad' else (cin, cout)
    items = reduced // 32 * k * k
    packed = torch.empty((items + items % 2, outc, 32), dtype=torch.bfloat16, device=w.device)
    _lib.check(_lib.load().cpn_conv_train_pack(_lib.ptr(w), _DTYPES[w.dtype], cout, cin, k, _lib.CONV_PACK_MODES[mode],
                                               _lib.ptr(packed), _lib.stream_ptr()), 'conv_train_pack')
    return packed


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


def weight_grad_info(n, h, w, cin, cout, k, slab_rows=0):
    """What ``conv2d_weight_grad`` would run -> dict(slabs, slab_rows, steps (MFMA steps per slab), reduce_chain, bias_chain).  Host
    arithmetic only: needs no GPU.  Raises like the launch for a call it rejects."""
    info = (ctypes.c_int32 * 5)()
    _lib.check(_lib.load().cpn_conv_wgrad_info(n, h, w, cin, cout, k, slab_rows, info), 'conv_wgrad_info')
    return dict(zip(('slabs', 'slab_rows', 'steps', 'reduce_chain', 'bias_chain'), (int(v) for v in info)))


def conv2d_weight_grad(x, grad_output, kernel_size, slab_rows=0, weight=True, bias=True, dtype=torch.float32, bias_dtype=None):
    """(x [N, Cin, H, W], grad_output [N, Cout, H, W]) -> (dW [Cout, Cin, k, k] | None, db [Cout] | None): the gradients ``conv2d``
    returns for its weight and bias, as fp32 sums over the bf16-rounded operands rounded once to ``dtype`` / ``bias_dtype``.
    ``slab_rows``: image rows per slab of the reduction (0: chosen by the library)."""
    _need_cuda(x, grad_output)
    k = int(kernel_size)
    n, cin, h, w = (int(v) for v in x.shape)
    cout = int(grad_output.shape[1])
    _check_channels(cin, cout, k)
    bias_dtype = dtype if bias_dtype is None else bias_dtype
    if dtype not in _DTYPES or bias_dtype not in _DTYPES:
        raise NotImplementedError(f'dtype {dtype} / {bias_dtype}: gradients are float32 or bfloat16')
    assert tuple(grad_output.shape) == (n, cout, h, w), (tuple(grad_output.shape), (n, cout, h, w))
    dw = torch.zeros((cout, cin, k, k), dtype=dtype, device=x.device) if weight else None
    db = torch.zeros((cout,), dtype=bias_dtype, device=x.device) if bias else None
    if n * h * w == 0 or not (weight or bias):
        return dw, db
    xs, gs = _nhwc_bf16(x.detach()), _nhwc_bf16(grad_output.detach())
    lib = _lib.load()
    nbytes = int(lib.cpn_conv_wgrad_workspace_bytes(n, h, w, cin, cout, k, slab_rows))
    if nbytes <= 0:
        _lib.check(lib.cpn_conv_wgrad_info(n, h, w, cin, cout, k, slab_rows, (ctypes.c_int32 * 5)()), 'conv_wgrad')
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    _lib.check(lib.cpn_conv_wgrad(_lib.ptr(xs), _lib.ptr(gs), n, h, w, cin, cout, k, slab_rows, _lib.ptr(dw), _DTYPES[dtype],
                                  _lib.ptr(db), _DTYPES[bias_dtype], _lib.ptr(ws), nbytes, _lib.stream_ptr()), 'conv_wgrad')
    return dw, db


class _Conv2dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        cout, cin, k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        xs = _nhwc_bf16(x.detach())
        b32 = None if bias is None else bias.detach().float().contiguous()
        out = _run_conv(xs, pack_weight(weight, 'forward'), b32, cin, cout, k)
        ctx.save_for_backward(xs, weight)
        ctx.x_dtype = x.dtype
        ctx.bias_dtype = None if bias is None else bias.dtype
        return out

    @staticmethod
    def backward(ctx, grad_output):
        xs, weight = ctx.saved_tensors
        cout, cin, k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        need_x, need_w, need_b = ctx.needs_input_grad
        need_b = need_b and ctx.bias_dtype is not None
        gs = _nhwc_bf16(grad_output.detach())
        dx = dw = db = None
        if need_x:  # the conv of grad_output with the flipped, channel-swapped weights
            dx = _run_conv(gs, pack_weight(weight, 'dgrad'), None, cout, cin, k).to(ctx.x_dtype)
        if need_w or need_b:
            dw, db = conv2d_weight_grad(xs, gs, k, weight=need_w, bias=need_b, dtype=weight.dtype,
                                        bias_dtype=ctx.bias_dtype or weight.dtype)
        return dx, dw, db


def _check_conv2d(x, weight, bias, padding=None):
    if x.dim() != 4:
        raise NotImplementedError(f'input of {x.dim()} dimensions: the trainable conv takes a 4-D [N, C, H, W] input')
    _check_weight(weight)
    k = int(weight.shape[2])
    if padding is not None:
        pad = (k // 2, k // 2) if padding == 'same' else _pair(padding)
        if isinstance(padding, str) and padding != 'same' or pad != (k // 2, k // 2):
            raise NotImplementedError(f'padding {padding}: the trainable conv pads k // 2 = {k // 2} zeros on every side')
    if x.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {x.dtype}: the trainable conv takes float32 or bfloat16 activations')
    if int(x.shape[1]) != int(weight.shape[1]):
        raise ValueError(f'input has {int(x.shape[1])} channels, weight expects {int(weight.shape[1])}')
    if bias is not None and (bias.dim() != 1 or bias.shape[0] != weight.shape[0] or bias.dtype not in _DTYPES):
        raise NotImplementedError(f'bias {tuple(bias.shape)} {bias.dtype}: the trainable conv takes a float32 or bfloat16 [Cout] bias')
    _need_cuda(x, weight, bias)


def conv2d(x, weight, bias=None, padding=None):
    """``torch.nn.functional.conv2d(x, weight, bias, stride=1, padding=k // 2)`` for the supported family (module docstring), with
    gradients for ``x``, ``weight`` and ``bias`` as autograd asks for them -> bf16 [N, Cout, H, W] in ``torch.channels_last``."""
    _check_conv2d(x, weight, bias, padding)
    return _Conv2dFunction.apply(x, weight, bias)


class _Conv2dForkFunction(torch.autograd.Function):
    """``conv2d`` whose second output is its input: the gradient that arrives there is added in the dgrad conv's epilogue."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.set_materialize_grads(False)  # an absent skip gradient arrives as None, not as a tensor of zeros
        return _Conv2dFunction.forward(ctx, x, weight, bias), x  # (an input returned as it is becomes an alias of it)

    @staticmethod
    def backward(ctx, grad_output, grad_skip):
        if grad_skip is None:
            return (None, None, None) if grad_output is None else _Conv2dFunction.backward(ctx, grad_output)
        if grad_output is None:
            return (grad_skip.to(ctx.x_dtype) if ctx.needs_input_grad[0] else None), None, None
        xs, weight = ctx.saved_tensors
        cout, cin, k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        need_x, need_w, need_b = ctx.needs_input_grad
        need_b = need_b and ctx.bias_dtype is not None
        gs = _nhwc_bf16(grad_output.detach())
        dx = dw = db = None
        if need_x:  # the dgrad conv with the skip's gradient as its residual operand: the sum in fp32, one rounding
            dx = _run_conv(gs, pack_weight(weight, 'dgrad'), None, cout, cin, k, res=_nhwc(grad_skip, torch.bfloat16)).to(ctx.x_dtype)
        if need_w or need_b:
            dw, db = conv2d_weight_grad(xs, gs, k, weight=need_w, bias=need_b, dtype=weight.dtype,
                                        bias_dtype=ctx.bias_dtype or weight.dtype)
        return dx, dw, db


def conv2d_fork(x, weight, bias=None):
    """``conv2d(x, weight, bias)`` at the head of a residual block -> ``(y, skip)``: ``y`` is ``conv2d``'s output bit for bit,
    ``skip`` is ``x`` (same storage, no copy) with this function as its ``grad_fn``, so autograd sees ONE consumer of ``x`` and the
    two gradients of the block's input are never added by a stock op: when a gradient arrives at ``skip`` it is rounded to bf16
    channels-last as ``grad_output`` is and becomes the residual operand of the dgrad conv, ``dx = round(dgrad(dy) + dskip)`` with
    the sum in fp32; when none arrives the backward is ``conv2d``'s."""
    _check_conv2d(x, weight, bias)
    return _Conv2dForkFunction.apply(x, weight, bias)


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _unsupported(kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels, transposed=False):
    """The first argument the trainable conv does not run, as a sentence, or None."""
    if transposed:
        return 'transposed convs are not run'
    if groups != 1:
        return f'groups {groups}: dense convs only'
    if _pair(stride) != (1, 1):
        return f'stride {stride}: stride 1 only'
    if _pair(dilation) != (1, 1):
        return f'dilation {dilation}: dilation 1 only'
    ks = _pair(kernel_size)
    if ks[0] != ks[1] or ks[0] not in KERNEL_SIZES:
        return f'kernel_size {kernel_size}: square odd kernels {KERNEL_SIZES} only'
    if isinstance(padding, str):
        if padding != 'same':
            return f"padding '{padding}': k // 2 zeros only"
    elif _pair(padding) != (ks[0] // 2, ks[0] // 2):
        return f'padding {padding}: k // 2 = {ks[0] // 2} zeros only'
    if padding_mode != 'zeros':
        return f"padding_mode '{padding_mode}': zeros only"
    if in_channels < 32 or in_channels % 32:
        return f'in_channels {in_channels}: multiples of 32 only'
    if out_channels < 32 or out_channels % 32:
        return f'out_channels {out_channels}: multiples of 32 only'
    return None


def is_supported(conv):
    """Whether ``convert_conv2d_`` replaces this ``torch.nn.Conv2d``."""
    return _why_not(conv) is None


def _why_not(conv):
    if not isinstance(conv, torch.nn.Conv2d) or isinstance(conv, Conv2d):
        return 'not a torch.nn.Conv2d'
    if type(conv) is not torch.nn.Conv2d:
        return f'a subclass of torch.nn.Conv2d ({type(conv).__name__}): its forward may differ'
    if conv.weight.dtype not in _DTYPES:
        return f'weight dtype {conv.weight.dtype}: float32 or bfloat16 only'
    return _unsupported(conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.padding_mode, conv.in_channels,
                        conv.out_channels, conv.transposed)


class Conv2d(torch.nn.Conv2d):
    """``torch.nn.Conv2d`` with torch's constructor arguments and parameter names (``weight``, ``bias``: ``state_dict``s
    interchange) whose forward is ``conv2d``.  ``padding`` defaults to ``kernel_size // 2``; an argument outside the supported family
    raises ``NotImplementedError`` naming it."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=None, dilation=1, groups=1, bias=True,
                 padding_mode='zeros', device=None, dtype=None):
        ks = _pair(kernel_size)
        padding = ks[0] // 2 if padding is None else padding
        why = _unsupported(kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels)
        if why is not None:
            raise NotImplementedError(why)
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device, dtype)

    def forward(self, x, fork=False):
        return conv2d_fork(x, self.weight, self.bias) if fork else conv2d(x, self.weight, self.bias)


def _from_torch(conv):
    new = Conv2d.__new__(Conv2d)
    new.__dict__.update(conv.__dict__)  # the same Parameter objects, hooks, training flag and constructor attributes
    new._parameters = dict(conv._parameters)  # (the registry itself is the new module's own)
    return new


def convert_conv2d_(module):
    """Replaces every eligible ``torch.nn.Conv2d`` below ``module`` in place by a ``Conv2d`` that shares its ``Parameter`` objects
    (optimisers and ``state_dict`` keys are unaffected) -> (names replaced, {name left: reason}).  ``module`` itself is not replaced
    when it is a conv: it is reported as left."""
    replaced, left = [], {}
    if isinstance(module, torch.nn.Conv2d) and not isinstance(module, (Conv2d, StridedConv1x1, CatConv2d, StemConv2d)):
        left[''] = _why_not(module) or 'the root module cannot be replaced in place: convert its parent'
    for name, parent in list(module.named_modules()):
        for child_name, child in list(parent.named_children()):
            full = f'{name}.{child_name}' if name else child_name
            if isinstance(child, (Conv2d, DropoutConv1x1, GroupedConv2d, StridedConv1x1, CatConv2d, StemConv2d)) or \
                    not isinstance(child, torch.nn.modules.conv._ConvNd):
                continue
            why = _why_not(child) if isinstance(child, torch.nn.Conv2d) else f'{type(child).__name__}: 2-D convs only'
            if why is None:
                setattr(parent, child_name, _from_torch(child))
                replaced.append(full)
            else:
                left[full] = why
    return replaced, left


# ---- batch normalisation with an optional fused ReLU ("Trainable batch normalisation" of include/cpn_hip.h, csrc/batch_norm.hip)
#
# In the reference model every trainable conv is followed by BatchNorm2d and ReLU.  ``batch_norm`` runs both as one autograd
# function on the channels-last tensor the conv hands over: statistics (1 read), apply (1 read, 1 write), backward reduce (2 reads),
# backward input (2 reads, 1 write).  It saves ``x`` and per-channel fp32 vectors only: the ReLU mask is recomputed bit for bit from
# ``x`` by the forward's own fma.  Sums over pixels are fp64 in a fixed order (no floating-point atomics); supported: a 4-D input
# on the GPU, float32 or bfloat16, ``C`` a positive multiple of 8.  With ``residual`` the apply adds it before the ReLU (3 passes) and
# the backward masks by the stored output (4 + 3 passes; ``x`` and ``y`` saved).  Known limit: statistics not folded into the conv
# epilogue.

ACTIVATIONS = (None, 'relu')
_INFO_KEYS = ('slabs', 'slab_pixels', 'rows', 'channel_blocks', 'chain')


def batch_norm_info(m, c, slab_pixels=0):
    """What the batch-norm kernels would run on ``m`` pixels of ``c`` channels -> dict(slabs, slab_pixels, rows (pixels per step of
    the first channel block), channel_blocks, chain (terms of the fp64 chain of one channel sum)).  Host arithmetic only: needs no
    GPU.  Raises like the launch for a call it rejects."""
    info = (ctypes.c_int64 * 5)()
    _lib.check(_lib.load().cpn_bn_info(int(m), int(c), int(slab_pixels), info), 'bn_info')
    return dict(zip(_INFO_KEYS, (int(v) for v in info)))


def _check_bn(x, running_mean, running_var, weight, bias, activation):
    """Raises NotImplementedError naming the argument the kernels do not run."""
    if activation not in ACTIVATIONS:
        raise NotImplementedError(f'activation {activation!r}: the fused batch norm runs {ACTIVATIONS} only')
    if x.dim() != 4:
        raise NotImplementedError(f'input of {x.dim()} dimensions: the batch norm takes a 4-D [N, C, H, W] input')
    if x.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {x.dtype}: the batch norm takes float32 or bfloat16 activations')
    c = int(x.shape[1])
    if c < 8 or c % 8:
        raise NotImplementedError(f'num_features {c}: the batch norm needs a positive multiple of 8 channels')
    for name, t in (('weight', weight), ('bias', bias), ('running_mean', running_mean), ('running_var', running_var)):
        if t is not None and (t.dtype not in _DTYPES or tuple(t.shape) != (c,)):
            raise NotImplementedError(f'{name} {tuple(t.shape)} {t.dtype}: the batch norm takes a float32 or bfloat16 [{c}] vector')
    for name, t in (('running_mean', running_mean), ('running_var', running_var)):
        if t is not None and not t.is_contiguous():
            raise NotImplementedError(f'{name} with strides {t.stride()}: the batch norm updates a contiguous buffer in place')
    if (running_mean is None) != (running_var is None) or \
            (running_mean is not None and running_mean.dtype != running_var.dtype):
        raise NotImplementedError('running_mean / running_var: both or neither, of one dtype')


def _dt(t):
    return 0 if t is None else _DTYPES[t.dtype]


def _nhwc(t, dtype=None):
    """[N, C, H, W] -> a detached tensor whose memory is NHWC from a 16-byte aligned address, as the kernels' 16-byte loads need:
    no copy for an aligned channels-last tensor of that dtype; a view into the middle of a buffer is cloned."""
    t = t.detach().to(dtype or t.dtype).contiguous(memory_format=torch.channels_last)
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.preserve_format)


def _workspace(lib, m, c, slab_pixels, device):
    nbytes = int(lib.cpn_bn_workspace_bytes(m, c, slab_pixels))
    if nbytes <= 0:
        _lib.check(lib.cpn_bn_info(m, c, slab_pixels, (ctypes.c_int64 * 5)()), 'bn')
    return torch.empty((nbytes,), dtype=torch.uint8, device=device), nbytes


def _bn_forward(xs, running_mean, running_var, weight, bias, use_batch, momentum, eps, relu, slab_pixels, residual=None):
    """xs (and residual, if any, of its dtype and shape): channels-last, on the GPU -> (y, save_mean, save_invstd, scale, shift);
    updates the running buffers when use_batch."""
    n, c, h, w = (int(v) for v in xs.shape)
    m = n * h * w
    lib = _lib.load()
    coeffs = torch.empty((4, c), dtype=torch.float32, device=xs.device)
    mean, invstd, scale, shift = coeffs[0], coeffs[1], coeffs[2], coeffs[3]
    y = torch.empty_like(xs, memory_format=torch.channels_last)
    if use_batch:
        ws, nbytes = _workspace(lib, m, c, slab_pixels, xs.device)
        _lib.check(lib.cpn_bn_train_stats(_lib.ptr(xs), _dt(xs), m, c, slab_pixels, _lib.ptr(weight), _dt(weight), _lib.ptr(bias),
                                          _dt(bias), _lib.ptr(running_mean), _lib.ptr(running_var), _dt(running_mean),
                                          float(momentum), float(eps), _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(scale),
                                          _lib.ptr(shift), _lib.ptr(ws), nbytes, _lib.stream_ptr()), 'bn_train_stats')
    else:
        _lib.check(lib.cpn_bn_eval_coeffs(c, _lib.ptr(weight), _dt(weight), _lib.ptr(bias), _dt(bias), _lib.ptr(running_mean),
                                          _lib.ptr(running_var), _dt(running_mean), float(eps), _lib.ptr(mean), _lib.ptr(invstd),
                                          _lib.ptr(scale), _lib.ptr(shift), _lib.stream_ptr()), 'bn_eval_coeffs')
    if residual is not None:
        _lib.check(lib.cpn_residual_bn_apply(_lib.ptr(xs), _lib.ptr(residual), _lib.ptr(y), _dt(xs), m, c, slab_pixels, _lib.ptr(scale),
                                             _lib.ptr(shift), int(relu), _lib.stream_ptr()), 'bn_apply_residual')
        return y, mean, invstd, scale, shift
    _lib.check(lib.cpn_bn_apply(_lib.ptr(xs), _lib.ptr(y), _dt(xs), m, c, slab_pixels, _lib.ptr(scale), _lib.ptr(shift), int(relu),
                                _lib.stream_ptr()), 'bn_apply')
    return y, mean, invstd, scale, shift


def _prepare(x, running_mean, running_var, weight, bias, training, activation, residual=None):
    _check_bn(x, running_mean, running_var, weight, bias, activation)
    if residual is not None:
        if not isinstance(residual, torch.Tensor) or tuple(residual.shape) != tuple(x.shape):
            raise NotImplementedError(f'residual of shape {tuple(getattr(residual, "shape", ()))}: the batch norm adds a tensor of the '
                                      f"input's shape {tuple(x.shape)}")
        if residual.dtype not in _DTYPES:
            raise NotImplementedError(f'residual dtype {residual.dtype}: the batch norm adds a float32 or bfloat16 tensor')
        _need_cuda(residual)
    use_batch = bool(training) or running_mean is None
    n, c, h, w = (int(v) for v in x.shape)
    if use_batch and n * h * w == 1:
        raise ValueError(f'Expected more than 1 value per channel when training, got input size {tuple(x.shape)}')
    if n * h * w == 0:
        raise NotImplementedError(f'input of shape {tuple(x.shape)}: the batch norm needs at least one pixel')
    _need_cuda(x, running_mean, running_var, weight, bias)
    return use_batch


def batch_norm_forward(x, running_mean, running_var, weight=None, bias=None, training=False, momentum=0.1, eps=1e-5,
                       activation=None, slab_pixels=0, residual=None):
    """The forward of ``batch_norm`` without autograd -> (y, save_mean, save_invstd, scale, shift): ``y`` in ``x``'s dtype and
    ``torch.channels_last``, four fp32 ``[C]`` vectors (eval: the running mean, its invstd and the coefficients from them).  In
    training the running buffers are updated in place.  ``slab_pixels``: pixels per slab of the sums (0: chosen by the library).
    ``residual``: as in ``batch_norm``."""
    use_batch = _prepare(x, running_mean, running_var, weight, bias, training, activation, residual)
    det = [None if t is None else t.detach().contiguous() for t in (weight, bias)]
    xs = _nhwc(x)
    rs = None if residual is None else _nhwc(residual, xs.dtype)
    return _bn_forward(xs, running_mean, running_var, det[0], det[1], use_batch, momentum, eps, activation == 'relu', slab_pixels, rs)


class _BatchNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, use_batch, momentum, eps, relu, slab_pixels):
        xs = _nhwc(x)
        wd = None if weight is None else weight.detach().contiguous()
        bd = None if bias is None else bias.detach().contiguous()
        y, mean, invstd, scale, shift = _bn_forward(xs, running_mean, running_var, wd, bd, use_batch, momentum, eps, relu, slab_pixels)
        ctx.save_for_backward(xs, weight, mean, invstd, scale, shift)
        ctx.use_batch, ctx.relu, ctx.slab_pixels = use_batch, relu, slab_pixels
        ctx.bias_dtype = None if bias is None else bias.dtype
        return y

    @staticmethod
    def backward(ctx, grad_output):
        xs, weight, mean, invstd, scale, shift = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_w = need_w and weight is not None
        need_b = need_b and ctx.bias_dtype is not None
        n, c, h, w = (int(v) for v in xs.shape)
        m, sp, relu = n * h * w, ctx.slab_pixels, int(ctx.relu)
        lib = _lib.load()
        gs = _nhwc(grad_output, xs.dtype)
        wd = None if weight is None else weight.detach().contiguous()
        dx = dw = db = abc = None
        if need_w or need_b or (need_x and ctx.use_batch):
            dw = torch.empty((c,), dtype=weight.dtype, device=xs.device) if need_w else None
            db = torch.empty((c,), dtype=ctx.bias_dtype, device=xs.device) if need_b else None
            abc = torch.empty((3, c), dtype=torch.float32, device=xs.device) if need_x and ctx.use_batch else None
            ws, nbytes = _workspace(lib, m, c, sp, xs.device)
            _lib.check(lib.cpn_bn_backward_reduce(_lib.ptr(xs), _lib.ptr(gs), _dt(xs), m, c, sp, _lib.ptr(scale), _lib.ptr(shift), relu,
                                                  _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(wd), _dt(wd), _lib.ptr(dw), _dt(dw),
                                                  _lib.ptr(db), _dt(db), _lib.ptr(abc), _lib.ptr(ws), nbytes, _lib.stream_ptr()),
                       'bn_backward_reduce')
        if need_x:
            dx = torch.empty_like(xs, memory_format=torch.channels_last)
            a, b, cc = (abc[0], abc[1], abc[2]) if ctx.use_batch else (scale, None, None)
            _lib.check(lib.cpn_bn_backward_input(_lib.ptr(xs), _lib.ptr(gs), _lib.ptr(dx), _dt(xs), m, c, sp, _lib.ptr(scale),
                                                 _lib.ptr(shift), relu, _lib.ptr(a), _lib.ptr(b), _lib.ptr(cc), _lib.stream_ptr()),
                       'bn_backward_input')
        return dx, dw, db, None, None, None, None, None, None, None


class _BatchNormResidualFunction(torch.autograd.Function):
    """activation(bn(x) + residual).  Saves x, its own output y and the per-channel vectors -- not the residual: the ReLU mask is
    ``y > 0`` on the stored output, as in torch's own ReLU backward."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean, running_var, use_batch, momentum, eps, relu, slab_pixels):
        xs = _nhwc(x)
        rs = _nhwc(residual, xs.dtype)
        wd = None if weight is None else weight.detach().contiguous()
        bd = None if bias is None else bias.detach().contiguous()
        y, mean, invstd, scale, shift = _bn_forward(xs, running_mean, running_var, wd, bd, use_batch, momentum, eps, relu, slab_pixels,
                                                    rs)
        ctx.save_for_backward(xs, y, weight, mean, invstd, scale, shift)
        ctx.use_batch, ctx.relu, ctx.slab_pixels = use_batch, relu, slab_pixels
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.residual_dtype = residual.dtype
        return y

    @staticmethod
    def backward(ctx, grad_output):
        xs, y, weight, mean, invstd, scale, shift = ctx.saved_tensors
        need_x, need_r, need_w, need_b = ctx.needs_input_grad[:4]
        need_w = need_w and weight is not None
        need_b = need_b and ctx.bias_dtype is not None
        n, c, h, w = (int(v) for v in xs.shape)
        m, sp = n * h * w, ctx.slab_pixels
        lib = _lib.load()
        gs = _nhwc(grad_output, xs.dtype)
        wd = None if weight is None else weight.detach().contiguous()
        dx = dw = db = abc = None
        sums = need_w or need_b or (need_x and ctx.use_batch)
        g = gs  # without ReLU g = dy: nothing is masked and nothing is written
        if sums or (ctx.relu and (need_x or need_r)):
            dw = torch.empty((c,), dtype=weight.dtype, device=xs.device) if need_w else None
            db = torch.empty((c,), dtype=ctx.bias_dtype, device=xs.device) if need_b else None
            abc = torch.empty((3, c), dtype=torch.float32, device=xs.device) if need_x and ctx.use_batch else None
            if ctx.relu:
                g = torch.empty_like(xs, memory_format=torch.channels_last)
            ws, nbytes = _workspace(lib, m, c, sp, xs.device)
            _lib.check(lib.cpn_residual_bn_backward_reduce(_lib.ptr(xs), _lib.ptr(gs), _lib.ptr(y), _lib.ptr(g), _dt(xs), m, c, sp,
                                                           _lib.ptr(scale), _lib.ptr(shift), int(ctx.relu), _lib.ptr(mean),
                                                           _lib.ptr(invstd), _lib.ptr(wd), _dt(wd), _lib.ptr(dw), _dt(dw), _lib.ptr(db),
                                                           _dt(db), _lib.ptr(abc), _lib.ptr(ws), nbytes, _lib.stream_ptr()),
                       'bn_backward_reduce_residual')
        if need_x:
            dx = torch.empty_like(xs, memory_format=torch.channels_last)
            a, b, cc = (abc[0], abc[1], abc[2]) if ctx.use_batch else (scale, None, None)
            _lib.check(lib.cpn_bn_backward_input(_lib.ptr(xs), _lib.ptr(g), _lib.ptr(dx), _dt(xs), m, c, sp, _lib.ptr(None),
                                                 _lib.ptr(None), 0, _lib.ptr(a), _lib.ptr(b), _lib.ptr(cc), _lib.stream_ptr()),
                       'bn_backward_input')
        dr = g.to(ctx.residual_dtype) if need_r else None
        return dx, dr, dw, db, None, None, None, None, None, None, None


def batch_norm(x, running_mean, running_var, weight=None, bias=None, training=False, momentum=0.1, eps=1e-5, activation=None,
               slab_pixels=0, residual=None):
    """``torch.nn.functional.batch_norm`` (its argument order) for a 4-D input on the GPU, followed by ``activation`` (None |
    'relu') in the same kernels, with gradients for ``x``, ``weight`` and ``bias`` as autograd asks for them -> ``x``'s dtype in
    ``torch.channels_last``.  Batch statistics are used when ``training`` or when the running buffers are absent; in training the
    running buffers are updated in place with ``momentum``.  Anything unsupported raises ``NotImplementedError`` naming the
    argument; training on a single value per channel raises ``ValueError`` like torch.

    ``residual`` (``[N, C, H, W]``, float32 | bfloat16, brought to ``x``'s dtype and channels-last as ``grad_output`` is): the tail
    of a residual block, ``activation(bn(x) + residual)`` in one pass behind the unchanged statistics: ``t = fmaf(x, scale, shift)``
    and ``t + residual`` are fp32 operations, the result is rounded once to the dtype.  Its backward takes the ReLU mask from the
    stored output (``y > 0``), so it saves ``x`` and its own output ``y``, which the next conv saves anyway, and not ``residual``; an
    in-place operation on ``y`` downstream therefore makes autograd raise.  The masked gradient is the residual's gradient bit for
    bit (returned in ``residual``'s dtype).  ``residual=None``: the same launches and bits as without the argument."""
    use_batch = _prepare(x, running_mean, running_var, weight, bias, training, activation, residual)
    if residual is not None:
        return _BatchNormResidualFunction.apply(x, residual, weight, bias, running_mean, running_var, use_batch, float(momentum),
                                                float(eps), activation == 'relu', int(slab_pixels))
    return _BatchNormFunction.apply(x, weight, bias, running_mean, running_var, use_batch, float(momentum), float(eps),
                                    activation == 'relu', int(slab_pixels))


_MODULE_S = object()  # BatchNorm2d.forward(activation=...): "the module's own"


class BatchNorm2d(torch.nn.BatchNorm2d):
    """``torch.nn.BatchNorm2d`` with torch's constructor arguments, parameter and buffer names (``state_dict``s interchange) plus
    ``activation`` (None | 'relu'), whose forward is ``batch_norm``.  ``num_batches_tracked`` and ``momentum=None`` (cumulative
    average) behave as in torch."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, device=None, dtype=None,
                 activation=None):
        if activation not in ACTIVATIONS:
            raise NotImplementedError(f'activation {activation!r}: the fused batch norm runs {ACTIVATIONS} only')
        if num_features < 8 or num_features % 8:
            raise NotImplementedError(f'num_features {num_features}: the batch norm needs a positive multiple of 8 channels')
        super().__init__(num_features, eps, momentum, affine, track_running_stats, device, dtype)
        self.activation = activation

    def forward(self, x, residual=None, activation=_MODULE_S):
        """``residual``, ``activation`` (default: the module's): as in ``batch_norm``, for this call."""
        activation = self.activation if activation is _MODULE_S else activation
        factor = 0. if self.momentum is None else self.momentum
        if self.training and self.track_running_stats and self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
            if self.momentum is None:
                factor = 1. / float(self.num_batches_tracked)
        use_buffers = not self.training or self.track_running_stats
        return batch_norm(x, self.running_mean if use_buffers else None, self.running_var if use_buffers else None, self.weight,
                          self.bias, self.training or self.running_mean is None, factor, self.eps, activation, residual=residual)

    def extra_repr(self):
        return super().extra_repr() + f', activation={self.activation!r}'


def _bn_why_not(bn):
    if type(bn) is not torch.nn.BatchNorm2d:
        return f'{type(bn).__name__}: torch.nn.BatchNorm2d itself only'
    if bn.num_features < 8 or bn.num_features % 8:
        return f'num_features {bn.num_features}: multiples of 8 only'
    for name, t in list(bn.named_parameters(recurse=False)) + list(bn.named_buffers(recurse=False)):
        if name != 'num_batches_tracked' and t.dtype not in _DTYPES:
            return f'{name} dtype {t.dtype}: float32 or bfloat16 only'
    return None


def _bn_from_torch(bn, activation):
    new = BatchNorm2d.__new__(BatchNorm2d)
    new.__dict__.update(bn.__dict__)  # the same Parameter and buffer objects, hooks, training flag and constructor attributes
    new._parameters, new._buffers = dict(bn._parameters), dict(bn._buffers)  # (the registries are the new module's own)
    new.activation = activation
    return new


def convert_batchnorm2d_(module, fuse_relu=True):
    """Replaces every eligible ``torch.nn.BatchNorm2d`` below ``module`` in place by a ``BatchNorm2d`` that shares its ``Parameter``
    and buffer objects -> (names replaced, names whose ReLU was fused, {name left: reason}).  With ``fuse_relu``, where the parent is
    an ``nn.Sequential`` and the slot right behind the norm holds exactly a ``torch.nn.ReLU`` that occurs once in the whole tree (as
    does the norm), the norm gets ``activation='relu'`` and the ReLU's slot becomes ``torch.nn.Identity()``: indices and
    ``state_dict`` keys do not move.  A norm object that sits in several slots is replaced by one object in all of them."""
    replaced, fused, left = [], [], {}
    if isinstance(module, torch.nn.modules.batchnorm._NormBase) and not isinstance(module, BatchNorm2d):
        left[''] = _bn_why_not(module) or 'the root module cannot be replaced in place: convert its parent'
    uses = {}  # slots per ReLU or norm object in the whole tree: one that sits in two slots runs twice and is not fused
    for parent in module.modules():
        for child in parent._modules.values():
            if type(child) in (torch.nn.ReLU, torch.nn.BatchNorm2d):
                uses[id(child)] = uses.get(id(child), 0) + 1
    swapped = {}  # id of a replaced norm -> its replacement: a norm in two slots stays one object
    for name, parent in list(module.named_modules()):
        slots = [(n, c) for n, c in parent._modules.items() if c is not None]  # (named_children() drops repeated objects)
        for i, (child_name, child) in enumerate(slots):
            full = f'{name}.{child_name}' if name else child_name
            if isinstance(child, BatchNorm2d) or not isinstance(child, torch.nn.modules.batchnorm._NormBase):
                continue
            why = _bn_why_not(child)
            if why is not None:
                left[full] = why
                continue
            nxt = slots[i + 1] if i + 1 < len(slots) else None
            fuse = fuse_relu and isinstance(parent, torch.nn.Sequential) and nxt is not None and type(nxt[1]) is torch.nn.ReLU and \
                uses.get(id(nxt[1])) == 1 and uses.get(id(child)) == 1
            if id(child) not in swapped:
                swapped[id(child)] = _bn_from_torch(child, 'relu' if fuse else None)
            setattr(parent, child_name, swapped[id(child)])
            replaced.append(full)
            if fuse:
                setattr(parent, nxt[0], torch.nn.Identity())
                fused.append(full)
    return replaced, fused, left


# ---- the ReadOut tail: Dropout2d fused into a 1x1 conv to few channels ("Trainable ReadOut tail" of include/cpn_hip.h,
# csrc/readout_tail.hip)
#
# The last two modules of a ReadOut head read the largest activation of a training step.  Stock torch moves it about seven times
# (dropout forward and backward, conv forward, weight gradient, input gradient) and saves two copies; ``dropout_conv1x1`` reads it
# once forward and once backward, writes ``dx`` once and saves ``x`` alone.  The dropout never touches ``x``: the weight operand of
# the MFMA is masked per image and the factor 1 / (1 - p) is applied to the fp32 sum, so ``x / (1 - p)`` is never rounded to bf16.
# Supported: a 4-D input on the GPU, float32 or bfloat16, ``Cin`` a positive multiple of 32 up to 1024, 1 <= ``Cout`` <= 32.

TAIL_MAX_CIN, TAIL_MAX_COUT = 1024, 32
_TAIL_INFO_KEYS = ('slabs', 'slab_pixels', 'steps', 'reduce_chain', 'bias_chain', 'forward_chain', 'slabs_per_image', 'dx_steps')


def readout_tail_info(n, hw, cin, cout, slab_pixels=0):
    """What the ReadOut-tail kernels would run on ``n`` images of ``hw`` pixels -> dict(slabs, slab_pixels, steps (MFMA steps per
    slab), reduce_chain, bias_chain, forward_chain, slabs_per_image, dx_steps).  Host arithmetic only: needs no GPU.  Raises like
    the launch for a call it rejects."""
    info = (ctypes.c_int64 * 8)()
    _lib.check(_lib.load().cpn_tail_info(int(n), int(hw), int(cin), int(cout), int(slab_pixels), info), 'tail_info')
    return dict(zip(_TAIL_INFO_KEYS, (int(v) for v in info)))


def _tail_channels(cin, cout):
    """The first channel count the tail kernels do not run, as a sentence, or None."""
    if cin < 32 or cin % 32 or cin > TAIL_MAX_CIN:
        return f'in_channels {cin}: positive multiples of 32 up to {TAIL_MAX_CIN} only'
    if cout < 1 or cout > TAIL_MAX_COUT:
        return f'out_channels {cout}: 1 ... {TAIL_MAX_COUT} only'
    return None


def _check_tail(x, weight, bias, p, keep, out_dtype):
    """Raises NotImplementedError naming the argument the kernels do not run -> (keep as [N, Cin] or None)."""
    if x.dim() != 4:
        raise NotImplementedError(f'input of {x.dim()} dimensions: the ReadOut tail takes a 4-D [N, C, H, W] input')
    if x.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {x.dtype}: the ReadOut tail takes float32 or bfloat16 activations')
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (1, 1):
        raise NotImplementedError(f'kernel_size / weight {tuple(weight.shape)}: the ReadOut tail runs [Cout, Cin, 1, 1] weights only')
    if weight.dtype not in _DTYPES:
        raise NotImplementedError(f'weight dtype {weight.dtype}: the ReadOut tail takes float32 or bfloat16 parameters')
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    why = _tail_channels(cin, cout)
    if why is not None:
        raise NotImplementedError(why)
    if int(x.shape[1]) != cin:
        raise ValueError(f'input has {int(x.shape[1])} channels, weight expects {cin}')
    if bias is not None and (bias.dim() != 1 or int(bias.shape[0]) != cout or bias.dtype not in _DTYPES):
        raise NotImplementedError(f'bias {tuple(bias.shape)} {bias.dtype}: the ReadOut tail takes a float32 or bfloat16 [{cout}] bias')
    if not isinstance(p, (int, float)) or not 0. <= p <= 1.:
        raise NotImplementedError(f'p {p!r}: a dropout probability in [0, 1]')
    if out_dtype not in _DTYPES:
        raise NotImplementedError(f'out_dtype {out_dtype}: float32 or bfloat16 only')
    if int(x.shape[0]) * int(x.shape[2]) * int(x.shape[3]) == 0:
        raise NotImplementedError(f'input of shape {tuple(x.shape)}: the ReadOut tail needs at least one pixel')
    if keep is not None:
        n = int(x.shape[0])
        if keep.dtype not in (torch.bool, torch.uint8) or keep.numel() != n * cin or \
                tuple(keep.shape) not in ((n, cin), (n, cin, 1, 1)):
            raise NotImplementedError(f'keep {tuple(keep.shape)} {keep.dtype}: a bool or uint8 [{n}, {cin}] mask of the channels kept')


def _tail_scale(p):
    return 0. if p >= 1. else 1. / (1. - p)


def _plane_grad(grad_output):
    g = grad_output.detach()
    return (g if g.dtype in _DTYPES else g.float()).contiguous()


def _tail_backward(xs, grad_output, weight, keep, scale, slab_pixels, need_x, need_w, need_b, bias_dtype):
    """xs: bf16 NHWC memory, 16-byte aligned; keep: uint8 [N, Cin] or None -> (dx bf16 channels-last, dW, db), None where not asked."""
    n, cin, h, w = (int(v) for v in xs.shape)
    cout = int(weight.shape[0])
    lib = _lib.load()
    g = _plane_grad(grad_output)
    assert tuple(g.shape) == (n, cout, h, w), (tuple(g.shape), (n, cout, h, w))
    wd = weight.detach().reshape(cout, cin).contiguous()
    dx = torch.empty_like(xs, memory_format=torch.channels_last) if need_x else None
    dw = torch.empty((cout, cin, 1, 1), dtype=weight.dtype, device=xs.device) if need_w else None
    db = torch.empty((cout,), dtype=bias_dtype, device=xs.device) if need_b else None
    if not (need_x or need_w or need_b):
        return None, None, None
    ws, nbytes = None, 0
    if need_w or need_b:
        nbytes = int(lib.cpn_tail_workspace_bytes(n, h * w, cin, cout, slab_pixels))
        if nbytes <= 0:
            _lib.check(lib.cpn_tail_info(n, h * w, cin, cout, slab_pixels, (ctypes.c_int64 * 8)()), 'tail_backward')
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=xs.device)
    _lib.check(lib.cpn_tail_backward(_lib.ptr(xs), _lib.ptr(g), _dt(g), _lib.ptr(wd), _dt(wd), _lib.ptr(keep), float(scale), n, h * w,
                                     cin, cout, int(slab_pixels), _lib.ptr(dx), _lib.ptr(dw), _dt(dw), _lib.ptr(db), _dt(db),
                                     _lib.ptr(ws), nbytes, _lib.stream_ptr()), 'tail_backward')
    return dx, dw, db


class _DropoutConv1x1Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, keep, scale, out_dtype, slab_pixels):
        xs = _nhwc(x, torch.bfloat16)
        n, cin, h, w = (int(v) for v in xs.shape)
        cout = int(weight.shape[0])
        wd = weight.detach().reshape(cout, cin).contiguous()
        bd = None if bias is None else bias.detach().contiguous()
        y = torch.empty((n, cout, h, w), dtype=out_dtype, device=xs.device)
        _lib.check(_lib.load().cpn_tail_forward(_lib.ptr(xs), _lib.ptr(wd), _dt(wd), _lib.ptr(bd), _dt(bd), _lib.ptr(keep), float(scale),
                                                n, h * w, cin, cout, _lib.ptr(y), _dt(y), _lib.stream_ptr()), 'tail_forward')
        ctx.save_for_backward(xs, weight, keep)
        ctx.scale, ctx.slab_pixels, ctx.x_dtype = scale, slab_pixels, x.dtype
        ctx.bias_dtype = None if bias is None else bias.dtype
        return y

    @staticmethod
    def backward(ctx, grad_output):
        xs, weight, keep = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and ctx.bias_dtype is not None
        dx, dw, db = _tail_backward(xs, grad_output, weight, keep, ctx.scale, ctx.slab_pixels, need_x, need_w, need_b, ctx.bias_dtype)
        return (None if dx is None else dx.to(ctx.x_dtype)), dw, db, None, None, None, None


def _tail_mask(x, p, training, keep):
    """-> (keep as contiguous uint8 [N, Cin] on x's device or None, s)."""
    if not (training and p > 0):
        return None, 1.
    n, cin = int(x.shape[0]), int(x.shape[1])
    if keep is None:
        if p >= 1.:
            keep = torch.zeros((n, cin), dtype=torch.uint8, device=x.device)
        else:
            keep = torch.empty((n, cin, 1, 1), dtype=x.dtype, device=x.device).bernoulli_(1 - p) != 0
    return keep.detach().reshape(n, cin).to(torch.uint8).contiguous(), _tail_scale(p)


def dropout_conv1x1(x, weight, bias=None, p=0., training=False, keep=None, out_dtype=torch.float32, slab_pixels=0):
    """``F.conv2d(F.dropout2d(x, p, training), weight, bias)`` for a 1x1 ``weight`` ``[Cout <= 32, Cin, 1, 1]`` as one autograd
    function, with gradients for ``x``, ``weight`` and ``bias`` as autograd asks for them -> ``[N, Cout, H, W]``, contiguous NCHW,
    in ``out_dtype`` (float32 | bfloat16).  ``dx`` comes in ``x``'s dtype and ``torch.channels_last``, ``dW`` and ``db`` in the
    parameter's dtype.

    ``keep``: bool / uint8 ``[N, Cin]``, the channels kept per image.  When ``training and p > 0`` and ``keep`` is None it is drawn
    as ``torch.empty((N, Cin, 1, 1), dtype=x.dtype, device=x.device).bernoulli_(1 - p)`` from torch's default generator, so it is
    reproducible under ``torch.manual_seed``; ``p == 1`` drops everything without a draw (the output is the bias).  In eval, or
    with ``p == 0``, nothing is dropped, nothing is drawn and ``keep`` is not looked at.  The kept channels are scaled by
    ``1 / (1 - p)`` on the fp32 sum, never on ``x``.  ``slab_pixels``: pixels per slab of the weight gradient's reduction (0:
    chosen by the library).  Anything unsupported raises ``NotImplementedError`` naming the argument; there is no fallback."""
    _check_tail(x, weight, bias, p, keep, out_dtype)
    _need_cuda(x, weight, bias, keep)
    mask, scale = _tail_mask(x, float(p), bool(training), keep)
    return _DropoutConv1x1Function.apply(x, weight, bias, mask, scale, out_dtype, int(slab_pixels))


def dropout_conv1x1_backward(x, grad_output, weight, keep=None, p=0., slab_pixels=0, input_grad=True, weight_grad=True,
                             bias_grad=True, bias_dtype=None):
    """The gradients ``dropout_conv1x1`` returns for an explicit mask, without autograd: (x [N, Cin, H, W], grad_output [N, Cout, H,
    W], weight, keep [N, Cin] | None = all kept, p) -> (dx bf16 in ``torch.channels_last``, dW in ``weight``'s dtype, db in
    ``bias_dtype`` (default: ``weight``'s)), None for a gradient not asked for."""
    _check_tail(x, weight, None, p, keep, torch.float32)
    _need_cuda(x, grad_output, weight, keep)
    mask = None if keep is None else keep.detach().reshape(int(x.shape[0]), int(x.shape[1])).to(torch.uint8).contiguous()
    scale = _tail_scale(float(p)) if mask is not None else 1.
    return _tail_backward(_nhwc(x, torch.bfloat16), grad_output, weight, mask, scale, int(slab_pixels), input_grad, weight_grad,
                          bias_grad, bias_dtype or weight.dtype)


def _tail_unsupported(kernel_size, stride, padding, dilation, groups, in_channels, out_channels, transposed=False):
    """The first argument the ReadOut tail does not run, as a sentence, or None."""
    if transposed:
        return 'transposed convs are not run'
    if _pair(kernel_size) != (1, 1):
        return f'kernel_size {kernel_size}: 1x1 only'
    if groups != 1:
        return f'groups {groups}: dense convs only'
    if _pair(stride) != (1, 1):
        return f'stride {stride}: stride 1 only'
    if _pair(dilation) != (1, 1):
        return f'dilation {dilation}: dilation 1 only'
    if padding not in ('same', 'valid') and (isinstance(padding, str) or _pair(padding) != (0, 0)):
        return f'padding {padding}: no padding only'
    return _tail_channels(in_channels, out_channels)


class DropoutConv1x1(torch.nn.Conv2d):
    """``torch.nn.Conv2d`` (1x1, torch's constructor arguments and parameter names: ``state_dict``s interchange) with the
    ``Dropout2d(p)`` in front of it folded in: its forward is ``dropout_conv1x1(x, weight, bias, p, training)``."""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 padding_mode='zeros', device=None, dtype=None, p=0.):
        why = _tail_unsupported(kernel_size, stride, padding, dilation, groups, in_channels, out_channels)
        if why is not None:
            raise NotImplementedError(why)
        if not 0. <= p <= 1.:
            raise NotImplementedError(f'p {p!r}: a dropout probability in [0, 1]')
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device, dtype)
        self.p = float(p)

    def forward(self, x):
        return dropout_conv1x1(x, self.weight, self.bias, self.p, self.training)

    def extra_repr(self):
        return super().extra_repr() + f', p={self.p}'


def _tail_why_not(conv):
    if type(conv) is not torch.nn.Conv2d:
        return f'a subclass of torch.nn.Conv2d ({type(conv).__name__}): its forward may differ'
    if conv.weight.dtype not in _DTYPES:
        return f'weight dtype {conv.weight.dtype}: float32 or bfloat16 only'
    return _tail_unsupported(conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.in_channels,
                             conv.out_channels, conv.transposed)


def _tail_from_torch(conv, p):
    new = DropoutConv1x1.__new__(DropoutConv1x1)
    new.__dict__.update(conv.__dict__)  # the same Parameter objects, hooks, training flag and constructor attributes
    new._parameters = dict(conv._parameters)  # (the registry itself is the new module's own)
    new.p = float(p)
    return new


def convert_readout_tail_(module):
    """Replaces, in every ``nn.Sequential`` below ``module`` (and ``module`` itself when it is one), each eligible 1x1
    ``torch.nn.Conv2d`` with at most 32 output channels in place by a ``DropoutConv1x1`` that shares its ``Parameter`` objects ->
    (names replaced, {name left: reason}).  Where the slot right in front holds exactly a ``torch.nn.Dropout2d`` and both modules
    occur once in the whole tree, the conv takes its ``p`` and that slot becomes ``torch.nn.Identity()``: indices and ``state_dict``
    keys do not move; otherwise the conv is replaced with ``p = 0``.  ``left`` names every other 1x1 conv (convs this library
    already runs excepted) with the reason.  Works before or after ``convert_conv2d_`` and ``convert_batchnorm2d_``."""
    replaced, left = [], {}
    uses = {}  # slots per Dropout2d or conv object in the whole tree: one that sits in two slots runs twice and is not fused
    for parent in module.modules():
        for child in parent._modules.values():
            if type(child) in (torch.nn.Dropout2d, torch.nn.Conv2d):
                uses[id(child)] = uses.get(id(child), 0) + 1
    if isinstance(module, torch.nn.Conv2d) and not isinstance(module, (Conv2d, DropoutConv1x1, StridedConv1x1, CatConv2d)) and \
            _pair(module.kernel_size) == (1, 1):
        left[''] = _tail_why_not(module) or 'the root module cannot be replaced in place: convert its parent'
    swapped = {}  # id of a replaced conv -> its replacement: a conv in two slots stays one object
    for name, parent in list(module.named_modules()):
        slots = [(n, c) for n, c in parent._modules.items() if c is not None]  # (named_children() drops repeated objects)
        for i, (child_name, child) in enumerate(slots):
            full = f'{name}.{child_name}' if name else child_name
            if not isinstance(child, torch.nn.Conv2d) or isinstance(child, (Conv2d, DropoutConv1x1, StridedConv1x1, CatConv2d)) or \
                    _pair(child.kernel_size) != (1, 1):
                continue
            why = _tail_why_not(child)
            if why is None and not isinstance(parent, torch.nn.Sequential):
                why = f'its parent is a {type(parent).__name__}, not an nn.Sequential'
            if why is not None:
                left[full] = why
                continue
            prev = slots[i - 1] if i > 0 else None
            fuse = prev is not None and type(prev[1]) is torch.nn.Dropout2d and uses.get(id(prev[1])) == 1 and \
                uses.get(id(child)) == 1
            if id(child) not in swapped:
                swapped[id(child)] = _tail_from_torch(child, prev[1].p if fuse else 0.)
            setattr(parent, child_name, swapped[id(child)])
            replaced.append(full)
            if fuse:
                setattr(parent, prev[0], torch.nn.Identity())
    return replaced, left


# ---- the grouped 3x3 conv of a ResNeXt bottleneck block ("Trainable grouped convolution" of include/cpn_hip.h,
# csrc/grouped_conv_train.hip, csrc/grouped_conv.h)
#
# ``conv2`` of every block of a ResNeXt encoder: C -> C channels in groups of ``C / groups`` in {4, 8, 16, 32, 64}, 3x3, padding 1,
# stride 1 or 2.  It runs as ``C / bw`` block-diagonal dense convs ("bundles") of bw = 32 | 64 channels, the geometry of
# ``pack._bundle_geometry``: forward and input gradient are ``cpn_conv2d`` on records packed on the device every step, the weight
# gradient computes the diagonal 32 x 32 fragments only.  Stride 2 goes through zero-dilation: ``dZ[2i][2j] = dY[i][j]``, then the
# stride-1 input and weight gradients of ``dZ`` are those of the strided conv.  Known limit: that does 4 x the minimal work of the
# three strided convs of an encoder and holds one more tensor of ``x``'s size.  ``groups = 1`` with ``C`` = 32 or 64 is the
# one-bundle edge of the family and runs through ``grouped_conv2d``; ``GroupedConv2d`` and ``convert_grouped_conv2d_`` take
# ``groups > 1`` only (dense convs are ``Conv2d``'s).

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
    info = (ctypes.c_int32 * 5)()
    cig = channels // groups if groups > 0 and channels % groups == 0 else 0
    _lib.check(_lib.load().cpn_grouped_conv_wgrad_info(n, h, w, channels, cig, stride, slab_rows, info), 'grouped_conv_wgrad_info')
    return dict(zip(('slabs', 'slab_rows', 'steps', 'reduce_chain', 'bias_chain'), (int(v) for v in info)))


def grouped_conv2d_weight_grad(x, grad_output, groups, stride=1, slab_rows=0, weight=True, bias=True, dtype=torch.float32,
                               bias_dtype=None, dilated=None):
    """(x [N, C, H, W], grad_output [N, C, Hout, Wout]) -> (dW [C, C / groups, 3, 3] | None, db [C] | None): the gradients
    ``grouped_conv2d`` returns for its weight and bias, as fp32 sums over the bf16-rounded operands rounded once to ``dtype`` /
    ``bias_dtype``.  ``slab_rows``: image rows per slab of the reduction (0: chosen by the library); ``dilated``: stride 2, the
    result of ``grouped_dilate(grad_output, (H, W))`` when the caller has it already."""
    _need_cuda(x, grad_output)
    n, c, h, w = (int(v) for v in x.shape)
    bias_dtype = dtype if bias_dtype is None else bias_dtype
    if dtype not in _DTYPES or bias_dtype not in _DTYPES:
        raise NotImplementedError(f'dtype {dtype} / {bias_dtype}: gradients are float32 or bfloat16')
    cig, stride = _grouped_args(c, int(grad_output.shape[1]), stride, groups)
    want = (n, c, (h - 1) // stride + 1, (w - 1) // stride + 1)
    assert tuple(grad_output.shape) == want, (tuple(grad_output.shape), want)
    dw = torch.zeros((c, cig, 3, 3), dtype=dtype, device=x.device) if weight else None
    db = torch.zeros((c,), dtype=bias_dtype, device=x.device) if bias else None
    if n * h * w == 0 or not (weight or bias):
        return dw, db
    xs, gs = _nhwc(x, torch.bfloat16), _nhwc(grad_output, torch.bfloat16)
    dz = gs
    if stride == 2 and weight:
        dz = grouped_dilate(gs, (h, w)) if dilated is None else dilated
    lib = _lib.load()
    nbytes = int(lib.cpn_grouped_conv_wgrad_workspace_bytes(n, h, w, c, cig, stride, slab_rows))
    if nbytes <= 0:
        _lib.check(lib.cpn_grouped_conv_wgrad_info(n, h, w, c, cig, stride, slab_rows, (ctypes.c_int32 * 5)()), 'grouped_conv_wgrad')
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    _lib.check(lib.cpn_grouped_conv_wgrad(_lib.ptr(xs), _lib.ptr(dz), _lib.ptr(gs), n, h, w, c, cig, stride, slab_rows, _lib.ptr(dw),
                                          _DTYPES[dtype], _lib.ptr(db), _DTYPES[bias_dtype], _lib.ptr(ws), nbytes, _lib.stream_ptr()),
               'grouped_conv_wgrad')
    return dw, db


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
    of the supported family (comment above), with gradients for ``x``, ``weight`` and ``bias`` as autograd asks for them -> bf16
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


def _grouped_from_torch(conv):
    new = GroupedConv2d.__new__(GroupedConv2d)
    new.__dict__.update(conv.__dict__)  # the same Parameter objects, hooks, training flag and constructor attributes
    new._parameters = dict(conv._parameters)  # (the registry itself is the new module's own)
    return new


def convert_grouped_conv2d_(module):
    """Replaces every eligible plain ``torch.nn.Conv2d`` with ``groups > 1`` below ``module`` in place by a ``GroupedConv2d`` that
    shares its ``Parameter`` objects (optimisers and ``state_dict`` keys are unaffected) -> (names replaced, {name left: reason}).
    ``left`` names every other grouped conv with the reason; dense convs are not its business.  ``module`` itself is not replaced
    when it is such a conv: it is reported as left.  A conv object that sits in several slots is replaced by one object in all of
    them.  Works before or after the other converts."""
    replaced, left = [], {}
    ours = (Conv2d, DropoutConv1x1, GroupedConv2d, StridedConv1x1, CatConv2d)
    if isinstance(module, torch.nn.Conv2d) and not isinstance(module, ours) and module.groups > 1:
        left[''] = _grouped_why_not(module) or 'the root module cannot be replaced in place: convert its parent'
    swapped = {}  # id of a replaced conv -> its replacement: a conv in two slots stays one object
    for name, parent in list(module.named_modules()):
        slots = [(n, c) for n, c in parent._modules.items() if c is not None]  # (named_children() drops repeated objects)
        for child_name, child in slots:
            full = f'{name}.{child_name}' if name else child_name
            if not isinstance(child, torch.nn.Conv2d) or isinstance(child, ours) or child.groups <= 1:
                continue
            why = _grouped_why_not(child)
            if why is not None:
                left[full] = why
                continue
            if id(child) not in swapped:
                swapped[id(child)] = _grouped_from_torch(child)
            setattr(parent, child_name, swapped[id(child)])
            replaced.append(full)
    return replaced, left


# ---- the bottleneck block of a ResNeXt encoder ("Trainable bottleneck block" of include/cpn_hip.h)
#
# Three pieces beside the convs and norms above make a whole block run here: the norm's residual tail (``batch_norm(...,
# residual=)``), the strided 1x1 shortcut conv of a stage entry (``strided_conv1x1``) and the block-input gradient in the epilogue of
# conv1's dgrad conv (``conv2d_fork``).  ``Bottleneck`` puts them together, ``convert_bottleneck_`` swaps eligible blocks in place.

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


def _strided_from_torch(conv):
    new = StridedConv1x1.__new__(StridedConv1x1)
    new.__dict__.update(conv.__dict__)  # the same Parameter objects, hooks, training flag and constructor attributes
    new._parameters = dict(conv._parameters)  # (the registry itself is the new module's own)
    return new


class Bottleneck(torch.nn.Module):
    """The bottleneck block of a ResNet / ResNeXt encoder under torchvision's child names (``conv1``, ``bn1``, ``conv2``, ``bn2``,
    ``conv3``, ``bn3``, ``relu``, ``downsample``: ``state_dict`` keys do not move), made of this module's pieces::

        h, skip = conv1(x, fork=True)
        h = bn1(h, activation='relu');  h = bn2(conv2(h), activation='relu');  h = conv3(h)
        return bn3(h, residual=skip if downsample is None else downsample(skip), activation='relu')

    ``conv1`` / ``conv3``: ``Conv2d`` (1x1); ``conv2``: ``GroupedConv2d`` or a 3x3 ``Conv2d``; the norms: ``BatchNorm2d``;
    ``downsample``: None or ``Sequential(Conv2d | StridedConv1x1, BatchNorm2d)``.  ``relu`` is kept for its name only: the three
    ReLUs run inside the norms.  Forward hooks on the children fire.  The output is saved by ``bn3``'s backward: an in-place
    operation on it makes autograd raise."""

    def __init__(self, conv1, bn1, conv2, bn2, conv3, bn3, downsample=None):
        super().__init__()
        self.conv1, self.bn1, self.conv2, self.bn2, self.conv3, self.bn3 = conv1, bn1, conv2, bn2, conv3, bn3
        self.relu = torch.nn.ReLU(inplace=True)
        self.downsample = downsample
        why = _block_why_not(self, converted=True)
        if why is not None:
            raise NotImplementedError(why)

    def forward(self, x):
        h, skip = self.conv1(x, fork=True)
        h = self.bn1(h, activation='relu')
        h = self.bn2(self.conv2(h), activation='relu')
        h = self.conv3(h)
        return self.bn3(h, residual=skip if self.downsample is None else self.downsample(skip), activation='relu')


_BLOCK_CHILDREN = ('conv1', 'bn1', 'conv2', 'bn2', 'conv3', 'bn3', 'relu', 'downsample')


def _is_torchvision_bottleneck(cls):
    """Whether the class's forward IS torchvision's ``Bottleneck.forward`` (told by its names: torchvision is not imported)."""
    f = getattr(cls, 'forward', None)
    return getattr(f, '__module__', None) == 'torchvision.models.resnet' and getattr(f, '__qualname__', None) == 'Bottleneck.forward'


def _pointwise_why_not(conv, converted):
    """conv1 / conv3: a 1x1 conv of ``conv2d``'s family."""
    if isinstance(conv, Conv2d):
        return None if _pair(conv.kernel_size) == (1, 1) else f'kernel_size {conv.kernel_size}: 1x1 only'
    if converted or not isinstance(conv, torch.nn.Conv2d):
        return f'{type(conv).__name__}: not a Conv2d of this library' if converted else f'{type(conv).__name__}: not a torch.nn.Conv2d'
    if _pair(conv.kernel_size) != (1, 1):
        return f'kernel_size {conv.kernel_size}: 1x1 only'
    return _why_not(conv)


def _conv2_why_not(conv, converted):
    """conv2: ``grouped_conv2d``'s family (stride 1 or 2) or a dense 3x3 stride-1 conv of ``conv2d``'s."""
    if isinstance(conv, GroupedConv2d):
        return None
    if isinstance(conv, Conv2d):
        return None if _pair(conv.kernel_size) == (3, 3) else f'kernel_size {conv.kernel_size}: 3x3 only'
    if converted or not isinstance(conv, torch.nn.Conv2d):
        return f'{type(conv).__name__}: not a conv of this library' if converted else f'{type(conv).__name__}: not a torch.nn.Conv2d'
    if _pair(conv.kernel_size) != (3, 3):
        return f'kernel_size {conv.kernel_size}: 3x3 only'
    return _grouped_why_not(conv) if conv.groups > 1 else _why_not(conv)


def _norm_why_not(bn, converted):
    if isinstance(bn, BatchNorm2d):
        return None
    if converted:
        return f'{type(bn).__name__}: not a BatchNorm2d of this library'
    return _bn_why_not(bn)


def _shortcut_why_not(conv, converted):
    """downsample.0: a 1x1 conv without padding, of stride 1 (``conv2d``'s family) or 2 (``strided_conv1x1``'s)."""
    if isinstance(conv, StridedConv1x1):
        return None
    if isinstance(conv, Conv2d):
        return None if _pair(conv.kernel_size) == (1, 1) else f'kernel_size {conv.kernel_size}: 1x1 only'
    if converted or not isinstance(conv, torch.nn.Conv2d):
        return f'{type(conv).__name__}: not a conv of this library' if converted else f'{type(conv).__name__}: not a torch.nn.Conv2d'
    if _pair(conv.kernel_size) != (1, 1):
        return f'kernel_size {conv.kernel_size}: 1x1 only'
    return _strided_why_not(conv) if _pair(conv.stride) != (1, 1) else _why_not(conv)


def _block_why_not(block, converted=False):
    """The first child that keeps a block out of ``Bottleneck``, as ``'<attribute>: <reason>'``, or None.  ``converted``: the
    children must be this library's modules already."""
    for name in _BLOCK_CHILDREN:
        if not hasattr(block, name):
            return f'{name}: the block has no such attribute'
    for name, check in (('conv1', _pointwise_why_not), ('bn1', _norm_why_not), ('conv2', _conv2_why_not), ('bn2', _norm_why_not),
                        ('conv3', _pointwise_why_not), ('bn3', _norm_why_not)):
        why = check(getattr(block, name), converted)
        if why is not None:
            return f'{name}: {why}'
    if type(block.relu) is not torch.nn.ReLU:
        return f'relu: {type(block.relu).__name__}: torch.nn.ReLU itself only'
    down = block.downsample
    if down is not None:
        if type(down) is not torch.nn.Sequential or len(down) != 2:
            inside = ', '.join(type(m).__name__ for m in down) if isinstance(down, torch.nn.Sequential) else type(down).__name__
            return f'downsample: ({inside}): None or Sequential(1x1 conv, BatchNorm2d) only'
        why = _shortcut_why_not(down[0], converted)
        if why is not None:
            return f'downsample.0: {why}'
        why = _norm_why_not(down[1], converted)
        if why is not None:
            return f'downsample.1: {why}'
    # the channel counts and the stride must fit together, or the residual add has no meaning
    cin, mid, cout = block.conv1.in_channels, block.conv1.out_channels, block.conv3.out_channels
    stride = _pair(block.conv2.stride)
    if (block.conv2.in_channels, block.conv2.out_channels, block.conv3.in_channels) != (mid, mid, mid):
        return f'conv2: {block.conv2.in_channels} -> {block.conv2.out_channels} channels between conv1 (-> {mid}) and conv3 ' \
               f'({block.conv3.in_channels} ->)'
    for name, bn, c in (('bn1', block.bn1, mid), ('bn2', block.bn2, mid), ('bn3', block.bn3, cout)):
        if bn.num_features != c:
            return f'{name}: num_features {bn.num_features} behind a conv of {c} channels'
    if down is None:
        if stride != (1, 1) or cin != cout:
            return f'downsample: None with stride {stride} and {cin} -> {cout} channels: the identity shortcut needs stride 1 and ' \
                   f'equal channel counts'
    else:
        if _pair(down[0].stride) != stride or (down[0].in_channels, down[0].out_channels) != (cin, cout) or down[1].num_features != cout:
            return f'downsample.0: {down[0].in_channels} -> {down[0].out_channels} channels at stride {down[0].stride} beside a ' \
                   f'block of {cin} -> {cout} channels at stride {stride}'
    return None


def _convert_child(child):
    """A stock child of an eligible block -> this library's module sharing its Parameter and buffer objects."""
    if isinstance(child, (Conv2d, GroupedConv2d, StridedConv1x1, BatchNorm2d)):
        return child
    if isinstance(child, torch.nn.BatchNorm2d):
        return _bn_from_torch(child, None)
    if child.groups > 1:
        return _grouped_from_torch(child)
    return _strided_from_torch(child) if _pair(child.stride) != (1, 1) else _from_torch(child)


def _block_from_torch(block):
    new = Bottleneck.__new__(Bottleneck)
    new.__dict__.update(block.__dict__)  # hooks, training flag and the block's own attributes (stride, ...)
    new._modules, new._parameters, new._buffers = dict(block._modules), dict(block._parameters), dict(block._buffers)
    for name in ('conv1', 'bn1', 'conv2', 'bn2', 'conv3', 'bn3'):
        setattr(new, name, _convert_child(getattr(block, name)))
    if block.downsample is not None:  # the Sequential stays the object it is: its two slots are filled anew
        block.downsample[0], block.downsample[1] = _convert_child(block.downsample[0]), _convert_child(block.downsample[1])
    return new


def convert_bottleneck_(module, block_types=()):
    """Replaces every eligible bottleneck block below ``module`` in place by a ``Bottleneck`` -> (names replaced, {name left:
    reason}).  A module is a candidate when its class's ``forward`` is torchvision's ``Bottleneck.forward`` (a class that assigns
    that very function qualifies; one that merely has the same attribute names does not) or when its class is listed in
    ``block_types``.  Eligible: ``conv1`` / ``conv3`` of ``conv2d``'s family, ``conv2`` of ``grouped_conv2d``'s (stride 1 or 2) or a
    dense 3x3 stride-1 conv, the norms of ``batch_norm``'s, ``relu`` exactly ``torch.nn.ReLU``, ``downsample`` None or
    ``Sequential(1x1 conv of stride 1 | 2 without padding, BatchNorm2d)``; the children may be stock or already converted by the
    other converts, in any order: the result is the same, and ``Parameter`` and buffer objects are shared.  Everything else is left
    with a reason naming the attribute; a block object that sits in two slots is left.  ``module`` itself is not replaced when it is
    a candidate: it is reported as left.  The other converts, run afterwards, leave a converted block alone."""
    block_types = tuple(block_types)
    replaced, left = [], {}

    def candidate(m):
        return not isinstance(m, Bottleneck) and (_is_torchvision_bottleneck(type(m)) or type(m) in block_types)

    if candidate(module):
        left[''] = _block_why_not(module) or 'the root module cannot be replaced in place: convert its parent'
    uses = {}  # slots per candidate object in the whole tree: one that sits in two slots runs twice on different inputs
    for parent in module.modules():
        for child in parent._modules.values():
            if child is not None and candidate(child):
                uses[id(child)] = uses.get(id(child), 0) + 1
    for name, parent in list(module.named_modules()):
        for child_name, child in [(n, c) for n, c in parent._modules.items() if c is not None]:
            if not candidate(child):
                continue
            full = f'{name}.{child_name}' if name else child_name
            why = _block_why_not(child)
            if why is None and uses[id(child)] > 1:
                why = f'the block sits in {uses[id(child)]} slots'
            if why is not None:
                left[full] = why
                continue
            setattr(parent, child_name, _block_from_torch(child))
            replaced.append(full)
    return replaced, left


# ---- the first conv of a U-Net decoder level: nearest resize + concat + conv ("Trainable concat convolution" of
# include/cpn_hip.h, csrc/cat_conv_train.hip, csrc/nearest_adjoint.h)
#
# Every level of the reference decoder runs its block on ``cat((lateral, interpolate(top, size=lateral.shape[2:])), 1)``.  Stock torch
# writes the resized and the concatenated tensor and saves the latter; ``cat_conv2d`` reads both sources in the conv's loader and in
# the weight gradient's staging, and saves the lateral and the low-resolution top only.  The input gradient is two dgrad convs
# (one per source, each run only when asked for); the top's goes through the adjoint of the resize, ``nearest_resize_backward``.
# ``UNetDecoder`` also applies the level's 1x1 ``inner`` conv BEFORE the resize (per pixel the same bits, at the low resolution).
# Known limits: the top's gradient at the lateral's size (``T``) is written and read once; the forward is not decomposed into
# sub-pixel phases.

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
    info = (ctypes.c_int32 * 5)()
    _lib.check(_lib.load().cpn_cat_conv_wgrad_info(n, h, w, c0, c1, int(top_size[0]), int(top_size[1]), cout, k, slab_rows, info),
               'cat_conv_wgrad_info')
    return dict(zip(('slabs', 'slab_rows', 'steps', 'reduce_chain', 'bias_chain'), (int(v) for v in info)))


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
    bias_dtype = dtype if bias_dtype is None else bias_dtype
    if dtype not in _DTYPES or bias_dtype not in _DTYPES:
        raise NotImplementedError(f'dtype {dtype} / {bias_dtype}: gradients are float32 or bfloat16')
    assert int(grad_output.shape[0]) == n and (lateral is None or tuple(lateral.shape) == (n, c0, h, w)) and \
        (lateral is not None or (h, w) == (2 * h1, 2 * w1)), (tuple(grad_output.shape), tuple(top.shape))
    if not (weight or bias):
        return None, None
    dw = torch.empty((cout, c0 + c1, k, k), dtype=dtype, device=top.device) if weight else None
    db = torch.empty((cout,), dtype=bias_dtype, device=top.device) if bias else None
    ls = None if lateral is None else _nhwc(lateral, torch.bfloat16)
    ts, gs = _nhwc(top, torch.bfloat16), _nhwc(grad_output, torch.bfloat16)
    lib = _lib.load()
    nbytes = int(lib.cpn_cat_conv_wgrad_workspace_bytes(n, h, w, c0, c1, h1, w1, cout, k, slab_rows))
    if nbytes <= 0:
        _lib.check(lib.cpn_cat_conv_wgrad_info(n, h, w, c0, c1, h1, w1, cout, k, slab_rows, (ctypes.c_int32 * 5)()), 'cat_conv_wgrad')
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=top.device)
    _lib.check(lib.cpn_cat_conv_wgrad(_lib.ptr(ls), _lib.ptr(ts), _lib.ptr(gs), n, h, w, c0, c1, h1, w1, cout, k, slab_rows, _lib.ptr(dw),
                                      _DTYPES[dtype], _lib.ptr(db), _DTYPES[bias_dtype], _lib.ptr(ws), nbytes, _lib.stream_ptr()),
               'cat_conv_wgrad')
    return dw, db


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


def _cat_from_torch(conv):
    new = CatConv2d.__new__(CatConv2d)
    new.__dict__.update(conv.__dict__)  # the same Parameter objects, hooks, training flag and constructor attributes
    new._parameters = dict(conv._parameters)  # (the registry itself is the new module's own)
    return new


def _is_reference_unet(cls):
    """Whether the class's forward IS the reference's ``GeneralizedUNet.forward`` (told by its names: the reference is not imported)."""
    f = getattr(cls, 'forward', None)
    return getattr(f, '__module__', None) == 'celldetection.models.unet' and getattr(f, '__qualname__', None) == 'GeneralizedUNet.forward'


_DECODER_FLAGS = ('block_cat', 'block_interpolate', 'bridge_block_interpolate')
_DECODER_ATTRIBUTES = ('inner_blocks', 'layer_blocks', 'has_lat', 'bridges', 'interpolate', 'cat_order') + _DECODER_FLAGS + \
    ('extra_blocks', 'out_layer', 'final_interpolate', 'final_activation', 'keep_features', 'features_prefix')


def _slot0_why_not(conv, converted):
    """Slot 0 of a layer block: a stride-1 conv of ``conv2d``'s family, stock or this library's."""
    if isinstance(conv, (CatConv2d, Conv2d)):
        return None if not converted or isinstance(conv, CatConv2d) else f'{type(conv).__name__}: not a CatConv2d'
    if converted or not isinstance(conv, torch.nn.Conv2d):
        return f'{type(conv).__name__}: not a CatConv2d' if converted else f'{type(conv).__name__}: not a torch.nn.Conv2d'
    return _why_not(conv)


def _decoder_why_not(dec, converted=False):
    """The first attribute that keeps a decoder out of ``UNetDecoder``, as ``'<attribute>: <reason>'``, or None.  ``converted``:
    slot 0 of every layer block must be a ``CatConv2d`` and every inner conv a ``Conv2d`` of this library already."""
    for name in _DECODER_ATTRIBUTES:
        if not hasattr(dec, name):
            return f'{name}: the decoder has no such attribute'
    if dec.interpolate != 'nearest':
        return f"interpolate: {dec.interpolate!r}: 'nearest' only"
    if dec.cat_order != 0:
        return f'cat_order: {dec.cat_order}: 0 (the lateral first) only'
    for name in _DECODER_FLAGS:
        if getattr(dec, name):
            return f'{name}: {getattr(dec, name)!r}: the block must not resize or concatenate itself'
    if dec.extra_blocks is not None:
        return f'extra_blocks: {type(dec.extra_blocks).__name__}: None only'
    inner, layers = dec.inner_blocks, dec.layer_blocks
    if not isinstance(inner, torch.nn.ModuleList) or not isinstance(layers, torch.nn.ModuleList) or len(inner) != len(layers) or \
            len(layers) < 1:
        return f'layer_blocks: {len(layers) if hasattr(layers, "__len__") else "?"} blocks beside ' \
               f'{len(inner) if hasattr(inner, "__len__") else "?"} inner blocks: two ModuleLists of one length >= 1'
    try:
        [dec.has_lat[i] for i in range(len(layers))]
    except (KeyError, IndexError, TypeError):
        return f'has_lat: {dec.has_lat!r}: one entry per level 0 ... {len(layers) - 1}'
    top_channels = None  # of the deepest level: the encoder's, not known here
    for i in range(len(layers) - 1, -1, -1):
        m = inner[i]
        if type(m) is not torch.nn.Identity:
            why = _pointwise_why_not(m, converted)
            if why is not None:
                return f'inner_blocks.{i}: {why}'
            if top_channels is not None and m.in_channels != top_channels:
                return f'inner_blocks.{i}: in_channels {m.in_channels} behind a level of {top_channels} channels'
            top_channels = m.out_channels
        block = layers[i]
        # (the reference's TwoConvNormRelu IS such a subclass: nn.Sequential with a constructor and no forward of its own)
        if not isinstance(block, torch.nn.Sequential) or type(block).forward is not torch.nn.Sequential.forward or len(block) < 1:
            return f'layer_blocks.{i}: {type(block).__name__}: an nn.Sequential (or a subclass that keeps its forward) with the conv ' \
                   f'in slot 0 only'
        conv = block[0]
        why = _slot0_why_not(conv, converted)
        if why is not None:
            return f'layer_blocks.{i}.0: {why}'
        if top_channels is not None:
            lateral = conv.in_channels - top_channels
            if dec.has_lat[i] and (lateral < 32 or lateral % 32):
                return f'layer_blocks.{i}.0: in_channels {conv.in_channels} = {lateral} lateral + {top_channels} top channels: the ' \
                       f'lateral needs a positive multiple of 32'
            if not dec.has_lat[i] and lateral != 0:
                return f'layer_blocks.{i}.0: in_channels {conv.in_channels} on a bridge level whose top has {top_channels} channels'
        elif dec.has_lat[i] and conv.in_channels < 64:
            return f'layer_blocks.{i}.0: in_channels {conv.in_channels}: lateral + top need at least 32 + 32 channels'
        outs = [m.out_channels for m in block if isinstance(m, torch.nn.modules.conv._ConvNd)]
        top_channels = outs[-1]
    return None


class UNetDecoder(torch.nn.Module):
    """The reference's ``GeneralizedUNet`` decoder (default path: nearest resize, the lateral first in the concat) on this library's
    pieces, under the reference's child names ``inner_blocks`` and ``layer_blocks`` (``state_dict`` keys do not move)::

        for i in levels, deepest first:
            top  = inner_blocks[i](last)                                  # the 1x1 conv BEFORE the resize; Identity stays Identity
            h    = layer_blocks[i][0](lateral if has_lat[i] else None, top)    # CatConv2d: resize + concat + conv in one function
            last = layer_blocks[i][1:](h)                                 # the remaining slots, in order

    The reference resizes first and applies the inner conv at the lateral's size; a 1x1 conv commutes with the nearest resize pixel
    by pixel, so the values are the same at a quarter of the work.  The tail -- the final bilinear resize to ``size``, ``out_layer``,
    ``final_activation``, the result dict with ``'out'`` and the ``encoder.*`` keys of ``keep_features`` -- is the reference's, in
    stock torch ops.  ``has_lat``: per level, whether it has a lateral (False: a bridge level, resized by exactly 2);
    ``bridges``: the number of bridge levels.  Forward hooks on a level's children (the convs, the norms) fire; hooks on a level's
    ``Sequential`` itself do not, because its slots are called one by one."""

    def __init__(self, inner_blocks, layer_blocks, has_lat, bridges=0, out_layer=None, final_activation=None,
                 final_interpolate='bilinear', keep_features=True, features_prefix='encoder'):
        super().__init__()
        self.inner_blocks, self.layer_blocks = inner_blocks, layer_blocks
        self.has_lat = dict(has_lat) if isinstance(has_lat, dict) else dict(enumerate(has_lat))
        self.bridges = int(bridges)
        self.interpolate, self.cat_order = 'nearest', 0
        self.block_cat = self.block_interpolate = self.bridge_block_interpolate = False
        self.extra_blocks = None
        self.out_layer, self.final_activation, self.final_interpolate = out_layer, final_activation, final_interpolate
        self.keep_features, self.features_prefix = keep_features, features_prefix
        why = _decoder_why_not(self, converted=True)
        if why is not None:
            raise NotImplementedError(why)

    @property
    def depth(self):
        return len(self.layer_blocks)

    def forward(self, x, size=None):
        features = x
        names = list(x.keys())
        x = list(x.values())
        last = x[-1]
        results = [last]
        for i in range(len(self.layer_blocks) - 1, -1, -1):
            lateral = x[i - self.bridges] if self.has_lat[i] else None
            top = self.inner_blocks[i](last)
            slots = list(self.layer_blocks[i])
            last = slots[0](lateral, top)
            for m in slots[1:]:
                last = m(last)
            results.insert(0, last)
        if size is None:
            final = results[0]
        else:
            final = torch.nn.functional.interpolate(last, size=size, mode=self.final_interpolate, align_corners=False)
        if self.out_layer is not None:
            final = self.out_layer(final)
        if self.final_activation is not None:
            final = self.final_activation(final)
        if self.out_layer is not None:
            return final
        results.insert(0, final)
        names.insert(0, 'out')
        out = dict(zip(names, results))
        if self.keep_features:
            out.update(('.'.join([self.features_prefix, k]), v) for k, v in features.items())
        return out


def _decoder_from_torch(dec):
    new = UNetDecoder.__new__(UNetDecoder)
    new.__dict__.update(dec.__dict__)  # hooks, training flag and the decoder's own attributes (has_lat, bridges, out_channels, ...)
    new._modules, new._parameters, new._buffers = dict(dec._modules), dict(dec._parameters), dict(dec._buffers)
    for i, m in enumerate(dec.inner_blocks):  # the ModuleLists and Sequentials stay the objects they are: their slots are filled anew
        if type(m) is torch.nn.Conv2d:
            dec.inner_blocks[i] = _from_torch(m)
    for block in dec.layer_blocks:
        if not isinstance(block[0], CatConv2d):
            block[0] = _cat_from_torch(block[0])
    return new


def convert_unet_decoder_(module, decoder_types=()):
    """Replaces every eligible U-Net decoder below ``module`` in place by a ``UNetDecoder`` -> (names replaced, {name left:
    reason}).  A module is a candidate when its class's ``forward`` is the reference's ``GeneralizedUNet.forward`` (told by the names
    ``celldetection.models.unet`` / ``GeneralizedUNet.forward``; a class that merely has the same attributes does not qualify) or
    when its class is listed in ``decoder_types``.  Eligible: ``interpolate == 'nearest'``, ``cat_order == 0``, ``block_cat``,
    ``block_interpolate`` and ``bridge_block_interpolate`` all false, ``extra_blocks is None``, every inner block ``Identity`` or a
    1x1 conv of ``conv2d``'s family, every layer block an ``nn.Sequential`` -- itself or a subclass that does not override ``forward``, as the reference's
    ``TwoConvNormRelu`` is; its slots are called one by one -- whose slot 0 is a stride-1 conv of that family with
    ``in_channels`` = lateral + top channels (= top on a bridge level).  Slot 0 becomes a ``CatConv2d`` and a stock inner conv a
    ``Conv2d``, stock or already converted by the other converts, in any order: the result is the same, and ``Parameter`` objects are
    shared.  Everything else is left with a reason naming the attribute; a decoder object that sits in two slots is left.
    ``module`` itself is not replaced when it is a candidate: it is reported as left.  The other converts, run afterwards, take the
    remaining slots of the levels and leave the ``CatConv2d`` alone."""
    decoder_types = tuple(decoder_types)
    replaced, left = [], {}

    def candidate(m):
        return not isinstance(m, UNetDecoder) and (_is_reference_unet(type(m)) or type(m) in decoder_types)

    if candidate(module):
        left[''] = _decoder_why_not(module) or 'the root module cannot be replaced in place: convert its parent'
    uses = {}
    for parent in module.modules():
        for child in parent._modules.values():
            if child is not None and candidate(child):
                uses[id(child)] = uses.get(id(child), 0) + 1
    for name, parent in list(module.named_modules()):
        for child_name, child in [(n, c) for n, c in parent._modules.items() if c is not None]:
            if not candidate(child):
                continue
            full = f'{name}.{child_name}' if name else child_name
            why = _decoder_why_not(child)
            if why is None and uses[id(child)] > 1:
                why = f'the decoder sits in {uses[id(child)]} slots'
            if why is not None:
                left[full] = why
                continue
            setattr(parent, child_name, _decoder_from_torch(child))
            replaced.append(full)
    return replaced, left


# ---- the stem of a ResNet encoder and the max-pool ("Trainable stem and max-pool" of include/cpn_hip.h, csrc/stem_train.hip,
# csrc/pool_adjoint.h)
#
# The first two modules a step runs: ``Conv2d(in_channels <= 4, 64, 7, stride=2, padding=3)`` and ``MaxPool2d(3, 2, 1)`` (the
# reference's ``models/resnet.py:274-284``), and the ``MaxPool2d(2, 2)`` of the U-Net encoders.  ``stem_conv2d`` converts the image
# to the padded 4-channel bf16 layout of the inference stem (csrc/stem.hip), in which the 7 taps of a filter row are contiguous,
# and saves that tensor alone; the weight gradient is seven MFMA products per slab, one per filter row, with the flat output pixel as
# the reduction index.  The image gets no gradient.  ``max_pool2d`` stores one ``uint8`` tap index per output element and saves
# nothing else; its backward is a gather in a fixed order (no atomics, no scatter).

STEM_OUT_CHANNELS = (32, 64)
STEM_MAX_IN_CHANNELS = 4
POOL_GEOMETRIES = ((3, 2, 1), (2, 2, 0))


def _stem_unsupported(kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels, transposed=False):
    """The first argument the trainable stem does not run, as a sentence, or None."""
    if transposed:
        return 'transposed convs are not run'
    if _pair(kernel_size) != (7, 7):
        return f'kernel_size {kernel_size}: 7x7 only'
    if _pair(stride) != (2, 2):
        return f'stride {stride}: stride 2 only'
    if isinstance(padding, str) or _pair(padding) != (3, 3):
        return f'padding {padding}: 3 zeros only'
    if _pair(dilation) != (1, 1):
        return f'dilation {dilation}: dilation 1 only'
    if groups != 1:
        return f'groups {groups}: dense convs only'
    if padding_mode != 'zeros':
        return f"padding_mode '{padding_mode}': zeros only"
    if not 1 <= in_channels <= STEM_MAX_IN_CHANNELS:
        return f'in_channels {in_channels}: 1 ... {STEM_MAX_IN_CHANNELS} only'
    if out_channels not in STEM_OUT_CHANNELS:
        return f'out_channels {out_channels}: {STEM_OUT_CHANNELS} only'
    return None


def _check_stem_weight(weight):
    if weight.dim() != 4:
        raise NotImplementedError(f'weight of {weight.dim()} dimensions: the trainable stem needs [Cout, C, 7, 7]')
    if tuple(weight.shape[2:]) != (7, 7):
        raise NotImplementedError(f'kernel_size {tuple(weight.shape[2:])}: the trainable stem runs 7x7 kernels only')
    if weight.dtype not in _DTYPES:
        raise NotImplementedError(f'weight dtype {weight.dtype}: the trainable stem takes float32 or bfloat16 parameters')
    if not 1 <= int(weight.shape[1]) <= STEM_MAX_IN_CHANNELS:
        raise NotImplementedError(f'in_channels {int(weight.shape[1])}: the trainable stem takes 1 ... {STEM_MAX_IN_CHANNELS}')
    if int(weight.shape[0]) not in STEM_OUT_CHANNELS:
        raise NotImplementedError(f'out_channels {int(weight.shape[0])}: the trainable stem writes {STEM_OUT_CHANNELS} only')


def _check_stem_input(x):
    if x.dim() != 4:
        raise NotImplementedError(f'input of {x.dim()} dimensions: the trainable stem takes a 4-D [N, C, H, W] input')
    if x.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {x.dtype}: the trainable stem takes float32 or bfloat16 images')
    if not 1 <= int(x.shape[1]) <= STEM_MAX_IN_CHANNELS:
        raise NotImplementedError(f'input of {int(x.shape[1])} channels: the trainable stem takes 1 ... {STEM_MAX_IN_CHANNELS}')
    if min(int(v) for v in x.shape) < 1:
        raise NotImplementedError(f'input of size {tuple(x.shape)}: the trainable stem needs at least one pixel')


def stem_pack_weight(weight):
    """weight [Cout, C, 7, 7] (float32 | bfloat16, on the GPU) -> the bf16 records [7][Cout][32] the stem loop reads, packed on the
    device: filter row, output channel, (kx 0..7, c 0..3) with zeros at kx = 7 and c >= C."""
    _check_stem_weight(weight)
    _need_cuda(weight)
    w = weight.detach().contiguous()
    cout, c = int(w.shape[0]), int(w.shape[1])
    packed = torch.empty((7, cout, 32), dtype=torch.bfloat16, device=w.device)
    _lib.check(_lib.load().cpn_stem_train_pack(_lib.ptr(w), _DTYPES[w.dtype], cout, c, _lib.ptr(packed), _lib.stream_ptr()),
               'stem_train_pack')
    return packed


def _stem_pad(x):
    """x [N, C <= 4, H, W] -> the padded input bf16 [N, H + 6, W + 8, 4] (zero border, zeros in the channels >= C)."""
    n, c, h, w = (int(v) for v in x.shape)
    src = x.detach().float().contiguous()  # (bf16 -> fp32 is exact; the kernel rounds fp32 to bf16, to nearest even)
    xp = torch.empty((n, h + 6, w + 8, 4), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.load().cpn_convert_input_stem(_lib.ptr(src), 0, _lib.ptr(xp), n, c, h, w, None, _lib.stream_ptr()),
               'convert_input_stem')
    return xp


def _stem_forward(xp, size, packed, bias):
    n, h, w = size
    cout = int(packed.shape[1])
    out = torch.empty((n, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=torch.bfloat16, device=xp.device,
                      memory_format=torch.channels_last)
    _lib.check(_lib.load().cpn_stem_train_forward(_lib.ptr(xp), _lib.ptr(packed), _lib.ptr(bias), n, h, w, cout, _lib.ptr(out),
                                                  _lib.stream_ptr()), 'stem_train_forward')
    return out


def stem_weight_grad_info(n, h, w, cout, slab_rows=0):
    """What ``stem_weight_grad`` would run on an ``h x w`` image -> dict(slabs, slab_rows (output rows per slab), steps (MFMA steps
    per slab), reduce_chain, bias_chain).  Host arithmetic only: needs no GPU.  Raises like the launch for a call it rejects."""
    info = (ctypes.c_int32 * 5)()
    _lib.check(_lib.load().cpn_stem_wgrad_info(n, h, w, cout, slab_rows, info), 'stem_wgrad_info')
    return dict(zip(('slabs', 'slab_rows', 'steps', 'reduce_chain', 'bias_chain'), (int(v) for v in info)))


def _stem_wgrad(xp, size, c, gs, slab_rows, weight, bias, dtype, bias_dtype):
    """xp: the padded input; gs: bf16 NHWC memory, 16-byte aligned -> (dW | None, db | None)."""
    n, h, w = size
    cout = int(gs.shape[1])
    dw = torch.zeros((cout, c, 7, 7), dtype=dtype, device=xp.device) if weight else None
    db = torch.zeros((cout,), dtype=bias_dtype, device=xp.device) if bias else None
    if not (weight or bias):
        return dw, db
    lib = _lib.load()
    nbytes = int(lib.cpn_stem_wgrad_workspace_bytes(n, h, w, cout, slab_rows))
    if nbytes <= 0:
        _lib.check(lib.cpn_stem_wgrad_info(n, h, w, cout, slab_rows, (ctypes.c_int32 * 5)()), 'stem_wgrad')
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=xp.device)
    _lib.check(lib.cpn_stem_wgrad(_lib.ptr(xp), _lib.ptr(gs), n, h, w, c, cout, slab_rows, _lib.ptr(dw), _DTYPES[dtype], _lib.ptr(db),
                                  _DTYPES[bias_dtype], _lib.ptr(ws), nbytes, _lib.stream_ptr()), 'stem_wgrad')
    return dw, db


def stem_weight_grad(x, grad_output, slab_rows=0, weight=True, bias=True, dtype=torch.float32, bias_dtype=None):
    """(x [N, C <= 4, H, W], grad_output [N, Cout, Hout, Wout]) -> (dW [Cout, C, 7, 7] | None, db [Cout] | None): the gradients
    ``stem_conv2d`` returns for its weight and bias, as fp32 sums over the bf16-rounded operands rounded once to ``dtype`` /
    ``bias_dtype``.  ``slab_rows``: output rows per slab of the reduction (0: chosen by the library)."""
    _check_stem_input(x)
    n, c, h, w = (int(v) for v in x.shape)
    cout = int(grad_output.shape[1])
    if cout not in STEM_OUT_CHANNELS:
        raise NotImplementedError(f'out_channels {cout}: the trainable stem writes {STEM_OUT_CHANNELS} only')
    bias_dtype = dtype if bias_dtype is None else bias_dtype
    if dtype not in _DTYPES or bias_dtype not in _DTYPES:
        raise NotImplementedError(f'dtype {dtype} / {bias_dtype}: gradients are float32 or bfloat16')
    want = (n, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
    assert tuple(grad_output.shape) == want, (tuple(grad_output.shape), want)
    _need_cuda(x, grad_output)
    return _stem_wgrad(_stem_pad(x), (n, h, w), c, _nhwc(grad_output, torch.bfloat16), slab_rows, weight, bias, dtype, bias_dtype)


class _StemConv2dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        n, c, h, w = (int(v) for v in x.shape)
        xp = _stem_pad(x)
        b32 = None if bias is None else bias.detach().float().contiguous()
        out = _stem_forward(xp, (n, h, w), stem_pack_weight(weight), b32)
        ctx.save_for_backward(xp)  # the padded bf16 input alone: neither x nor the weight is needed again
        ctx.size, ctx.c = (n, h, w), c
        ctx.weight_dtype = weight.dtype
        ctx.bias_dtype = None if bias is None else bias.dtype
        return out

    @staticmethod
    def backward(ctx, grad_output):
        xp, = ctx.saved_tensors
        _, need_w, need_b = ctx.needs_input_grad
        need_b = need_b and ctx.bias_dtype is not None
        dw = db = None
        if need_w or need_b:
            dw, db = _stem_wgrad(xp, ctx.size, ctx.c, _nhwc(grad_output, torch.bfloat16), 0, need_w, need_b, ctx.weight_dtype,
                                 ctx.bias_dtype or ctx.weight_dtype)
        return None, dw, db


def stem_conv2d(x, weight, bias=None):
    """``torch.nn.functional.conv2d(x, weight, bias, stride=2, padding=3)`` for a 7x7 ``weight [Cout in {32, 64}, C <= 4, 7, 7]`` ->
    bf16 [N, Cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1] in ``torch.channels_last``, with gradients for ``weight`` and ``bias`` as
    autograd asks for them.  The image gets no gradient: ``x.requires_grad`` raises ``NotImplementedError``."""
    _check_stem_input(x)
    _check_stem_weight(weight)
    if int(x.shape[1]) != int(weight.shape[1]):
        raise ValueError(f'input has {int(x.shape[1])} channels, weight expects {int(weight.shape[1])}')
    if bias is not None and (bias.dim() != 1 or bias.shape[0] != weight.shape[0] or bias.dtype not in _DTYPES):
        raise NotImplementedError(f'bias {tuple(bias.shape)} {bias.dtype}: the trainable stem takes a float32 or bfloat16 [Cout] bias')
    if x.requires_grad:
        raise NotImplementedError('x requires a gradient: the trainable stem has no input gradient (the image needs none; detach x)')
    _need_cuda(x, weight, bias)
    return _StemConv2dFunction.apply(x, weight, bias)


class StemConv2d(torch.nn.Conv2d):
    """``torch.nn.Conv2d`` with torch's constructor arguments and parameter names (``weight``, ``bias``: ``state_dict``s
    interchange) whose forward is ``stem_conv2d``.  ``kernel_size``, ``stride`` and ``padding`` default to 7, 2 and 3; an argument
    outside the supported family raises ``NotImplementedError`` naming it."""

    def __init__(self, in_channels, out_channels, kernel_size=7, stride=2, padding=3, dilation=1, groups=1, bias=True,
                 padding_mode='zeros', device=None, dtype=None):
        why = _stem_unsupported(kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels)
        if why is not None:
            raise NotImplementedError(why)
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device, dtype)

    def forward(self, x):
        return stem_conv2d(x, self.weight, self.bias)


def _stem_why_not(conv):
    if type(conv) is not torch.nn.Conv2d:
        return f'a subclass of torch.nn.Conv2d ({type(conv).__name__}): its forward may differ'
    if conv.weight.dtype not in _DTYPES:
        return f'weight dtype {conv.weight.dtype}: float32 or bfloat16 only'
    return _stem_unsupported(conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.padding_mode,
                             conv.in_channels, conv.out_channels, conv.transposed)


def _stem_from_torch(conv):
    new = StemConv2d.__new__(StemConv2d)
    new.__dict__.update(conv.__dict__)  # the same Parameter objects, hooks, training flag and constructor attributes
    new._parameters = dict(conv._parameters)  # (the registry itself is the new module's own)
    return new


def _our_convs():
    return Conv2d, DropoutConv1x1, GroupedConv2d, StridedConv1x1, CatConv2d, StemConv2d


def _is_stem_business(conv):
    """A conv from at most 4 channels, or a 7x7 conv of stride 2: what a reader would take for a stem."""
    return conv.in_channels <= STEM_MAX_IN_CHANNELS or (_pair(conv.kernel_size) == (7, 7) and _pair(conv.stride) == (2, 2))


def convert_stem_conv2d_(module):
    """Replaces every eligible plain ``torch.nn.Conv2d`` below ``module`` -- ``in_channels <= 4``, ``out_channels`` 32 or 64, 7x7,
    stride 2, padding 3 with zeros, dilation 1, groups 1 -- in place by a ``StemConv2d`` that shares its ``Parameter`` objects
    (optimisers and ``state_dict`` keys are unaffected) -> (names replaced, {name left: reason}).  ``left`` names every other conv
    from at most 4 channels and every other 7x7 conv of stride 2 with the reason; the remaining convs are not its business.
    ``module`` itself is not replaced when it is such a conv: it is reported as left.  A conv object that sits in several slots is
    replaced by one object in all of them.  Works before or after the other converts."""
    replaced, left = [], {}
    ours = _our_convs()
    if isinstance(module, torch.nn.Conv2d) and not isinstance(module, ours) and _is_stem_business(module):
        left[''] = _stem_why_not(module) or 'the root module cannot be replaced in place: convert its parent'
    swapped = {}  # id of a replaced conv -> its replacement: a conv in two slots stays one object
    for name, parent in list(module.named_modules()):
        slots = [(n, c) for n, c in parent._modules.items() if c is not None]  # (named_children() drops repeated objects)
        for child_name, child in slots:
            full = f'{name}.{child_name}' if name else child_name
            if not isinstance(child, torch.nn.Conv2d) or isinstance(child, ours) or not _is_stem_business(child):
                continue
            why = _stem_why_not(child)
            if why is not None:
                left[full] = why
                continue
            if id(child) not in swapped:
                swapped[id(child)] = _stem_from_torch(child)
            setattr(parent, child_name, swapped[id(child)])
            replaced.append(full)
    return replaced, left


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


def _pool_from_torch(pool):
    new = MaxPool2d.__new__(MaxPool2d)
    new.__dict__.update(pool.__dict__)  # hooks, training flag and constructor attributes
    return new


def convert_maxpool2d_(module):
    """Replaces every plain ``torch.nn.MaxPool2d`` of the two geometries below ``module`` in place by a ``MaxPool2d`` -> (names
    replaced, {name left: reason}).  Every other max-pool is left with a reason naming the argument (``C % 8`` shows at run time
    only: there the forward raises).  ``module`` itself is not replaced when it is a pool: it is reported as left.  A pool object
    that sits in several slots is replaced by one object in all of them.  Works before or after the other converts."""
    replaced, left = [], {}
    if isinstance(module, torch.nn.MaxPool2d) and not isinstance(module, MaxPool2d):
        left[''] = _pool_why_not(module) or 'the root module cannot be replaced in place: convert its parent'
    swapped = {}
    for name, parent in list(module.named_modules()):
        slots = [(n, c) for n, c in parent._modules.items() if c is not None]  # (named_children() drops repeated objects)
        for child_name, child in slots:
            full = f'{name}.{child_name}' if name else child_name
            if not isinstance(child, torch.nn.MaxPool2d) or isinstance(child, MaxPool2d):
                continue
            why = _pool_why_not(child)
            if why is not None:
                left[full] = why
                continue
            if id(child) not in swapped:
                swapped[id(child)] = _pool_from_torch(child)
            setattr(parent, child_name, swapped[id(child)])
            replaced.append(full)
    return replaced, left


# ---- the bilinear resize behind the heads ("Trainable bilinear resize" of include/cpn_hip.h, csrc/bilinear_train.hip,
# csrc/bilinear_adjoint.h)
#
# The reference's ``CPNCore`` enlarges the refinement features to the input's size in front of the refinement head
# (``refinement_full_res``) and every head map that is smaller than the input (``_equal_size``, ``models/cpn.py:109-115, 277-279``).
# ``resized_conv2d`` runs the first as one autograd function on the low-resolution features: the conv's loader blends (MODE_BL of
# the inference path), the weight gradient blends while it stages, the input gradient goes through the adjoint of the resize as a
# gather, ``bilinear_resize_backward``; the resized tensor -- the largest activation of the net -- is neither written nor saved.
# ``bilinear_resize`` is the resize on its own, for activations and for the fp32 head maps; it saves nothing but the sizes.
# ``CPNCore`` / ``convert_cpn_core_`` put both where the reference's core has ``F.interpolate``.  Known limits: the gradient at the
# input's size (``T``) is written and read once; the training forward is not decomposed into sub-pixel phases; upward resizes,
# ``'bilinear'`` and k in {3, 5, 7} only.

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
    info = (ctypes.c_int32 * 5)()
    _lib.check(_lib.load().cpn_resized_conv_wgrad_info(n, h, w, cin, int(low_size[0]), int(low_size[1]), cout, k, slab_rows, info),
               'resized_conv_wgrad_info')
    return dict(zip(('slabs', 'slab_rows', 'steps', 'reduce_chain', 'bias_chain'), (int(v) for v in info)))


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
    bias_dtype = dtype if bias_dtype is None else bias_dtype
    if dtype not in _DTYPES or bias_dtype not in _DTYPES:
        raise NotImplementedError(f'dtype {dtype} / {bias_dtype}: gradients are float32 or bfloat16')
    assert int(grad_output.shape[0]) == n, (tuple(grad_output.shape), tuple(x.shape))
    if not (weight or bias):
        return None, None
    dw = torch.empty((cout, cin, k, k), dtype=dtype, device=x.device) if weight else None
    db = torch.empty((cout,), dtype=bias_dtype, device=x.device) if bias else None
    xs, gs = _nhwc(x, torch.bfloat16), _nhwc(grad_output, torch.bfloat16)
    lib = _lib.load()
    nbytes = int(lib.cpn_resized_conv_wgrad_workspace_bytes(n, H, W, cin, h, w, cout, k, slab_rows))
    if nbytes <= 0:
        _lib.check(lib.cpn_resized_conv_wgrad_info(n, H, W, cin, h, w, cout, k, slab_rows, (ctypes.c_int32 * 5)()), 'resized_conv_wgrad')
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    _lib.check(lib.cpn_resized_conv_wgrad(_lib.ptr(xs), _lib.ptr(gs), n, H, W, cin, h, w, cout, k, slab_rows, _lib.ptr(dw), _DTYPES[dtype],
                                          _lib.ptr(db), _DTYPES[bias_dtype], _lib.ptr(ws), nbytes, _lib.stream_ptr()),
               'resized_conv_wgrad')
    return dw, db


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


def _resized_from(conv):
    new = ResizedConv2d.__new__(ResizedConv2d)
    new.__dict__.update(conv.__dict__)  # the same Parameter objects, hooks, training flag and constructor attributes
    new._parameters = dict(conv._parameters)  # (the registry itself is the new module's own)
    return new


def _is_reference_core(cls):
    """Whether the class's forward IS the reference's ``CPNCore.forward`` (told by its names: the reference is not imported)."""
    f = getattr(cls, 'forward', None)
    return getattr(f, '__module__', None) == 'celldetection.models.cpn' and getattr(f, '__qualname__', None) == 'CPNCore.forward'


_CORE_HEADS = ('score', 'location', 'fourier', 'uncertainty', 'refinement')
_CORE_FEATURES = ('score_features', 'contour_features', 'location_features', 'uncertainty_features', 'refinement_features')
_CORE_ATTRIBUTES = ('backbone',) + tuple(f'{h}_{part}' for h in _CORE_HEADS for part in ('fuse', 'head')) + _CORE_FEATURES + \
    ('refinement_interpolation', 'refinement_full_res')


def _core_why_not(core, converted=False):
    """The first attribute that keeps a core out of ``CPNCore``, as ``'<attribute>: <reason>'``, or None.  ``converted``: slot 0 of
    the refinement head's block must be a ``ResizedConv2d`` already."""
    for name in _CORE_ATTRIBUTES:
        if not hasattr(core, name):
            return f'{name}: the core has no such attribute'
    if core.refinement_interpolation != 'bilinear':
        return f"refinement_interpolation: {core.refinement_interpolation!r}: 'bilinear' only"
    for name in ('score_head', 'location_head', 'fourier_head'):
        if getattr(core, name) is None:
            return f'{name}: None: the core needs this head'
    head = core.refinement_head
    if head is None or not core.refinement_full_res:
        return None  # nothing is resized in front of a conv: the head maps alone go through bilinear_resize
    block = getattr(head, 'block', None)
    if not isinstance(block, torch.nn.Sequential) or type(block).forward is not torch.nn.Sequential.forward or len(block) < 1:
        return f'refinement_head.block: {type(block).__name__}: an nn.Sequential (or a subclass that keeps its forward) with the ' \
               f'conv in slot 0 only'
    if getattr(head, 'attention', None) is not None:
        return f'refinement_head.attention: {type(head.attention).__name__}: None only (it would run on the resized features)'
    conv = block[0]
    if converted:
        return None if isinstance(conv, ResizedConv2d) else f'refinement_head.block.0: {type(conv).__name__}: not a ResizedConv2d'
    if not isinstance(conv, torch.nn.Conv2d):
        return f'refinement_head.block.0: {type(conv).__name__}: not a torch.nn.Conv2d'
    why = _resized_why_not(conv)
    return None if why is None else f'refinement_head.block.0: {why}'


# the order in which the core runs its heads (it fixes the order of the dropout draws) and the attribute that names each head's
# feature key(s)
_CORE_ROUTES = (('score', 'score_features'), ('location', 'location_features'), ('fourier', 'contour_features'),
                ('uncertainty', 'uncertainty_features'), ('refinement', 'refinement_features'))


def _head_input(features, key):
    """What a head reads of the backbone's result: a backbone that returns one tensor feeds every head with it; from a mapping a
    single key picks one feature and a list or tuple of keys picks a list of features, for the head's ``fuse`` module."""
    if torch.is_tensor(features):
        return features
    several = isinstance(key, (list, tuple))
    picked = [features[name] for name in (key if several else (key,))]
    return picked if several else picked[0]


class CPNCore(torch.nn.Module):
    """The reference's ``CPNCore`` (``models/cpn.py:238-283``) on this library's pieces, under the reference's child names --
    ``backbone``, ``score_fuse`` / ``score_head`` and the same for ``location``, ``fourier``, ``uncertainty`` and ``refinement``
    (``state_dict`` keys do not move) -> ``(scores, locations, refinement, fourier, uncertainty)``.

    With ``refinement_full_res`` the reference enlarges the refinement features to the input's size and runs the head on the result;
    here slot 0 of ``refinement_head.block``, a ``ResizedConv2d``, takes the low-resolution features and the input's size, the remaining slots
    and the head's ``activation`` follow, so the enlarged tensor is never written.  The final ``_equal_size`` of the head map is
    ``bilinear_resize``.  ``refinement_interpolation`` is ``'bilinear'``.  Forward hooks on the head's children fire; hooks on the
    refinement head and on its ``block`` themselves do not when the features are resized, because the slots are called one by
    one."""

    def __init__(self, backbone, score_head, location_head, fourier_head, refinement_head=None, uncertainty_head=None,
                 score_fuse=None, location_fuse=None, fourier_fuse=None, refinement_fuse=None, uncertainty_fuse=None,
                 score_features='1', contour_features='1', location_features='1', uncertainty_features='1', refinement_features='0',
                 refinement_full_res=True):
        super().__init__()
        self.backbone = backbone
        self.score_fuse, self.score_head = score_fuse, score_head
        self.location_fuse, self.location_head = location_fuse, location_head
        self.fourier_fuse, self.fourier_head = fourier_fuse, fourier_head
        self.uncertainty_fuse, self.uncertainty_head = uncertainty_fuse, uncertainty_head
        self.refinement_fuse, self.refinement_head = refinement_fuse, refinement_head
        self.score_features, self.contour_features, self.location_features = score_features, contour_features, location_features
        self.uncertainty_features, self.refinement_features = uncertainty_features, refinement_features
        self.refinement_interpolation, self.refinement_full_res = 'bilinear', bool(refinement_full_res)
        why = _core_why_not(self, converted=True)
        if why is not None:
            raise NotImplementedError(why)

    def forward(self, inputs):
        size = tuple(int(v) for v in inputs.shape[2:])
        features = self.backbone(inputs)
        maps = {}
        for name, key_attribute in _CORE_ROUTES:
            head, fuse = getattr(self, f'{name}_head'), getattr(self, f'{name}_fuse')
            if head is None:  # (the uncertainty and the refinement head are optional)
                maps[name] = None
                continue
            source = _head_input(features, getattr(self, key_attribute))
            if fuse is not None:
                source = fuse(source)
            maps[name] = self._refinement(head, source, size) if name == 'refinement' else head(source)
        return maps['score'], maps['location'], maps['refinement'], maps['fourier'], maps['uncertainty']

    def _refinement(self, head, source, size):
        """The refinement map at the input's ``size``: with ``refinement_full_res`` the head runs on the enlarged features -- slot 0
        of its block resizes and convolves in one function --, and a map that is still smaller than the input is enlarged."""
        if self.refinement_full_res and tuple(source.shape[2:]) != size:
            first, *rest = head.block
            out = first(source, size)  # ResizedConv2d
            for module in rest:
                out = module(out)
            if getattr(head, 'activation', None) is not None:
                out = head.activation(out)
        else:
            out = head(source)
        return out if tuple(out.shape[2:]) == size else bilinear_resize(out, size)


def _core_from_torch(core):
    new = CPNCore.__new__(CPNCore)
    new.__dict__.update(core.__dict__)  # hooks, training flag and the core's own attributes (order, feature keys, ...)
    new._modules, new._parameters, new._buffers = dict(core._modules), dict(core._parameters), dict(core._buffers)
    head = core.refinement_head
    if head is not None and core.refinement_full_res and not isinstance(head.block[0], ResizedConv2d):
        head.block[0] = _resized_from(head.block[0])  # the Sequential stays the object it is: its slot is filled anew
    return new


def convert_cpn_core_(module, core_types=()):
    """Replaces every eligible CPN core below ``module`` in place by a ``CPNCore`` -> (names replaced, {name left: reason}).  A
    module is a candidate when its class's ``forward`` is the reference's ``CPNCore.forward`` (told by the names
    ``celldetection.models.cpn`` / ``CPNCore.forward``; a class that merely has the same attributes does not qualify) or when its
    class is listed in ``core_types``.  Eligible: ``refinement_interpolation == 'bilinear'``, the score, location and fourier heads
    present, and -- with ``refinement_full_res`` and a refinement head -- a head whose ``block`` is an ``nn.Sequential`` (itself or a
    subclass that does not override ``forward``) with a stride-1 conv of ``resized_conv2d``'s family in slot 0 and no ``attention``.
    Slot 0 becomes a ``ResizedConv2d``, from a stock conv or from a ``Conv2d`` of this library, so the swap works before or after the
    other converts with the same result; ``Parameter`` objects are shared and ``state_dict`` keys do not move.  Everything else is
    left with a reason naming the attribute; a core object that sits in two slots is left.  ``module`` itself is not replaced when
    it is a candidate: it is reported as left."""
    core_types = tuple(core_types)
    replaced, left = [], {}

    def candidate(m):
        return not isinstance(m, CPNCore) and (_is_reference_core(type(m)) or type(m) in core_types)

    if candidate(module):
        left[''] = _core_why_not(module) or 'the root module cannot be replaced in place: convert its parent'
    uses = {}
    for parent in module.modules():
        for child in parent._modules.values():
            if child is not None and candidate(child):
                uses[id(child)] = uses.get(id(child), 0) + 1
    for name, parent in list(module.named_modules()):
        for child_name, child in [(n, c) for n, c in parent._modules.items() if c is not None]:
            if not candidate(child):
                continue
            full = f'{name}.{child_name}' if name else child_name
            why = _core_why_not(child)
            if why is None and uses[id(child)] > 1:
                why = f'the core sits in {uses[id(child)]} slots'
            if why is not None:
                left[full] = why
                continue
            setattr(parent, child_name, _core_from_torch(child))
            replaced.append(full)
    return replaced, left
