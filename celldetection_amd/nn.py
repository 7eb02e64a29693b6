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
there is no CPU fallback.  Known limit: the final 1x1 convs of the heads (1 / 2 / 20 output channels) and the strided or grouped
encoder convs of the reference model stay stock torch operations (``convert_conv2d_`` leaves them and says why).

Arithmetic: activations and weights are rounded to bf16 (round to nearest even), products accumulate in fp32, the forward output
and the input gradient are stored as bf16, the weight and bias gradients are fp32 sums rounded once to the parameter's dtype.  ``x``
may be bf16 or fp32 (rounded to bf16 on the way in, as autocast would); the output is bf16 in ``torch.channels_last``.  A
channels-last ``[N, C, H, W]`` tensor is NHWC in memory, the layout of ``cpn_conv2d``: no layout copy is made for such inputs, any
other layout is made channels-last first.
"""
import ctypes

import torch

from . import _lib
from .ops import _need_cuda

__all__ = ['conv2d', 'Conv2d', 'convert_conv2d_', 'is_supported', 'pack_weight', 'conv2d_weight_grad', 'weight_grad_info']

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


def _run_conv(src, packed, bias, cin, cout, k):
    """cpn_conv2d on a bf16 tensor whose memory is NHWC -> bf16 [N, cout, H, W] in channels_last."""
    n, _, h, w = src.shape
    out = torch.empty((n, cout, h, w), dtype=torch.bfloat16, device=src.device, memory_format=torch.channels_last)
    if out.numel() == 0:
        return out
    d = _conv_desc(cin, cout, k, bias is not None)
    _lib.check(_lib.load().cpn_conv2d(ctypes.byref(d), _lib.ptr(src), cin, _lib.ptr(None), 0, _lib.ptr(None), 0, _lib.ptr(out), cout,
                                      n, h, w, _lib.ptr(packed), _lib.ptr(bias), _lib.stream_ptr()), 'conv2d')
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


def conv2d(x, weight, bias=None, padding=None):
    """``torch.nn.functional.conv2d(x, weight, bias, stride=1, padding=k // 2)`` for the supported family (module docstring), with
    gradients for ``x``, ``weight`` and ``bias`` as autograd asks for them -> bf16 [N, Cout, H, W] in ``torch.channels_last``."""
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
    return _Conv2dFunction.apply(x, weight, bias)


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

    def forward(self, x):
        return conv2d(x, self.weight, self.bias)


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
    if isinstance(module, torch.nn.Conv2d) and not isinstance(module, Conv2d):
        left[''] = _why_not(module) or 'the root module cannot be replaced in place: convert its parent'
    for name, parent in list(module.named_modules()):
        for child_name, child in list(parent.named_children()):
            full = f'{name}.{child_name}' if name else child_name
            if isinstance(child, Conv2d) or not isinstance(child, torch.nn.modules.conv._ConvNd):
                continue
            why = _why_not(child) if isinstance(child, torch.nn.Conv2d) else f'{type(child).__name__}: 2-D convs only'
            if why is None:
                setattr(parent, child_name, _from_torch(child))
                replaced.append(full)
            else:
                left[full] = why
    return replaced, left
