"""The trainable dense convolution ("Trainable convolution" of include/cpn_hip.h, csrc/conv_train.hip, csrc/conv_igemm.hip):
``conv2d`` (one ``torch.autograd.Function``), ``conv2d_fork`` and the ``nn.Conv2d`` drop-in ``Conv2d``.

A training step of the reference model under PyTorch-ROCm spends >= 99.9 % of its FLOPs in convolutions; the four 7x7 ReadOut
convs and the UNet decoder convs (93 % of them) are dense stride-1 convs whose channel counts are multiples of 32.  For that family
forward, input gradient and weight gradient run in this library's HIP kernels:

* forward: ``cpn_conv2d`` (csrc/conv_igemm.hip) on weights packed on the device every step;
* input gradient: for stride 1 and ``padding = k // 2`` again such a conv, of ``grad_output``, with the taps flipped and the channel
  roles swapped -- the same kernel on the dgrad pack;
* weight gradient: the bf16 MFMA kernel of csrc/conv_train.hip, which reduces over pixels in slabs and adds the slabs' fp32 partial
  sums in a fixed order (no floating-point atomics: bit-identical from run to run); the bias gradient comes from a small kernel
  of its own.

Supported: ``groups = 1``, ``stride = 1``, ``dilation = 1``, a square odd ``k`` in {1, 3, 5, 7}, ``padding = k // 2`` with zeros,
``Cin`` and ``Cout`` multiples of 32, a 4-D input on the GPU.  Everything else raises ``NotImplementedError`` naming the argument;
there is no CPU fallback.  ``convert_conv2d_`` leaves every other conv and says why: the grouped 3x3 convs of the encoder are the
business of ``grouped_conv2d`` (grouped.py), the final 1x1 convs of the heads (1 / 2 / 20 output channels) of ``dropout_conv1x1``
(readout_tail.py), the stem (a 7x7 stride-2 conv from at most 4 channels) of ``stem_conv2d`` (stem.py).

Arithmetic: activations and weights are rounded to bf16 (round to nearest even), products accumulate in fp32, the forward output
and the input gradient are stored as bf16, the weight and bias gradients are fp32 sums rounded once to the parameter's dtype.  ``x``
may be bf16 or fp32 (rounded to bf16 on the way in, as autocast would); the output is bf16 in ``torch.channels_last``.  A
channels-last ``[N, C, H, W]`` tensor is NHWC in memory, the layout of ``cpn_conv2d``: no layout copy is made for such inputs, any
other layout is made channels-last first, and a view that does not start at a 16-byte address is cloned.
"""
import torch

from .. import _lib
from ..ops import _need_cuda
from ._common import _DTYPES, _grad_dtypes, _nhwc, _pair, _run_conv, _weight_grad, _weight_grad_info


KERNEL_SIZES = (1, 3, 5, 7)


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


def weight_grad_info(n, h, w, cin, cout, k, slab_rows=0):
    """What ``conv2d_weight_grad`` would run -> dict(slabs, slab_rows, steps (MFMA steps per slab), reduce_chain, bias_chain).  Host
    arithmetic only: needs no GPU.  Raises like the launch for a call it rejects."""
    return _weight_grad_info('conv', n, h, w, cin, cout, k, slab_rows)


def conv2d_weight_grad(x, grad_output, kernel_size, slab_rows=0, weight=True, bias=True, dtype=torch.float32, bias_dtype=None):
    """(x [N, Cin, H, W], grad_output [N, Cout, H, W]) -> (dW [Cout, Cin, k, k] | None, db [Cout] | None): the gradients ``conv2d``
    returns for its weight and bias, as fp32 sums over the bf16-rounded operands rounded once to ``dtype`` / ``bias_dtype``.
    ``slab_rows``: image rows per slab of the reduction (0: chosen by the library).  An empty input: zeros."""
    _need_cuda(x, grad_output)
    k = int(kernel_size)
    n, cin, h, w = (int(v) for v in x.shape)
    cout = int(grad_output.shape[1])
    _check_channels(cin, cout, k)
    dtypes = _grad_dtypes(dtype, bias_dtype)
    assert tuple(grad_output.shape) == (n, cout, h, w), (tuple(grad_output.shape), (n, cout, h, w))
    return _weight_grad('conv', (n, h, w, cin, cout, k, slab_rows), lambda: (_nhwc(x, torch.bfloat16), _nhwc(grad_output, torch.bfloat16)),
                        (cout, cin, k, k), x.device, weight, bias, dtypes, torch.zeros, no_pixels=n * h * w == 0)


def _conv_backward(ctx, grad_output, grad_skip=None):
    """The backward of ``conv2d`` and ``conv2d_fork``.  ``grad_skip``: the gradient of the fork's second output, the residual
    operand of the dgrad conv."""
    xs, weight = ctx.saved_tensors
    cout, cin, k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
    need_x, need_w, need_b = ctx.needs_input_grad
    need_b = need_b and ctx.bias_dtype is not None
    gs = _nhwc(grad_output, torch.bfloat16)
    dx = dw = db = None
    if need_x:  # the conv of grad_output with the flipped, channel-swapped weights; with a skip gradient: the sum in fp32, one rounding
        res = None if grad_skip is None else _nhwc(grad_skip, torch.bfloat16)
        dx = _run_conv(gs, pack_weight(weight, 'dgrad'), None, cout, cin, k, res=res).to(ctx.x_dtype)
    if need_w or need_b:
        dw, db = conv2d_weight_grad(xs, gs, k, weight=need_w, bias=need_b, dtype=weight.dtype,
                                    bias_dtype=ctx.bias_dtype or weight.dtype)
    return dx, dw, db


class _Conv2dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        cout, cin, k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        xs = _nhwc(x, torch.bfloat16)
        b32 = None if bias is None else bias.detach().float().contiguous()
        out = _run_conv(xs, pack_weight(weight, 'forward'), b32, cin, cout, k)
        ctx.save_for_backward(xs, weight)
        ctx.x_dtype = x.dtype
        ctx.bias_dtype = None if bias is None else bias.dtype
        return out

    @staticmethod
    def backward(ctx, grad_output):
        return _conv_backward(ctx, grad_output)


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
            return (None, None, None) if grad_output is None else _conv_backward(ctx, grad_output)
        if grad_output is None:
            return (grad_skip.to(ctx.x_dtype) if ctx.needs_input_grad[0] else None), None, None
        return _conv_backward(ctx, grad_output, grad_skip)


def conv2d_fork(x, weight, bias=None):
    """``conv2d(x, weight, bias)`` at the head of a residual block -> ``(y, skip)``: ``y`` is ``conv2d``'s output bit for bit,
    ``skip`` is ``x`` (same storage, no copy) with this function as its ``grad_fn``, so autograd sees ONE consumer of ``x`` and the
    two gradients of the block's input are never added by a stock op: when a gradient arrives at ``skip`` it is rounded to bf16
    channels-last as ``grad_output`` is and becomes the residual operand of the dgrad conv, ``dx = round(dgrad(dy) + dskip)`` with
    the sum in fp32; when none arrives the backward is ``conv2d``'s."""
    _check_conv2d(x, weight, bias)
    return _Conv2dForkFunction.apply(x, weight, bias)


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
