"""The convs that read the padded 4-channel image: one description, ``ImageFamily``, and the one implementation of everything the
trainable stem (stem.py) and the trainable image conv (image_conv.py) do with it -- the rule of what is supported, the weight and
input checks, pack, pad, forward, weight gradient, the autograd ``Function``, the functional form and the module.  A member of the
family is a module of constants that binds its description to these functions; the C side is csrc/image_train.h."""
import dataclasses
import typing

import torch

from .. import _lib
from ..ops import _need_cuda
from ._common import _DTYPES, _grad_dtypes, _nhwc, _pair, _weight_grad, _weight_grad_info


@dataclasses.dataclass(frozen=True)
class ImageFamily:
    """A ``Conv2d(C <= max_in_channels, Cout in out_channels, kernel, stride, padding)`` on the padded bf16 image
    ``[N, H + pad_rows, W + pad_cols, 4]`` with weight records ``[kernel][Cout][record]``."""
    noun: str  # in messages: 'the trainable stem'
    kernel: int
    stride: int
    padding: int
    out_channels: tuple
    pad_rows: int
    pad_cols: int
    record: int
    pack: str  # the C entry points, without 'cpn_'
    pad: str
    pad_args: typing.Callable  # (src, dst, n, c, h, w, stream) -> the arguments of ``pad`` in its order
    forward: str
    wgrad: str  # the family of cpn_<wgrad>_wgrad, _wgrad_workspace_bytes and _wgrad_info
    max_in_channels: int = 4

    @property
    def kxk(self):
        return f'{self.kernel}x{self.kernel}'

    def out_size(self, h, w):
        return tuple((v + 2 * self.padding - self.kernel) // self.stride + 1 for v in (h, w))


def unsupported(f, kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels, transposed=False):
    """The first argument the conv does not run, as a sentence, or None."""
    if transposed:
        return 'transposed convs are not run'
    if _pair(kernel_size) != (f.kernel, f.kernel):
        return f'kernel_size {kernel_size}: {f.kxk} only'
    if _pair(stride) != (f.stride, f.stride):
        return f'stride {stride}: stride {f.stride} only'
    if isinstance(padding, str) or _pair(padding) != (f.padding, f.padding):
        return f'padding {padding}: {f.padding} zero{"s" if f.padding != 1 else ""} only'
    if _pair(dilation) != (1, 1):
        return f'dilation {dilation}: dilation 1 only'
    if groups != 1:
        return f'groups {groups}: dense convs only'
    if padding_mode != 'zeros':
        return f"padding_mode '{padding_mode}': zeros only"
    if not 1 <= in_channels <= f.max_in_channels:
        return f'in_channels {in_channels}: 1 ... {f.max_in_channels} only'
    if out_channels not in f.out_channels:
        return f'out_channels {out_channels}: {f.out_channels} only'
    return None


def _check_out_channels(f, cout):
    if cout not in f.out_channels:
        raise NotImplementedError(f'out_channels {cout}: {f.noun} writes {f.out_channels} only')


def check_weight(f, weight):
    if weight.dim() != 4:
        raise NotImplementedError(f'weight of {weight.dim()} dimensions: {f.noun} needs [Cout, C, {f.kernel}, {f.kernel}]')
    if tuple(weight.shape[2:]) != (f.kernel, f.kernel):
        raise NotImplementedError(f'kernel_size {tuple(weight.shape[2:])}: {f.noun} runs {f.kxk} kernels only')
    if weight.dtype not in _DTYPES:
        raise NotImplementedError(f'weight dtype {weight.dtype}: {f.noun} takes float32 or bfloat16 parameters')
    if not 1 <= int(weight.shape[1]) <= f.max_in_channels:
        raise NotImplementedError(f'in_channels {int(weight.shape[1])}: {f.noun} takes 1 ... {f.max_in_channels}')
    _check_out_channels(f, int(weight.shape[0]))


def check_input(f, x):
    if x.dim() != 4:
        raise NotImplementedError(f'input of {x.dim()} dimensions: {f.noun} takes a 4-D [N, C, H, W] input')
    if x.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {x.dtype}: {f.noun} takes float32 or bfloat16 images')
    if not 1 <= int(x.shape[1]) <= f.max_in_channels:
        raise NotImplementedError(f'input of {int(x.shape[1])} channels: {f.noun} takes 1 ... {f.max_in_channels}')
    if min(int(v) for v in x.shape) < 1:
        raise NotImplementedError(f'input of size {tuple(x.shape)}: {f.noun} needs at least one pixel')


def pack_weight(f, weight):
    """weight [Cout, C, k, k] (float32 | bfloat16, on the GPU) -> the bf16 records [k][Cout][record] the loop reads, packed on the
    device."""
    check_weight(f, weight)
    _need_cuda(weight)
    w = weight.detach().contiguous()
    cout, c = int(w.shape[0]), int(w.shape[1])
    packed = torch.empty((f.kernel, cout, f.record), dtype=torch.bfloat16, device=w.device)
    _lib.check(getattr(_lib.load(), 'cpn_' + f.pack)(_lib.ptr(w), _DTYPES[w.dtype], cout, c, _lib.ptr(packed), _lib.stream_ptr()), f.pack)
    return packed


def pad(f, x):
    """x [N, C <= 4, H, W] -> the padded input bf16 [N, H + pad_rows, W + pad_cols, 4] (zero border, zeros in the channels >= C)."""
    n, c, h, w = (int(v) for v in x.shape)
    src = x.detach().float().contiguous()  # (bf16 -> fp32 is exact; the kernel rounds fp32 to bf16, to nearest even)
    xp = torch.empty((n, h + f.pad_rows, w + f.pad_cols, 4), dtype=torch.bfloat16, device=x.device)
    _lib.check(getattr(_lib.load(), 'cpn_' + f.pad)(*f.pad_args(_lib.ptr(src), _lib.ptr(xp), n, c, h, w, _lib.stream_ptr())), f.pad)
    return xp


def run_forward(f, xp, size, packed, bias):
    n, h, w = size
    cout = int(packed.shape[1])
    out = torch.empty((n, cout, *f.out_size(h, w)), dtype=torch.bfloat16, device=xp.device, memory_format=torch.channels_last)
    _lib.check(getattr(_lib.load(), 'cpn_' + f.forward)(_lib.ptr(xp), _lib.ptr(packed), _lib.ptr(bias), n, h, w, cout, _lib.ptr(out),
                                                        _lib.stream_ptr()), f.forward)
    return out


def weight_grad_info(f, n, h, w, cout, slab_rows=0):
    return _weight_grad_info(f.wgrad, n, h, w, cout, slab_rows)


def wgrad(f, xp, size, c, gs, slab_rows, weight, bias, dtype, bias_dtype):
    """xp: the padded input; gs: bf16 NHWC memory, 16-byte aligned -> (dW | None, db | None).  The launch takes the image's channel
    count ``c``; the workspace query does not."""
    n, h, w = size
    cout = int(gs.shape[1])
    return _weight_grad(f.wgrad, (n, h, w, cout, slab_rows), lambda: (xp, gs), (cout, c, f.kernel, f.kernel), xp.device, weight, bias,
                        (dtype, bias_dtype), torch.zeros, launch_geometry=(n, h, w, c, cout, slab_rows))


def weight_grad(f, x, grad_output, slab_rows=0, weight=True, bias=True, dtype=torch.float32, bias_dtype=None):
    check_input(f, x)
    n, c, h, w = (int(v) for v in x.shape)
    cout = int(grad_output.shape[1])
    _check_out_channels(f, cout)
    dtype, bias_dtype = _grad_dtypes(dtype, bias_dtype)
    want = (n, cout, *f.out_size(h, w))
    assert tuple(grad_output.shape) == want, (tuple(grad_output.shape), want)
    _need_cuda(x, grad_output)
    return wgrad(f, pad(f, x), (n, h, w), c, _nhwc(grad_output, torch.bfloat16), slab_rows, weight, bias, dtype, bias_dtype)


class ImageConv2dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, x, weight, bias):
        n, c, h, w = (int(v) for v in x.shape)
        xp = pad(f, x)
        b32 = None if bias is None else bias.detach().float().contiguous()
        out = run_forward(f, xp, (n, h, w), pack_weight(f, weight), b32)
        ctx.save_for_backward(xp)  # the padded bf16 input alone: neither x nor the weight is needed again
        ctx.family, ctx.size, ctx.c = f, (n, h, w), c
        ctx.weight_dtype = weight.dtype
        ctx.bias_dtype = None if bias is None else bias.dtype
        return out

    @staticmethod
    def backward(ctx, grad_output):
        xp, = ctx.saved_tensors
        _, _, need_w, need_b = ctx.needs_input_grad
        need_b = need_b and ctx.bias_dtype is not None
        dw = db = None
        if need_w or need_b:
            dw, db = wgrad(ctx.family, xp, ctx.size, ctx.c, _nhwc(grad_output, torch.bfloat16), 0, need_w, need_b, ctx.weight_dtype,
                           ctx.bias_dtype or ctx.weight_dtype)
        return None, None, dw, db


def conv2d(f, x, weight, bias=None):
    check_input(f, x)
    check_weight(f, weight)
    if int(x.shape[1]) != int(weight.shape[1]):
        raise ValueError(f'input has {int(x.shape[1])} channels, weight expects {int(weight.shape[1])}')
    if bias is not None and (bias.dim() != 1 or bias.shape[0] != weight.shape[0] or bias.dtype not in _DTYPES):
        raise NotImplementedError(f'bias {tuple(bias.shape)} {bias.dtype}: {f.noun} takes a float32 or bfloat16 [Cout] bias')
    if x.requires_grad:
        raise NotImplementedError(f'x requires a gradient: {f.noun} has no input gradient (the image needs none; detach x)')
    _need_cuda(x, weight, bias)
    return ImageConv2dFunction.apply(f, x, weight, bias)


class ImageFamilyConv2d(torch.nn.Conv2d):
    """``torch.nn.Conv2d`` whose forward is ``conv2d`` of the subclass's ``family``; an argument outside it raises
    ``NotImplementedError`` naming it.  A subclass states the family and torch's constructor signature with its own defaults."""
    family = None

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device, dtype):
        why = unsupported(self.family, kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels)
        if why is not None:
            raise NotImplementedError(why)
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device, dtype)

    def forward(self, x):
        return conv2d(self.family, x, self.weight, self.bias)


def why_not(f, conv):
    if type(conv) is not torch.nn.Conv2d:
        return f'a subclass of torch.nn.Conv2d ({type(conv).__name__}): its forward may differ'
    if conv.weight.dtype not in _DTYPES:
        return f'weight dtype {conv.weight.dtype}: float32 or bfloat16 only'
    return unsupported(f, conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.padding_mode, conv.in_channels,
                       conv.out_channels, conv.transposed)
