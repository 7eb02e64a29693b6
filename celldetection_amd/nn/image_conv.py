"""The first conv of a U-Net encoder ("Trainable image conv" of include/cpn_hip.h, csrc/image_conv_train.hip)

The first module a step of the reference's ``UNetEncoder`` runs (``models/unet.py:29-58``: ``CpnU22``, ``CpnSlimU22``,
``CpnWideU22``, ``U17``, ``U12``): ``Conv2d(in_channels <= 4, 32 | 64 | 128, 3, stride=1, padding=1)`` on the image itself.
``image_conv2d`` converts the image to a padded 4-channel bf16 layout in which the 3 taps of a filter row are contiguous, and saves
that tensor alone; the forward is one MFMA step per filter row, the weight gradient three MFMA products per slab with the flat
output pixel as the reduction index.  The image gets no gradient.

After ``convert_image_conv2d_``, ``convert_conv2d_``, ``convert_batchnorm2d_`` and ``convert_maxpool2d_``, in any order, such an
encoder runs without a stock operation.  Known limits: the 1x1 shortcut and the ``ResBlock`` of ``ResUNet`` are not run; no input
gradient; the norm's statistics are not folded into the epilogue; the conv's output is saved by the norm behind it, not recomputed
in the norm's backward; no fp8; ``cda.models.*`` stay inference-only.
"""
import torch

from .. import _lib
from ..ops import _need_cuda
from ._common import _DTYPES, _grad_dtypes, _nhwc, _pair, _weight_grad, _weight_grad_info

IMAGE_OUT_CHANNELS = (32, 64, 128)
IMAGE_MAX_IN_CHANNELS = 4


def _image_unsupported(kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels, transposed=False):
    """The first argument the trainable image conv does not run, as a sentence, or None."""
    if transposed:
        return 'transposed convs are not run'
    if _pair(kernel_size) != (3, 3):
        return f'kernel_size {kernel_size}: 3x3 only'
    if _pair(stride) != (1, 1):
        return f'stride {stride}: stride 1 only'
    if isinstance(padding, str) or _pair(padding) != (1, 1):
        return f'padding {padding}: 1 zero only'
    if _pair(dilation) != (1, 1):
        return f'dilation {dilation}: dilation 1 only'
    if groups != 1:
        return f'groups {groups}: dense convs only'
    if padding_mode != 'zeros':
        return f"padding_mode '{padding_mode}': zeros only"
    if not 1 <= in_channels <= IMAGE_MAX_IN_CHANNELS:
        return f'in_channels {in_channels}: 1 ... {IMAGE_MAX_IN_CHANNELS} only'
    if out_channels not in IMAGE_OUT_CHANNELS:
        return f'out_channels {out_channels}: {IMAGE_OUT_CHANNELS} only'
    return None


def _check_image_weight(weight):
    if weight.dim() != 4:
        raise NotImplementedError(f'weight of {weight.dim()} dimensions: the trainable image conv needs [Cout, C, 3, 3]')
    if tuple(weight.shape[2:]) != (3, 3):
        raise NotImplementedError(f'kernel_size {tuple(weight.shape[2:])}: the trainable image conv runs 3x3 kernels only')
    if weight.dtype not in _DTYPES:
        raise NotImplementedError(f'weight dtype {weight.dtype}: the trainable image conv takes float32 or bfloat16 parameters')
    if not 1 <= int(weight.shape[1]) <= IMAGE_MAX_IN_CHANNELS:
        raise NotImplementedError(f'in_channels {int(weight.shape[1])}: the trainable image conv takes 1 ... {IMAGE_MAX_IN_CHANNELS}')
    if int(weight.shape[0]) not in IMAGE_OUT_CHANNELS:
        raise NotImplementedError(f'out_channels {int(weight.shape[0])}: the trainable image conv writes {IMAGE_OUT_CHANNELS} only')


def _check_image_input(x):
    if x.dim() != 4:
        raise NotImplementedError(f'input of {x.dim()} dimensions: the trainable image conv takes a 4-D [N, C, H, W] input')
    if x.dtype not in _DTYPES:
        raise NotImplementedError(f'input dtype {x.dtype}: the trainable image conv takes float32 or bfloat16 images')
    if not 1 <= int(x.shape[1]) <= IMAGE_MAX_IN_CHANNELS:
        raise NotImplementedError(f'input of {int(x.shape[1])} channels: the trainable image conv takes 1 ... {IMAGE_MAX_IN_CHANNELS}')
    if min(int(v) for v in x.shape) < 1:
        raise NotImplementedError(f'input of size {tuple(x.shape)}: the trainable image conv needs at least one pixel')


def image_pack_weight(weight):
    """weight [Cout, C, 3, 3] (float32 | bfloat16, on the GPU) -> the bf16 records [3][Cout][16] the conv's loop reads, packed on the
    device: filter row, output channel, (kx 0..3, c 0..3) with zeros at kx = 3 and c >= C."""
    _check_image_weight(weight)
    _need_cuda(weight)
    w = weight.detach().contiguous()
    cout, c = int(w.shape[0]), int(w.shape[1])
    packed = torch.empty((3, cout, 16), dtype=torch.bfloat16, device=w.device)
    _lib.check(_lib.load().cpn_image_conv_pack(_lib.ptr(w), _DTYPES[w.dtype], cout, c, _lib.ptr(packed), _lib.stream_ptr()),
               'image_conv_pack')
    return packed


def _image_pad(x):
    """x [N, C <= 4, H, W] -> the padded input bf16 [N, H + 2, W + 3, 4] (zero border, zeros in the channels >= C)."""
    n, c, h, w = (int(v) for v in x.shape)
    src = x.detach().float().contiguous()  # (bf16 -> fp32 is exact; the kernel rounds fp32 to bf16, to nearest even)
    xq = torch.empty((n, h + 2, w + 3, 4), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.load().cpn_image_conv_pad(_lib.ptr(src), n, c, h, w, _lib.ptr(xq), _lib.stream_ptr()), 'image_conv_pad')
    return xq


def _image_forward(xq, size, packed, bias):
    n, h, w = size
    cout = int(packed.shape[1])
    out = torch.empty((n, cout, h, w), dtype=torch.bfloat16, device=xq.device, memory_format=torch.channels_last)
    _lib.check(_lib.load().cpn_image_conv_forward(_lib.ptr(xq), _lib.ptr(packed), _lib.ptr(bias), n, h, w, cout, _lib.ptr(out),
                                                  _lib.stream_ptr()), 'image_conv_forward')
    return out


def image_weight_grad_info(n, h, w, cout, slab_rows=0):
    """What ``image_weight_grad`` would run on an ``h x w`` image -> dict(slabs, slab_rows (image rows per slab), steps (MFMA steps
    per slab), reduce_chain, bias_chain).  Host arithmetic only: needs no GPU.  Raises like the launch for a call it rejects."""
    return _weight_grad_info('image_conv', n, h, w, cout, slab_rows)


def _image_wgrad(xq, size, c, gs, slab_rows, weight, bias, dtype, bias_dtype):
    """xq: the padded input; gs: bf16 NHWC memory, 16-byte aligned -> (dW | None, db | None).  The launch takes the image's channel
    count ``c``; the workspace query does not."""
    n, h, w = size
    cout = int(gs.shape[1])
    return _weight_grad('image_conv', (n, h, w, cout, slab_rows), lambda: (xq, gs), (cout, c, 3, 3), xq.device, weight, bias,
                        (dtype, bias_dtype), torch.zeros, launch_geometry=(n, h, w, c, cout, slab_rows))


def image_weight_grad(x, grad_output, slab_rows=0, weight=True, bias=True, dtype=torch.float32, bias_dtype=None):
    """(x [N, C <= 4, H, W], grad_output [N, Cout, H, W]) -> (dW [Cout, C, 3, 3] | None, db [Cout] | None): the gradients
    ``image_conv2d`` returns for its weight and bias, as fp32 sums over the bf16-rounded operands rounded once to ``dtype`` /
    ``bias_dtype``.  ``slab_rows``: image rows per slab of the reduction (0: chosen by the library)."""
    _check_image_input(x)
    n, c, h, w = (int(v) for v in x.shape)
    cout = int(grad_output.shape[1])
    if cout not in IMAGE_OUT_CHANNELS:
        raise NotImplementedError(f'out_channels {cout}: the trainable image conv writes {IMAGE_OUT_CHANNELS} only')
    dtype, bias_dtype = _grad_dtypes(dtype, bias_dtype)
    want = (n, cout, h, w)
    assert tuple(grad_output.shape) == want, (tuple(grad_output.shape), want)
    _need_cuda(x, grad_output)
    return _image_wgrad(_image_pad(x), (n, h, w), c, _nhwc(grad_output, torch.bfloat16), slab_rows, weight, bias, dtype, bias_dtype)


class _ImageConv2dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        n, c, h, w = (int(v) for v in x.shape)
        xq = _image_pad(x)
        b32 = None if bias is None else bias.detach().float().contiguous()
        out = _image_forward(xq, (n, h, w), image_pack_weight(weight), b32)
        ctx.save_for_backward(xq)  # the padded bf16 input alone: neither x nor the weight is needed again
        ctx.size, ctx.c = (n, h, w), c
        ctx.weight_dtype = weight.dtype
        ctx.bias_dtype = None if bias is None else bias.dtype
        return out

    @staticmethod
    def backward(ctx, grad_output):
        xq, = ctx.saved_tensors
        _, need_w, need_b = ctx.needs_input_grad
        need_b = need_b and ctx.bias_dtype is not None
        dw = db = None
        if need_w or need_b:
            dw, db = _image_wgrad(xq, ctx.size, ctx.c, _nhwc(grad_output, torch.bfloat16), 0, need_w, need_b, ctx.weight_dtype,
                                  ctx.bias_dtype or ctx.weight_dtype)
        return None, dw, db


def image_conv2d(x, weight, bias=None):
    """``torch.nn.functional.conv2d(x, weight, bias, stride=1, padding=1)`` for a 3x3 ``weight [Cout in {32, 64, 128}, C <= 4, 3, 3]``
    -> bf16 [N, Cout, H, W] in ``torch.channels_last``, with gradients for ``weight`` and ``bias`` as autograd asks for them.  The
    image gets no gradient: ``x.requires_grad`` raises ``NotImplementedError``.  Image values must be finite."""
    _check_image_input(x)
    _check_image_weight(weight)
    if int(x.shape[1]) != int(weight.shape[1]):
        raise ValueError(f'input has {int(x.shape[1])} channels, weight expects {int(weight.shape[1])}')
    if bias is not None and (bias.dim() != 1 or bias.shape[0] != weight.shape[0] or bias.dtype not in _DTYPES):
        raise NotImplementedError(f'bias {tuple(bias.shape)} {bias.dtype}: the trainable image conv takes a float32 or bfloat16 [Cout] bias')
    if x.requires_grad:
        raise NotImplementedError('x requires a gradient: the trainable image conv has no input gradient (the image needs none; '
                                  'detach x)')
    _need_cuda(x, weight, bias)
    return _ImageConv2dFunction.apply(x, weight, bias)


class ImageConv2d(torch.nn.Conv2d):
    """``torch.nn.Conv2d`` with torch's constructor arguments and parameter names (``weight``, ``bias``: ``state_dict``s
    interchange) whose forward is ``image_conv2d``.  ``kernel_size``, ``stride`` and ``padding`` default to 3, 1 and 1; an argument
    outside the supported family raises ``NotImplementedError`` naming it."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=1, bias=True,
                 padding_mode='zeros', device=None, dtype=None):
        why = _image_unsupported(kernel_size, stride, padding, dilation, groups, padding_mode, in_channels, out_channels)
        if why is not None:
            raise NotImplementedError(why)
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device, dtype)

    def forward(self, x):
        return image_conv2d(x, self.weight, self.bias)


def _image_why_not(conv):
    if type(conv) is not torch.nn.Conv2d:
        return f'a subclass of torch.nn.Conv2d ({type(conv).__name__}): its forward may differ'
    if conv.weight.dtype not in _DTYPES:
        return f'weight dtype {conv.weight.dtype}: float32 or bfloat16 only'
    return _image_unsupported(conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.padding_mode,
                              conv.in_channels, conv.out_channels, conv.transposed)


def _is_image_business(conv):
    """A 3x3 conv from at most 4 channels: what a reader would take for the first conv of a U-Net encoder."""
    return conv.in_channels <= IMAGE_MAX_IN_CHANNELS and _pair(conv.kernel_size) == (3, 3)
