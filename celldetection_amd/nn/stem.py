"""The stem of a ResNet encoder and the max-pool ("Trainable stem and max-pool" of include/cpn_hip.h, csrc/stem_train.hip,
csrc/pool_adjoint.h)

The first two modules a step runs: ``Conv2d(in_channels <= 4, 64, 7, stride=2, padding=3)`` and ``MaxPool2d(3, 2, 1)`` (the
reference's ``models/resnet.py:274-284``), and the ``MaxPool2d(2, 2)`` of the U-Net encoders.  ``stem_conv2d`` converts the image
to the padded 4-channel bf16 layout of the inference stem (csrc/stem.hip), in which the 7 taps of a filter row are contiguous,
and saves that tensor alone; the weight gradient is seven MFMA products per slab, one per filter row, with the flat output pixel as
the reduction index.  The image gets no gradient.  ``max_pool2d`` stores one ``uint8`` tap index per output element and saves
nothing else; its backward is a gather in a fixed order (no atomics, no scatter).

After ``convert_conv2d_``, ``convert_batchnorm2d_``, ``convert_grouped_conv2d_``, ``convert_bottleneck_``, ``convert_stem_conv2d_`` and
``convert_maxpool2d_``, in any order, an encoder runs without a stock operation.  Known limits: batch-norm statistics are not
folded into the stem's epilogue; the pool is not fused into the norm's apply; the sum of the pool's gradient and a lateral's stays
autograd's add; 7x7 / stride 2 only (the 3x3 stride-1 first conv of the ``U22`` encoders is ``image_conv2d``, nn/image_conv.py);
``cda.models.*`` stay inference-only.
"""
import torch

from .. import _lib
from ..ops import _need_cuda
from ._common import _DTYPES, _grad_dtypes, _nhwc, _pair, _weight_grad, _weight_grad_info

STEM_OUT_CHANNELS = (32, 64)
STEM_MAX_IN_CHANNELS = 4


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
    return _weight_grad_info('stem', n, h, w, cout, slab_rows)


def _stem_wgrad(xp, size, c, gs, slab_rows, weight, bias, dtype, bias_dtype):
    """xp: the padded input; gs: bf16 NHWC memory, 16-byte aligned -> (dW | None, db | None).  The launch takes the image's channel
    count ``c``; the workspace query does not."""
    n, h, w = size
    cout = int(gs.shape[1])
    return _weight_grad('stem', (n, h, w, cout, slab_rows), lambda: (xp, gs), (cout, c, 7, 7), xp.device, weight, bias,
                        (dtype, bias_dtype), torch.zeros, launch_geometry=(n, h, w, c, cout, slab_rows))


def stem_weight_grad(x, grad_output, slab_rows=0, weight=True, bias=True, dtype=torch.float32, bias_dtype=None):
    """(x [N, C <= 4, H, W], grad_output [N, Cout, Hout, Wout]) -> (dW [Cout, C, 7, 7] | None, db [Cout] | None): the gradients
    ``stem_conv2d`` returns for its weight and bias, as fp32 sums over the bf16-rounded operands rounded once to ``dtype`` /
    ``bias_dtype``.  ``slab_rows``: output rows per slab of the reduction (0: chosen by the library)."""
    _check_stem_input(x)
    n, c, h, w = (int(v) for v in x.shape)
    cout = int(grad_output.shape[1])
    if cout not in STEM_OUT_CHANNELS:
        raise NotImplementedError(f'out_channels {cout}: the trainable stem writes {STEM_OUT_CHANNELS} only')
    dtype, bias_dtype = _grad_dtypes(dtype, bias_dtype)
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


def _is_stem_business(conv):
    """A conv from at most 4 channels, or a 7x7 conv of stride 2: what a reader would take for a stem."""
    return conv.in_channels <= STEM_MAX_IN_CHANNELS or (_pair(conv.kernel_size) == (7, 7) and _pair(conv.stride) == (2, 2))
