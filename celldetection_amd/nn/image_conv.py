"""The first conv of a U-Net encoder ("Trainable image conv" of include/cpn_hip.h, csrc/image_conv_train.hip,
csrc/image_train.h; the Python it shares with the stem: nn/_image_family.py)

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
import functools

import torch

from . import _image_family as _family

IMAGE_OUT_CHANNELS = (32, 64, 128)
IMAGE_MAX_IN_CHANNELS = 4

IMAGE = _family.ImageFamily(noun='the trainable image conv', kernel=3, stride=1, padding=1, out_channels=IMAGE_OUT_CHANNELS, pad_rows=2,
                            pad_cols=3, record=16, pack='image_conv_pack', pad='image_conv_pad',
                            pad_args=lambda src, dst, n, c, h, w, stream: (src, n, c, h, w, dst, stream),
                            forward='image_conv_forward', wgrad='image_conv', max_in_channels=IMAGE_MAX_IN_CHANNELS)

_image_pad = functools.partial(_family.pad, IMAGE)  # x -> the padded input bf16 [N, H + 2, W + 3, 4]
_image_forward = functools.partial(_family.run_forward, IMAGE)
_image_wgrad = functools.partial(_family.wgrad, IMAGE)
_image_why_not = functools.partial(_family.why_not, IMAGE)
_ImageConv2dFunction = _family.ImageConv2dFunction


def image_pack_weight(weight):
    """weight [Cout, C, 3, 3] (float32 | bfloat16, on the GPU) -> the bf16 records [3][Cout][16] the conv's loop reads, packed on the
    device: filter row, output channel, (kx 0..3, c 0..3) with zeros at kx = 3 and c >= C."""
    return _family.pack_weight(IMAGE, weight)


def image_weight_grad_info(n, h, w, cout, slab_rows=0):
    """What ``image_weight_grad`` would run on an ``h x w`` image -> dict(slabs, slab_rows (image rows per slab), steps (MFMA steps
    per slab), reduce_chain, bias_chain).  Host arithmetic only: needs no GPU.  Raises like the launch for a call it rejects."""
    return _family.weight_grad_info(IMAGE, n, h, w, cout, slab_rows)


def image_weight_grad(x, grad_output, slab_rows=0, weight=True, bias=True, dtype=torch.float32, bias_dtype=None):
    """(x [N, C <= 4, H, W], grad_output [N, Cout, H, W]) -> (dW [Cout, C, 3, 3] | None, db [Cout] | None): the gradients
    ``image_conv2d`` returns for its weight and bias, as fp32 sums over the bf16-rounded operands rounded once to ``dtype`` /
    ``bias_dtype``.  ``slab_rows``: image rows per slab of the reduction (0: chosen by the library)."""
    return _family.weight_grad(IMAGE, x, grad_output, slab_rows, weight, bias, dtype, bias_dtype)


def image_conv2d(x, weight, bias=None):
    """``torch.nn.functional.conv2d(x, weight, bias, stride=1, padding=1)`` for a 3x3 ``weight [Cout in {32, 64, 128}, C <= 4, 3, 3]``
    -> bf16 [N, Cout, H, W] in ``torch.channels_last``, with gradients for ``weight`` and ``bias`` as autograd asks for them.  The
    image gets no gradient: ``x.requires_grad`` raises ``NotImplementedError``.  Image values must be finite."""
    return _family.conv2d(IMAGE, x, weight, bias)


class ImageConv2d(_family.ImageFamilyConv2d):
    """``torch.nn.Conv2d`` with torch's constructor arguments and parameter names (``weight``, ``bias``: ``state_dict``s
    interchange) whose forward is ``image_conv2d``.  ``kernel_size``, ``stride`` and ``padding`` default to 3, 1 and 1; an argument
    outside the supported family raises ``NotImplementedError`` naming it."""
    family = IMAGE

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=1, bias=True,
                 padding_mode='zeros', device=None, dtype=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device, dtype)


def _is_image_business(conv):
    """A 3x3 conv from at most 4 channels: what a reader would take for the first conv of a U-Net encoder."""
    return conv.in_channels <= IMAGE_MAX_IN_CHANNELS and _family._pair(conv.kernel_size) == (3, 3)
