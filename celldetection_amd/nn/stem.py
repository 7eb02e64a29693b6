"""The stem of a ResNet encoder and the max-pool ("Trainable stem and max-pool" of include/cpn_hip.h, csrc/stem_train.hip,
csrc/image_train.h, csrc/pool_train.hip, csrc/pool_adjoint.h; the Python both convs share: nn/_image_family.py)

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
import functools

import torch

from . import _image_family as _family

STEM_OUT_CHANNELS = (32, 64)
STEM_MAX_IN_CHANNELS = 4

# the pad is the inference stem's input conversion (csrc/stem.hip), which takes more arguments than the image needs
STEM = _family.ImageFamily(noun='the trainable stem', kernel=7, stride=2, padding=3, out_channels=STEM_OUT_CHANNELS, pad_rows=6, pad_cols=8,
                           record=32, pack='stem_train_pack', pad='convert_input_stem',
                           pad_args=lambda src, dst, n, c, h, w, stream: (src, 0, dst, n, c, h, w, None, stream),
                           forward='stem_train_forward', wgrad='stem', max_in_channels=STEM_MAX_IN_CHANNELS)

_stem_pad = functools.partial(_family.pad, STEM)  # x -> the padded input bf16 [N, H + 6, W + 8, 4]
_stem_forward = functools.partial(_family.run_forward, STEM)
_stem_wgrad = functools.partial(_family.wgrad, STEM)
_stem_why_not = functools.partial(_family.why_not, STEM)
_StemConv2dFunction = _family.ImageConv2dFunction


def stem_pack_weight(weight):
    """weight [Cout, C, 7, 7] (float32 | bfloat16, on the GPU) -> the bf16 records [7][Cout][32] the stem loop reads, packed on the
    device: filter row, output channel, (kx 0..7, c 0..3) with zeros at kx = 7 and c >= C."""
    return _family.pack_weight(STEM, weight)


def stem_weight_grad_info(n, h, w, cout, slab_rows=0):
    """What ``stem_weight_grad`` would run on an ``h x w`` image -> dict(slabs, slab_rows (output rows per slab), steps (MFMA steps
    per slab), reduce_chain, bias_chain).  Host arithmetic only: needs no GPU.  Raises like the launch for a call it rejects."""
    return _family.weight_grad_info(STEM, n, h, w, cout, slab_rows)


def stem_weight_grad(x, grad_output, slab_rows=0, weight=True, bias=True, dtype=torch.float32, bias_dtype=None):
    """(x [N, C <= 4, H, W], grad_output [N, Cout, Hout, Wout]) -> (dW [Cout, C, 7, 7] | None, db [Cout] | None): the gradients
    ``stem_conv2d`` returns for its weight and bias, as fp32 sums over the bf16-rounded operands rounded once to ``dtype`` /
    ``bias_dtype``.  ``slab_rows``: output rows per slab of the reduction (0: chosen by the library)."""
    return _family.weight_grad(STEM, x, grad_output, slab_rows, weight, bias, dtype, bias_dtype)


def stem_conv2d(x, weight, bias=None):
    """``torch.nn.functional.conv2d(x, weight, bias, stride=2, padding=3)`` for a 7x7 ``weight [Cout in {32, 64}, C <= 4, 7, 7]`` ->
    bf16 [N, Cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1] in ``torch.channels_last``, with gradients for ``weight`` and ``bias`` as
    autograd asks for them.  The image gets no gradient: ``x.requires_grad`` raises ``NotImplementedError``."""
    return _family.conv2d(STEM, x, weight, bias)


class StemConv2d(_family.ImageFamilyConv2d):
    """``torch.nn.Conv2d`` with torch's constructor arguments and parameter names (``weight``, ``bias``: ``state_dict``s
    interchange) whose forward is ``stem_conv2d``.  ``kernel_size``, ``stride`` and ``padding`` default to 7, 2 and 3; an argument
    outside the supported family raises ``NotImplementedError`` naming it."""
    family = STEM

    def __init__(self, in_channels, out_channels, kernel_size=7, stride=2, padding=3, dilation=1, groups=1, bias=True,
                 padding_mode='zeros', device=None, dtype=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode, device, dtype)


def _is_stem_business(conv):
    """A conv from at most 4 channels, or a 7x7 conv of stride 2: what a reader would take for a stem."""
    return conv.in_channels <= STEM_MAX_IN_CHANNELS or (_family._pair(conv.kernel_size) == (7, 7) and _family._pair(conv.stride) == (2, 2))
