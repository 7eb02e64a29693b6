"""Training on the MI355X: the operations a training step of the reference model runs, each as one ``torch.autograd.Function`` on
this library's HIP kernels, the drop-in ``torch.nn`` modules on top of them and the converts that put those into a stock model
in place.  Nothing here falls back to a stock operation: what a family does not run raises ``NotImplementedError`` naming the
argument, and a convert leaves it and says why.  One module per family holds the functional form, the module and the rule of what
is supported (with its known limits), in the order a step meets them:

* stem.py: ``stem_conv2d`` / ``StemConv2d``, the 7x7 stride-2 conv from at most 4 channels; pool.py: ``max_pool2d`` / ``MaxPool2d``;
* image_conv.py: ``image_conv2d`` / ``ImageConv2d``, the 3x3 stride-1 conv from at most 4 channels that a U-Net encoder starts with;
* conv.py: ``conv2d`` / ``Conv2d``, dense stride-1 convs with channel counts in multiples of 32, and ``conv2d_fork``;
* batch_norm.py: ``batch_norm`` / ``BatchNorm2d`` with an optional fused ReLU and an optional residual operand;
* grouped.py: ``grouped_conv2d`` / ``GroupedConv2d``, the 3x3 ``conv2`` of a ResNeXt block at stride 1 and 2, and the strided 1x1
  shortcut ``strided_conv1x1`` / ``StridedConv1x1`` with ``subsample2d``;
* cat_conv.py: ``cat_conv2d`` / ``CatConv2d``, the decoder's nearest resize + concat + conv, and ``nearest_resize_backward``;
* readout_tail.py: ``dropout_conv1x1`` / ``DropoutConv1x1``, the ``Dropout2d -> Conv 1x1`` tail of a ReadOut head;
* resize.py: ``bilinear_resize``, its adjoint ``bilinear_resize_backward`` and ``resized_conv2d`` / ``ResizedConv2d``;
* blocks.py: ``Bottleneck``, ``UNetDecoder`` and ``CPNCore``, the three blocks made of the modules above;
* convert.py: ``convert_conv2d_``, ``convert_batchnorm2d_``, ``convert_readout_tail_``, ``convert_grouped_conv2d_``,
  ``convert_stem_conv2d_``, ``convert_image_conv2d_``, ``convert_maxpool2d_`` and the block-level ``convert_bottleneck_``,
  ``convert_unet_decoder_`` and ``convert_cpn_core_``.  They work in any order with the same result; after all ten a training step
  of the reference model, with a ResNet, ResNeXt or U-Net encoder, has no stock operation between the image and the head maps.

_common.py holds what the families share.  The rules are the "Trainable ..." sections of include/cpn_hip.h; ``cda.models.*`` stay
inference-only.  The step ends outside this package: ``cda.optim`` clips the gradients by their global norm and applies AdamW on the
same library ("Optimizer step" of the header).
"""
from .batch_norm import ACTIVATIONS, BatchNorm2d, batch_norm, batch_norm_forward, batch_norm_info
from .blocks import Bottleneck, CPNCore, UNetDecoder
from .cat_conv import CAT_KERNEL_SIZES, CatConv2d, cat_conv2d, cat_conv2d_weight_grad, cat_weight_grad_info, nearest_resize_backward
from .conv import KERNEL_SIZES, Conv2d, conv2d, conv2d_fork, conv2d_weight_grad, is_supported, pack_weight, weight_grad_info
from .convert import (convert_batchnorm2d_, convert_bottleneck_, convert_conv2d_, convert_cpn_core_, convert_grouped_conv2d_,
                      convert_image_conv2d_, convert_maxpool2d_, convert_readout_tail_, convert_stem_conv2d_, convert_unet_decoder_)
from .grouped import (GROUP_WIDTHS, GroupedConv2d, StridedConv1x1, grouped_conv2d, grouped_conv2d_weight_grad, grouped_dilate,
                      grouped_pack_weight, grouped_weight_grad_info, strided_conv1x1, subsample2d)
from .image_conv import (IMAGE_MAX_IN_CHANNELS, IMAGE_OUT_CHANNELS, ImageConv2d, image_conv2d, image_pack_weight, image_weight_grad,
                         image_weight_grad_info)
from .pool import POOL_GEOMETRIES, MaxPool2d, max_pool2d
from .readout_tail import (TAIL_MAX_CIN, TAIL_MAX_COUT, DropoutConv1x1, dropout_conv1x1, dropout_conv1x1_backward,
                           readout_tail_info)
from .resize import (RESIZED_KERNEL_SIZES, ResizedConv2d, bilinear_resize, bilinear_resize_backward, resized_conv2d,
                     resized_conv2d_weight_grad, resized_weight_grad_info)
from .stem import (STEM_MAX_IN_CHANNELS, STEM_OUT_CHANNELS, StemConv2d, stem_conv2d, stem_pack_weight, stem_weight_grad,
                   stem_weight_grad_info)

__all__ = ['conv2d', 'Conv2d', 'convert_conv2d_', 'is_supported', 'pack_weight', 'conv2d_weight_grad', 'weight_grad_info',
           'batch_norm', 'batch_norm_forward', 'batch_norm_info', 'BatchNorm2d', 'convert_batchnorm2d_',
           'dropout_conv1x1', 'dropout_conv1x1_backward', 'readout_tail_info', 'DropoutConv1x1', 'convert_readout_tail_',
           'grouped_conv2d', 'GroupedConv2d', 'convert_grouped_conv2d_', 'grouped_weight_grad_info', 'grouped_conv2d_weight_grad',
           'grouped_pack_weight', 'grouped_dilate',
           'conv2d_fork', 'strided_conv1x1', 'StridedConv1x1', 'subsample2d', 'Bottleneck', 'convert_bottleneck_',
           'cat_conv2d', 'CatConv2d', 'cat_conv2d_weight_grad', 'cat_weight_grad_info', 'nearest_resize_backward', 'UNetDecoder',
           'convert_unet_decoder_',
           'stem_conv2d', 'StemConv2d', 'convert_stem_conv2d_', 'stem_pack_weight', 'stem_weight_grad', 'stem_weight_grad_info',
           'image_conv2d', 'ImageConv2d', 'convert_image_conv2d_', 'image_pack_weight', 'image_weight_grad', 'image_weight_grad_info',
           'max_pool2d', 'MaxPool2d', 'convert_maxpool2d_',
           'bilinear_resize', 'bilinear_resize_backward', 'resized_conv2d', 'ResizedConv2d', 'resized_conv2d_weight_grad',
           'resized_weight_grad_info', 'CPNCore', 'convert_cpn_core_']
