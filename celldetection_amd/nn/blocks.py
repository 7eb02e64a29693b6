"""The three blocks that are made of the families' modules, each with the rule that says which stock block it can stand for:
``Bottleneck``, ``UNetDecoder`` and ``CPNCore``.  convert.py swaps eligible blocks in place.

The bottleneck block of a ResNeXt encoder ("Trainable bottleneck block" of include/cpn_hip.h).  Three pieces beside the convs and
norms make a whole block run here: the norm's residual tail (``batch_norm(..., residual=)``), the strided 1x1 shortcut conv of a
stage entry (``strided_conv1x1``) and the block-input gradient in the epilogue of conv1's dgrad conv (``conv2d_fork``).
``Bottleneck`` puts them together.  Known limit: at a stage entry the shortcut's norm and the tail are two kernels
(``relu(bn3(h) + bn_d(h_d))`` is not one pass).

The decoder of the reference's ``GeneralizedUNet`` ("Trainable concat convolution" of include/cpn_hip.h; cat_conv.py):
``UNetDecoder`` runs every level's first conv as a ``CatConv2d`` and the level's 1x1 ``inner`` conv before the resize.

The reference's ``CPNCore`` ("Trainable bilinear resize" of include/cpn_hip.h; resize.py): ``CPNCore`` puts ``ResizedConv2d`` and
``bilinear_resize`` where the reference's core calls ``F.interpolate``.
"""
import torch

from ._common import _pair
from .batch_norm import BatchNorm2d, _bn_why_not
from .cat_conv import CatConv2d
from .conv import Conv2d, _why_not
from .grouped import GroupedConv2d, StridedConv1x1, _grouped_why_not, _strided_why_not
from .resize import ResizedConv2d, _resized_why_not, bilinear_resize


class Bottleneck(torch.nn.Module):
    """The bottleneck block of a ResNet / ResNeXt encoder under torchvision's child names (``conv1``, ``bn1``, ``conv2``, ``bn2``,
    ``conv3``, ``bn3``, ``relu``, ``downsample``: ``state_dict`` keys do not move), made of this package's pieces::

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
