"""The in-place converts: each replaces the stock modules one family (or one block) runs by this library's drop-ins, which share
the ``Parameter`` and buffer objects of what they replace, and says what it left and why.  One walker, ``_walk``, and one adopt,
``_adopt``, serve all ten; the families' ``_*_why_not`` rules decide.  This module imports the families, never the reverse."""
import torch

from ._common import _pair
from .batch_norm import BatchNorm2d, _bn_why_not
from .blocks import (Bottleneck, CPNCore, UNetDecoder, _block_why_not, _core_why_not, _decoder_why_not, _is_reference_core,
                     _is_reference_unet, _is_torchvision_bottleneck)
from .cat_conv import CatConv2d
from .conv import Conv2d, _why_not
from .grouped import GroupedConv2d, StridedConv1x1, _grouped_why_not
from .image_conv import ImageConv2d, _image_why_not, _is_image_business
from .pool import MaxPool2d, _pool_why_not
from .readout_tail import DropoutConv1x1, _tail_why_not
from .resize import ResizedConv2d
from .stem import StemConv2d, _is_stem_business, _stem_why_not

# the convs of this library (ResizedConv2d is a Conv2d): what the per-module converts of convs skip
_OUR_CONVS = (Conv2d, DropoutConv1x1, GroupedConv2d, StridedConv1x1, CatConv2d, StemConv2d, ImageConv2d)


def _adopt(cls, module, **attributes):
    """``module`` as a ``cls`` without running a constructor: the same ``Parameter``, buffer and child objects, hooks, training flag
    and constructor attributes (``__dict__`` is shared entry by entry), the three registries the new module's own; ``attributes``
    are set on top (``p``, ``activation``)."""
    new = cls.__new__(cls)
    new.__dict__.update(module.__dict__)
    new._parameters, new._buffers, new._modules = dict(module._parameters), dict(module._buffers), dict(module._modules)
    for name, value in attributes.items():
        setattr(new, name, value)
    return new


def _walk(module, candidate, why_not, make, fuse=None, several=None):
    """The tree walk of every convert -> (names replaced, {name left: reason}).  Every slot of every module below ``module`` whose
    content ``candidate`` accepts is either left with the sentence ``why_not(child, parent)`` gives or filled with ``make(child,
    *extra)``, made once per object: an object that sits in several slots is replaced by one object in all of them.  ``several``
    (the block-level converts): what to call an object that sits in more than one slot, which is left instead, because it would
    run twice on different inputs.  ``fuse(parent, slots, i, uses, name)`` (the converts that take a neighbouring slot in) -> the
    ``extra`` arguments of ``make``; ``slots``: the parent's (name, module) pairs, ``uses``: slots per object id in the whole tree.
    The hook does that convert's slot surgery itself, before the replacement is made: where it takes the neighbour in, it puts
    ``torch.nn.Identity()`` into the neighbour's slot of ``parent`` and records what its convert reports.
    ``module`` itself cannot be replaced in place: a candidate is reported as left under the name ``''``."""
    replaced, left = [], {}
    if candidate(module):
        left[''] = why_not(module, None) or 'the root module cannot be replaced in place: convert its parent'
    uses = {}
    for parent in module.modules():
        for child in parent._modules.values():
            if child is not None:
                uses[id(child)] = uses.get(id(child), 0) + 1
    swapped = {}  # id of a replaced object -> its replacement
    for name, parent in list(module.named_modules()):
        slots = [(n, c) for n, c in parent._modules.items() if c is not None]  # (named_children() drops repeated objects)
        for i, (child_name, child) in enumerate(slots):
            if not candidate(child):
                continue
            full = f'{name}.{child_name}' if name else child_name
            why = why_not(child, parent)
            if why is None and several is not None and uses[id(child)] > 1:
                why = f'the {several} sits in {uses[id(child)]} slots'
            if why is not None:
                left[full] = why
                continue
            extra = () if fuse is None else fuse(parent, slots, i, uses, full)
            if id(child) not in swapped:
                swapped[id(child)] = make(child, *extra)
            setattr(parent, child_name, swapped[id(child)])
            replaced.append(full)
    return replaced, left


def _lone_neighbour(cls, slots, i, j, uses):
    """The module in slot ``j`` when it is exactly a ``cls`` and both it and the module in slot ``i`` occur once in the whole tree
    (one that sits in two slots runs twice and is not fused), else None."""
    near = slots[j][1] if 0 <= j < len(slots) else None
    return near if type(near) is cls and uses[id(near)] == 1 and uses[id(slots[i][1])] == 1 else None


def convert_conv2d_(module):
    """Replaces every eligible ``torch.nn.Conv2d`` below ``module`` in place by a ``Conv2d`` that shares its ``Parameter`` objects
    (optimisers and ``state_dict`` keys are unaffected) -> (names replaced, {name left: reason}).  ``module`` itself is not replaced
    when it is a conv: it is reported as left, by the rule for a child (a conv of this library is not reported, a ``_ConvNd`` that
    is not 2-D is).  A conv object that sits in several slots is replaced by one object in all of them;
    every other ``_ConvNd`` (1-D, 3-D, transposed) is left as not 2-D."""
    def why_not(conv, parent):
        return _why_not(conv) if isinstance(conv, torch.nn.Conv2d) else f'{type(conv).__name__}: 2-D convs only'

    return _walk(module, lambda m: isinstance(m, torch.nn.modules.conv._ConvNd) and not isinstance(m, _OUR_CONVS), why_not,
                 lambda conv: _adopt(Conv2d, conv))


def convert_batchnorm2d_(module, fuse_relu=True):
    """Replaces every eligible ``torch.nn.BatchNorm2d`` below ``module`` in place by a ``BatchNorm2d`` that shares its ``Parameter``
    and buffer objects -> (names replaced, names whose ReLU was fused, {name left: reason}).  With ``fuse_relu``, where the parent is
    an ``nn.Sequential`` and the slot right behind the norm holds exactly a ``torch.nn.ReLU`` that occurs once in the whole tree (as
    does the norm), the norm gets ``activation='relu'`` and the ReLU's slot becomes ``torch.nn.Identity()``: indices and
    ``state_dict`` keys do not move.  A norm object that sits in several slots is replaced by one object in all of them."""
    fused = []

    def fuse(parent, slots, i, uses, name):  # -> (activation,)
        if not (fuse_relu and isinstance(parent, torch.nn.Sequential)) or _lone_neighbour(torch.nn.ReLU, slots, i, i + 1, uses) is None:
            return (None,)
        setattr(parent, slots[i + 1][0], torch.nn.Identity())
        fused.append(name)
        return ('relu',)

    replaced, left = _walk(module, lambda m: isinstance(m, torch.nn.modules.batchnorm._NormBase) and not isinstance(m, BatchNorm2d),
                           lambda bn, parent: _bn_why_not(bn), lambda bn, activation: _adopt(BatchNorm2d, bn, activation=activation), fuse)
    return replaced, fused, left


def convert_readout_tail_(module):
    """Replaces, in every ``nn.Sequential`` below ``module`` (and ``module`` itself when it is one), each eligible 1x1
    ``torch.nn.Conv2d`` with at most 32 output channels in place by a ``DropoutConv1x1`` that shares its ``Parameter`` objects ->
    (names replaced, {name left: reason}).  Where the slot right in front holds exactly a ``torch.nn.Dropout2d`` and both modules
    occur once in the whole tree, the conv takes its ``p`` and that slot becomes ``torch.nn.Identity()``: indices and ``state_dict``
    keys do not move; otherwise the conv is replaced with ``p = 0``.  ``left`` names every other 1x1 conv (convs this library
    already runs excepted) with the reason.  Works before or after ``convert_conv2d_`` and ``convert_batchnorm2d_``."""
    def why_not(conv, parent):
        why = _tail_why_not(conv)
        if why is None and parent is not None and not isinstance(parent, torch.nn.Sequential):
            why = f'its parent is a {type(parent).__name__}, not an nn.Sequential'
        return why

    def fuse(parent, slots, i, uses, name):  # -> (p,)
        dropout = _lone_neighbour(torch.nn.Dropout2d, slots, i, i - 1, uses)
        if dropout is None:
            return (0.,)
        setattr(parent, slots[i - 1][0], torch.nn.Identity())
        return (dropout.p,)

    return _walk(module, lambda m: isinstance(m, torch.nn.Conv2d) and not isinstance(m, _OUR_CONVS) and _pair(m.kernel_size) == (1, 1),
                 why_not, lambda conv, p: _adopt(DropoutConv1x1, conv, p=float(p)), fuse)


def _convert_plain_conv2d(module, business, why_not, cls):
    """The walk of the converts whose candidate is a ``torch.nn.Conv2d`` that is none of this library's convs and that
    ``business`` takes for theirs; each becomes a ``cls`` unless ``why_not`` names a reason."""
    return _walk(module, lambda m: isinstance(m, torch.nn.Conv2d) and not isinstance(m, _OUR_CONVS) and business(m),
                 lambda conv, parent: why_not(conv), lambda conv: _adopt(cls, conv))


def convert_grouped_conv2d_(module):
    """Replaces every eligible plain ``torch.nn.Conv2d`` with ``groups > 1`` below ``module`` in place by a ``GroupedConv2d`` that
    shares its ``Parameter`` objects (optimisers and ``state_dict`` keys are unaffected) -> (names replaced, {name left: reason}).
    ``left`` names every other grouped conv with the reason; dense convs are not its business.  ``module`` itself is not replaced
    when it is such a conv: it is reported as left.  A conv object that sits in several slots is replaced by one object in all of
    them.  Works before or after the other converts."""
    return _convert_plain_conv2d(module, lambda m: m.groups > 1, _grouped_why_not, GroupedConv2d)


def convert_stem_conv2d_(module):
    """Replaces every eligible plain ``torch.nn.Conv2d`` below ``module`` -- ``in_channels <= 4``, ``out_channels`` 32 or 64, 7x7,
    stride 2, padding 3 with zeros, dilation 1, groups 1 -- in place by a ``StemConv2d`` that shares its ``Parameter`` objects
    (optimisers and ``state_dict`` keys are unaffected) -> (names replaced, {name left: reason}).  ``left`` names every other conv
    from at most 4 channels and every other 7x7 conv of stride 2 with the reason; the remaining convs are not its business.
    ``module`` itself is not replaced when it is such a conv: it is reported as left.  A conv object that sits in several slots is
    replaced by one object in all of them.  Works before or after the other converts."""
    return _convert_plain_conv2d(module, _is_stem_business, _stem_why_not, StemConv2d)


def convert_image_conv2d_(module):
    """Replaces every eligible plain ``torch.nn.Conv2d`` below ``module`` -- ``in_channels <= 4``, ``out_channels`` 32, 64 or 128,
    3x3, stride 1, padding 1 with zeros, dilation 1, groups 1: the first conv of a U-Net encoder -- in place by an ``ImageConv2d``
    that shares its ``Parameter`` objects (optimisers and ``state_dict`` keys are unaffected) -> (names replaced, {name left:
    reason}).  ``left`` names every other 3x3 conv from at most 4 channels with the reason; the remaining convs are not its business.
    ``module`` itself is not replaced when it is such a conv: it is reported as left.  A conv object that sits in several slots is
    replaced by one object in all of them.  Works before or after the other converts."""
    return _convert_plain_conv2d(module, _is_image_business, _image_why_not, ImageConv2d)


def convert_maxpool2d_(module):
    """Replaces every plain ``torch.nn.MaxPool2d`` of the two geometries below ``module`` in place by a ``MaxPool2d`` -> (names
    replaced, {name left: reason}).  Every other max-pool is left with a reason naming the argument (``C % 8`` shows at run time
    only: there the forward raises).  ``module`` itself is not replaced when it is a pool: it is reported as left.  A pool object
    that sits in several slots is replaced by one object in all of them.  Works before or after the other converts."""
    return _walk(module, lambda m: isinstance(m, torch.nn.MaxPool2d) and not isinstance(m, MaxPool2d),
                 lambda pool, parent: _pool_why_not(pool), lambda pool: _adopt(MaxPool2d, pool))


def _convert_child(child):
    """A stock child of an eligible block -> this library's module sharing its Parameter and buffer objects."""
    if isinstance(child, (Conv2d, GroupedConv2d, StridedConv1x1, BatchNorm2d)):
        return child
    if isinstance(child, torch.nn.BatchNorm2d):
        return _adopt(BatchNorm2d, child, activation=None)
    if child.groups > 1:
        return _adopt(GroupedConv2d, child)
    return _adopt(StridedConv1x1 if _pair(child.stride) != (1, 1) else Conv2d, child)


def _block_from_torch(block):
    new = _adopt(Bottleneck, block)  # with the block's own attributes (stride, ...)
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
    return _walk(module, lambda m: not isinstance(m, Bottleneck) and (_is_torchvision_bottleneck(type(m)) or type(m) in block_types),
                 lambda block, parent: _block_why_not(block), _block_from_torch, several='block')


def _decoder_from_torch(dec):
    new = _adopt(UNetDecoder, dec)  # with the decoder's own attributes (has_lat, bridges, out_channels, ...)
    for i, m in enumerate(dec.inner_blocks):  # the ModuleLists and Sequentials stay the objects they are: their slots are filled anew
        if type(m) is torch.nn.Conv2d:
            dec.inner_blocks[i] = _adopt(Conv2d, m)
    for block in dec.layer_blocks:
        if not isinstance(block[0], CatConv2d):
            block[0] = _adopt(CatConv2d, block[0])
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
    return _walk(module, lambda m: not isinstance(m, UNetDecoder) and (_is_reference_unet(type(m)) or type(m) in decoder_types),
                 lambda dec, parent: _decoder_why_not(dec), _decoder_from_torch, several='decoder')


def _core_from_torch(core):
    new = _adopt(CPNCore, core)  # with the core's own attributes (order, feature keys, ...)
    head = core.refinement_head
    if head is not None and core.refinement_full_res and not isinstance(head.block[0], ResizedConv2d):
        head.block[0] = _adopt(ResizedConv2d, head.block[0])  # the Sequential stays the object it is: its slot is filled anew
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
    return _walk(module, lambda m: not isinstance(m, CPNCore) and (_is_reference_core(type(m)) or type(m) in core_types),
                 lambda core, parent: _core_why_not(core), _core_from_torch, several='core')
