"""Component labelling on the MI355X: ``relabel_`` / ``stack_labels`` / ``unary_masks2labels`` / ``fill_label_gaps_`` /
``remove_partials_`` of the reference's ``cd.data`` (celldetection/data/segmentation.py:10-41, 106-167), ``masks2labels``
(celldetection/data/cpn.py:147-176) and ``rgb_to_scalar`` (celldetection/data/misc.py:264-280), backed by ``csrc/components.hip``.
It is the entry of the label pipeline: annotations and segmentation results become label images in which every object is one
``(channel, value)`` pair with exactly one connected component, which is what every other label function of this package assumes:

    stack = cda.stack_labels(gray_map, rgb_map)               # int32 [H, W, 2] on the GPU, relabelled
    labels = cda.masks2labels(masks, reduce=None)             # binary masks [N, H, W] -> int32 [H, W, N]
    flat = cda.resolve_label_channels(labels)[..., None]      # may cut an object in two ...
    cda.relabel_(flat)                                        # ... each piece becomes an object of its own
    contours = cda.labels2contours(flat)                      # never reports a fragmented object now

The rule of ``label_components`` (restated in ``tests/components_oracle.py``, ``include/cpn_hip.h`` and the kernel file, pinned to
the reference's recorded results in ``tests/golden/components.npz``).  Every channel is labelled on its own.  A pixel takes part
if it is foreground; two neighbouring foreground pixels are linked if they are equal.  ``mode='equal'``: foreground is ``v > 0``,
equal is the same value.  ``mode='nonzero'``: foreground is ``v != 0`` and any two foreground pixels are equal.  Neighbours are the 4
edge neighbours (``connectivity=4``) or the 8 neighbours (``connectivity=8``).  Components are numbered ``first, first + 1, ...`` by
channel ascending and, within a channel, by the raster index ``y * W + x`` of their first pixel.  Pixels that take no part keep
their value: zeros, and in ``'equal'`` mode negatives.  This is ``skimage.measure.label(background=0)`` per channel with a
numbering that runs on across the channels; ``relabel_`` calls it with full connectivity (8 in 2-D), and the components it skips
because they hold a negative pixel are, under the equal-value rule, exactly the components of negative value.

``masks2labels`` is ``'nonzero'`` mode per mask with the running offset of the reference's loop, its two counting quirks
included: a mask without foreground still advances the count by 1, and a mask without any background pixel advances it by one
more than its components.  Numbering inside one mask is raster-first for both connectivities.  For ``connectivity=8`` OpenCV's
default algorithm scans 2 x 2 blocks and may number the components of one mask in another order: there the partition and the set
of labels per mask are the contract, the order within a mask is ours.

OpenCV and skimage are absent from the build image: ``skimage.morphology.label`` and ``cv2.connectedComponents`` are third-party
arithmetic restated from their documentation, and unpinned; the fixture pins the reference's own code around them.

Known limits.  ``relabel_`` and ``stack_labels`` take the channel axis last only (``axis=2``); 2-D images only (no 3-D
labelling); ``rle2mask`` and ``boxes2masks`` are not implemented.
"""
import numpy as np
import torch

from . import _lib
from ._label_input import INT32_MAX, check_labels, to_int32, upload_numpy
from ._lib import check, ptr, stream_ptr
from .targets import _inplace_int32, filter_instances_

__all__ = ['label_components', 'relabel_', 'stack_labels', 'rgb_to_scalar', 'unary_masks2labels', 'masks2labels',
           'fill_label_gaps_', 'remove_partials_']

MAX_CHANNELS = 65535


def _check_rule(name, connectivity, mode, first=1):
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f'{name}: connectivity must be 4 or 8 (got {connectivity!r})')
    if not isinstance(mode, str) or mode not in _lib.COMPONENTS_MODES:
        raise ValueError(f"{name}: mode must be 'equal' or 'nonzero' (got {mode!r})")
    if isinstance(first, bool) or not isinstance(first, (int, np.integer)) or not 1 <= int(first) <= INT32_MAX:
        raise ValueError(f'{name}: first must be an int from 1 to 2 ** 31 - 1 (got {first!r})')


def _check_size(name, C, H, W):
    if H * W > INT32_MAX:
        raise NotImplementedError(f'{name}: more than 2 ** 31 - 1 pixels')
    if C > MAX_CHANNELS:
        raise NotImplementedError(f'{name}: more than {MAX_CHANNELS} channels')


def _as_tensor(x, name, what='labels'):
    """A Tensor as it is, a numpy array uploaded."""
    if isinstance(x, np.ndarray):
        if x.dtype == np.bool_:
            x = x.astype(np.uint8)
        if x.dtype.kind not in 'iu':
            raise TypeError(f'{name}: {what} must hold integers (got {x.dtype})')
        return upload_numpy(x, name, f'{what} holds values')
    return x


def _run(x, strides, C, H, W, connectivity, mode, first, out, out_strides):
    """One cpn_components_label call on int32 tensors -> counts int32 [C] on the device."""
    lib = _lib.load()
    with torch.cuda.device(x.device):
        counts = torch.empty((C,), dtype=torch.int32, device=x.device)
        nbytes = int(lib.cpn_components_workspace_bytes(C, H, W))
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=x.device)
        check(lib.cpn_components_label(ptr(x), strides[0], strides[1], C, H, W, connectivity, _lib.COMPONENTS_MODES[mode], int(first),
                                       ptr(out), out_strides[0], out_strides[1], ptr(counts), ptr(ws), stream_ptr()),
              'components_label')
    return counts


def label_components(labels, connectivity=8, mode='equal', first=1, out=None):
    """Label image Tensor[H, W, C] or [H, W] (integers, on the GPU, or a numpy array that is uploaded) -> ``(labels, counts)``:
    the image with every component numbered by the rule of the module text, and the components per channel, int32 [C] on the
    GPU.  ``out=None`` returns a new tensor of the input's dtype; ``out=labels`` works in place; any other ``out`` must be an
    int32 contiguous GPU tensor of the input's shape.  More than ``2 ** 31 - first`` components raise instead of wrapping."""
    _check_rule('label_components', connectivity, mode, first)
    labels = _as_tensor(labels, 'label_components')
    if out is not None and out is not labels:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or not out.is_contiguous() or \
                tuple(out.shape) != tuple(getattr(labels, 'shape', ())):
            raise ValueError('label_components: out must be labels itself or an int32 contiguous Tensor of the same shape')
    check_labels(labels, 'label_components', ranks=(2, 3))
    if out is not None and out.device != labels.device:
        raise RuntimeError('celldetection_amd.label_components runs on the MI355X only (out on another device).')
    H, W = int(labels.shape[0]), int(labels.shape[1])
    C = int(labels.shape[2]) if labels.ndim == 3 else 1
    _check_size('label_components', C, H, W)
    box = []

    def run(x, dst=None):
        dst = x if dst is None else dst
        box.append(_run(x, (C, 1), C, H, W, connectivity, mode, first, dst, (C, 1)))
        top = torch.iinfo(labels.dtype).max
        if top < INT32_MAX and (out is None or out is labels) and int(first) - 1 + int(box[0].sum(dtype=torch.int64)) > top:
            raise ValueError(f'label_components: the largest new label does not fit {labels.dtype}')  # before any write-back

    if out is labels:
        _inplace_int32(labels, 'label_components', run)
        return labels, box[0]
    x = to_int32(labels, 'label_components: labels holds values that do not fit int32')
    if out is None:
        out = x if x.data_ptr() != labels.data_ptr() else torch.empty_like(x)  # a converted copy is ours to overwrite
        run(x, out)
        return out.to(labels.dtype), box[0]
    run(x, out)
    return out, box[0]


def relabel_(label_stack, axis=2):
    """The reference's ``cd.data.relabel_`` (data/segmentation.py:106-130), in place on the GPU tensor (or numpy array)
    ``label_stack`` [H, W, C]: afterwards every 8-connected equal-value component of every channel is an object of its own, numbered
    from 1 on, cumulatively over the channels, in raster order of the components' first pixels.  Zeros and negative values are
    untouched.  Only the last axis can be the channel axis."""
    if not isinstance(label_stack, (torch.Tensor, np.ndarray)):
        raise TypeError(f'relabel_: label_stack must be a Tensor on the GPU or a numpy array (got {type(label_stack).__name__})')
    if label_stack.ndim != 3:
        raise ValueError(f'relabel_: label_stack must be [H, W, C] (got {tuple(label_stack.shape)})')
    if isinstance(axis, bool) or axis not in (2, -1):
        raise NotImplementedError(f'relabel_: only the last axis can be the channel axis, axis=2 (got axis={axis!r}); move the '
                                  'channel axis last')
    if isinstance(label_stack, np.ndarray):
        x = _as_tensor(label_stack, 'relabel_', 'label_stack')
        _, counts = label_components(x, 8, 'equal', 1, out=x)
        if int(counts.sum(dtype=torch.int64)) > np.iinfo(label_stack.dtype).max:
            raise ValueError(f'relabel_: the largest new label does not fit {label_stack.dtype}')
        label_stack[...] = x.cpu().numpy().astype(label_stack.dtype)
        return
    check_labels(label_stack, 'relabel_')
    label_components(label_stack, 8, 'equal', 1, out=label_stack)


def _torch_dtype(dtype, name):
    if isinstance(dtype, torch.dtype):
        dt = dtype
    else:
        try:
            dt = getattr(torch, np.dtype(dtype).name, None)
        except TypeError:
            dt = None
    if not isinstance(dt, torch.dtype) or dt.is_floating_point or dt.is_complex or dt == torch.bool:
        raise TypeError(f'{name}: dtype must be an integer dtype that torch computes with (got {dtype!r})')
    return dt


def rgb_to_scalar(inputs, dtype='int32'):
    """The reference's ``cd.data.rgb_to_scalar`` (data/misc.py:264-280): colour-coded Tensor[..., 3] (or numpy array) ->
    Tensor[...] of ``dtype`` on the GPU, ``(red << 16) + (green << 8) + blue`` computed in ``dtype``: distinct colours stay
    distinct.  Plain tensor operations (one elementwise pass)."""
    dt = _torch_dtype(dtype, 'rgb_to_scalar')
    inputs = _as_tensor(inputs, 'rgb_to_scalar', 'inputs')
    if not isinstance(inputs, torch.Tensor):
        raise TypeError(f'rgb_to_scalar: inputs must be a Tensor on the GPU or a numpy array (got {type(inputs).__name__})')
    if inputs.ndim < 1 or inputs.shape[-1] < 3:
        raise ValueError(f'rgb_to_scalar: inputs must be [..., 3] (got {tuple(inputs.shape)})')
    if inputs.is_floating_point() or inputs.is_complex():
        raise TypeError(f'rgb_to_scalar: inputs must hold integers (got {inputs.dtype})')
    if not inputs.is_cuda:
        raise RuntimeError('celldetection_amd.rgb_to_scalar runs on the MI355X only (got a CPU tensor).')
    red, green, blue = inputs[..., 0], inputs[..., 1], inputs[..., 2]
    rgb = red.to(dt)
    rgb = (rgb << 8) + green
    rgb = (rgb << 8) + blue
    return rgb


def stack_labels(*maps, axis=2, dtype='int32', relabel=True):
    """The reference's ``cd.data.stack_labels`` (data/segmentation.py:133-150): label maps [H, W] and colour-coded maps [H, W, 3]
    (Tensors on the GPU or numpy arrays) -> Tensor[H, W, len(maps)] of ``dtype`` on the GPU; colour-coded maps go through
    ``rgb_to_scalar``; with ``relabel`` the stack goes through ``relabel_``.  Only ``axis=2`` is implemented."""
    dt = _torch_dtype(dtype, 'stack_labels')
    if isinstance(axis, bool) or axis not in (2, -1):
        raise NotImplementedError(f'stack_labels: only the last axis can be the stacking axis, axis=2 (got axis={axis!r})')
    if not maps:
        raise ValueError('stack_labels: needs at least one map')
    if len(maps) > MAX_CHANNELS:
        raise NotImplementedError(f'stack_labels: more than {MAX_CHANNELS} maps')
    planes = []
    for i, m in enumerate(maps):
        if not isinstance(m, (torch.Tensor, np.ndarray)):
            raise TypeError(f'stack_labels: map {i} must be a Tensor on the GPU or a numpy array (got {type(m).__name__})')
        if not (m.ndim == 2 or (m.ndim == 3 and m.shape[2] == 3)):
            raise ValueError(f'stack_labels: map {i} must be [H, W] or [H, W, 3] (got {tuple(m.shape)})')
        if tuple(m.shape[:2]) != tuple(maps[0].shape[:2]):
            raise ValueError(f'stack_labels: map {i} is {tuple(m.shape[:2])}, map 0 is {tuple(maps[0].shape[:2])}')
        m = _as_tensor(m, 'stack_labels', f'map {i}')
        if m.is_floating_point() or m.is_complex():
            raise TypeError(f'stack_labels: map {i} must hold integers (got {m.dtype})')
        if not m.is_cuda:
            raise RuntimeError('celldetection_amd.stack_labels runs on the MI355X only (got a CPU tensor).')
        planes.append(rgb_to_scalar(m, dtype=dt) if m.ndim == 3 else m.to(dt))
    stack = torch.stack(planes, 2)
    if relabel:
        relabel_(stack, 2)
    return stack


def _stack_masks(masks, name):
    if isinstance(masks, (list, tuple)):
        if not len(masks):
            raise ValueError(f'{name}: needs at least one mask')
        masks = [_as_tensor(m, name, 'masks') for m in masks]
        for m in masks:
            if not isinstance(m, torch.Tensor) or m.ndim != 2 or m.shape != masks[0].shape:
                raise ValueError(f'{name}: a list holds masks [H, W] of one size')
        if any(not m.is_cuda for m in masks):
            raise RuntimeError(f'celldetection_amd.{name} runs on the MI355X only (got a CPU tensor).')
        masks = torch.stack(masks)
    masks = _as_tensor(masks, name, 'masks')
    if not isinstance(masks, torch.Tensor):
        raise TypeError(f'{name}: masks must be a Tensor[N, H, W] on the GPU, a numpy array or a list of masks [H, W] '
                        f'(got {type(masks).__name__})')
    if masks.ndim != 3:
        raise ValueError(f'{name}: masks must be [N, H, W] (got {tuple(masks.shape)})')
    if masks.is_complex():
        raise TypeError(f'{name}: masks must be real (got {masks.dtype})')
    if not masks.is_cuda:
        raise RuntimeError(f'celldetection_amd.{name} runs on the MI355X only (got a CPU tensor).')
    return masks


def unary_masks2labels(unary_masks, transpose=True):
    """The reference's ``cd.data.unary_masks2labels`` (data/segmentation.py:153-167): one mask per object, Tensor[N, H, W] (or a
    list of [H, W]) -> int64 label image [H, W, N] (``transpose``) or [N, H, W]: mask ``i`` holds ``i + 1`` where it is ``> 0``.
    Plain tensor operations (one elementwise pass)."""
    m = _stack_masks(unary_masks, 'unary_masks2labels')
    lbl = (m > 0) * torch.arange(1, m.shape[0] + 1, dtype=torch.int64, device=m.device)[:, None, None]
    return lbl.permute(1, 2, 0) if transpose else lbl


def masks2labels(masks, connectivity=8, label_axis=2, count=False, reduce='max', keepdims=True):
    """The reference's ``cd.data.masks2labels`` (data/cpn.py:147-176): binary masks Tensor[N, H, W] (or a list of [H, W]; any
    non-zero element is foreground) -> int32 label maps, one per mask, stacked along ``label_axis`` and reduced over it by
    ``reduce`` (``'max'`` or ``np.max``; ``None``: not reduced); with ``count`` also the reference's running count.  The offset of
    every mask follows the reference's loop, its two counting quirks included (module text); inside a mask the components are
    numbered in raster order of their first pixels."""
    _check_rule('masks2labels', connectivity, 'nonzero')
    if not (reduce is None or reduce is np.max or (isinstance(reduce, str) and reduce == 'max')):
        raise TypeError(f"masks2labels: reduce must be 'max', np.max or None (got {reduce!r})")
    if isinstance(label_axis, bool) or label_axis not in (0, 1, 2, -1, -2, -3):
        raise ValueError(f'masks2labels: label_axis must be 0, 1 or 2 (got {label_axis!r})')
    m = _stack_masks(masks, 'masks2labels')
    N, H, W = (int(s) for s in m.shape)
    if N < 1:
        raise ValueError('masks2labels: needs at least one mask')
    _check_size('masks2labels', N, H, W)
    x = (m != 0).to(torch.int32) if m.is_floating_point() or m.dtype == torch.bool else \
        to_int32(m, 'masks2labels: masks holds values that do not fit int32')
    out = torch.empty((N, H, W), dtype=torch.int32, device=x.device)
    comps = _run(x, (1, H * W), N, H, W, connectivity, 'nonzero', 1, out, (1, H * W)).cpu().numpy().astype(np.int64)
    has_zero = (x == 0).flatten(1).any(1).cpu().numpy() if H * W else np.zeros(N, bool)
    # cv2.connectedComponents returns a = components + 1; the reference adds a - (1 if (a > 1 and 0 in b) else 0) to its count
    a = comps + 1
    advance = a - ((a > 1) & has_zero)
    before = np.concatenate([[0], np.cumsum(advance)[:-1]])  # the reference's cnt when it reaches mask i
    extra = before - np.concatenate([[0], np.cumsum(comps)[:-1]])  # ours is the plain running number of components
    cnt = int(advance.sum())
    if cnt > INT32_MAX:
        raise ValueError('masks2labels: the running count does not fit int32')
    if extra.any():
        out += torch.as_tensor(extra, dtype=torch.int32).to(out.device)[:, None, None] * (out > 0)
    labels = torch.movedim(out, 0, label_axis)
    if reduce is not None:
        labels = labels.amax(dim=label_axis, keepdim=bool(keepdims))
    return (labels, cnt) if count else labels


def fill_label_gaps_(labels):
    """The reference's ``cd.data.fill_label_gaps_`` (data/segmentation.py:22-40), in place on the GPU tensor ``labels`` [H, W, C] or
    [H, W]: afterwards the ``n`` distinct positive labels are ``1 .. n``; labels ``<= n`` stay, labels ``> n`` take the missing
    values, largest label to largest gap.  Values ``<= 0`` stay.  The table ``filter_instances_`` builds, and nothing else of it."""
    return filter_instances_(labels, partials=False, min_area=None, max_area=None, continuous=True)


def remove_partials_(label_stack, border=1, constant=-1):
    """The reference's ``cd.data.remove_partials_`` (data/segmentation.py:10-19), in place on the GPU tensor ``label_stack``
    [H, W, C] or [H, W]: every value other than 0 that occurs in the outer ``border`` rows or columns becomes ``constant``
    wherever it occurs.  -> ``(label_stack, mask)``, ``mask`` the bool tensor of the changed elements (``None`` for ``border < 1``)."""
    check_labels(label_stack, 'remove_partials_', ranks=(2, 3))
    if border < 1:
        return label_stack, None
    b = int(border)
    edge = torch.unique(torch.cat([s.reshape(-1) for s in (label_stack[:, :b], label_stack[:, -b:], label_stack[:b], label_stack[-b:])]))
    mask = torch.isin(label_stack, edge[edge != 0])
    filter_instances_(label_stack, partials=True, partials_border=b, min_area=None, max_area=None, constant=constant, continuous=False)
    return label_stack, mask
