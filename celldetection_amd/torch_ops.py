"""PyTorch custom-op registration (``torch.library``) of the HIP kernels behind the C ABI.

``BASELINE.json.north_star``: the kernels are "called from Python via PyTorch-ROCm custom ops (thin C-ABI)".  The ops of
``celldetection_amd.ops`` are registered in the ``cpn_hip`` namespace so that they are addressable as
``torch.ops.cpn_hip.<name>`` (dispatcher-visible, GPU only -- there is no CPU kernel, a CPU tensor raises), and
``install_torchvision_nms()`` provides ``torch.ops.torchvision.nms`` on ROCm systems without torchvision, which is the
operator the reference calls directly (celldetection/ops/cpn.py:181,211,216,223; celldetection_scripts/cpn_inference.py:407,
426; celldetection/models/lightning_cpn.py:167): with it those call sites run on the HIP NMS without being edited.
"""
import torch
from typing import Optional

from torch import Tensor

from . import ops as _ops

__all__ = ['install_torchvision_nms', 'NAMESPACE']

NAMESPACE = 'cpn_hip'
OVERLAY_NAMESPACE = 'celldetection_amd'  # torch.ops.celldetection_amd.contours2overlay / .label_cmap / .labels2contours_packed / .resample_contours / .labels2distances / .cpn_objective
_lib_keepalive = []


@torch.library.custom_op(f'{NAMESPACE}::nms', mutates_args=(), device_types='cuda')
def nms(boxes: Tensor, scores: Tensor, iou_threshold: float) -> Tensor:
    """torchvision.ops.nms semantics on the HIP kernels (dense bit mask or spatially binned, by size)."""
    return _ops.nms(boxes, scores, iou_threshold)


@nms.register_fake
def _(boxes, scores, iou_threshold):
    return boxes.new_empty((torch.library.get_ctx().new_dynamic_size(),), dtype=torch.int64)


@torch.library.custom_op(f'{NAMESPACE}::fouriers2contours', mutates_args=(), device_types='cuda')
def fouriers2contours(fourier: Tensor, locations: Tensor, samples: int) -> Tensor:
    """celldetection/ops/cpn.py:44-95 (default sampling): [..., order, 4], [..., 2] -> [..., samples, 2]."""
    return _ops.fouriers2contours(fourier, locations, samples)[0]


@fouriers2contours.register_fake
def _(fourier, locations, samples):
    return fourier.new_empty(fourier.shape[:-2] + (samples, 2), dtype=torch.float32)


@torch.library.custom_op(f'{NAMESPACE}::local_refinement', mutates_args=(), device_types='cuda')
def local_refinement(contours: Tensor, refinement: Tensor, num_loops: int, b: Tensor, num_buckets: int) -> Tensor:
    """celldetection/models/cpn.py:63-85."""
    return _ops.local_refinement(contours, refinement, num_loops, b, num_buckets=num_buckets)


@local_refinement.register_fake
def _(contours, refinement, num_loops, b, num_buckets):
    return torch.empty_like(contours, dtype=torch.float32)


@torch.library.custom_op(f'{NAMESPACE}::remove_border_contours', mutates_args=(), device_types='cuda')
def remove_border_contours(contours: Tensor, height: int, width: int, padding: float, sides: int, offset_x: float,
                           offset_y: float) -> Tensor:
    """celldetection/ops/cpn.py:258-290; sides: bit0 top, bit1 right, bit2 bottom, bit3 left."""
    return _ops.remove_border_contours(contours, (height, width), padding, top=bool(sides & 1), right=bool(sides & 2),
                                       bottom=bool(sides & 4), left=bool(sides & 8), offsets=(offset_x, offset_y))


@remove_border_contours.register_fake
def _(contours, height, width, padding, sides, offset_x, offset_y):
    return contours.new_empty((contours.shape[0],), dtype=torch.bool)


@torch.library.custom_op(f'{NAMESPACE}::box_votes', mutates_args=(), device_types='cuda')
def box_votes(boxes: Tensor, thresh: float) -> Tensor:
    """get_iou_voting, celldetection/ops/boxes.py:52-58."""
    from . import _lib
    bx = boxes.contiguous().float()
    votes = torch.empty((bx.shape[0],), dtype=torch.float32, device=bx.device)
    _lib.check(_lib.load().cpn_box_votes(_lib.ptr(bx), int(bx.shape[0]), float(thresh), _lib.ptr(votes),
                                         _lib.stream_ptr()), 'box_votes')
    return votes


@box_votes.register_fake
def _(boxes, thresh):
    return boxes.new_empty((boxes.shape[0],), dtype=torch.float32)


@torch.library.custom_op(f'{NAMESPACE}::label_pair_table', mutates_args=(), device_types='cuda')
def label_pair_table(inputs: Tensor, targets: Tensor) -> Tensor:
    """Pixel pass of the instance evaluation (celldetection/data/instance_eval.py:22-50): label images [H, W(, C)] ->
    int64 [N, 2] rows (key, count), keys ascending; see ``instance_eval.label_pair_table``."""
    from . import instance_eval
    return instance_eval.label_pair_table(inputs, targets)


@label_pair_table.register_fake
def _(inputs, targets):
    return inputs.new_empty((torch.library.get_ctx().new_dynamic_size(), 2), dtype=torch.int64)


@torch.library.custom_op(f'{NAMESPACE}::resolve_label_channels', mutates_args=(), device_types='cuda')
def resolve_label_channels(labels: Tensor, max_iter: int) -> Tensor:
    """Flat label image (celldetection/data/cpn.py:361-399, default kernel): label image [H, W, C] -> [H, W]; see
    ``flat_labels.resolve_label_channels``."""
    from . import flat_labels
    return flat_labels.resolve_label_channels(labels, max_iter=max_iter)


@resolve_label_channels.register_fake
def _(labels, max_iter):
    return labels.new_empty(labels.shape[:2])


@torch.library.custom_op(f'{NAMESPACE}::region_properties', mutates_args=(), device_types='cuda')
def region_properties(labels: Tensor, properties: str, spacing_row: float, spacing_col: float) -> Tensor:
    """Region property table (celldetection/data/misc.py:320-347): label image [H, W(, C)] and comma-separated property names
    -> float64 [rows, columns], integer columns converted; see ``region_props.region_properties`` for names and order."""
    from . import region_props
    cols = region_props.region_properties(labels, tuple(p for p in properties.split(',') if p), spacing=(spacing_row, spacing_col))
    if not cols:
        return labels.new_empty((0, 0), dtype=torch.float64)
    return torch.stack([c.to(torch.float64) for c in cols.values()], 1)


@region_properties.register_fake
def _(labels, properties, spacing_row, spacing_col):
    from . import region_props
    names, _ = region_props._column_names(region_props._resolve(tuple(p for p in properties.split(',') if p)), '-', 0)
    return labels.new_empty((torch.library.get_ctx().new_dynamic_size(), len(names)), dtype=torch.float64)


@torch.library.custom_op(f'{OVERLAY_NAMESPACE}::contours2overlay', mutates_args=(), device_types='cuda')
def contours2overlay(contours: Tensor, colors: Tensor, height: int, width: int) -> Tensor:
    """RGBA overlay image (celldetection/data/cpn.py:811-855, default arguments): contours [K, S, 2] and their uint8 colours
    [K, 3] -> uint8 [height, width, 4]; see ``overlay.contours2overlay``."""
    from . import overlay
    return overlay.contours2overlay(contours, (height, width), colors=colors)


@contours2overlay.register_fake
def _(contours, colors, height, width):
    return contours.new_empty((height, width, 4), dtype=torch.uint8)


@torch.library.custom_op(f'{OVERLAY_NAMESPACE}::label_cmap', mutates_args=(), device_types='cuda')
def label_cmap(labels: Tensor, table: Tensor) -> Tensor:
    """Colour-mapped label image (celldetection/visualization/cmaps.py:21-77 with ubyte=True): label image [H, W(, C)] and
    float colours [n, 3 | 4] in [0, 1] -> uint8 [H, W, 4]; see ``overlay.label_cmap``."""
    from . import overlay
    return overlay.label_cmap(labels, colors=table, ubyte=True)


@label_cmap.register_fake
def _(labels, table):
    return labels.new_empty(tuple(labels.shape[:2]) + (4,), dtype=torch.uint8)


@torch.library.custom_op(f'{OVERLAY_NAMESPACE}::labels2contours_packed', mutates_args=(), device_types='cuda')
def labels2contours_packed(labels: Tensor, raise_fragmented: bool) -> tuple[Tensor, Tensor, Tensor]:
    """Contours of a label image (celldetection/data/cpn.py:93-144, RETR_EXTERNAL / CHAIN_APPROX_NONE): label image [H, W, C] ->
    ids int32 [K], offsets int64 [K + 1], points int32 [P, 2]; fragmented objects raise or are skipped (flagging in place is
    left to the Python function); see ``label_contours.labels2contours_packed``."""
    from . import label_contours
    return label_contours.labels2contours_packed(labels, raise_fragmented=raise_fragmented)


@labels2contours_packed.register_fake
def _(labels, raise_fragmented):
    ctx = torch.library.get_ctx()
    k, p = ctx.new_dynamic_size(), ctx.new_dynamic_size()
    return (labels.new_empty((k,), dtype=torch.int32), labels.new_empty((k + 1,), dtype=torch.int64),
            labels.new_empty((p, 2), dtype=torch.int32))


@torch.library.custom_op(f'{OVERLAY_NAMESPACE}::resample_contours', mutates_args=(), device_types='cuda')
def resample_contours(points: Tensor, offsets: Tensor, num: int, close: bool, epsilon: float) -> Tensor:
    """Equidistant points on packed contours (celldetection/data/misc.py:371-405): points [P, 2], offsets int64 [K + 1] ->
    float64 [K, num, 2]; see ``label_contours.resample_contours_packed``."""
    from . import label_contours
    return label_contours.resample_contours_packed(points, offsets, num, close, epsilon)


@resample_contours.register_fake
def _(points, offsets, num, close, epsilon):
    return points.new_empty((offsets.shape[0] - 1, num, 2), dtype=torch.float64)


@torch.library.custom_op(f'{OVERLAY_NAMESPACE}::labels2distances', mutates_args=(), device_types='cuda')
def labels2distances(labels: Tensor, distance_type: int, per_instance: bool, protected_size: int) -> tuple[Tensor, Tensor]:
    """Distance map of a label image (celldetection/data/cpn.py:432-497, overlap_zero=True): label image [H, W(, C)] -> distances
    float32 [H, W] and the labels [H, W, C] with overlap pixels set to -1; see ``targets.labels2distances``."""
    from . import targets
    return targets.labels2distances(labels, distance_type=distance_type, per_instance=per_instance, protected_size=protected_size)


@labels2distances.register_fake
def _(labels, distance_type, per_instance, protected_size):
    return (labels.new_empty(tuple(labels.shape[:2]), dtype=torch.float32),
            labels.new_empty(tuple(labels.shape[:2]) + (labels.shape[2] if labels.ndim == 3 else 1,)))


@torch.library.custom_op(f'{OVERLAY_NAMESPACE}::cpn_objective', mutates_args=(), device_types='cuda')
def cpn_objective(scores: Tensor, locations: Tensor, refinement: Optional[Tensor], fourier: Tensor, labels: Tensor,
                  target_fourier: Tensor, target_locations: Tensor, target_contours: Tensor, sampling: Tensor, height: int, width: int,
                  classes: int, refinement_iterations: int, refinement_buckets: int,
                  order_weights: bool) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """CPN training objective (celldetection/models/cpn.py:441-692) with the reference's default weights: the four head maps and
    the batch targets -> float32 [9] (the eight terms in the reference's order, NaN where a term does not apply, then the loss)
    and the gradients of the loss by scores, locations, fourier and refinement (an empty tensor without a refinement map); see
    ``objective.CPNObjective``, which is the differentiable form."""
    from . import objective
    obj = objective.CPNObjective(int(target_fourier.shape[2]), int(sampling.shape[1]), classes=classes, refinement=refinement is not None,
                                 refinement_iterations=refinement_iterations, refinement_buckets=refinement_buckets,
                                 order_weights=order_weights)
    targets = dict(labels=labels, fourier=target_fourier, locations=target_locations, sampled_contours=target_contours,
                   sampling=sampling)
    out, _, grads, _ = objective._run(obj, scores, locations, refinement, fourier, targets, (height, width), [True] * 4, False)
    return out, grads[0], grads[1], grads[3], grads[2] if grads[2] is not None else scores.new_empty((0,))


@cpn_objective.register_fake
def _(scores, locations, refinement, fourier, labels, target_fourier, target_locations, target_contours, sampling, height, width,
      classes, refinement_iterations, refinement_buckets, order_weights):
    return (scores.new_empty((9,)), torch.empty_like(scores), torch.empty_like(locations), torch.empty_like(fourier),
            torch.empty_like(refinement) if refinement is not None and refinement_iterations > 0 else scores.new_empty((0,)))


def install_torchvision_nms(force: bool = False) -> bool:
    """Defines ``torchvision::nms`` (schema of torchvision's operator) with the HIP implementation for GPU tensors when
    torchvision is not installed, so that the reference's ``torch.ops.torchvision.nms(...)`` call sites dispatch to
    libcpn_hip.so unchanged.  With torchvision present nothing is touched unless ``force`` (then the CUDA/HIP kernel of
    the existing operator is overridden).  Returns True when the HIP implementation is active."""
    try:
        has = hasattr(torch.ops.torchvision, 'nms') and torch.ops.torchvision.nms is not None
        if has:
            torch.ops.torchvision.nms.default  # resolves only when the operator really exists
    except (AttributeError, RuntimeError):
        has = False
    impl = lambda dets, scores, iou_threshold: _ops.nms(dets, scores, float(iou_threshold))
    if not has:
        lib = torch.library.Library('torchvision', 'DEF')
        lib.define('nms(Tensor dets, Tensor scores, float iou_threshold) -> Tensor')
        lib.impl('nms', impl, 'CUDA')
        _lib_keepalive.append(lib)
        return True
    if force:
        lib = torch.library.Library('torchvision', 'IMPL')
        lib.impl('nms', impl, 'CUDA', allow_override=True) if 'allow_override' in lib.impl.__code__.co_varnames \
            else lib.impl('nms', impl, 'CUDA')
        _lib_keepalive.append(lib)
        return True
    return False
