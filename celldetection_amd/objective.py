"""CPN training objective on the MI355X: the loss terms of the reference's ``CPN.forward(inputs, targets)`` in training mode
(celldetection/models/cpn.py:561-692, ``compute_loss`` :441-559) and the gradients of the four head maps, backed by
``csrc/cpn_objective.hip``.  It consumes what ``CPNTargetGenerator`` builds:

    objective = cda.CPNObjective(order=5, samples=64, refinement_buckets=6)
    targets = cda.collate_cpn_targets(generators)                    # fed CPNTargetGenerators, one per image
    loss, losses = objective(scores, locations, refinement, fourier, targets, size=(H, W))
    loss.backward()                                                  # fills the .grad of the four maps

The four maps are what the reference's ``CPNCore.forward`` returns (raw score logits, relative locations, the refinement map or
``None``, the Fourier map), float32 on the GPU.  ``losses`` is the reference's ``OrderedDict`` (``fourier``, ``location``,
``contour``, ``score``, ``refinement``, ``boxes``, ``iou``, ``uncertainty``): float32 scalars on the GPU, ``None`` for a term that did
not apply; ``loss`` is their float32 sum in that order.  The rule is stated in ``include/cpn_hip.h`` ("Training objective"),
restated in ``tests/objective_oracle.py`` and pinned to the reference's recorded results in ``tests/golden/objective.npz``.

The call is one ``torch.autograd.Function``: its forward computes the terms and the gradients of the maps that require grad,
``backward`` only scales the stored gradients by the incoming scalar.  Only ``loss`` carries a gradient; the entries of ``losses``
are detached.  With ``objective.full_detail = True`` a call leaves ``objective.last_detail``: ``proposals`` [P, S, 2], ``refined``
(list of [P, S, 2], one per iteration, clamped), ``boxes`` [P, 4] and ``index`` (b, y, x).

Stated departures and limits.
* Every term is a float64 sum and mean rounded to float32 once, where the reference sums and divides in float32; the loss is the
  float32 sum of these terms.  The gradients are the analytic float64 derivatives rounded once.
* A mean that is not finite counts as 0 like ``add_to_loss_dict``, but the gradients do not know: inputs are taken to be finite.
  ``order=1`` with ``order_weights=True`` gives NaN weights in the reference (0 / 0 in ``order_weighting``) and so a zero fourier
  term with NaN gradients at every proposal; this is reproduced.
* ``samples`` must equal the length of ``targets['sampling']`` (the reference ignores ``samples`` when a sampling is given).
* The call synchronises twice: ``targets['sampling']`` goes to the host (the cos / sin and bucket tables are built there with
  the reference's expressions, as ``ops.fouriers2contours`` does), and the number of proposals is read for sizing.
* A map that is not contiguous is copied.
* Not implemented (``NotImplementedError``): an uncertainty map or head (``BoxNpllLoss``), a ``boxes`` objective or explicit
  ``boxes`` targets, ``hires_sampled_contours``, ``certainty_thresh``, ``functional=True``, user-supplied objective modules.
"""
from collections import OrderedDict
from ctypes import byref

import numpy as np
import torch

from . import _lib
from ._lib import check, stream_ptr

__all__ = ['CPNObjective', 'collate_cpn_targets', 'order_weighting', 'LOSS_KEYS', 'DEFAULT_WEIGHTS']

LOSS_KEYS = ('fourier', 'location', 'contour', 'score', 'refinement', 'boxes', 'iou', 'uncertainty')
DEFAULT_WEIGHTS = {'fourier': 1., 'location': 1., 'contour': 3., 'score_bg': 1., 'score_fg': 1., 'refinement': 1., 'boxes': .88,
                   'iou': 1., 'uncertainty': 1.}  # models/cpn.py:425-435
MAX_LABEL = 1 << 24  # the reference moves labels through float32 (downsample_labels)
MAX_ORDER = 64


class DeviceError(RuntimeError, ValueError):
    """A tensor that is not on the GPU: there is no CPU fallback."""


def order_weighting(order, max_w=5, min_w=1, spread=None):
    """ops/cpn.py:230-235 -> float32 [order, 1] on the CPU."""
    x = torch.arange(order).float()
    if spread is None:
        spread = order - 1
    y = min_w + (max_w - min_w) * (1 - (x / spread).clamp(0., 1.)) ** 2
    return y[:, None]


def _tables(sampling, order, buckets, device):
    """cos / sin [N, order, S] and, with buckets > 1, bucket index / weight [N, 3, S] of every image's sampling, built on the host
    with the reference's expressions (ops/cpn.py:66-78, 238-255)."""
    t = sampling.detach().to(torch.float32).cpu()
    c = float(np.pi) * 2 * (torch.arange(1, order + 1)[..., None]) * t[:, None, :]
    out = [torch.cos(c).contiguous().to(device), torch.sin(c).contiguous().to(device), None, None]
    if buckets > 1:
        base = t * buckets
        whole = base.long()
        idx, wgt = [], []
        for j in (whole - 1, whole, whole + 1):
            dist = torch.abs(j + 0.5 - base)
            wgt.append(torch.where(dist > 1, torch.zeros_like(dist), 1. - dist))
            idx.append(j % buckets)
        out[2] = torch.stack(idx, 1).to(torch.int32).contiguous().to(device)
        out[3] = torch.stack(wgt, 1).to(torch.float32).contiguous().to(device)
    return out


def _check(scores, locations, refinement, fourier, targets, size, obj):
    """Types and shapes, then the device.  Returns the shape numbers."""
    name = 'CPNObjective'
    if not isinstance(targets, dict):
        raise TypeError(f'{name}: targets must be a dict of tensors')
    for key, what in (('boxes', 'explicit boxes targets'), ('hires_sampled_contours', 'hires_sampled_contours')):
        if targets.get(key) is not None:
            raise NotImplementedError(f'{name}: {what} are not implemented')
    maps = OrderedDict(scores=scores, locations=locations, fourier=fourier)
    if refinement is not None:
        maps['refinement'] = refinement
    need = ['labels', 'fourier', 'locations', 'sampled_contours', 'sampling']
    for key in need:
        if targets.get(key) is None:
            raise ValueError(f"{name}: targets['{key}'] is missing")
    tensors = dict(maps)
    tensors.update({f"targets['{k}']": targets[k] for k in need})
    if targets.get('classes') is not None:
        tensors["targets['classes']"] = targets['classes']
    for key, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{name}: {key} must be a Tensor (got {type(t).__name__})')
    for key, t in maps.items():
        if t.dtype != torch.float32 or t.ndim != 4:
            raise TypeError(f'{name}: {key} must be a float32 Tensor[N, C, h, w] (got {t.dtype}, {tuple(t.shape)})')
    labels = targets['labels']
    if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise TypeError(f"{name}: targets['labels'] must hold integers (got {labels.dtype})")
    if len(size) != 2:
        raise ValueError(f'{name}: size must be (H, W)')
    H, W = (int(s) for s in size)
    N, cs, h, w = (int(s) for s in scores.shape)
    want_cs = 1 if obj.classes in (1, 2) else obj.classes
    shapes = {'scores': (N, want_cs, h, w), 'locations': (N, 2, h, w), "targets['labels']": (N, H, W)}
    if refinement is not None:
        shapes['refinement'] = (N, 2 * obj.refinement_buckets, H, W)
    for key, shape in shapes.items():
        if tuple(tensors[key].shape) != shape:
            raise ValueError(f'{name}: {key} must have the shape {shape} (got {tuple(tensors[key].shape)})')
    if tuple(fourier.shape[:1] + fourier.shape[2:]) != (N, h, w) or fourier.shape[1] % 4 or fourier.shape[1] < 4 * obj.order:
        raise ValueError(f'{name}: fourier must have the shape ({N}, 4 * order_core, {h}, {w}) with order_core >= {obj.order} '
                         f'(got {tuple(fourier.shape)})')
    if not 1 <= h <= H or not 1 <= w <= W:
        raise ValueError(f'{name}: the head grid {(h, w)} must not be larger than size {(H, W)}')
    sampling = targets['sampling']
    if sampling.ndim != 2 or sampling.shape[0] != N or sampling.shape[1] != obj.samples:
        raise ValueError(f"{name}: targets['sampling'] must have the shape ({N}, samples = {obj.samples}) (got {tuple(sampling.shape)})")
    S = obj.samples
    tf = targets['fourier']
    if tf.ndim != 4 or tf.shape[0] != N or tuple(tf.shape[2:]) != (obj.order, 4):
        raise ValueError(f"{name}: targets['fourier'] must have the shape ({N}, K, {obj.order}, 4) (got {tuple(tf.shape)})")
    K = int(tf.shape[1])
    shapes = {"targets['locations']": (N, K, 2), "targets['sampled_contours']": (N, K, S, 2)}
    if targets.get('classes') is not None:
        shapes["targets['classes']"] = (N, K)
    for key, shape in shapes.items():
        if tuple(tensors[key].shape) != shape:
            raise ValueError(f'{name}: {key} must have the shape {shape} (got {tuple(tensors[key].shape)})')
    for key, t in tensors.items():
        if not t.is_cuda:
            raise DeviceError(f'celldetection_amd.CPNObjective runs on the MI355X GPU only ({key} is on {t.device}); there is '
                              f'no CPU fallback.')
        if t.device != scores.device:
            raise ValueError(f'{name}: {key} is on {t.device}, scores on {scores.device}')
    return N, cs, h, w, H, W, K, S


def _run(obj, scores, locations, refinement, fourier, targets, size, need, detail):
    """One call of the kernels.  need: which of (scores, locations, refinement, fourier) get a gradient buffer.
    -> (out float32 [9]: the eight terms and the loss, present bits, gradients (four, None where not needed), detail or None)."""
    N, cs, h, w, H, W, K, S = _check(scores, locations, refinement, fourier, targets, size, obj)
    dev = scores.device
    lib = _lib.load()
    refine = refinement is not None and obj.refinement and obj.refinement_iterations > 0
    maps = [t.detach().contiguous() for t in (scores, locations, fourier)]
    ref = refinement.detach().contiguous() if refine else None
    labels = targets['labels'].detach()
    if labels.dtype not in (torch.int32, torch.int64):
        labels = labels.to(torch.int32)
    labels = labels.contiguous()
    f32 = lambda t: t.detach().to(torch.float32).contiguous()
    tf, tl, tc = f32(targets['fourier']), f32(targets['locations']), f32(targets['sampled_contours'])
    cls = targets.get('classes')
    cls = cls.detach().to(torch.int32).contiguous() if cls is not None and cs > 1 else None
    ow = obj.order_weights_tensor
    ow = None if ow is None else ow.to(torch.float32).reshape(-1).contiguous().to(dev)
    with torch.cuda.device(dev):
        cos_t, sin_t, bidx, bw = _tables(targets['sampling'], obj.order, obj.refinement_buckets if refine else 1, dev)
        grads = [torch.empty_like(m) if n else None for m, n in zip((maps[0], maps[1], ref, maps[2]),
                                                                   (need[0], need[1], need[2] and refine, need[3]))]
        a = _lib.ObjectiveArgs()
        p = lambda t: None if t is None else t.data_ptr()
        a.scores, a.locations, a.fourier, a.refinement, a.labels = p(maps[0]), p(maps[1]), p(maps[2]), p(ref), p(labels)
        a.t_fourier, a.t_locations, a.t_contours, a.t_classes = p(tf), p(tl), p(tc), p(cls)
        a.cos_table, a.sin_table, a.bucket_index, a.bucket_weight, a.order_weights = p(cos_t), p(sin_t), p(bidx), p(bw), p(ow)
        a.g_scores, a.g_locations, a.g_refinement, a.g_fourier = (p(g) for g in grads)
        wt = obj.weights
        a.w_fourier, a.w_location, a.w_contour, a.w_refinement, a.w_iou = (float(wt[k]) for k in (
            'fourier', 'location', 'contour', 'refinement', 'iou'))
        a.w_score_fg, a.w_score_bg = float(wt['score_fg']), float(wt['score_bg'])
        a.N, a.score_channels, a.h, a.w, a.H, a.W = N, cs, h, w, H, W
        a.order_total, a.order, a.samples, a.K = int(fourier.shape[1]) // 4, obj.order, S, K
        a.iterations, a.buckets = (obj.refinement_iterations if refine else 0), (obj.refinement_buckets if refine else 1)
        a.labels_i64 = int(labels.dtype == torch.int64)
        nbytes = int(lib.cpn_objective_head_workspace_bytes(N, h, w))
        if nbytes <= 0:
            raise NotImplementedError('CPNObjective: N * h * w must stay below 2^31')
        head_ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        indices = torch.empty(N * h * w, dtype=torch.int32, device=dev)
        meta = torch.empty(N + 1 + _lib.OBJECTIVE_META_WORDS, dtype=torch.int32, device=dev)
        check(lib.cpn_objective_head(byref(a), indices.data_ptr(), meta.data_ptr(), head_ws.data_ptr(), nbytes, stream_ptr()),
              'objective_head')
        host = meta.cpu().tolist()  # the one read of this call: P, the background count, the checks
        P, n_bg, flags = host[N], host[N + 1], host[N + 2]
        if flags & _lib.OBJECTIVE_FLAG_LABEL_RANGE:
            raise ValueError(f'CPNObjective: labels above 2^24 = {MAX_LABEL} (the reference moves labels through float32)')
        if flags & _lib.OBJECTIVE_FLAG_LABEL_ROWS:
            raise ValueError(f'CPNObjective: a label is larger than the number of target rows K = {K}')
        if flags & _lib.OBJECTIVE_FLAG_CLASS_RANGE:
            raise ValueError(f"CPNObjective: targets['classes'] holds a class outside 0 .. {cs - 1}")
        present = [P > 0, P > 0, P > 0, P > 0 or n_bg > 0, P > 0 and refine, False, P > 0, False]
        bits = sum(1 << k for k, on in enumerate(present) if on)
        det = None
        if detail:
            det = dict(proposals=torch.empty((P, S, 2), dtype=torch.float32, device=dev),
                       refined=torch.empty((a.iterations, P, S, 2), dtype=torch.float32, device=dev),
                       boxes=torch.empty((P, 4), dtype=torch.float32, device=dev))
            a.detail_proposals, a.detail_refined, a.detail_boxes = p(det['proposals']), p(det['refined']), p(det['boxes'])
        nbytes2 = int(lib.cpn_objective_workspace_bytes(byref(a), P))
        if nbytes2 <= 0:
            raise NotImplementedError('CPNObjective: proposals * samples * iterations * (3 with buckets) must stay below 2^32')
        ws = torch.empty(nbytes2, dtype=torch.uint8, device=dev)
        out = torch.empty(9, dtype=torch.float32, device=dev)
        check(lib.cpn_objective_proposals(byref(a), indices.data_ptr(), P, meta.data_ptr(), bits, head_ws.data_ptr(), ws.data_ptr(),
                                          nbytes2, out.data_ptr(), stream_ptr()), 'objective_proposals')
        if det is not None:
            lin = indices[:P].to(torch.int64)
            det['index'] = (lin // (h * w), (lin % (h * w)) // w, lin % w)
            det['refined'] = list(det['refined'].unbind(0)) if P else []
    return out, present, grads, det


class _Objective(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obj, targets, size, grad, scores, locations, refinement, fourier):
        # grad: the caller's grad mode (inside forward it is always off)
        need = [grad and t is not None and ctx.needs_input_grad[4 + i] for i, t in enumerate((scores, locations, refinement, fourier))]
        out, present, grads, det = _run(obj, scores, locations, refinement, fourier, targets, size, need, obj.full_detail)
        ctx.grads = grads
        obj._present = present
        obj.last_detail = det
        loss, terms = out[8], out[:8]
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, g_loss, _g_terms):
        return (None, None, None, None) + tuple(None if g is None else g * g_loss for g in ctx.grads)


class CPNObjective:
    """The objective of the reference's ``CPN`` in training mode; the attributes mirror it.  See the module text."""

    def __init__(self, order, samples, classes=2, refinement=True, refinement_iterations=4, refinement_buckets=1, order_weights=True,
                 weights=None, uncertainty_head=False, certainty_thresh=None, functional=False, objectives=None):
        for on, what in ((uncertainty_head, 'an uncertainty head (BoxNpllLoss)'), (certainty_thresh is not None, 'certainty_thresh'),
                         (functional, 'functional=True'), (objectives is not None, 'user-supplied objective modules')):
            if on:
                raise NotImplementedError(f'CPNObjective: {what} is not implemented')
        for name, v, lo, hi in (('order', order, 1, MAX_ORDER), ('samples', samples, 1, 1 << 20), ('classes', classes, 1, 1 << 15),
                                ('refinement_iterations', refinement_iterations, 0, _lib.OBJECTIVE_MAX_ITERATIONS),
                                ('refinement_buckets', refinement_buckets, 1, 1 << 10)):
            if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
                raise ValueError(f'CPNObjective: {name} must be an int in {lo} .. {hi} (got {v!r})')
        self.order, self.samples, self.classes = int(order), int(samples), int(classes)
        self.score_channels = 1 if self.classes in (1, 2) else self.classes
        self.refinement = bool(refinement)
        self.refinement_iterations, self.refinement_buckets = int(refinement_iterations), int(refinement_buckets)
        if isinstance(order_weights, bool):
            self.order_weights = order_weighting(self.order) if order_weights else 1.
        else:
            if not isinstance(order_weights, torch.Tensor) or order_weights.numel() != self.order:
                raise ValueError(f'CPNObjective: order_weights must be a bool or a Tensor[{self.order}, 1]')
            self.order_weights = order_weights
        self.weights = dict(DEFAULT_WEIGHTS)
        if weights is not None:
            unknown = set(weights) - set(DEFAULT_WEIGHTS)
            if unknown:
                raise ValueError(f'CPNObjective: unknown weights {sorted(unknown)}')
            self.weights.update(weights)
        self.full_detail = False
        self.last_detail = None
        self._present = (False,) * 8

    @property
    def order_weights_tensor(self):
        return self.order_weights if isinstance(self.order_weights, torch.Tensor) else None

    def __call__(self, scores, locations, refinement, fourier, targets, size, uncertainty=None):
        if uncertainty is not None:
            raise NotImplementedError('CPNObjective: an uncertainty map is not implemented')
        if self.refinement and self.refinement_iterations > 0 and refinement is None:
            raise ValueError('CPNObjective: refinement=True needs the refinement map')
        if not self.refinement:
            refinement = None
        loss, terms = _Objective.apply(self, targets, tuple(size), torch.is_grad_enabled(), scores, locations, refinement, fourier)
        present = self._present
        losses = OrderedDict((k, terms[i] if present[i] else None) for i, k in enumerate(LOSS_KEYS))
        return loss, losses


def _pad_and_stack(labels, fourier, locations, contours, sampling):
    """Lists with one entry per image -> the batch dict: labels stacked, the three target tables zero-padded along K to the
    largest, sampling stacked as float32 (what ``universal_dict_collate_fn`` does to the reference's demo items, data/misc.py:136)."""
    n = len(labels)
    if not n or not (len(fourier) == len(locations) == len(contours) == len(sampling) == n):
        raise ValueError('collate_cpn_targets: need the same number (at least one) of every item')
    dev = labels[0].device
    for name, items, tail in (('reduced_labels', labels, None), ('fourier', fourier, 1), ('locations', locations, 1),
                              ('sampled_contours', contours, 1)):
        shapes = {tuple(t.shape) if tail is None else tuple(t.shape[tail:]) for t in items}
        if len(shapes) != 1:
            raise ValueError(f'collate_cpn_targets: {name} differs in shape between the images: {sorted(shapes)}')
    ks = [int(t.shape[0]) for t in fourier]
    if ks != [int(t.shape[0]) for t in locations] or ks != [int(t.shape[0]) for t in contours]:
        raise ValueError('collate_cpn_targets: fourier, locations and sampled_contours of an image differ in their number of rows')
    K = max(ks)

    def pad(items):
        out = torch.zeros((n, K) + tuple(items[0].shape[1:]), dtype=torch.float32, device=dev)
        for i, t in enumerate(items):
            out[i, :t.shape[0]] = t
        return out

    s = np.stack([np.asarray(t, np.float64) for t in sampling])
    if s.ndim != 2 or s.shape[1] != contours[0].shape[1]:
        raise ValueError('collate_cpn_targets: every sampling must have as many values as the contours have samples')
    return OrderedDict(labels=torch.stack(list(labels)), fourier=pad(fourier), locations=pad(locations), sampled_contours=pad(contours),
                       sampling=torch.as_tensor(s.astype(np.float32)).to(dev))


def collate_cpn_targets(generators):
    """List of fed ``CPNTargetGenerator`` s, one per image -> the reference's batch dict on the GPU: ``labels`` [N, H, W] (the
    reduced labels), ``fourier`` [N, K, order, 4], ``locations`` [N, K, 2], ``sampled_contours`` [N, K, S, 2] (zero-padded along K
    to the largest image), ``sampling`` [N, S] float32."""
    generators = list(generators)
    for g in generators:
        if getattr(g, 'reduced_labels', None) is None:
            raise ValueError('collate_cpn_targets: every generator must have been fed (CPNTargetGenerator.feed)')
        if not g.reduced_labels.is_cuda:
            raise DeviceError('celldetection_amd.collate_cpn_targets runs on the MI355X GPU only; there is no CPU fallback.')
    return _pad_and_stack([g.reduced_labels for g in generators], [g.fourier for g in generators],
                          [g.locations for g in generators], [g.sampled_contours for g in generators],
                          [g.sampling for g in generators])
