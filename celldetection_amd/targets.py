"""CPN training targets on the MI355X: ``labels2distances`` / ``mask_labels_by_distance_`` / ``CPNTargetGenerator`` of the
reference's ``cd.data`` (celldetection/data/cpn.py:424-644) and ``filter_instances_`` (celldetection/data/segmentation.py:67-103),
backed by ``csrc/label_distances.hip``.  A label image that lies on the GPU becomes a full set of CPN targets there:

    gen = cda.CPNTargetGenerator(samples=64, order=5)
    gen.feed(labels)                                  # int [H, W, C] on the GPU; filtered and flagged IN PLACE
    gen.reduced_labels, gen.distances                 # score target, distance map
    gen.fourier, gen.locations, gen.sampled_contours  # contour targets, rows label - 1

The rule of ``labels2distances`` (restated in ``tests/targets_oracle.py``, ``include/cpn_hip.h`` and the kernel file, pinned to
the reference's recorded results in ``tests/golden/targets.npz``).  ``owner(p)`` is the one positive label at ``p`` when exactly
one channel is ``> 0``, otherwise 0.  ``t(p)`` is OpenCV's 3 x 3 chamfer distance in 16-bit fixed point (``distance_type`` 2 =
DIST_L2: weights 0.955 / 1.3693; 1 = DIST_L1: 1 / 2; 3 = DIST_C: 1 / 1) to the nearest zero pixel.  ``per_instance=True``: a zero
pixel for ``p`` is every pixel with another owner, pixels outside the image included; per label with ``n`` owner pixels and
largest value ``tmax``: ``d = float32(t) * 2^-16``, divided by ``float32(tmax) * 2^-16`` when ``n > protected_size`` and ``tmax > 0``,
clipped to [0, 1].  ``per_instance=False``: a zero pixel is a pixel with owner 0 inside the image; ``d`` is divided by
``max(float32(tmax) * 2^-16, 1e-6)`` for every label.  The returned labels are a copy with every channel of an overlap pixel -1.

OpenCV and skimage are absent from the build image: ``cv2.distanceTransform`` and ``regionprops`` are third-party arithmetic
restated from OpenCV's published source and skimage's documentation, and unpinned; the fixture pins the reference's own code
around them.

Known limits and stated departures.
* ``overlap_zero=False`` raises ``NotImplementedError`` in both modes: the reference's result then depends on the order in which
  objects overwrite and re-divide shared pixels.
* ``per_instance=False`` on an image without any owner-0 pixel raises ``ValueError``; OpenCV returns a sentinel-sized number there.
* H, W <= 32768, so that every distance fits the transform's uint32.
* ``filter_instances_`` with ``continuous=True``: with ``n`` distinct positive labels every label ``<= n`` stays and the labels
  ``> n`` take the missing values of ``1 .. n``, largest label to largest gap.  The reference pairs them in CPython's set iteration
  order, which is unspecified, so equality with it is defined up to a bijection on the moved labels.
* ``filter_instances_`` never counts out values ``<= 0``.  The reference drops the first unique value whatever it is, so with
  negatives present and ``max_area`` set it can erase label 0.
* An object wider than the halo needs one launch per 8 pixels of its inradius (``profiles/targets.txt`` has the time).
"""
from collections import OrderedDict
from ctypes import c_int64

import numpy as np
import torch

from . import _lib
from ._label_input import INT32_MAX, INT32_MIN, check_labels, to_int32
from ._lib import check, ptr, stream_ptr
from ._tables import default_capacity
from .fourier import _check_order, efd_packed
from .label_contours import _split, labels2contours_packed, resample_contours_packed

__all__ = ['labels2distances', 'mask_labels_by_distance_', 'filter_instances_', 'CPNTargetGenerator']

DIST_L1, DIST_L2, DIST_C = _lib.DIST_L1, _lib.DIST_L2, _lib.DIST_C  # = cv2's enum values
MAX_STEPS = _lib.LABEL_DISTANCES_MAX_STEPS  # synchronous steps per launch
MAX_SIDE = 32768


def labels2distances(labels, distance_type=DIST_L2, overlap_zero=True, per_instance=True, protected_size=36,
                     return_stats=False):
    """Label image Tensor[H, W, C] or [H, W] (integers, on the GPU) -> ``(distances float32 [H, W], labels [H, W, C])`` on the GPU
    with exactly the values of the reference's function (data/cpn.py:432-497; the rule is in the module text).  The input is
    never changed; the returned labels have the input's dtype.
    return_stats: additionally ``dict(launches, steps, active_tiles, changed_pixels, table_capacity)``."""
    if isinstance(distance_type, (bool, str)) or distance_type not in (DIST_L1, DIST_L2, DIST_C):
        raise ValueError(f'labels2distances: distance_type must be 1 (DIST_L1), 2 (DIST_L2) or 3 (DIST_C) (got {distance_type!r})')
    if not overlap_zero:
        raise NotImplementedError('labels2distances: overlap_zero=False is not implemented (the reference result depends on the '
                                  'order in which objects overwrite shared pixels)')
    if isinstance(protected_size, bool) or int(protected_size) != protected_size or not 0 <= int(protected_size) <= INT32_MAX:
        raise ValueError(f'labels2distances: protected_size must be a non-negative int (got {protected_size!r})')
    check_labels(labels, 'labels2distances', ranks=(2, 3))
    x = labels[..., None] if labels.ndim == 2 else labels
    H, W, C = (int(s) for s in x.shape)
    if H > MAX_SIDE or W > MAX_SIDE:
        raise NotImplementedError(f'labels2distances: H and W are at most {MAX_SIDE}')
    x = to_int32(x, 'labels2distances: labels holds values that do not fit int32')
    dev = x.device
    lib = _lib.load()
    status = (c_int64 * 2)()
    inst = int(bool(per_instance))
    launches, active, changed = 0, [], []
    with torch.cuda.device(dev):
        dist = torch.empty((H, W), dtype=torch.float32, device=dev)
        out = torch.empty((H, W, C), dtype=torch.int32, device=dev)
        nbytes = int(lib.cpn_label_distances_workspace_bytes(H, W))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(lib.cpn_label_distances_classify(ptr(x), C, H, W, distance_type, inst, ptr(ws), nbytes, status, stream_ptr()),
              'label_distances_classify')
        if not inst and H * W and int(status[0]) == 0:
            raise ValueError('labels2distances: per_instance=False needs at least one pixel without an owner (background, a '
                             'negative value or overlap); OpenCV returns a sentinel-sized distance there')
        while H * W:
            check(lib.cpn_label_distances_step(H, W, MAX_STEPS, distance_type, inst, launches, ptr(ws), nbytes, status,
                                               stream_ptr()), 'label_distances_step')
            launches += 1
            changed.append(int(status[0]))
            active.append(int(status[1]))
            if int(status[0]) == 0:
                break
        cap = default_capacity(H * W, 64)
        while True:
            table = torch.empty(int(lib.cpn_label_distances_table_bytes(cap)), dtype=torch.uint8, device=dev)
            check(lib.cpn_label_distances_reduce(H, W, ptr(ws), nbytes, ptr(table), cap, status, stream_ptr()),
                  'label_distances_reduce')
            if int(status[0]) == 0:
                break
            if cap >= 1 << 28:
                raise RuntimeError('labels2distances: more labels than the largest table holds')
            cap *= 4
        check(lib.cpn_label_distances_finalise(ptr(x), C, H, W, inst, int(protected_size), ptr(ws), nbytes, ptr(table), cap,
                                               ptr(dist), ptr(out), stream_ptr()), 'label_distances_finalise')
    out = out.to(labels.dtype)
    if return_stats:
        return dist, out, dict(launches=launches, steps=launches * MAX_STEPS, active_tiles=active, changed_pixels=changed,
                               table_capacity=cap)
    return dist, out


def _inplace_int32(labels, name, fn):
    """Runs fn on an int32 contiguous image of ``labels`` and writes the result back when that image is a copy."""
    x = to_int32(labels, f'{name}: labels holds values that do not fit int32')
    fn(x)
    if x.data_ptr() != labels.data_ptr() or x.dtype != labels.dtype:
        labels.copy_(x)
    return labels


def mask_labels_by_distance_(labels, distances, max_bg_dist, min_fg_dist, return_reduced=False):
    """The reference's function (data/cpn.py:424-429), in place on the GPU tensor ``labels`` [H, W, C]: pixels with any channel
    ``> 0`` and ``d <= max_bg_dist`` get all channels 0, then pixels with ``max_bg_dist < d < min_fg_dist`` all channels -1; the
    thresholds are rounded to float32 before comparing.  return_reduced: returns the channel maximum [H, W] of the result."""
    if not isinstance(distances, torch.Tensor) or not distances.is_floating_point():
        raise TypeError('mask_labels_by_distance_: distances must be a float Tensor on the GPU')
    if isinstance(labels, torch.Tensor) and labels.ndim == 3 and tuple(distances.shape) != tuple(labels.shape[:2]):
        raise ValueError(f'mask_labels_by_distance_: distances must be {tuple(labels.shape[:2])} (got {tuple(distances.shape)})')
    check_labels(labels, 'mask_labels_by_distance_')
    if not distances.is_cuda or distances.device != labels.device:
        raise RuntimeError('celldetection_amd.mask_labels_by_distance_ runs on the MI355X only (distances on another device).')
    H, W, C = (int(s) for s in labels.shape)
    d = distances.to(torch.float32).contiguous()
    reduced = torch.empty((H, W), dtype=torch.int32, device=labels.device) if return_reduced else None

    def run(x):
        with torch.cuda.device(x.device):
            check(_lib.load().cpn_label_distances_mask(ptr(x), C, H * W, ptr(d), float(max_bg_dist), float(min_fg_dist), ptr(reduced),
                                                       stream_ptr()), 'label_distances_mask')

    _inplace_int32(labels, 'mask_labels_by_distance_', run)
    return reduced.to(labels.dtype) if return_reduced else None


def _filter_table(uni, cnt, border, min_area, max_area, constant, continuous):
    """The value table of filter_instances_ on the host: unique values and counts -> the value each one becomes."""
    def merge(keys, counts, values):  # counts of the mapped values
        u, inv = np.unique(values, return_inverse=True)
        return u, np.bincount(inv.reshape(-1), weights=counts, minlength=len(u)).astype(np.int64)

    cur = uni.copy()  # cur[i]: what uni[i] has become
    if border is not None:
        cur[np.isin(cur, border[border != 0])] = constant
    if max_area is not None or min_area is not None:
        u, c = merge(uni, cnt, cur)
        bad = np.zeros(len(u), bool)
        if max_area:
            bad |= c > max_area
        if min_area:
            bad |= c < min_area
        bad &= u > 0
        cur[np.isin(cur, u[bad])] = constant
    if continuous:
        u = np.unique(cur[cur > 0])
        n = len(u)
        gaps, moved = np.setdiff1d(np.arange(1, n + 1), u), u[u > n]
        if len(moved):
            idx = np.searchsorted(moved, cur)
            hit = (idx < len(moved)) & (moved[np.minimum(idx, len(moved) - 1)] == cur)
            cur[hit] = gaps[idx[hit]]
    return cur


def filter_instances_(labels, partials=True, partials_border=1, min_area=4, max_area=None, constant=-1, continuous=True):
    """The reference's ``filter_instances_`` (data/segmentation.py:67-103), in place on the GPU tensor ``labels`` [H, W, C] or
    [H, W]: objects touching the outer ``partials_border`` pixels (``partials``), objects of fewer than ``min_area`` or more than
    ``max_area`` elements (counted over all channels) become ``constant``; with ``continuous`` the label gaps are filled.  The
    table of values is built with stock tensor operations, the image is rewritten by one HIP pass.  The two departures from
    the reference are in the module text."""
    check_labels(labels, 'filter_instances_', ranks=(2, 3))
    if labels.numel() == 0:
        return labels
    uni, cnt = torch.unique(labels, return_counts=True)
    border = None
    if partials and partials_border >= 1:
        b = int(partials_border)
        border = torch.unique(torch.cat([s.reshape(-1) for s in (labels[:, :b], labels[:, -b:], labels[:b], labels[-b:])]))
        border = border.cpu().numpy().astype(np.int64)
    uni_h = uni.cpu().numpy().astype(np.int64)
    new = _filter_table(uni_h, cnt.cpu().numpy().astype(np.int64), border, min_area, max_area, int(constant), continuous)
    change = new != uni_h
    if not change.any():
        return labels
    info = torch.iinfo(labels.dtype)
    if new.min() < max(info.min, INT32_MIN) or new.max() > min(info.max, INT32_MAX):
        raise ValueError(f'filter_instances_: constant {constant!r} does not fit {labels.dtype}')
    keys = torch.as_tensor(uni_h[change], dtype=torch.int32).to(labels.device)  # ascending: torch.unique sorts
    values = torch.as_tensor(new[change], dtype=torch.int32).to(labels.device)

    def run(x):
        with torch.cuda.device(x.device):
            check(_lib.load().cpn_label_remap(ptr(x), x.numel(), ptr(keys), ptr(values), int(keys.numel()), stream_ptr()),
                  'label_remap')

    return _inplace_int32(labels, 'filter_instances_', run)


class CPNTargetGenerator:
    """The reference's ``cd.data.CPNTargetGenerator`` (data/cpn.py:500-644) on the GPU: same arguments, same laziness, same
    order of operations in ``feed``.  Every property is a GPU tensor except ``sampling`` (numpy, drawn on the host exactly as the
    reference draws it, so a seeded ``np.random`` gives the same values) and ``contours`` (``OrderedDict`` label -> int32
    [n, 1, 2] on the GPU).  ``fourier`` / ``locations`` are float32 with row ``label - 1``, ``sampled_contours`` float32
    [max_label, samples, 2], ``resampled_contours`` float64 [max_label, samples, 2]."""

    def __init__(self, samples, order, random_sampling=True, remove_partials=False, min_fg_dist=.75, max_bg_dist=.5,
                 flag_fragmented=True, flag_fragmented_constant=-1):
        self.samples = samples
        self.order = _check_order(order, 'CPNTargetGenerator')
        self.random_sampling = random_sampling
        self.remove_partials = remove_partials
        self.min_fg_dist = min_fg_dist
        self.max_bg_dist = max_bg_dist
        self.flag_fragmented = flag_fragmented
        self.flag_fragmented_constant = flag_fragmented_constant
        self.labels = None
        self.labels_red = None
        self.distances = None
        self._reset()

    def _reset(self):
        self._sampling = self._packed = self._contours = self._fourier = self._locations = None
        self._sampled_contours = self._sampled_sizes = self._resampled_contours = self._reduced = None

    def feed(self, labels, border=1, min_area=1, max_area=None, **kwargs):
        """``labels``: one label image, Tensor[H, W, C] or [H, W] on the GPU; it is filtered and flagged in place.  ``kwargs`` go
        to ``labels2distances``."""
        self._reset()
        check_labels(labels, 'CPNTargetGenerator.feed', ranks=(2, 3))
        if labels.ndim == 2:
            labels = labels[..., None]
        filter_instances_(labels, partials=self.remove_partials, partials_border=border, min_area=min_area, max_area=max_area,
                          constant=-1, continuous=True)
        self.labels = labels
        _ = self.packed_contours  # flags fragmented objects in place before the distances are taken
        self.distances, self.labels_red = labels2distances(labels, **kwargs)
        self._reduced = mask_labels_by_distance_(self.labels_red, self.distances, self.max_bg_dist, self.min_fg_dist,
                                                 return_reduced=True)

    @property
    def reduced_labels(self):
        return self._reduced

    @property
    def sampling(self):
        if self._sampling is None:
            if self.random_sampling:
                self._sampling = np.random.uniform(0., 1., self.samples)
            else:
                self._sampling = np.linspace(0., 1., self.samples)
            self._sampling.sort()
        return self._sampling

    @property
    def packed_contours(self):
        """``(ids int32 [K], offsets int64 [K + 1], points int32 [P, 2])`` of ``labels2contours_packed``."""
        if self._packed is None:
            self._packed = labels2contours_packed(self.labels, flag_fragmented_inplace=self.flag_fragmented,
                                                  constant=self.flag_fragmented_constant, raise_fragmented=False)
        return self._packed

    @property
    def contours(self):
        if self._contours is None:
            ids, offsets, points = self.packed_contours
            self._contours = OrderedDict((i, c[:, None]) for i, c in zip(ids.tolist(), _split(offsets, points)))
        return self._contours

    def _rows(self):
        ids = self.packed_contours[0]
        return ids.to(torch.int64) - 1, (int(ids.max()) if ids.numel() else 0)

    def _efd(self):
        ids, offsets, points = self.packed_contours
        rows, top = self._rows()
        self._fourier = torch.zeros((top, self.order, 4), dtype=torch.float32, device=points.device)
        self._locations = torch.zeros((top, 2), dtype=torch.float32, device=points.device)
        if top:
            coeff, loc = efd_packed(points, offsets, self.order, dtype=torch.float32)
            self._fourier[rows] = coeff
            self._locations[rows] = loc

    @property
    def fourier(self):
        if self._fourier is None:
            self._efd()
        return self._fourier

    @property
    def locations(self):
        if self._locations is None:
            self._efd()
        return self._locations

    @property
    def sampled_contours(self):
        """Tensor[max_label, samples, 2]."""
        if self._sampled_contours is None:
            from . import ops
            if self.fourier.shape[0]:
                self._sampled_contours = ops.fouriers2contours(self.fourier, self.locations, samples=self.samples,
                                                               sampling=torch.as_tensor(self.sampling))[0]
            else:
                self._sampled_contours = torch.zeros((0, self.samples, 2), dtype=torch.float32, device=self.fourier.device)
        return self._sampled_contours

    @property
    def resampled_contours(self):
        """Tensor[max_label, samples, 2], float64."""
        if self._resampled_contours is None:
            ids, offsets, points = self.packed_contours
            rows, top = self._rows()
            out = torch.zeros((top, self.samples, 2), dtype=torch.float64, device=points.device)
            if top:
                out[rows] = resample_contours_packed(points, offsets, self.samples)
            self._resampled_contours = out
        return self._resampled_contours

    @property
    def sampled_sizes(self):
        """Tensor[max_label, 2]: extent of every sampled contour in x and y."""
        if self._sampled_sizes is None:
            c = self.sampled_contours
            self._sampled_sizes = c.max(1).values - c.min(1).values if c.shape[0] else c.new_zeros((0, 2))
        return self._sampled_sizes
