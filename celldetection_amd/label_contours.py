"""Contours of label images on the MI355X: ``labels2contours`` / ``labels2contour_list`` of the reference's ``cd.data``
(celldetection/data/cpn.py:93-144) and ``resample_contours`` (celldetection/data/misc.py:371-405), backed by
``csrc/label_contours.hip`` and ``csrc/contour_trace.h``.  The inverse of ``contours2labels``:

    flat = cda.resolve_label_channels(labels)                # int32 [H, W]
    contours = cda.labels2contours(flat)                     # list of int32 [n_k, 2] (x, y), by ascending label
    contours = cda.resample_contours(contours, num=64)       # list of float64 [64, 2]
    labels = cda.contours2labels(torch.stack(contours), flat.shape)

The rule for contours (restated in ``tests/label_contours_oracle.py``, ``include/cpn_hip.h`` and the kernel file).  An OBJECT is
a pair (channel, value ``v > 0``); values ``<= 0`` take no part (skimage's ``regionprops`` ignores them).  Its COMPONENTS are the
8-connected sets of pixels of that channel holding ``v``.  An object with exactly one component yields one contour: Suzuki-Abe
border following of the outer border, which is what ``cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE)`` does.  The start is the
raster-first pixel of the component (smallest ``y``, then smallest ``x``); the first search goes clockwise on screen from its west
neighbour, every further search counter-clockwise, starting after the pixel just left; it stops when the start pixel is
re-entered from the first found neighbour.  Every visit is a point, so one-pixel-wide parts appear once per passage.
Coordinates are (x, y) in image coordinates.  A contour of one point is emitted twice (data/cpn.py:133-134).  An object with
more than one component is FRAGMENTED: with ``flag_fragmented_inplace`` every pixel of every channel that holds its value becomes
``constant`` (the GPU tensor is modified in place), otherwise with ``raise_fragmented`` a ``ValueError`` is raised, otherwise it
is skipped.  Contours are returned by ascending label; of a value that occurs in several channels the contour of the highest
channel in which it is unfragmented is returned (the reference's loop overwrites).

One stated departure: a component lying in a hole of another component of the same value counts as a component here, so such an
object is fragmented.  cv2's answer for that case depends on the ring's thickness and on the OpenCV version (RETR_EXTERNAL
either never sees the inner component or reports it), so no single behaviour could be copied.

OpenCV and skimage are absent from the build image: the border following is third-party arithmetic restated from the
publication and OpenCV's documentation, and unpinned, like the polygon fill of ``contours2labels``.  What
``tests/golden/label_contours.npz`` pins is the reference's own code around it (channel loop, offsets, dictionary order, the
doubling, the overwrite across channels) and all of ``resample_contours``, which is pure numpy in the reference.

Known limit: one lane follows one border, so a very long contour (an object as wide as a slide) runs on a single lane;
``profiles/label_contours.txt`` has its time.  ``resample_contours`` computes in float64 whatever the input dtype; that equals
the reference for integer and float64 input (numpy would compute float32 input in float32).
"""
from collections import OrderedDict
from ctypes import c_int64

import torch

from . import _lib
from ._label_input import INT32_MAX, check_labels, to_int32
from ._lib import check, ptr, stream_ptr

__all__ = ['labels2contours_packed', 'labels2contours', 'labels2contour_list', 'resample_contours_packed', 'resample_contours']

RETR_EXTERNAL, CHAIN_APPROX_NONE = 0, 1  # cv2's enum values
TILE = _lib.CONTOURS_TILE


def _check_mode(mode, method):
    if mode != RETR_EXTERNAL:
        raise NotImplementedError(f'labels2contours: only mode=0 (cv2.RETR_EXTERNAL) is implemented (got {mode!r})')
    if method != CHAIN_APPROX_NONE:
        raise NotImplementedError(f'labels2contours: only method=1 (cv2.CHAIN_APPROX_NONE) is implemented (got {method!r})')


def _trace(labels, name, timings=None):
    """-> (ids int32 [K], offsets int64 [K + 1], points int32 [P, 2], values of the fragmented objects int32 [F], unique)."""
    H, W, C = (int(s) for s in labels.shape)
    if H * W > INT32_MAX:
        raise NotImplementedError(f'{name}: more than 2 ** 31 - 1 pixels')
    if C > 65535:
        raise NotImplementedError(f'{name}: more than 65535 channels')
    x = to_int32(labels, f'{name}: labels holds values that do not fit int32')
    dev = x.device
    lib = _lib.load()
    status = (c_int64 * 2)()
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    empty = (new((0,), torch.int32), torch.zeros((1,), dtype=torch.int64, device=dev), new((0, 2), torch.int32),
             new((0,), torch.int32))

    def timed(what, fn):
        if timings is None:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        timings[what] = a.elapsed_time(b)
        return r

    with torch.cuda.device(dev):
        roots = new((C, H, W), torch.int32)
        nbytes = int(lib.cpn_contours_workspace_bytes(0))
        ws = new((nbytes,), torch.uint8)
        timed('components', lambda: check(lib.cpn_contours_components(ptr(x), C, H, W, ptr(roots), ptr(ws), nbytes, status,
                                                                      stream_ptr()), 'contours_components'))
        n = int(status[0])
        if n == 0:
            return empty
        nbytes = int(lib.cpn_contours_workspace_bytes(n))
        ws = new((nbytes,), torch.uint8)
        table, frag = new((4, n), torch.int32), new((n,), torch.int32)
        timed('table', lambda: check(lib.cpn_contours_table(ptr(x), C, H, W, ptr(roots), n, ptr(table), ptr(frag), ptr(ws), nbytes,
                                                            status, stream_ptr()), 'contours_table'))
        K, n_frag = int(status[0]), int(status[1])
        frag = torch.unique(frag[frag > 0]) if n_frag else empty[3]  # the rare path: stock tensor operations
        if K == 0:
            return empty[:3] + (frag,)
        ids, chan, root, npix = (table[i, :K] for i in range(4))
        lengths, offsets = new((K,), torch.int64), new((K + 1,), torch.int64)
        timed('count', lambda: check(lib.cpn_contours_count(ptr(roots), C, H, W, K, ptr(chan), ptr(root), ptr(npix), ptr(lengths),
                                                            ptr(offsets), ptr(ws), nbytes, status, stream_ptr()), 'contours_count'))
        points = new((int(status[0]), 2), torch.int32)
        timed('write', lambda: check(lib.cpn_contours_write(ptr(roots), C, H, W, K, ptr(chan), ptr(root), ptr(npix), ptr(offsets),
                                                            ptr(points), ptr(ws), nbytes, stream_ptr()), 'contours_write'))
    return ids.clone(), offsets, points, frag


def labels2contours_packed(labels, mode=RETR_EXTERNAL, method=CHAIN_APPROX_NONE, flag_fragmented_inplace=False,
                           raise_fragmented=True, constant=-1, timings=None):
    """Label image Tensor[H, W, C] (integers, on the GPU) -> ``(ids, offsets, points)`` on the GPU: ``ids`` int32 [K] ascending,
    ``offsets`` int64 [K + 1], ``points`` int32 [P, 2] as (x, y); contour ``k`` is ``points[offsets[k]:offsets[k + 1]]``.  The
    rule is in the module text.  Only ``mode=0`` (cv2.RETR_EXTERNAL) and ``method=1`` (cv2.CHAIN_APPROX_NONE) are implemented.
    ``timings``: a dict that receives the milliseconds per pass (tools/label_contours_microbench.py)."""
    _check_mode(mode, method)
    check_labels(labels, 'labels2contours')
    ids, offsets, points, frag = _trace(labels, 'labels2contours', timings)
    if frag.numel():
        if flag_fragmented_inplace:
            labels[torch.isin(labels, frag.to(labels.dtype))] = constant
        elif raise_fragmented:
            raise ValueError('Object labeled with multiple connected components.')
    return ids, offsets, points


def _split(offsets, points):
    sizes = (offsets[1:] - offsets[:-1]).tolist()
    return torch.split(points, sizes) if sizes else ()


def labels2contours(labels, **kwargs):
    """The reference's ``cd.data.cpn.labels2contours``: ``OrderedDict`` label -> int32 [n, 1, 2], by ascending label.  The
    entries are views of one points tensor."""
    ids, offsets, points = labels2contours_packed(labels, **kwargs)
    return OrderedDict((i, c[:, None]) for i, c in zip(ids.tolist(), _split(offsets, points)))


def labels2contour_list(labels, **kwargs):
    """The reference's ``cd.data.labels2contours`` (= ``labels2contour_list``): [H, W, C] or [H, W] -> list of int32 [n, 2]."""
    _check_mode(kwargs.get('mode', RETR_EXTERNAL), kwargs.get('method', CHAIN_APPROX_NONE))
    check_labels(labels, 'labels2contours', ranks=(2, 3))
    if labels.ndim == 2:
        labels = labels[..., None]  # a view: flagging reaches the caller's tensor
    _, offsets, points = labels2contours_packed(labels, **kwargs)
    return list(_split(offsets, points))


def _check_num(num):
    if num is None or isinstance(num, float):
        raise NotImplementedError('resample_contours: num=None or a float (ragged output lengths) is not implemented; pass an int')
    if isinstance(num, bool) or int(num) != num or int(num) < 1 or int(num) > INT32_MAX:
        raise ValueError(f'resample_contours: num must be a positive int (got {num!r})')
    return int(num)


def resample_contours_packed(points, offsets, num, close=True, epsilon=1e-6, dtype=torch.float64):
    """``points`` [P, 2] (any real dtype) and ``offsets`` int64 [K + 1] on the GPU -> Tensor[K, num, 2] of ``dtype``: ``num``
    points at equal arc length steps on every contour, the reference's arithmetic in float64, rounded once to ``dtype``."""
    num = _check_num(num)
    for t, what in ((points, 'points'), (offsets, 'offsets')):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'resample_contours: {what} must be a Tensor on the GPU (got {type(t).__name__})')
        if not t.is_cuda:
            raise RuntimeError('celldetection_amd.resample_contours runs on the MI355X only (got a CPU tensor).')
    if points.ndim != 2 or points.shape[1] != 2 or points.is_complex() or points.dtype == torch.bool:
        raise ValueError(f'resample_contours: points must be real [P, 2] (got {points.dtype} {tuple(points.shape)})')
    if offsets.ndim != 1 or offsets.numel() < 1 or offsets.is_floating_point():
        raise ValueError('resample_contours: offsets must be integers [K + 1]')
    K, P = int(offsets.numel()) - 1, int(points.shape[0])
    off = offsets.to(torch.int64).contiguous()
    if K:
        lengths = off[1:] - off[:-1]
        lo, first, last = int(lengths.min()), int(off[0]), int(off[-1])
        if first != 0 or last != P or lo < (1 if close else 2):
            raise ValueError('resample_contours: offsets must run from 0 to the number of points and every contour needs '
                             f'at least {1 if close else 2} point(s)')
    pts = points.to(torch.float64).contiguous()
    with torch.cuda.device(pts.device):
        out = torch.empty((K, num, 2), dtype=torch.float64, device=pts.device)
        cum = torch.empty((P + K,), dtype=torch.float64, device=pts.device)
        check(_lib.load().cpn_resample_contours(ptr(pts), ptr(off), K, P, num, int(bool(close)), float(epsilon), ptr(cum), ptr(out),
                                                stream_ptr()), 'resample_contours')
    return out.to(dtype)


def resample_contours(contours, num=None, close=True, epsilon=1e-6, dtype=torch.float64):
    """The reference's ``cd.data.resample_contours``: a Tensor[..., n, 2] of any real dtype -> Tensor[..., num, 2], or a list or
    tuple of Tensor[n_k, 2] -> the same container of Tensor[num, 2] (one launch for all of them).  On the GPU only."""
    num = _check_num(num)
    if isinstance(contours, (list, tuple)):
        for c in contours:
            if not isinstance(c, torch.Tensor) or c.ndim != 2 or c.shape[1] != 2:
                raise ValueError('resample_contours: a list holds Tensors [n, 2]')
            if not c.is_cuda:
                raise RuntimeError('celldetection_amd.resample_contours runs on the MI355X only (got a CPU tensor).')
        if not len(contours):
            return type(contours)()
        dev = contours[0].device
        offsets = torch.tensor([0] + [int(c.shape[0]) for c in contours], dtype=torch.int64).cumsum(0).to(dev)
        points = torch.cat([c.to(torch.float64) for c in contours])
        return type(contours)(resample_contours_packed(points, offsets, num, close, epsilon, dtype).unbind(0))
    if not isinstance(contours, torch.Tensor):
        raise TypeError(f'resample_contours: contours must be a Tensor or a list of Tensors (got {type(contours).__name__})')
    if contours.ndim < 2 or contours.shape[-1] != 2:
        raise ValueError(f'resample_contours: contours must be [..., n, 2] (got {tuple(contours.shape)})')
    if not contours.is_cuda:
        raise RuntimeError('celldetection_amd.resample_contours runs on the MI355X only (got a CPU tensor).')
    lead, n = tuple(contours.shape[:-2]), int(contours.shape[-2])
    flat = contours.reshape(-1, 2)
    B = flat.shape[0] // n if n else 0
    offsets = torch.arange(B + 1, dtype=torch.int64, device=contours.device) * n
    return resample_contours_packed(flat, offsets, num, close, epsilon, dtype).reshape(lead + (num, 2))
