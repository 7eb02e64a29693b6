"""Flat label images on the MI355X: ``resolve_label_channels`` of the reference's ``cd.data`` (celldetection/data/cpn.py:361-399,
called from celldetection_scripts/cpn_inference.py:817), backed by ``csrc/flat_labels.hip``.

    labels = cda.contours2labels(y['contours'][0], x.shape[2:])   # int32 [H, W, C]: overlapping objects in different channels
    flat = cda.resolve_label_channels(labels)                     # int32 [H, W]: what is saved, viewed and measured

The rule (the reference's, restated in ``tests/flat_labels_oracle.py`` and pinned to outputs of the reference's own function in
``tests/golden/flat_labels.npz``): a pixel with more than one channel ``> 0`` is an overlap pixel, with exactly one a core pixel.
Without any overlap pixel the result is the plain channel maximum (negative maxima included).  Otherwise core pixels keep
their label, everything else starts at 0, and in at most ``max_iter`` synchronous steps every overlap pixel that still holds 0
takes the largest label among its neighbours, all pixels at once from the values of the previous step; neighbours outside the
image take no part.  It stops when nothing is unresolved or a step changes nothing; overlap pixels no label reaches stay 0.

The reference computes a step with ``cv2.dilate`` and builds the default kernel with ``cv2.getStructuringElement(1, (3, 3))``.
OpenCV is absent from the build image, so these two are third-party arithmetic restated from OpenCV's documentation (shape 1
is ``MORPH_CROSS``; the default border of ``dilate`` never wins a maximum) and unpinned, like the polygon fill of
``contours2labels``; the reference's own code around them is what the fixture pins.
"""
from ctypes import c_int64

import numpy as np
import torch

from . import _lib
from ._label_input import INT32_MAX, aligned16, to_int32
from ._lib import check, ptr, stream_ptr

__all__ = ['resolve_label_channels']

CROSS = 0o272  # footprint bits, bit 3 * row + column: 010 / 111 / 010
MAX_STEPS = _lib.FLAT_MAX_STEPS  # synchronous steps per launch


def _footprint(kernel):
    """``kernel`` of the reference -> 9 footprint bits."""
    if isinstance(kernel, (tuple, list)):
        if len(kernel) == 2 and all(isinstance(k, (int, np.integer)) for k in kernel):
            if tuple(int(k) for k in kernel) == (3, 3):
                return CROSS
            raise NotImplementedError(f'resolve_label_channels: kernel size {tuple(kernel)} is not implemented on the HIP path '
                                      '(only (3, 3), the 4-neighbourhood, or an explicit 3 x 3 array)')
        raise NotImplementedError('resolve_label_channels: a tuple or list kernel is a size and only (3, 3) is implemented; '
                                  'pass an explicit footprint as a 3 x 3 array')
    if isinstance(kernel, torch.Tensor):
        kernel = kernel.detach().cpu().numpy()
    if isinstance(kernel, np.ndarray) and kernel.shape == (3, 3):
        return sum(1 << k for k, v in enumerate(kernel.reshape(-1).tolist()) if v != 0)
    raise NotImplementedError('resolve_label_channels: only (3, 3) or an explicit 3 x 3 array is implemented as kernel '
                              f'(got {getattr(kernel, "shape", kernel)!r})')


def resolve_label_channels(labels, method='dilation', max_iter=999, kernel=(3, 3), return_stats=False):
    """Label image Tensor[H, W, C] (integers, on the GPU) -> Tensor[H, W] of the same dtype on the GPU, with exactly the
    values of the reference's function (data/cpn.py:361-399; cv2's dilate restated, see the module text).

    kernel: ``(3, 3)`` is the reference's default, the 4-neighbourhood; a 3 x 3 array is an explicit footprint (non-zero
    entries, anchor at the centre; all ones: the 8-neighbourhood); anything else raises ``NotImplementedError``.
    return_stats: additionally ``dict(overlap_pixels, unresolved_pixels, steps, launches, active_tiles)``: ``steps`` counts
    the synchronous steps executed (<= ``max_iter``; it may exceed the reference's count by the steps of the last launch that
    changed nothing), ``active_tiles`` the 32 x 32 tiles run per launch."""
    if method != 'dilation':
        raise ValueError(f'Invalid method: {method}')
    fp = _footprint(kernel)
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f'resolve_label_channels: labels must be a Tensor on the GPU (got {type(labels).__name__})')
    if labels.ndim != 3:
        raise ValueError(f'resolve_label_channels: labels must be [H, W, C] (got {tuple(labels.shape)})')
    if labels.shape[2] < 1:
        raise ValueError('resolve_label_channels: labels has no channel')
    if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise TypeError(f'resolve_label_channels: labels must hold integers (got {labels.dtype})')
    if not labels.is_cuda:
        raise RuntimeError('celldetection_amd.resolve_label_channels runs on the MI355X only (got a CPU tensor).')
    H, W, C = (int(s) for s in labels.shape)
    if H * W > INT32_MAX:
        raise NotImplementedError('resolve_label_channels: more than 2 ** 31 - 1 pixels')
    x = aligned16(to_int32(labels, 'resolve_label_channels: labels holds values that do not fit int32'))
    lib = _lib.load()
    max_iter = int(max_iter)
    status = (c_int64 * 2)()
    steps, launches, active = 0, 0, []
    with torch.cuda.device(x.device):
        out = torch.empty((H, W), dtype=torch.int32, device=x.device)
        nbytes = int(lib.cpn_flat_workspace_bytes(H, W))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        check(lib.cpn_flat_classify(ptr(x), C, H, W, 0, ptr(out), ptr(ws), nbytes, status, stream_ptr()), 'flat_classify')
        overlap, negative = int(status[0]), int(status[1])
        unresolved = overlap
        if overlap == 0:
            if negative:  # the plain maximum keeps negative values (data/cpn.py:398)
                check(lib.cpn_flat_classify(ptr(x), C, H, W, 1, ptr(out), ptr(ws), nbytes, status, stream_ptr()),
                      'flat_classify')
        else:
            while unresolved > 0 and steps < max_iter:
                n = min(MAX_STEPS, max_iter - steps)
                check(lib.cpn_flat_step(ptr(out), H, W, n, fp, launches, ptr(ws), nbytes, status, stream_ptr()), 'flat_step')
                launches += 1
                steps += n
                active.append(int(status[1]))
                unresolved -= int(status[0])
                if int(status[0]) == 0:
                    break
            if unresolved > 0:
                check(lib.cpn_flat_finish(ptr(out), H, W, ptr(ws), nbytes, stream_ptr()), 'flat_finish')
    out = out.to(labels.dtype)
    if return_stats:
        return out, dict(overlap_pixels=overlap, unresolved_pixels=unresolved, steps=steps, launches=launches, active_tiles=active)
    return out
