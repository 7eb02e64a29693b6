"""Elliptic Fourier descriptors of contours on the MI355X: ``efd`` and ``contours2fourier`` of the reference's ``cd.data.cpn``
(celldetection/data/cpn.py:23-90, 213-227), backed by ``csrc/contour_fourier.hip`` and ``csrc/efd_chunks.h``.  The encoder that
``ops.fouriers2contours`` decodes: a CPN predicts ``fourier`` [K, order, 4] and ``locations`` [K, 2], and this module computes
them from contours.

    ids, fourier, locations = cda.labels2fourier(flat[..., None], order=5)   # label image -> descriptors, all on the GPU
    fourier, locations = cda.contours2fourier(cda.label_contours.labels2contours(labels))   # rows label - 1, as the reference
    coefficients, locations = cda.efd(contours, order=10)                     # Tensor[..., n, 2] or a list of Tensor[n_k, 2]

The rule (restated in ``tests/fourier_oracle.py``, ``include/cpn_hip.h``, ``csrc/efd_chunks.h`` and the kernel file).  A contour
is ``n >= 1`` points ``(x, y)``.

CLOSING.  The contour is closed if ``|first - last| <= 1e-8 + 1e-5 |last|`` holds for both coordinates (numpy's ``allclose`` with
``b = last``).  With ``autoclose`` and not closed the first point is appended; without ``autoclose`` and not closed the call is an
error.  For a dense tensor ``[..., n, 2]`` the reference makes one decision for the whole tensor: if any contour is open, all get
the point appended.  For a list or packed input the decision is per contour (the reference recurses per contour there, and
always with ``autoclose=True``).

SEGMENTS.  With ``N`` segments after closing, for ``i = 0 .. N - 1``: ``dx_i, dy_i`` are the point differences, ``dt_i = sqrt(dx_i^2 +
dy_i^2) + epsilon``, ``t_0 = 0``, ``t_(i+1) = t_i + dt_i``, ``T = t_N``.

COEFFICIENTS.  For ``k = 1 .. order`` with ``phi_(k,i) = k * (2 pi t_i / T)`` and ``C_k = T / (2 k^2 pi^2)``:
``coeff[k-1] = C_k * (sum dx_i/dt_i dcos, sum dx_i/dt_i dsin, sum dy_i/dt_i dcos, sum dy_i/dt_i dsin)`` where ``dcos = cos phi_(k,i+1) -
cos phi_(k,i)`` and ``dsin`` likewise.

LOCATION.  With ``X_i = sum_(j<=i) dx_j``: ``a0 = (1/T) sum [dx_i/(2 dt_i) (t_(i+1)^2 - t_i^2) + (X_i - dx_i/dt_i t_(i+1)) dt_i]``, ``c0`` the
same with ``y``; ``location = first point + (a0, c0)``.

SPECIAL CASES of the reference, mirrored: a one-point contour (``N = 0``) gives coefficients 0 and location NaN; the doubled point
that ``labels2contours`` emits for a one-pixel object (``N = 1``, ``T = epsilon``) gives coefficients 0 and exactly that point.

One stated departure, the same as ``resample_contours`` makes: all arithmetic is float64 whatever the input dtype (numpy would
compute float32 input partly in float32).  Bit equality with numpy is not possible (its ``sum`` is pairwise, its ``sin``/``cos`` are
glibc's); ``tests/test_fourier.py`` measures the bound the results are held to.  The order of summation is fixed by the contour
alone (chunks of ``CHUNK`` segments counted from its first segment), so a contour's result is bit-identical from run to run and
wherever it lies among other contours.  ``order`` runs from 1 to ``MAX_ORDER``.
"""
from ctypes import c_int64

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .label_contours import labels2contours_packed

__all__ = ['efd_packed', 'efd', 'contours2fourier', 'labels2fourier']

CHUNK, MAX_ORDER = _lib.EFD_CHUNK, _lib.EFD_MAX_ORDER
POINTS_I32, POINTS_F64 = 0, 1  # CPN_EFD_POINTS_*
CLOSE_NONE, CLOSE_ALL, CLOSE_EACH, TIMED = 0, 1, 2, 256  # CPN_EFD_CLOSE_*, CPN_EFD_TIMED
STATUS_WORDS = 8
PASSES = ('prepare', 'single', 'sums', 'partials', 'finish')  # status words 2 .. 6 of a timed call
_OPEN = 'Please make sure that contours are explicitly closed (first point must be equal to last point).'


def _check_order(order, name):
    if isinstance(order, bool) or not isinstance(order, int) or order < 1 or order > MAX_ORDER:
        raise ValueError(f'{name}: order must be an int from 1 to {MAX_ORDER} (got {order!r})')
    return order


def _check_tensor(t, name, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name}: {what} must be a Tensor on the GPU (got {type(t).__name__})')


def _check_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError(f'celldetection_amd.{name} runs on the MI355X only (got a CPU tensor).')


def _efd(points, offsets, order, epsilon, mode, dtype, name, timings=None):
    """points [P, 2] (any real dtype) and offsets (integers [K + 1]), both checked to be GPU tensors of these ranks."""
    K, P = int(offsets.numel()) - 1, int(points.shape[0])
    off = offsets.to(torch.int64).contiguous()
    pts = points if points.dtype in (torch.int32, torch.float64) else points.to(torch.float64)  # the kernels read these two
    pts = pts.contiguous()
    dev = pts.device
    lib = _lib.load()
    status = (c_int64 * STATUS_WORDS)()
    with torch.cuda.device(dev):
        coeff = torch.empty((K, order, 4), dtype=torch.float64, device=dev)
        loc = torch.empty((K, 2), dtype=torch.float64, device=dev)
        if K:
            if P < K:
                raise ValueError(f'{name}: offsets must run from 0 to the number of points and every contour needs a point')
            nbytes = int(lib.cpn_efd_workspace_bytes(K, P, order))
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            rc = lib.cpn_efd(ptr(pts), POINTS_I32 if pts.dtype == torch.int32 else POINTS_F64, ptr(off), K, P, order, float(epsilon),
                             mode | (TIMED if timings is not None else 0), ptr(ws), nbytes, ptr(coeff), ptr(loc), status, stream_ptr())
            if rc == _lib.E_INVALID:
                raise ValueError(f'{name}: {lib.cpn_last_error().decode()}')
            check(rc, 'efd')
            if mode == CLOSE_NONE and status[0]:
                raise ValueError(f'{name}: {_OPEN} ({int(status[0])} of {K} contours are not closed)')
            if timings is not None:
                timings.update({what: status[2 + i] * 1e-6 for i, what in enumerate(PASSES)})
                timings['chunks'] = int(status[1])
        elif P:
            raise ValueError(f'{name}: offsets must run from 0 to the number of points')
    return coeff.to(dtype), loc.to(dtype)


def _check_packed(points, offsets, name):
    _check_tensor(points, name, 'points')
    _check_tensor(offsets, name, 'offsets')
    if points.ndim != 2 or points.shape[1] != 2 or points.is_complex() or points.dtype == torch.bool:
        raise ValueError(f'{name}: points must be real [P, 2] (got {points.dtype} {tuple(points.shape)})')
    if offsets.ndim != 1 or offsets.numel() < 1 or offsets.is_floating_point() or offsets.is_complex() or offsets.dtype == torch.bool:
        raise ValueError(f'{name}: offsets must be integers [K + 1]')
    _check_gpu(points, name)
    _check_gpu(offsets, name)


def efd_packed(points, offsets, order=10, epsilon=1e-6, autoclose=True, dtype=torch.float64, timings=None):
    """``points`` [P, 2] (any real dtype; int32 and float64 are read as they are) and ``offsets`` int64 [K + 1] on the GPU ->
    ``(coefficients [K, order, 4], locations [K, 2])`` of ``dtype``: computed in float64, rounded once.  The closing decision is
    per contour; without ``autoclose`` a contour that is not closed raises ``ValueError``.  ``timings``: a dict that receives the
    milliseconds per pass (tools/fourier_microbench.py)."""
    order = _check_order(order, 'efd')
    _check_packed(points, offsets, 'efd')
    return _efd(points, offsets, order, epsilon, CLOSE_EACH if autoclose else CLOSE_NONE, dtype, 'efd', timings)


def _pack(contours, name):
    for c in contours:
        if not isinstance(c, torch.Tensor) or c.ndim != 2 or c.shape[1] != 2:
            raise ValueError(f'{name}: a list holds Tensors [n, 2]')
        if not c.is_cuda:
            raise RuntimeError(f'celldetection_amd.{name} runs on the MI355X only (got a CPU tensor).')
        if c.shape[0] < 1:
            raise ValueError(f'{name}: a contour needs at least one point')
    dev = contours[0].device
    offsets = torch.tensor([0] + [int(c.shape[0]) for c in contours], dtype=torch.int64).cumsum(0).to(dev)
    dtypes = {c.dtype for c in contours}
    points = torch.cat(list(contours)) if len(dtypes) == 1 else torch.cat([c.to(torch.float64) for c in contours])
    return points, offsets


def efd(contour, order=10, epsilon=1e-6, autoclose=True):
    """The reference's ``cd.data.cpn.efd`` on the GPU.  A Tensor[..., n, 2] -> ``(coefficients [..., order, 4], locations [..., 2])``
    with ONE closing decision for the whole tensor; a list or tuple of Tensor[n_k, 2] (the reference's object array) ->
    ``([K, order, 4], [K, 2])`` with the decision per contour and always closing.  float64 results."""
    order = _check_order(order, 'efd')
    if isinstance(contour, (list, tuple)):
        if not len(contour):
            raise ValueError('efd: an empty list of contours')
        points, offsets = _pack(contour, 'efd')
        return _efd(points, offsets, order, epsilon, CLOSE_EACH, torch.float64, 'efd')
    _check_tensor(contour, 'efd', 'contour')
    if contour.ndim < 2 or contour.shape[-1] != 2 or contour.shape[-2] < 1 or contour.is_complex() or contour.dtype == torch.bool:
        raise ValueError(f'efd: contour must be real [..., n, 2] with n >= 1 (got {contour.dtype} {tuple(contour.shape)})')
    _check_gpu(contour, 'efd')
    lead, n = tuple(contour.shape[:-2]), int(contour.shape[-2])
    flat = contour.reshape(-1, 2)
    B = flat.shape[0] // n
    mode = CLOSE_NONE
    if autoclose and B:  # the whole-tensor decision: numpy's allclose(first points, last points)
        first, last = contour[..., 0, :].to(torch.float64), contour[..., -1, :].to(torch.float64)
        if not bool(((first - last).abs() <= 1e-8 + 1e-5 * last.abs()).all()):
            mode = CLOSE_ALL
    offsets = torch.arange(B + 1, dtype=torch.int64, device=contour.device) * n
    coeff, loc = _efd(flat, offsets, order, epsilon, mode, torch.float64, 'efd')
    return coeff.reshape(lead + (order, 4)), loc.reshape(lead + (2,))


def contours2fourier(contours, order=5, dtype=torch.float32):
    """The reference's ``cd.data.cpn.contours2fourier``: the ``OrderedDict`` label -> Tensor[n, 1, 2] or [n, 2] of
    ``label_contours.labels2contours`` -> ``(fouriers [max_label, order, 4], locations [max_label, 2])`` of ``dtype`` on the GPU, row
    ``label - 1`` filled and the others zero.  One launch serves all contours.  A key below 1 raises ``ValueError`` (the reference
    would silently write row -1).  An empty dict returns shapes (0, order, 4), (0, 2) (on the current GPU)."""
    order = _check_order(order, 'contours2fourier')
    if not hasattr(contours, 'items'):
        raise TypeError(f'contours2fourier: contours must be a dict label -> Tensor (got {type(contours).__name__})')
    keys, values = [], []
    for key in contours:
        if isinstance(key, bool) or int(key) != key or int(key) < 1:
            raise ValueError(f'contours2fourier: labels start at 1 (got the key {key!r})')
    for key, c in contours.items():
        _check_tensor(c, 'contours2fourier', 'a contour')
        if c.ndim == 3 and c.shape[1] == 1:
            c = c[:, 0]
        if c.ndim != 2 or c.shape[1] != 2 or c.shape[0] < 1:
            raise ValueError(f'contours2fourier: a contour is [n, 1, 2] or [n, 2] with n >= 1 (got {tuple(c.shape)})')
        _check_gpu(c, 'contours2fourier')
        keys.append(int(key))
        values.append(c)
    if not keys:
        dev = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None
        if dev is None:
            raise RuntimeError('celldetection_amd.contours2fourier runs on the MI355X only (no GPU).')
        return torch.zeros((0, order, 4), dtype=dtype, device=dev), torch.zeros((0, 2), dtype=dtype, device=dev)
    points, offsets = _pack(values, 'contours2fourier')
    coeff, loc = _efd(points, offsets, order, 1e-6, CLOSE_EACH, dtype, 'contours2fourier')
    rows = torch.tensor(keys, dtype=torch.int64, device=points.device) - 1
    fouriers = torch.zeros((max(keys), order, 4), dtype=dtype, device=points.device)
    locations = torch.zeros((max(keys), 2), dtype=dtype, device=points.device)
    fouriers[rows] = coeff  # (a dict has every key once)
    locations[rows] = loc
    return fouriers, locations


def labels2fourier(labels, order=5, dtype=torch.float32, timings=None, **labels2contours_kwargs):
    """Label image Tensor[H, W, C] (integers, on the GPU) -> ``(ids int32 [K], fouriers [K, order, 4], locations [K, 2])``:
    ``labels2contours_packed`` followed by ``efd_packed`` on its int32 points, nothing leaving the GPU.  Compact (row ``k`` belongs
    to label ``ids[k]``) because slide labels near 2^31 make the dense table of ``contours2fourier`` impossible.  Fragmented
    objects are raised, flagged or skipped as ``labels2contours`` does."""
    order = _check_order(order, 'labels2fourier')
    ids, offsets, points = labels2contours_packed(labels, **labels2contours_kwargs)
    coeff, loc = _efd(points, offsets, order, 1e-6, CLOSE_EACH, dtype, 'labels2fourier', timings)
    return ids, coeff, loc
