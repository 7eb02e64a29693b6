"""Overlay images on the MI355X: ``contours2overlay`` of the reference's ``cd.data`` (celldetection/data/cpn.py:647-662,
699-723, 811-855) and ``label_cmap(..., ubyte=True)`` / ``random_colors_hsv`` of ``cd.visualization``
(celldetection/visualization/cmaps.py:10-77), the two ways ``--overlay`` of celldetection_scripts/cpn_inference.py:839-848
builds its RGBA image; backed by ``csrc/overlay.hip``.

    labels = cda.contours2labels(y['contours'][0], x.shape[2:])
    overlay = cda.label_cmap(labels, ubyte=True)                     # uint8 [H, W, 4], when label images exist
    overlay = cda.contours2overlay(y['contours'][0], x.shape[2:])    # uint8 [H, W, 4], from the contours alone

``contours2overlay``: every contour is rounded, clipped and filled exactly as ``contours2labels`` does; a pixel covered by
``n >= 1`` contours gets the floored mean of their colours and alpha 255, every other pixel is ``(0, 0, 0, 0)``.  The reference
sums into a full-image ``intermediate_dtype`` RGBA image plus a counter (10 bytes per pixel); here a 32 x 32 pixel tile
belongs to one workgroup that sums in LDS and writes each pixel once, so the output is the only full-image array.

``label_cmap``: the colour table is prepared on the host, the image is mapped (and, for ``[H, W, C]`` labels, reduced over
the channels with the alpha values as weights, in the reference's float32 order of operations) in one kernel.

Both rules are restated in ``tests/overlay_oracle.py`` and pinned to outputs of the reference's own functions in
``tests/golden/overlay.npz``.  Third-party arithmetic, restated from documentation and unpinned (OpenCV is absent from the
build image), like the polygon fill and ``dilate``: the HSV -> RGB conversion of ``random_colors_hsv``
(``cv2.cvtColor(..., COLOR_HSV2RGB)`` on 8-bit data) and ``skimage.img_as_ubyte`` on the colour table (``rint(x * 255)``).
"""
from ctypes import c_int32, c_uint32

import numpy as np
import torch

from . import _lib
from ._label_input import INT32_MAX, INT32_MIN
from ._lib import check, ptr, stream_ptr

__all__ = ['contours2overlay', 'label_cmap', 'random_colors_hsv']

TILE = _lib.OVERLAY_TILE
_SUM_BITS_LIMIT = (2 ** 32 - 1) // 255  # the kernel's sums are 32 bits wide
QUALITATIVE_MAPS = ('Pastel1', 'Pastel2', 'Paired', 'Accent', 'Dark2', 'Set1', 'Set2', 'Set3', 'tab10', 'tab20', 'tab20b', 'tab20c')


def hsv2rgb_ubyte(hsv):
    """OpenCV's documented 8-bit ``COLOR_HSV2RGB`` on uint8 ``[n, 3]``: H in [0, 180) is degrees / 2, S and V are out of 255;
    the sector formula of the documentation, every channel rounded to nearest.  Restated, unpinned."""
    hsv = np.asarray(hsv, np.uint8).reshape(-1, 3).astype(np.float64)
    h6, s, v = hsv[:, 0] / 30., hsv[:, 1] / 255., hsv[:, 2] / 255.
    sector = np.floor(h6)
    f = h6 - sector
    p, q, t = v * (1. - s), v * (1. - s * f), v * (1. - s * (1. - f))
    r = np.choose(sector.astype(np.int64) % 6, [v, q, p, p, t, v])
    g = np.choose(sector.astype(np.int64) % 6, [t, v, v, q, p, p])
    b = np.choose(sector.astype(np.int64) % 6, [p, p, t, v, v, q])
    return np.clip(np.rint(np.stack((r, g, b), 1) * 255.), 0, 255).astype(np.uint8)


def random_colors_hsv(num, hue_range=(0, 180), saturation_range=(60, 133), value_range=(180, 256), ubyte=False):
    """``num`` random colours, drawn in HSV as the reference does (cmaps.py:10-18): three ``np.random.randint(*range, num)``
    calls (hue, saturation, value), converted with the 8-bit HSV -> RGB rule.  -> numpy ``[num, 3]``, uint8 with ``ubyte``
    else float64 in [0, 1].  Host side; ``np.random.seed`` fixes the draw."""
    hsv = np.stack((np.random.randint(*hue_range, num), np.random.randint(*saturation_range, num),
                    np.random.randint(*value_range, num)), 1).astype('uint8')
    colors = hsv2rgb_ubyte(hsv)
    return colors if ubyte else colors / 255


def _as_device_contours(contours, what):
    """Tensor [K, S, 2] on the GPU, or a list of arrays of different lengths padded by repeating the last point (a zero-length
    edge draws the same pixel again and takes no part in the scanline fill: identical raster), as ``contours2labels``."""
    if isinstance(contours, torch.Tensor):
        return contours
    arrs = [np.asarray(c.detach().cpu() if isinstance(c, torch.Tensor) else c, np.float32).reshape(-1, 2) for c in contours]
    if any(len(a) == 0 for a in arrs):
        raise ValueError(f'{what}: zero-length contour at position {[i for i, a in enumerate(arrs) if len(a) == 0][0]}')
    smax = max([len(a) for a in arrs] + [1])
    arrs = [np.concatenate((a, np.repeat(a[-1:], smax - len(a), 0))) if len(a) < smax else a for a in arrs]
    t = torch.as_tensor(np.stack(arrs) if arrs else np.zeros((0, 1, 2), np.float32))
    return t.cuda() if torch.cuda.is_available() else t


def _tile_lists(lib, boxes, K, H, W):
    """The (tile, contour) lists of the paint pass from the boxes of ``cpn_labels_prepare``: count, exclusive scan, fill.
    -> (tile_begin int32 [tiles + 1], list int32 [pairs], pairs)."""
    tiles = -(-W // TILE) * -(-H // TILE)
    i32 = dict(dtype=torch.int32, device=boxes.device)
    begin = torch.zeros(tiles + 1, **i32)
    check(lib.cpn_overlay_bin_count(ptr(boxes), K, H, W, ptr(begin[1:]), stream_ptr()), 'overlay_bin_count')
    scan = torch.cumsum(begin, 0)  # int64
    pairs = int(scan[-1].item())
    if pairs > INT32_MAX:
        raise NotImplementedError(f'contours2overlay: {pairs} (tile, contour) pairs; at most 2 ** 31 - 1')
    begin = scan.to(torch.int32)
    del scan
    cursor = torch.zeros(tiles, **i32)
    lst = torch.empty(max(pairs, 1), **i32)
    check(lib.cpn_overlay_bin_fill(ptr(boxes), K, H, W, ptr(begin), ptr(cursor), ptr(lst), pairs, stream_ptr()),
          'overlay_bin_fill')
    return begin, lst, pairs


def contours2overlay(contours, size, hue_range=(0, 180), saturation_range=(60, 133), value_range=(180, 256), rounded=True,
                     clip=True, intermediate_dtype='uint16', thickness=-1, processes=None, colors=None, return_colors=False,
                     return_stats=False):
    """Contours [K, S, 2] (xy, one image; Tensor on the GPU, or a list of arrays) -> RGBA overlay image, uint8 Tensor[H, W, 4]
    on the GPU.  Arguments as in the reference (data/cpn.py:811-855); ``colors``, ``return_colors`` and ``return_stats`` are
    additions.

    colors: uint8 ``[K, 3]`` (array or Tensor), used as given: the way to a reproducible image.  Without it the colours are
        drawn on the host with ONE ``random_colors_hsv(K, ...)`` call.  The reference draws one colour per contour inside its
        loop, so even with the same ``np.random.seed`` its stream of random numbers, hence its colours, differ from ours (in
        its multiprocessing path they are unseeded altogether); ``return_colors`` returns the ``[K, 3]`` Tensor that was used.
    intermediate_dtype: an integer dtype.  Nothing is allocated in it; it only sets the reference's overflow limit: more than
        ``iinfo(intermediate_dtype).max // 255`` contours on one pixel (257 for uint16) make the reference's sums wrap
        silently, and raise ``ValueError`` with the largest overlap count here.
    thickness: only ``-1`` (filled contours).  processes: accepted and ignored.
    return_stats: additionally ``dict(max_overlap, pairs, tiles)``: the largest number of contours on one pixel, the number of
        (tile, contour) pairs and the number of 32 x 32 tiles."""
    if thickness != -1:
        raise NotImplementedError(f'contours2overlay: thickness={thickness!r} is not implemented on the HIP path (only -1, filled contours)')
    dt = np.dtype(intermediate_dtype)
    if dt.kind not in 'iu':
        raise NotImplementedError(f'contours2overlay: intermediate_dtype={intermediate_dtype!r} is not implemented on the HIP path '
                                  '(integer dtypes only)')
    limit = min(int(np.iinfo(dt).max) // 255, _SUM_BITS_LIMIT)
    H, W = int(size[0]), int(size[1])
    if contours is not None:
        contours = _as_device_contours(contours, 'contours2overlay')
        if not contours.is_cuda:
            raise RuntimeError('celldetection_amd.contours2overlay runs on the MI355X only (got a CPU tensor).')
        if contours.ndim != 3 or contours.shape[2] != 2:
            raise ValueError(f'contours2overlay: contours must be [K, S, 2] (got {tuple(contours.shape)})')
    K = 0 if contours is None else int(contours.shape[0])
    if colors is not None and K:
        colors = torch.as_tensor(colors)
        if colors.dtype != torch.uint8 or tuple(colors.shape) != (K, 3):
            raise ValueError(f'contours2overlay: colors must be uint8 [{K}, 3] (got {colors.dtype} {tuple(colors.shape)})')
    if isinstance(colors, torch.Tensor) and colors.is_cuda and contours is None:
        dev = colors.device
    else:
        dev = contours.device if contours is not None else torch.device('cuda', torch.cuda.current_device())
    tiles_x, tiles_y = -(-W // TILE), -(-H // TILE)
    tiles = tiles_x * tiles_y

    def result(out, col, stats):
        res = (out,) + ((col,) if return_colors else ()) + ((stats,) if return_stats else ())
        return res[0] if len(res) == 1 else res

    if K == 0:  # contours=None or no contour: zeros (data/cpn.py:848-855)
        return result(torch.zeros((H, W, 4), dtype=torch.uint8, device=dev), torch.zeros((0, 3), dtype=torch.uint8, device=dev),
                      dict(max_overlap=0, pairs=0, tiles=tiles))
    S = int(contours.shape[1])
    if S < 1:
        raise ValueError('contours2overlay: zero-length contour at position 0')
    if H * W > INT32_MAX:
        raise NotImplementedError('contours2overlay: more than 2 ** 31 - 1 pixels')
    if colors is None:
        colors = torch.as_tensor(random_colors_hsv(K, hue_range, saturation_range, value_range, ubyte=True))
    lib = _lib.load()
    with torch.cuda.device(dev):
        col = colors.to(dev).contiguous()
        con = contours.contiguous().float()
        i32 = dict(dtype=torch.int32, device=dev)
        pts = torch.empty((K, S, 2), **i32)
        boxes = torch.empty((K, 4), **i32)
        check(lib.cpn_labels_prepare(ptr(con), K, S, H, W, int(bool(rounded)), int(bool(clip)), ptr(pts), ptr(boxes),
                                     stream_ptr()), 'labels_prepare')
        if not clip:
            bmin = boxes[:, :2].min(0).values.cpu().tolist()
            bmax = boxes[:, 2:].max(0).values.cpu().tolist()
            if min(bmin) < 0:
                raise ValueError('contours2overlay: negative coordinates need clip=True')
            if bmax[0] >= W or bmax[1] >= H:
                raise ValueError('contours2overlay: contours outside the image need clip=True')
        begin, lst, pairs = _tile_lists(lib, boxes, K, H, W)
        out = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
        most = torch.zeros(1, **i32)
        host = c_uint32(0)
        check(lib.cpn_overlay_paint(ptr(pts), ptr(boxes), ptr(col), K, S, H, W, ptr(begin), ptr(lst), ptr(out), ptr(most), host,
                                    stream_ptr()), 'overlay_paint')
    max_overlap = int(host.value)
    if max_overlap > limit:
        raise ValueError(f'contours2overlay: {max_overlap} contours overlap on one pixel; intermediate_dtype={dt.name!r} holds the '
                         f'colour sums of at most {limit} (the reference wraps silently beyond)')
    return result(out, col, dict(max_overlap=max_overlap, pairs=pairs, tiles=tiles))


def _color_table(colors, n_rand, alpha):
    """The uint8 ``[n + 1, 4]`` table of ``label_cmap`` (cmaps.py:41-65 with rgba, zero_val = 0 and ubyte): row 0 is the zero
    label, row ``i + 1`` colour ``i``."""
    if isinstance(colors, str):
        if colors == 'rand':
            colors = random_colors_hsv(n_rand)
        else:
            if colors not in QUALITATIVE_MAPS:
                raise ValueError(f"label_cmap: colors={colors!r} is neither 'rand' nor one of matplotlib's qualitative maps "
                                 f'{QUALITATIVE_MAPS}')
            from matplotlib import pyplot as plt
            colors = plt.get_cmap(colors).colors
    if isinstance(colors, torch.Tensor):
        colors = colors.detach().cpu().numpy()
    colors = np.array(colors, dtype=np.float64)
    if colors.ndim != 2 or colors.shape[1] not in (3, 4) or len(colors) < 1:
        raise ValueError(f'label_cmap: colors must be [n, 3] or [n, 4] (got {colors.shape})')
    if colors.min() < 0. or colors.max() > 1.:
        raise ValueError('label_cmap: colors must lie in [0, 1]')
    if colors.shape[1] == 3:
        colors = np.concatenate((colors, np.ones((len(colors), 1))), -1)
    if alpha is not None:
        colors[:, -1] = alpha
    colors = np.concatenate((np.zeros_like(colors[:1]), colors))
    return np.clip(np.rint(colors * 255), 0, 255).astype(np.uint8)  # skimage.img_as_ubyte on floats: half to even


def label_cmap(labels, colors='rand', zero_val=0., rgba=True, alpha=None, reduce_axis=2, neg_alpha_factor=.5, ubyte=False):
    """Label image Tensor[H, W] or [H, W, C] (integers, on the GPU) -> RGBA image, uint8 Tensor[H, W, 4] on the GPU, with
    exactly the values of the reference's ``label_cmap(..., ubyte=True)`` (cmaps.py:21-77).  Arguments as there.

    colors: ``'rand'`` draws ``max(1, min(9999, labels.max()))`` colours with ``random_colors_hsv`` (one value is read back from
        the device); a matplotlib qualitative map name; or an ``[n, 3 | 4]`` float array in [0, 1].  Label ``v`` takes colour
        ``v % n`` (row ``v % n + 1`` of the table, whose row 0 is the zero label).
    ubyte: must be ``True`` (the float image is not implemented); likewise ``rgba=True``, ``zero_val=0`` and ``reduce_axis`` in
        ``(2, -1, None)``.  A negative label raises ``ValueError`` (the reference fails on that path with ``ubyte=True``:
        ``neg_alpha_factor`` cannot be applied to uint8 in place)."""
    if not ubyte:
        raise NotImplementedError('label_cmap: ubyte=False (a float image) is not implemented on the HIP path; pass ubyte=True')
    if not rgba:
        raise NotImplementedError('label_cmap: rgba=False is not implemented on the HIP path')
    if zero_val is None or isinstance(zero_val, (tuple, list, np.ndarray, torch.Tensor)) or float(zero_val) != 0.:
        raise NotImplementedError(f'label_cmap: zero_val={zero_val!r} is not implemented on the HIP path (only 0)')
    if reduce_axis not in (2, -1, None):
        raise NotImplementedError(f'label_cmap: reduce_axis={reduce_axis!r} is not implemented on the HIP path (only 2, -1 or None)')
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f'label_cmap: labels must be a Tensor on the GPU (got {type(labels).__name__})')
    if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise TypeError(f'label_cmap: labels must hold integers (got {labels.dtype})')
    if labels.ndim not in (2, 3):
        raise ValueError(f'label_cmap: labels must be [H, W] or [H, W, C] (got {tuple(labels.shape)})')
    if labels.ndim == 3 and reduce_axis is None:
        raise NotImplementedError('label_cmap: reduce_axis=None with [H, W, C] labels (an [H, W, C, 4] image) is not implemented '
                                  'on the HIP path')
    if labels.ndim == 3 and labels.shape[2] < 1:
        raise ValueError('label_cmap: labels has no channel')
    if not labels.is_cuda:
        raise RuntimeError('celldetection_amd.label_cmap runs on the MI355X only (got a CPU tensor).')
    H, W = int(labels.shape[0]), int(labels.shape[1])
    C = int(labels.shape[2]) if labels.ndim == 3 else 1
    if H * W > INT32_MAX:
        raise NotImplementedError('label_cmap: more than 2 ** 31 - 1 pixels')
    x = labels
    top = None
    if x.dtype not in (torch.int32, torch.int16, torch.int8, torch.uint8) and x.numel():
        low, top = int(x.min()), int(x.max())
        if low < INT32_MIN or top > INT32_MAX:
            raise ValueError('label_cmap: labels holds values that do not fit int32')
    x = x.to(torch.int32).contiguous()
    n_rand = 1
    if isinstance(colors, str) and colors == 'rand' and x.numel():
        n_rand = max(1, min(9999, int(x.max()) if top is None else top))
    table = _color_table(colors, n_rand, alpha)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        tab = torch.as_tensor(table).to(x.device)
        out = torch.empty((H, W, 4), dtype=torch.uint8, device=x.device)
        flag = torch.zeros(1, dtype=torch.int32, device=x.device)
        host = c_int32(0)
        check(lib.cpn_label_cmap(ptr(x), H * W, C, int(labels.ndim == 3), ptr(tab), int(tab.shape[0]), ptr(out), ptr(flag), host,
                                 stream_ptr()), 'label_cmap')
    if host.value:
        raise ValueError('label_cmap: negative labels are not supported on the HIP path')
    return out
