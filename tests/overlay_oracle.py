"""TEST INFRASTRUCTURE ONLY: the rules of ``contours2overlay`` (celldetection/data/cpn.py:647-662,699-723,811-855) and of
``label_cmap(..., ubyte=True)`` (celldetection/visualization/cmaps.py:21-77) restated in numpy.

Not a fallback: nothing in ``celldetection_amd`` imports this file.  ``tests/test_overlay.py`` pins it to outputs of the
reference's own functions (``tests/golden/overlay.npz``); the GPU tests then use it on cases the fixture does not hold.

    overlay:  points = np.round (half to even), clipped to the image, truncated to integers; every polygon filled with
              ``labels_oracle.fill_polygon``; n(p) = contours covering pixel p, S(p) = per-channel sum of their uint8 colours;
              out(p) = (Sr // n, Sg // n, Sb // n, 255) where n >= 1, (0, 0, 0, 0) elsewhere
    cmap:     table = rint(255 * [zero row; colours with alpha]) as uint8; label v -> row v % n + 1, 0 -> row 0; a 2-D image
              is table[row]; an [H, W, C] image is reduced per pixel in float32: den = float32(sum_c a_c) + 1e-12,
              w_c = a_c / den, acc_j += w_c * col_cj for c = 0 .. C-1 in order (separate multiply and add), truncated to uint8

``mutant`` selects a deliberately wrong rule (the fixture must tell each of them from the right one).
"""
import numpy as np

from labels_oracle import fill_polygon

OVERLAY_MUTANTS = ('rounded_mean', 'last_wins', 'no_normalisation', 'sums_8bit', 'truncated_points')
CMAP_MUTANTS = ('rounded_cast', 'float64', 'fma', 'no_plus_one', 'half_up_table')
MUTANTS = OVERLAY_MUTANTS + CMAP_MUTANTS


def pad_contours(contours):
    """A list of [S_i, 2] arrays -> [K, S, 2], the last point repeated (what ``cda.contours2overlay`` does with a list)."""
    arrs = [np.asarray(c, np.float32).reshape(-1, 2) for c in contours]
    smax = max(len(a) for a in arrs)
    return np.stack([np.concatenate((a, np.repeat(a[-1:], smax - len(a), 0))) for a in arrs])


def contours2overlay(contours, size, colors, rounded=True, clip=True, return_count=False, mutant=None):
    """contours: sequence of [S_i, 2] (xy) or None; colors uint8 [K, 3] -> uint8 [H, W, 4] (and the overlap count)."""
    assert mutant is None or mutant in OVERLAY_MUTANTS
    H, W = size
    total = np.zeros((H, W, 3), np.int64)
    n = np.zeros((H, W), np.int64)
    last = np.zeros((H, W, 3), np.int64)
    for k, contour in enumerate(contours if contours is not None else ()):
        c = np.array(contour, np.float32).reshape(-1, 2)
        if rounded and mutant != 'truncated_points':
            c = np.round(c)
        if clip:
            c[:, 0] = np.clip(c[:, 0], 0, W - 1)
            c[:, 1] = np.clip(c[:, 1], 0, H - 1)
        p = c.astype(np.int32)
        x0, y0, x1, y1 = max(p[:, 0].min(), 0), max(p[:, 1].min(), 0), min(p[:, 0].max(), W - 1), min(p[:, 1].max(), H - 1)
        m = np.zeros((H, W), bool)
        if x1 >= x0 and y1 >= y0:  # the fill never leaves the bounding box of the integer points
            m[y0:y1 + 1, x0:x1 + 1] = fill_polygon(p, x0, y0, x1 - x0 + 1, y1 - y0 + 1)
        col = np.asarray(colors[k], np.uint8).astype(np.int64)
        total[m] += col
        if mutant == 'sums_8bit':
            total &= 255
        last[m] = col
        n += m
    out = np.zeros((H, W, 4), np.uint8)
    cov = n > 0
    div = np.maximum(n, 1)[..., None]
    if mutant == 'rounded_mean':
        rgb = (2 * total + div) // (2 * div)
    elif mutant == 'last_wins':
        rgb = last
    elif mutant == 'no_normalisation':
        rgb = total
    else:
        rgb = total // div
    out[..., :3] = np.where(cov[..., None], rgb, 0).astype(np.uint8)  # astype wraps, as the reference's final cast does
    out[..., 3] = np.where(cov, 255, 0)
    return (out, n) if return_count else out


def color_table(colors, alpha=None, mutant=None):
    """float colours [n, 3 | 4] in [0, 1] -> uint8 [n + 1, 4] with the zero row in front."""
    colors = np.array(colors, np.float64)
    if colors.shape[1] == 3:
        colors = np.concatenate((colors, np.ones((len(colors), 1))), -1)
    if alpha is not None:
        colors[:, -1] = alpha
    colors = np.concatenate((np.zeros_like(colors[:1]), colors))
    if mutant == 'half_up_table':
        return np.floor(colors * 255 + .5).astype(np.uint8)
    return np.rint(colors * 255).astype(np.uint8)


def label_cmap(labels, colors, alpha=None, mutant=None):
    """int labels [H, W] or [H, W, C] (>= 0), float colours [n, 3 | 4] -> uint8 [H, W, 4]."""
    assert mutant is None or mutant in CMAP_MUTANTS
    labels = np.asarray(labels)
    assert labels.dtype.kind in 'iu' and labels.ndim in (2, 3) and (labels >= 0).all()
    table = color_table(colors, alpha, mutant)
    n = len(table) - 1
    x = labels.astype(np.int64)
    rows = np.where(x != 0, x % n + (0 if mutant == 'no_plus_one' else 1), 0)
    res = table[rows]
    if labels.ndim == 2:
        return res
    ft = np.float64 if mutant == 'float64' else np.float32
    a = res[..., 3]
    den = a.sum(-1, dtype=np.int64).astype(np.float32).astype(ft) + ft(1e-12)
    acc = np.zeros(labels.shape[:2] + (4,), ft)
    for c in range(labels.shape[2]):
        w = a[:, :, c].astype(ft) / den
        prod = w[..., None] * res[:, :, c].astype(ft)
        if mutant == 'fma':  # one rounding for multiply and add
            acc = (w[..., None].astype(np.float64) * res[:, :, c].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        else:
            acc = acc + prod
    if mutant == 'rounded_cast':
        return np.rint(acc).astype(np.uint8)
    return acc.astype(np.uint8)
