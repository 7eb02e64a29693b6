"""TEST INFRASTRUCTURE ONLY: the rule of ``resolve_label_channels`` (celldetection/data/cpn.py:361-399) restated in numpy.

Not a fallback: nothing in ``celldetection_amd`` imports this file.  ``tests/test_flat_labels.py`` pins it to outputs of the
reference's own function (``tests/golden/flat_labels.npz``); the GPU tests then use it on images the fixture does not hold.

    overlap pixel: more than one channel > 0;  core pixel: exactly one
    no overlap pixel at all -> the plain channel maximum
    otherwise lbl = channel maximum at core pixels, 0 elsewhere; per step every overlap pixel that still holds 0 takes the
    maximum of lbl over its footprint neighbours, all pixels at once from the previous step's values, neighbours outside
    the image taking no part; stop when no overlap pixel holds 0, when a step changes nothing, or after max_iter steps

``mutant`` selects a deliberately wrong rule (the fixture must tell each of them from the right one).
"""
import numpy as np

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
MUTANTS = ('inplace', 'smaller', 'eight', 'wrap', 'first_channel', 'plain_max', 'one_step')


def footprint(kernel):
    if isinstance(kernel, (tuple, list)):
        if tuple(kernel) != (3, 3):
            raise NotImplementedError(kernel)
        return CROSS
    kernel = np.asarray(kernel)
    assert kernel.shape == (3, 3)
    return (kernel != 0).astype(np.uint8)


def dilate(lbl, fp, wrap=False, smaller=False):
    """Maximum of ``lbl`` (int64 [H, W], values >= 0) over the footprint neighbours that lie inside the image.  ``wrap`` and
    ``smaller`` (minimum over the positive neighbours) are mutants."""
    h, w = lbl.shape
    big = np.iinfo(np.int64).max
    src = np.where(lbl > 0, lbl, big) if smaller else lbl
    fill = big if smaller else np.iinfo(np.int64).min
    out = np.full((h, w), fill, np.int64)
    for i in range(3):
        for j in range(3):
            if not fp[i, j]:
                continue
            dy, dx = i - 1, j - 1  # the neighbour at (y + dy, x + dx)
            if wrap:
                sh = np.roll(src, (-dy, -dx), (0, 1))
            else:
                sh = np.full((h, w), fill, np.int64)
                ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
                xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
                sh[yd, xd] = src[ys, xs]
            out = np.minimum(out, sh) if smaller else np.maximum(out, sh)
    if smaller:
        out[out == big] = 0
    return np.maximum(out, 0)  # no neighbour inside the image: nothing to take


def resolve_label_channels(labels, max_iter=999, kernel=(3, 3), return_stats=False, mutant=None):
    """int [H, W, C] -> [H, W] of the same dtype (and the stats of the run)."""
    assert mutant is None or mutant in MUTANTS
    labels = np.asarray(labels)
    assert labels.ndim == 3
    fp = np.ones((3, 3), np.uint8) if mutant == 'eight' else footprint(kernel)
    x = labels.astype(np.int64)
    count = (x > 0).sum(-1)
    overlap = count > 1
    stats = dict(overlap_pixels=int(overlap.sum()), unresolved_pixels=0, steps=0)
    if not overlap.any() or mutant == 'plain_max':
        out = x.max(-1)
    elif mutant == 'first_channel':
        first = np.take_along_axis(x, np.argmax(x > 0, -1)[..., None], -1)[..., 0]
        out = np.where(count > 0, first, 0)
    else:
        lbl = np.where(count == 1, x.max(-1), 0)
        for _ in range(1 if mutant == 'one_step' else max_iter):
            m = overlap & (lbl <= 0)
            if not m.any():
                break
            if mutant == 'inplace':  # raster sweep that reads what it has just written
                new = lbl.copy()
                for y, xx in zip(*np.nonzero(m)):
                    best = 0
                    for i in range(3):
                        for j in range(3):
                            yy, xj = y + i - 1, xx + j - 1
                            if fp[i, j] and 0 <= yy < new.shape[0] and 0 <= xj < new.shape[1]:
                                best = max(best, new[yy, xj])
                    new[y, xx] = best
            else:
                new = np.where(m, dilate(lbl, fp, wrap=mutant == 'wrap', smaller=mutant == 'smaller'), lbl)
            stats['steps'] += 1
            if np.array_equal(new, lbl):
                break
            lbl = new
        stats['unresolved_pixels'] = int((overlap & (lbl <= 0)).sum())
        out = lbl
    out = out.astype(labels.dtype)
    return (out, stats) if return_stats else out
