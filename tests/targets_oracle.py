"""CPN training targets restated in numpy: ``labels2distances``, ``mask_labels_by_distance_`` (celldetection/data/cpn.py:424-497)
and ``filter_instances_`` (celldetection/data/segmentation.py:67-103) of the reference, by rule and not by its code, so that the
tests can pin the rule to the reference's recorded results (tests/golden/targets.npz) and hold the GPU kernels to the rule.

The chamfer transform here is the two-pass raster algorithm of OpenCV's ``distanceTransform`` for a 3 x 3 mask (16-bit fixed
point, a border of DIST_MAX = 2^32 - 1 - DIAG around the image, forward pass over the upper and left neighbours, backward pass
over the lower and right ones, result float32(t) * 2^-16): ``chamfer_literal`` pixel by pixel, ``chamfer`` the same recurrences
with each row's left-to-right dependency written as a running minimum (asserted equal in tests/test_targets.py).  The GPU
kernels compute the same numbers as the fixed point of a relaxation, so oracle and kernel are independent statements.
``closed_form`` is the third: min over zero pixels of DIAG * min(|dx|, |dy|) + HV * (max - min).

``MUTANTS`` are wrong rules; the fixture's disc images are chosen so that each one changes the result there.
"""
import numpy as np

DIST_L1, DIST_L2, DIST_C = 1, 2, 3
SHIFT = 16
WEIGHTS = {DIST_L1: (1., 2.), DIST_L2: (.955, 1.3693), DIST_C: (1., 1.)}  # OpenCV's 3 x 3 masks: straight, diagonal
UINT_MAX = 2 ** 32 - 1
DISTANCE_MUTANTS = ('diag_2hv', 'no_ring', 'protected_ge', 'overlap_owner', 'clip_first')  # change the instance mode
FG_MUTANTS = ('diag_2hv', 'fg_ring', 'bbox_max', 'overlap_owner')  # change the fg mode
MASK_MUTANTS = ('bg_lt',)
FILTER_MUTANTS = ('count_per_channel',)
MUTANTS = tuple(dict.fromkeys(DISTANCE_MUTANTS + FG_MUTANTS + MASK_MUTANTS + FILTER_MUTANTS))


def weights(distance_type, mutant=None):
    """(HV, DIAG) in 16-bit fixed point: cvRound(w * 2^16)."""
    if distance_type not in WEIGHTS:
        raise ValueError(f'distance_type {distance_type!r}')
    hv, diag = (int(np.rint(w * (1 << SHIFT))) for w in WEIGHTS[distance_type])
    return (hv, 2 * hv) if mutant == 'diag_2hv' else (hv, diag)


def chamfer_literal(mask, distance_type=DIST_L2, mutant=None):
    """uint32 t of the two-pass algorithm, pixel by pixel (small arrays only)."""
    hv, diag = weights(distance_type, mutant)
    dmax = UINT_MAX - diag
    h, w = mask.shape
    tmp = [[dmax] * (w + 2) for _ in range(h + 2)]
    for i in range(1, h + 1):
        for j in range(1, w + 1):
            if not mask[i - 1, j - 1]:
                tmp[i][j] = 0
            else:
                t0 = min(tmp[i - 1][j - 1] + diag, tmp[i - 1][j] + hv, tmp[i - 1][j + 1] + diag, tmp[i][j - 1] + hv)
                tmp[i][j] = min(t0, dmax)
    out = np.zeros((h, w), np.uint32)
    for i in range(h, 0, -1):
        for j in range(w, 0, -1):
            t0 = tmp[i][j]
            if t0 > hv:
                t0 = min(t0, tmp[i + 1][j + 1] + diag, tmp[i + 1][j] + hv, tmp[i + 1][j - 1] + diag, tmp[i][j + 1] + hv)
                tmp[i][j] = t0
            out[i - 1, j - 1] = min(t0, dmax)
    return out


def chamfer(mask, distance_type=DIST_L2, mutant=None):
    """uint32 t of the two-pass algorithm; a row's dependency on its left (right) neighbour is the running minimum
    t[j] = j * HV + min over k <= j of (a[k] - k * HV), a = what the row above (below) and the pixel itself give."""
    hv, diag = weights(distance_type, mutant)
    dmax = UINT_MAX - diag
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    if h == 0 or w == 0:
        return np.zeros((h, w), np.uint32)
    ramp = np.arange(w, dtype=np.int64) * hv
    tmp = np.empty((h, w), np.int64)
    prev = np.full(w + 2, dmax, np.int64)
    for i in range(h):
        a = np.minimum(np.minimum(prev[:-2] + diag, prev[1:-1] + hv), prev[2:] + diag)
        a = np.minimum(a, dmax + hv)  # the left border
        a[~mask[i]] = 0
        row = np.minimum(np.minimum.accumulate(a - ramp) + ramp, dmax)
        row[~mask[i]] = 0
        tmp[i] = row
        prev[1:-1] = row
    prev = np.full(w + 2, dmax, np.int64)
    for i in range(h - 1, -1, -1):
        a = np.minimum(np.minimum(prev[:-2] + diag, prev[1:-1] + hv), prev[2:] + diag)
        a = np.minimum(np.minimum(a, tmp[i]), dmax + hv)
        row = np.minimum(np.minimum.accumulate((a + ramp)[::-1])[::-1] - ramp, tmp[i])
        tmp[i] = row
        prev[1:-1] = row
    return np.minimum(tmp, dmax).astype(np.uint32)


def closed_form(mask, distance_type=DIST_L2):
    """uint32 t = min over zero pixels q of DIAG * min(|dx|, |dy|) + HV * (max - min); needs a zero pixel."""
    hv, diag = weights(distance_type)
    mask = np.asarray(mask) != 0
    zy, zx = np.nonzero(~mask)
    py, px = np.nonzero(mask)
    out = np.zeros(mask.shape, np.uint32)
    for s in range(0, len(py), 4096):
        dy = np.abs(py[s:s + 4096, None] - zy[None]).astype(np.int64)
        dx = np.abs(px[s:s + 4096, None] - zx[None]).astype(np.int64)
        lo, hi = np.minimum(dy, dx), np.maximum(dy, dx)
        out[py[s:s + 4096], px[s:s + 4096]] = (diag * lo + hv * (hi - lo)).min(1)
    return out


def to_float(t):
    return t.astype(np.float32) * np.float32(2. ** -SHIFT)


def owner_image(labels, mutant=None):
    """The one positive label where exactly one channel is > 0, otherwise 0."""
    labels = np.asarray(labels)
    pos = labels > 0
    cnt = pos.sum(2)
    top = np.where(pos, labels, 0).max(2)
    return np.where((cnt >= 1) if mutant == 'overlap_owner' else (cnt == 1), top, 0)


def labels2distances(labels, distance_type=DIST_L2, overlap_zero=True, per_instance=True, protected_size=36, mutant=None):
    """-> (distances float32 [H, W], labels with every channel of an overlap pixel set to -1)."""
    if not overlap_zero:
        raise NotImplementedError('overlap_zero=False')
    labels = np.asarray(labels)
    if labels.ndim == 2:
        labels = labels[..., None]
    out = labels.copy()
    out[(labels > 0).sum(2) > 1] = -1
    own = owner_image(labels, mutant)
    h, w = own.shape
    dist = np.zeros((h, w), np.float32)
    values = np.unique(own[own > 0])
    if per_instance:
        py, px = np.nonzero(own > 0)
        order = np.argsort(own[py, px], kind='stable')  # the pixels of every label, found in one pass
        py, px = py[order], px[order]
        cuts = np.cumsum(np.unique(own[py, px], return_counts=True)[1])[:-1]
        for v, ys, xs in zip(values, np.split(py, cuts), np.split(px, cuts)):
            y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
            m = own[y0:y1, x0:x1] == v
            if mutant == 'no_ring':
                d = to_float(chamfer(m, distance_type, mutant))
            else:
                d = to_float(chamfer(np.pad(m, 1), distance_type, mutant)[1:-1, 1:-1])
            if mutant == 'clip_first':
                d = d.clip(0., 1.)
            n = int(m.sum())
            if (n >= protected_size) if mutant == 'protected_ge' else (n > protected_size):
                dm = d.max()
                if dm > 0:
                    d = d / dm
            d = d.clip(0., 1.)
            dist[y0:y1, x0:x1][m] = d[m]
    else:
        if own.size and (own != 0).all():
            raise ValueError('per_instance=False needs a pixel without an owner')
        if mutant == 'fg_ring':
            d = to_float(chamfer(np.pad(own != 0, 1), distance_type, mutant)[1:-1, 1:-1])
        else:
            d = to_float(chamfer(own != 0, distance_type, mutant))
        for v in values:
            m = own == v
            if mutant == 'bbox_max':
                ys, xs = np.nonzero(m)
                dm = d[ys.min():ys.max() + 1, xs.min():xs.max() + 1].max()
            else:
                dm = d[m].max()
            d[m] = d[m] / np.maximum(dm, np.float32(1e-6))
        dist = d
    return dist.clip(0., 1.).astype(np.float32), out


def mask_labels_by_distance(labels, distances, max_bg_dist, min_fg_dist, mutant=None):
    """-> (masked copy of labels [H, W, C], its channel maximum)."""
    out = np.array(labels)
    bg, fg = np.float32(max_bg_dist), np.float32(min_fg_dist)
    d = np.asarray(distances, np.float32)
    low = (d < bg) if mutant == 'bg_lt' else (d <= bg)
    out[np.any(out > 0, 2) & low] = 0
    out[(d > bg) & (d < fg)] = -1
    return out, out.max(2)


def filter_instances(labels, partials=True, partials_border=1, min_area=4, max_area=None, constant=-1, continuous=True,
                     mutant=None):
    """-> filtered copy.  Counts are over all elements of the array; values <= 0 are never counted out; with ``continuous`` the
    labels above n (= number of distinct positive labels) take the missing values of 1 .. n, largest label to largest gap."""
    out = np.array(labels)
    if partials and partials_border >= 1:
        b = partials_border
        bad = set(np.unique(out[:, :b])) | set(np.unique(out[:, -b:])) | set(np.unique(out[:b])) | set(np.unique(out[-b:]))
        out[np.isin(out, list(bad - {0}))] = constant
    if max_area is not None or min_area is not None:
        if mutant == 'count_per_channel':
            per = [np.unique(out[..., c], return_counts=True) for c in range(out.shape[-1])] if out.ndim == 3 else \
                [np.unique(out, return_counts=True)]
        else:
            per = [np.unique(out, return_counts=True)]
        bad = []
        for uni, cnt in per:
            keep = uni > 0
            uni, cnt = uni[keep], cnt[keep]
            if max_area:
                bad += list(uni[cnt > max_area])
            if min_area:
                bad += list(uni[cnt < min_area])
        if bad:
            out[np.isin(out, bad)] = constant
    if continuous:
        uni = np.unique(out[out > 0])
        n = len(uni)
        gaps = np.setdiff1d(np.arange(1, n + 1), uni)
        moved = uni[uni > n]
        assert len(gaps) == len(moved)
        src = out.copy()
        for a, b in zip(moved, gaps):  # both ascending: largest to largest
            out[src == a] = b
    return out


def same_partition(a, b):
    """True when a and b are equal up to a bijection of their values (the pixel partition is the same)."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    pairs = np.unique(np.stack((a, b), 1), axis=0)
    return a.shape == b.shape and len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))
