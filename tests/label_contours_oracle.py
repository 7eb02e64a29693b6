"""TEST INFRASTRUCTURE ONLY: the rules of ``labels2contours`` / ``labels2contour_list`` (celldetection/data/cpn.py:93-144) and of
``resample_contours`` (celldetection/data/misc.py:371-405) restated in numpy and plain Python.

Not a fallback: nothing in ``celldetection_amd`` imports this file.  ``tests/test_label_contours.py`` pins it to outputs of the
reference's own functions (``tests/golden/label_contours.npz``); the GPU tests then use it on cases the fixture does not hold.

    objects:     a pair (channel, value v > 0); values <= 0 take no part
    components:  8-connected sets of pixels of one channel that hold v, found by flood fill in raster order
    contour:     an object with ONE component: Suzuki-Abe border following of the outer border (cv2.findContours with
                 RETR_EXTERNAL, CHAIN_APPROX_NONE): start at the raster-first pixel; directions 0 .. 7 = E, NE, N, NW, W, SW, S, SE;
                 the first search goes clockwise on screen from the west neighbour (NW, N, NE, E, SE, S, SW, W); every further
                 search counter-clockwise, starting after the pixel just left; every visit is a point; stop when the start pixel
                 is re-entered from the neighbour the first search found; a single pixel is emitted twice; points are (x, y)
    fragmented:  an object with more than one component (a component enclosed by another one of the same value counts): every
                 pixel of every channel holding the value becomes ``constant`` / ValueError / skipped
    order:       ascending value; of a value in several channels the highest channel in which it is unfragmented
    resample:    float64: p closed by its first point; dt = sqrt(dx^2 + dy^2) + epsilon; cumsum sequentially; t_j = j * (total /
                 num); i = first index with t_j <= cumsum[i]; alpha = (t_j - cumsum0[i]) / dt[i]; p_i * (1 - alpha) + p_(i+1) * alpha

``mutant`` selects a deliberately wrong rule (the fixture must tell each of them from the right one).
"""
import numpy as np

CONTOUR_MUTANTS = ('clockwise', 'four_connected', 'wrong_start', 'thin_once', 'single_not_doubled', 'first_appearance',
                   'frag_four')
RESAMPLE_MUTANTS = ('resample_open', 'search_lt', 'no_epsilon', 't_num_minus_1')
MUTANTS = CONTOUR_MUTANTS + RESAMPLE_MUTANTS

DIRECTIONS = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))  # (dx, dy) of E, NE, N, NW, W, SW, S, SE


def components(channel, connectivity=8):
    """int [H, W] -> [(value, [flat indices into the image padded by one pixel, the raster-first one first])], in the order of
    their raster-first pixels; values <= 0 take no part."""
    H, W = channel.shape
    pad = np.zeros((H + 2, W + 2), np.int64)
    pad[1:-1, 1:-1] = channel
    wp = W + 2
    flat = pad.ravel().tolist()
    offs = (-wp, -1, 1, wp) if connectivity == 4 else (-wp - 1, -wp, -wp + 1, -1, 1, wp - 1, wp, wp + 1)
    seen = bytearray(len(flat))
    out = []
    for s in np.flatnonzero(pad.ravel() > 0).tolist():
        if seen[s]:
            continue
        v = flat[s]
        seen[s] = 1
        stack, comp = [s], []
        while stack:
            q = stack.pop()
            comp.append(q)
            for o in offs:
                r = q + o
                if not seen[r] and flat[r] == v:
                    seen[r] = 1
                    stack.append(r)
        out.append((v, comp))
    return out


def trace(pixels, wp, mutant=None):
    """pixels: flat indices (row stride ``wp``) of ONE component -> its contour as a list of flat indices."""
    inside = set(pixels)
    start = min(pixels)
    if mutant == 'wrong_start':  # the leftmost pixel (smallest x, then smallest y)
        start = min(pixels, key=lambda q: (q % wp, q // wp))
    step = [dx + dy * wp for dx, dy in DIRECTIONS]
    first_turn, turn = (1, -1) if mutant == 'clockwise' else (-1, 1)
    stride = 2 if mutant == 'four_connected' else 1

    def search(q, d, sense):
        for _ in range(8 // stride):
            d = (d + sense * stride) % 8
            if q + step[d] in inside:
                return d
        return None

    first = search(start, 4, first_turn)
    if first is None:
        return [start] if mutant == 'single_not_doubled' else [start, start]
    stop = start + step[first]
    out, q, came = [], start, first
    for _ in range(8 * len(pixels) + 8):
        d = search(q, came, turn)
        out.append(q)
        nxt = q + step[d]
        if nxt == start and q == stop:
            break
        q, came = nxt, (d + 4) % 8
    else:
        raise AssertionError('the trace did not close')
    if mutant == 'thin_once':
        seen = set()
        out = [p for p in out if not (p in seen or seen.add(p))]
    return out


def _xy(flat, wp):
    a = np.asarray(flat, np.int64)
    return np.stack((a % wp - 1, a // wp - 1), 1).astype(np.int32)


def find_contours(mask, offset=(0, 0), mutant=None):
    """The contours of every 8-connected component of ``mask != 0`` ([h, w]), each int32 [n, 1, 2] as (x, y) + offset: the
    stand-in for ``cv2.findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_NONE, offset=offset)[-2]`` under the rule above (a
    single pixel gives ONE point here, as in cv2; the reference doubles it)."""
    mask = np.asarray(mask)
    wp = mask.shape[1] + 2
    out = []
    for _, comp in components((mask != 0).astype(np.int64)):
        pts = trace(comp, wp, mutant)
        if len(comp) == 1:
            pts = pts[:1]
        out.append((_xy(pts, wp) + np.asarray(offset, np.int32))[:, None])
    return out


def labels2contours_packed(labels, flag_fragmented_inplace=False, raise_fragmented=True, constant=-1, mutant=None):
    """int [H, W, C] -> (ids int32 [K], offsets int64 [K + 1], points int32 [P, 2]).  May modify ``labels`` in place."""
    assert mutant is None or mutant in CONTOUR_MUTANTS
    assert labels.ndim == 3
    wp = labels.shape[1] + 2
    found, fragmented = {}, []
    for c in range(labels.shape[2]):
        by_value = {}
        for v, comp in components(labels[:, :, c]):
            by_value.setdefault(v, []).append(comp)
        for v in sorted(by_value):
            comps = by_value[v]
            n = len(comps)
            if mutant == 'frag_four':
                m = np.zeros((labels.shape[0] + 2) * wp, np.int64)
                m[sum(comps, [])] = 1
                n = len(components(m.reshape(-1, wp)[1:-1, 1:-1], 4))
            if n > 1:
                fragmented.append(v)
                continue
            found[v] = _xy(trace(comps[0], wp, mutant), wp)  # a higher channel overwrites (and keeps the first position)
    if fragmented:
        if flag_fragmented_inplace:
            labels[np.isin(labels, fragmented)] = constant
        elif raise_fragmented:
            raise ValueError('Object labeled with multiple connected components.')
    ids = list(found) if mutant == 'first_appearance' else sorted(found)
    offsets = np.cumsum([0] + [len(found[i]) for i in ids]).astype(np.int64)
    points = np.concatenate([found[i] for i in ids]) if ids else np.zeros((0, 2), np.int32)
    return np.asarray(ids, np.int32), offsets, points.astype(np.int32)


def labels2contour_list(labels, **kwargs):
    if labels.ndim == 2:
        labels = labels[..., None]
    _, offsets, points = labels2contours_packed(labels, **kwargs)
    return [points[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


def resample_contour(contour, num, close=True, epsilon=1e-6, mutant=None):
    """[n, 2] -> float64 [num, 2]."""
    assert mutant is None or mutant in RESAMPLE_MUTANTS
    p = np.asarray(contour, np.float64)
    if close and mutant != 'resample_open':
        p = np.concatenate((p, p[:1]))
    d = p[1:] - p[:-1]
    dt = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    if mutant != 'no_epsilon':
        dt = dt + epsilon
    cumsum = np.zeros(len(dt))
    s = 0.
    for i, v in enumerate(dt.tolist()):  # sequentially, in index order
        s = v if i == 0 else s + v
        cumsum[i] = s
    cumsum0 = np.concatenate(([0.], cumsum))
    t = np.arange(num) * (cumsum[-1] / (max(num - 1, 1) if mutant == 't_num_minus_1' else num))
    hit = (t[:, None] < cumsum[None]) if mutant == 'search_lt' else (t[:, None] <= cumsum[None])
    i = np.argmax(hit, 1)
    with np.errstate(all='ignore'):
        alpha = ((t - cumsum0[i]) / dt[i])[:, None]
        return p[i] * (1 - alpha) + p[i + 1] * alpha


def resample_contours(contours, num, close=True, epsilon=1e-6, mutant=None):
    """A list / tuple of [n_k, 2] -> the same container of [num, 2]; an array [..., n, 2] -> [..., num, 2]."""
    if isinstance(contours, (list, tuple)):
        return type(contours)(resample_contour(c, num, close, epsilon, mutant) for c in contours)
    contours = np.asarray(contours)
    lead = contours.shape[:-2]
    out = [resample_contour(c, num, close, epsilon, mutant) for c in contours.reshape((-1,) + contours.shape[-2:])]
    return np.stack(out).reshape(lead + (num, 2)) if out else np.zeros(lead + (num, 2))


def fill_holes(mask):
    """bool [H, W] -> the mask with its holes filled: everything the background cannot reach from outside the image through
    4-connected steps (the complement of an 8-connected object is 4-connected)."""
    H, W = mask.shape
    outside = components(np.pad(~mask, 1, constant_values=True).astype(np.int64), 4)[0][1]
    reach = np.zeros((H + 4) * (W + 4), bool)
    reach[outside] = True
    return ~reach.reshape(H + 4, W + 4)[2:-2, 2:-2]


def ragged_object(rng, h, w, steps):
    """bool [h, w]: the trail of a random walk with 8-connected steps from the centre (clipped to the grid), some steps two
    pixels wide: one 8-connected object with thin parts, diagonal links, holes and border contact."""
    m = np.zeros((h, w), bool)
    y, x = h // 2, w // 2
    for _ in range(steps):
        m[y, x] = True
        if rng.random() < .3:
            m[min(y + 1, h - 1), x] = True
        dx, dy = DIRECTIONS[int(rng.integers(8))]
        y, x = min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)
    return m
