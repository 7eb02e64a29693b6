"""Plain numpy restatement of component labelling (``celldetection_amd.components``; the contract is the "Component labelling"
section of ``include/cpn_hip.h``): a sequential union-find for the rule, and the loops of the reference's ``relabel_``,
``stack_labels``, ``unary_masks2labels`` (celldetection/data/segmentation.py:106-167), ``masks2labels`` (data/cpn.py:147-176) with
its ``cnt`` arithmetic, and ``rgb_to_scalar`` (data/misc.py:264-280) on top of it.  Shares no code with the stand-ins of
``tests/golden/make_golden_components.py`` (scipy.ndimage), so each checks the other.

``mutant`` selects a deliberately wrong rule; ``tests/test_components.py`` asserts that the fixture tells every one of them from
the right one.
"""
import numpy as np

MUTANTS = ('conn4', 'column_major', 'restart_per_channel', 'count_negatives', 'renumber_negatives', 'link_different',
           'cnt_empty_repaired', 'cnt_full_repaired', 'by_value')


def roots_image(channel, connectivity=8, mode='equal'):
    """int [H, W] -> int64 [H, W]: the raster index of the first pixel of every pixel's component, -1 where the pixel takes no
    part.  mode: 'equal' (v > 0, same value), 'nonzero' (v != 0, all alike), 'any_value' (v != 0, same value: what
    skimage.measure.label(background=0) links) or 'positive' (v > 0, all alike: a wrong rule)."""
    assert connectivity in (4, 8) and channel.ndim == 2
    H, W = channel.shape
    a = np.asarray(channel).astype(np.int64)
    if mode == 'nonzero':
        a = (a != 0).astype(np.int64)
    elif mode == 'positive':
        a = (a > 0).astype(np.int64)
    part = (a != 0) if mode == 'any_value' else (a > 0)
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    # the links (pixel, earlier neighbour) of the rule, found with array comparisons; the union-find itself is sequential
    idx = np.arange(H * W).reshape(H, W)
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])  # to the W, N, NW and NE neighbour
    for dy, dx in steps:
        ys, yn = slice(dy, H), slice(0, H - dy)
        xs, xn = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
        link = part[ys, xs] & part[yn, xn] & (a[ys, xs] == a[yn, xn])
        for i, j in zip(idx[ys, xs][link].tolist(), idx[yn, xn][link].tolist()):
            ra, rb = find(i), find(j)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)  # the root is the smallest index: the raster-first pixel
    out = np.full(H * W, -1, np.int64)
    for i in np.flatnonzero(part.reshape(-1)).tolist():
        out[i] = find(i)
    return out.reshape(H, W)


def label_components(labels, connectivity=8, mode='equal', first=1, mutant=None):
    """The rule: int [H, W, C] -> (labelled copy, components per channel int64 [C])."""
    assert mutant in (None,) + MUTANTS
    labels = np.asarray(labels)
    assert labels.ndim == 3
    if mutant == 'conn4':
        connectivity = 4
    out = labels.copy()
    counts = np.zeros(labels.shape[2], np.int64)
    H, W = labels.shape[:2]
    nxt = first
    for c in range(labels.shape[2]):
        ch = labels[:, :, c]
        link = mode
        if mutant == 'link_different' and mode == 'equal':
            link = 'positive'
        if mutant in ('count_negatives', 'renumber_negatives') and mode == 'equal':
            link = 'any_value'
        roots = roots_image(ch, connectivity, link)
        ids = np.unique(roots[roots >= 0])
        if mutant == 'column_major':
            key = {}
            ys, xs = np.nonzero(roots >= 0)
            for y, x in zip(ys.tolist(), xs.tolist()):
                r = int(roots[y, x])
                key[r] = min(key.get(r, H * W), x * H + y)
            ids = np.asarray(sorted(key, key=key.get), np.int64)
        elif mutant == 'by_value':
            ids = np.asarray(sorted(ids.tolist(), key=lambda r: (int(ch.reshape(-1)[r]), r)), np.int64)
        if mutant == 'restart_per_channel':
            nxt = first
        number = {}  # root -> the component's number
        for r in ids.tolist():
            negative = ch.reshape(-1)[r] < 0
            if negative and mutant == 'count_negatives':
                nxt += 1
                continue
            number[r] = nxt
            nxt += 1
            counts[c] += 1
        u, inv = np.unique(roots.reshape(-1), return_inverse=True)
        given = np.asarray([r in number for r in u.tolist()], bool)[inv].reshape(H, W)
        value = np.asarray([number.get(r, 0) for r in u.tolist()], np.int64)[inv].reshape(H, W)
        out[:, :, c][given] = value[given]
    return out, counts


def skimage_label(channel, connectivity=8):
    """skimage.measure.label(channel, background=0) with full connectivity: equal values of any sign link; 1, 2, ... in raster
    order of the first pixels."""
    roots = roots_image(channel, connectivity, 'any_value')
    out = np.zeros(channel.shape, np.int64)
    out[roots >= 0] = np.searchsorted(np.unique(roots[roots >= 0]), roots[roots >= 0]) + 1
    return out


def relabel(label_stack):
    """The reference's loop (relabel_), on a copy."""
    stack = np.array(label_stack)
    assert stack.ndim == 3
    neg = stack < 0
    cur_max = 0
    for channel in range(stack.shape[2]):
        lab = skimage_label(stack[:, :, channel])
        for u in sorted(set(np.unique(lab).tolist()) - {0}):
            mask = lab == u
            if np.any(mask & neg[:, :, channel]):
                continue
            cur_max += 1
            stack[mask, channel] = cur_max
    return stack


def rgb_to_scalar(inputs, dtype='int32'):
    red, green, blue = inputs[..., 0], inputs[..., 1], inputs[..., 2]
    rgb = red.astype(dtype)
    rgb = (rgb << 8) + green
    rgb = (rgb << 8) + blue
    return rgb


def stack_labels(*maps, dtype='int32', relabel_stack=True):
    maps = [rgb_to_scalar(m, dtype) if (m.ndim == 3 and m.shape[2] == 3) else m.astype(dtype) for m in maps]
    stack = np.stack(maps, 2)
    return relabel(stack) if relabel_stack else stack


def unary_masks2labels(masks, transpose=True):
    masks = np.asarray(masks)
    lbl = (masks > 0) * np.arange(1, len(masks) + 1)[:, None, None]
    return lbl.transpose((1, 2, 0)) if transpose else lbl


def connected_components(mask, connectivity=8):
    """cv2.connectedComponents as the contract states it: (number of labels with the background, int32 labels), components of
    non-zero pixels numbered 1, 2, ... in raster order of their first pixels."""
    roots = roots_image(np.asarray(mask), connectivity, 'nonzero')
    out = np.zeros(roots.shape, np.int32)
    ids = np.unique(roots[roots >= 0])
    out[roots >= 0] = np.searchsorted(ids, roots[roots >= 0]) + 1
    return len(ids) + 1, out


def masks2labels(masks, connectivity=8, label_axis=2, count=False, reduce=np.max, keepdims=True, mutant=None):
    """The reference's loop with its cnt arithmetic."""
    labels, cnt = [], 0
    for m in masks:
        a, b = connected_components(m, connectivity)
        if cnt > 0:
            b[b > 0] += cnt
        if mutant == 'cnt_empty_repaired':
            cnt += a - (1 if 0 in b else 0)  # a mask without foreground no longer advances the count
        elif mutant == 'cnt_full_repaired':
            cnt += a - (1 if a > 1 else 0)  # a mask without background no longer advances it by one more
        else:
            cnt += a - (1 if (a > 1 and 0 in b) else 0)
        labels.append(b)
    labels = np.stack(labels, label_axis)
    if reduce is not None:
        labels = reduce(labels, axis=label_axis, keepdims=keepdims)
    return (labels, cnt) if count else labels


def same_partition(a, b):
    """True when two label arrays split the same foreground into the same sets (the labels may be permuted)."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if a.shape != b.shape or not np.array_equal(a > 0, b > 0):
        return False
    pairs = np.unique(np.stack([a[a > 0], b[a > 0]], 1), axis=0)
    return len(pairs) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1]))
