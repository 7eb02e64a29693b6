"""numpy statement of the shape property contract of include/cpn_hip.h ("Shape property tables"): perimeter,
perimeter_crofton, euler_number, area_convex, solidity of celldetection_amd.shape_properties / labels2property_table.

scikit-image is third-party and not available here; the definitions of the header are restated with their order of
operations, and tests/test_shape_props.py holds them against independent restatements (scikit-image's histogram forms with
scipy.ndimage, components minus holes, scipy.spatial.ConvexHull with an exact point test) and hand-computed anchors.

Rows are those of tests/property_table_oracle.py: channel by channel, labels ascending, values <= 0 none.  ``MUTANTS`` are
deliberately wrong variants; the tests must tell every one apart from the rule."""
from collections import OrderedDict

import numpy as np
from scipy import ndimage as ndi

SUPPORTED = ('label', 'num_pixels', 'perimeter', 'perimeter_crofton', 'euler_number', 'area_convex', 'solidity')
ALIASES = dict(convex_area='area_convex')
INTEGER = ('label', 'num_pixels', 'euler_number')
MUTANTS = ('foreground', 'erosion8', 'border_inside', 'euler_plus_qd', 'crofton_two', 'open_hull', 'hull_centres',
           'spacing_ignored', 'spacing_squared')
N1, N2, N3 = (5, 7, 15, 17, 25, 27), (21, 33), (13, 23)


def _sh(a, dr, dc):
    """a shifted so that the result at (r, c) is a[r + dr, c + dc], zero outside."""
    out = np.zeros_like(a)
    h, w = a.shape
    out[max(-dr, 0):h - max(dr, 0), max(-dc, 0):w - max(dc, 0)] = a[max(dr, 0):h - max(-dr, 0), max(dc, 0):w - max(-dc, 0)]
    return out


def bounding_boxes(label_image):
    """-> {v: (r0, r1, c0, c1)} (half-open) for every value v > 0 of a 2-D label image."""
    a = np.asarray(label_image)
    if a.size == 0:
        return {}
    vals, inv = np.unique(a, return_inverse=True)
    dense = inv.reshape(a.shape) + 1
    boxes = ndi.find_objects(dense)
    return {int(v): (sl[0].start, sl[0].stop, sl[1].start, sl[1].stop) for v, sl in zip(vals.tolist(), boxes) if v > 0}


def crop(label_image, v, mutant=None, box=None, pad=None):
    """-> (M, P, r0, c0): the mask of label v in its bounding box with a margin of 3, and the predicate P that neighbours are
    tested with (the rule: P = M).  ``box`` / ``pad``: the bounding box and the image padded by 3, where the caller has them."""
    a = np.asarray(label_image)
    if box is None:
        rs, cs = np.nonzero(a == v)
        box = rs.min(), rs.max() + 1, cs.min(), cs.max() + 1
    r0, r1, c0, c1 = box
    if pad is None:
        pad = np.pad(a.astype(np.int64), 3)
    win = pad[r0:r1 + 6, c0:c1 + 6]
    M = win == v
    P = M
    if mutant == 'foreground':
        P = win > 0
    elif mutant == 'border_inside':
        outside = np.pad(np.zeros(a.shape, bool), 3, constant_values=True)[r0:r1 + 6, c0:c1 + 6]
        P = M | outside
    return M, P, int(r0) - 3, int(c0) - 3


def counts(M, P=None, mutant=None):
    """-> dict(n, n1, n2, n3, Nv, Nh, Nd, Na, q1, q3, qd) of a mask with an empty margin of at least 2."""
    P = M if P is None else P
    M, P = M.astype(bool), P.astype(bool)
    edge = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    diag = [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    out_nb = np.zeros(M.shape, bool)
    for dr, dc in edge + (diag if mutant == 'erosion8' else []):
        out_nb |= ~_sh(P, dr, dc)
    B = M & out_nb
    Bi = B.astype(np.int64)
    o = sum(_sh(Bi, dr, dc) for dr, dc in edge)
    d = sum(_sh(Bi, dr, dc) for dr, dc in diag)
    code = (1 + 2 * o + 10 * d)[B]
    res = dict(n=int(M.sum()), n1=int(np.isin(code, N1).sum()), n2=int(np.isin(code, N2).sum()), n3=int(np.isin(code, N3).sum()))
    res.update(Nv=int((M & ~_sh(P, -1, 0)).sum()), Nh=int((M & ~_sh(P, 0, 1)).sum()), Nd=int((M & ~_sh(P, -1, -1)).sum()),
               Na=int((M & ~_sh(P, 1, -1)).sum()))
    Q = (P if mutant in ('foreground', 'border_inside') else M).astype(np.int64)
    a, b, c, dd = Q[:-1, :-1], Q[:-1, 1:], Q[1:, :-1], Q[1:, 1:]
    s = a + b + c + dd
    res.update(q1=int((s == 1).sum()), q3=int((s == 3).sum()), qd=int(((s == 2) & (a == dd)).sum()))
    return res


def hull_lattice_count(M, mutant=None):
    """Integer points in the closed convex hull of the diamond points of the pixels of M, in exact integers (doubled
    coordinates): Andrew's monotone chain over ALL points, then every lattice point of the box against every hull edge."""
    rs, cs = np.nonzero(M)
    if mutant == 'hull_centres':
        pts = {(2 * int(r), 2 * int(c)) for r, c in zip(rs, cs)}
    else:
        pts = set()
        for r, c in zip(rs.tolist(), cs.tolist()):
            pts |= {(2 * r - 1, 2 * c), (2 * r + 1, 2 * c), (2 * r, 2 * c - 1), (2 * r, 2 * c + 1)}
    pts = sorted(pts)

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    if len(pts) > 2:
        lower, upper = [], []
        for p in pts:
            while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
                lower.pop()
            lower.append(p)
        for p in reversed(pts):
            while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
                upper.pop()
            upper.append(p)
        hull = lower[:-1] + upper[:-1]
    else:
        hull = pts
    rr, cc = np.meshgrid(np.arange(rs.min(), rs.max() + 1, dtype=np.int64), np.arange(cs.min(), cs.max() + 1, dtype=np.int64),
                         indexing='ij')
    y, x = 2 * rr, 2 * cc
    if len(hull) == 1:
        return int(((y == hull[0][0]) & (x == hull[0][1])).sum())
    inside = np.ones(rr.shape, bool)
    if len(hull) == 2 or all(cross(hull[0], hull[1], p) == 0 for p in hull):  # a segment (pixel centres on a line)
        (y0, x0), (y1, x1) = min(hull), max(hull)
        on = ((y1 - y0) * (x - x0) - (x1 - x0) * (y - y0) == 0) & (y >= min(y0, y1)) & (y <= max(y0, y1)) & (x >= min(x0, x1)) & \
            (x <= max(x0, x1))
        return 0 if mutant == 'open_hull' else int(on.sum())
    for (y0, x0), (y1, x1) in zip(hull, hull[1:] + hull[:1]):
        cr = (y1 - y0) * (x - x0) - (x1 - x0) * (y - y0)
        inside &= (cr > 0) if mutant == 'open_hull' else (cr >= 0)
    return int(inside.sum())


def finalise(cnt, hull, spacing=(1., 1.), mutant=None):
    """The header's expressions, in their order of operations, on Python floats (IEEE fp64, no contraction)."""
    sy, sx = float(spacing[0]), float(spacing[1])
    s = sy
    if mutant == 'spacing_ignored':
        s = sy = sx = 1.
    elif mutant == 'spacing_squared':
        s = sy * sy
    sqrt2, pi = float(np.sqrt(2.0)), float(np.pi)
    out = dict(num_pixels=cnt['n'])
    out['perimeter'] = (float(cnt['n1']) + float(cnt['n2']) * sqrt2 + float(cnt['n3']) * ((1.0 + sqrt2) / 2.0)) * s
    if mutant == 'crofton_two':
        out['perimeter_crofton'] = (float(cnt['Nv'] + cnt['Nh']) * (pi / 2.0)) * s
    else:
        out['perimeter_crofton'] = ((float(cnt['Nv'] + cnt['Nh']) + float(cnt['Nd'] + cnt['Na']) / sqrt2) * (pi / 4.0)) * s
    q = cnt['q1'] - cnt['q3'] + (2 if mutant == 'euler_plus_qd' else -2) * cnt['qd']
    out['euler_number'] = q // 4
    out['area_convex'] = float(hull) * (sy * sx)
    out['solidity'] = (float(cnt['n']) * (sy * sx)) / out['area_convex'] if hull else float('nan')
    return out


def object_properties(label_image, v, spacing=(1., 1.), mutant=None, hull=True, box=None, pad=None):
    M, P, _, _ = crop(label_image, v, mutant, box, pad)
    return finalise(counts(M, P, mutant), hull_lattice_count(M, mutant) if hull else 1, spacing, mutant)


def shape_table(labels, properties=('label', 'perimeter'), spacing=None, mutant=None):
    """Label image [H, W] or [H, W, C] -> (OrderedDict column -> array over all channels, channel of every row)."""
    labels = np.asarray(labels)
    if labels.ndim == 2:
        labels = labels[..., None]
    spacing = (1., 1.) if spacing is None else (spacing, spacing) if np.isscalar(spacing) else tuple(spacing)
    canon = [ALIASES.get(p, p) for p in properties]
    for p in canon:
        if p not in SUPPORTED:
            raise NotImplementedError(p)
    if spacing[0] != spacing[1] and ('perimeter' in canon or 'perimeter_crofton' in canon):
        raise NotImplementedError('isotropic spacings only')
    need_hull = 'area_convex' in canon or 'solidity' in canon
    rows, channel = [], []
    for z in range(labels.shape[2]):
        a = labels[..., z]
        boxes, pad = bounding_boxes(a), np.pad(a.astype(np.int64), 3)
        for v in sorted(boxes):
            row = object_properties(a, v, spacing, mutant, need_hull, boxes[v], pad)
            row['label'] = v
            rows.append(row)
            channel.append(z)
    cols = OrderedDict()
    for asked, p in zip(properties, canon):
        cols[asked] = np.array([r[p] for r in rows], dtype=np.int64 if p in INTEGER else np.float64).reshape(-1)
    return cols, np.array(channel, np.int64)
