"""numpy statement of the region property table (celldetection_amd.region_properties / labels2property_table).

The reference's ``labels2property_table`` (celldetection/data/misc.py:320-347) hands every channel to
``skimage.measure.regionprops_table``.  scikit-image is absent from the build image, so the property arithmetic below is written
from its documented behaviour: third-party, restated and unpinned.  It is this package's contract (include/cpn_hip.h, section
"Region property tables"): accumulators from a plain per-label ``np.nonzero``, the shift to the bounding box in Python
integers, then fp64 in exactly the written order of operations.

``regionprops_table`` has the signature of scikit-image's function for one 2-D label image; ``property_table`` loops over the
channels as the reference does.  ``mutant`` selects a deliberately wrong rule (``MUTANTS``); the fixture and the tests must
tell each from the right one.
"""
import math
from collections import OrderedDict

import numpy as np

MUTANTS = ('swap_ac', 'sign_b', 'closed_bbox', 'spacing_once', 'centroid_no_spacing', 'sort_across_channels', 'count_nonpositive',
           'sum32')
SUPPORTED = ('label', 'bbox', 'num_pixels', 'area', 'area_bbox', 'extent', 'equivalent_diameter_area', 'centroid',
             'centroid_local', 'inertia_tensor', 'inertia_tensor_eigvals', 'axis_major_length', 'axis_minor_length',
             'eccentricity', 'orientation', 'intensity_mean', 'intensity_min', 'intensity_max')
ALIASES = dict(bbox_area='area_bbox', equivalent_diameter='equivalent_diameter_area', major_axis_length='axis_major_length',
               minor_axis_length='axis_minor_length', local_centroid='centroid_local', mean_intensity='intensity_mean',
               min_intensity='intensity_min', max_intensity='intensity_max')
EXACT = ('label', 'bbox', 'num_pixels', 'area', 'area_bbox', 'extent', 'centroid', 'centroid_local', 'inertia_tensor',
         'intensity_mean', 'intensity_min', 'intensity_max')  # integers, or + - * / only
SQRT = ('equivalent_diameter_area', 'inertia_tensor_eigvals', 'axis_major_length', 'axis_minor_length', 'eccentricity')
ALL_GEOMETRY = SUPPORTED[:15]


def accumulate(label_image, intensity_image=None, mutant=None):
    """2-D label image -> list of dicts (label ascending): n, sums (sr, sc, srr, src, scc as Python ints over global
    coordinates), bbox (r0, c0, r1, c1 half-open), per intensity channel isum / imin / imax."""
    label_image = np.asarray(label_image)
    assert label_image.ndim == 2
    img = None
    if intensity_image is not None:
        img = np.asarray(intensity_image)
        img = img[:, :, None] if img.ndim == 2 else img
    values = np.unique(label_image)
    rows = []
    for v in values.tolist():
        if v <= 0 and not (mutant == 'count_nonpositive' and v == 0):
            continue
        r, c = np.nonzero(label_image == v)
        r, c = r.astype(np.int64), c.astype(np.int64)  # exact: every sum stays below 2 ** 63 for images of the supported sizes
        row = dict(label=v, n=int(r.size), sr=int(r.sum()), sc=int(c.sum()), srr=int((r * r).sum()), src=int((r * c).sum()),
                   scc=int((c * c).sum()), r0=int(r.min()), c0=int(c.min()), r1=int(r.max()) + 1, c1=int(c.max()) + 1)
        if mutant == 'closed_bbox':
            row['r1'], row['c1'] = row['r1'] - 1, row['c1'] - 1
        if mutant == 'sum32':
            row['srr'] &= 0xffffffff
        if img is not None:
            px = img[r, c].reshape(r.size, -1)
            row['isum'] = [int(px[:, k].astype(np.int64).sum()) for k in range(img.shape[2])]
            row['imin'] = [px[:, k].min() for k in range(img.shape[2])]
            row['imax'] = [px[:, k].max() for k in range(img.shape[2])]
        rows.append(row)
    return rows


def finalise(row, spacing=(1., 1.), mutant=None):
    """One accumulator row -> dict property -> scalar / tuple / 2 x 2 nested tuple, fp64 in the contract's order."""
    sy, sx = (float(s) for s in spacing)
    n, r0, c0, r1, c1 = row['n'], row['r0'], row['c0'], row['r1'], row['c1']
    # shift to the corner of the bounding box, Python integers
    sr, sc = row['sr'] - n * r0, row['sc'] - n * c0
    srr = row['srr'] - 2 * r0 * row['sr'] + n * r0 * r0
    src = row['src'] - r0 * row['sc'] - c0 * row['sr'] + n * r0 * c0
    scc = row['scc'] - 2 * c0 * row['sc'] + n * c0 * c0
    nd, fsr, fsc = float(n), float(sr), float(sc)
    out = OrderedDict()
    out['label'] = row['label']
    out['bbox'] = (r0, c0, r1, c1)
    out['num_pixels'] = n
    area = nd * (sy * sx)
    area_bbox = float((r1 - r0) * (c1 - c0)) * (sy * sx)
    out['area'], out['area_bbox'] = area, area_bbox
    out['extent'] = area / area_bbox if area_bbox != 0 else math.inf
    out['equivalent_diameter_area'] = math.sqrt(4 * area / math.pi)
    out['centroid'] = ((float(row['sr']) / nd) * sy, (float(row['sc']) / nd) * sx)
    out['centroid_local'] = ((fsr / nd) * sy, (fsc / nd) * sx)
    if mutant == 'centroid_no_spacing':
        out['centroid'], out['centroid_local'] = (float(row['sr']) / nd, float(row['sc']) / nd), (fsr / nd, fsc / nd)
    qy, qx, qyx = (sy, sx, math.sqrt(sy * sx)) if mutant == 'spacing_once' else (sy * sy, sx * sx, sy * sx)
    mu20 = (float(srr) - fsr * fsr / nd) * qy
    mu02 = (float(scc) - fsc * fsc / nd) * qx
    mu11 = (float(src) - fsr * fsc / nd) * qyx
    a, b, c = mu02 / nd, -mu11 / nd, mu20 / nd
    if mutant == 'swap_ac':
        a, c = c, a
    if mutant == 'sign_b':
        b = -b
    out['inertia_tensor'] = ((a, b), (b, c))
    m, d = (a + c) / 2, (a - c) / 2
    s = math.sqrt(d * d + b * b)
    l1, l2 = m + s, max(m - s, 0.)
    out['inertia_tensor_eigvals'] = (l1, l2)
    out['axis_major_length'] = 4 * math.sqrt(l1)
    out['axis_minor_length'] = 4 * math.sqrt(l2)
    out['eccentricity'] = 0. if l1 == 0 else math.sqrt(1 - l2 / l1)
    out['orientation'] = (math.pi / 4 if b < 0 else -math.pi / 4) if a - c == 0 else 0.5 * math.atan2(-2 * b, c - a)
    if 'isum' in row:
        K = len(row['isum'])
        one = K == 1  # columns carry a channel suffix only with more than one intensity channel
        mean = tuple(float(s) / nd for s in row['isum'])
        out['intensity_mean'] = mean[0] if one else mean
        out['intensity_min'] = row['imin'][0] if one else tuple(row['imin'])
        out['intensity_max'] = row['imax'][0] if one else tuple(row['imax'])
    return out


def _columns(name, value, sep):
    if isinstance(value, tuple):
        for i, v in enumerate(value):
            yield from _columns(f'{name}{sep}{i}', v, sep)
    else:
        yield name, value


def regionprops_table(label_image, intensity_image=None, properties=('label', 'bbox'), *, cache=True, separator='-',
                      extra_properties=None, spacing=None, mutant=None):
    """``skimage.measure.regionprops_table`` for one 2-D label image and the supported properties: dict column -> array."""
    assert extra_properties is None
    label_image = np.asarray(label_image)
    if label_image.ndim != 2:
        raise NotImplementedError('restatement: 2-D label images only')
    for p in properties:
        if ALIASES.get(p, p) not in SUPPORTED:
            raise NotImplementedError(p)
    spacing = (1., 1.) if spacing is None else (spacing, spacing) if np.isscalar(spacing) else tuple(spacing)
    img = None if intensity_image is None else np.asarray(intensity_image)
    rows = accumulate(label_image, img, mutant)
    K = 0 if img is None else 1 if img.ndim == 2 else img.shape[2]
    # names and dtypes from a template row, so that a table without rows has its columns
    template = dict(label=1, n=1, sr=0, sc=0, srr=0, src=0, scc=0, r0=0, c0=0, r1=1, c1=1)
    if img is not None:
        z = img.dtype.type(0)
        template.update(isum=[0] * K, imin=[z] * K, imax=[z] * K)
    fin = [finalise(r, spacing, mutant) for r in rows]
    tfin = finalise(template, spacing)
    out = OrderedDict()
    for p in properties:
        canon = ALIASES.get(p, p)
        for j, (name, tv) in enumerate(_columns(p, tfin[canon], separator)):
            if canon in ('intensity_min', 'intensity_max'):
                dt = img.dtype
            else:
                dt = np.int64 if isinstance(tv, (int, np.integer)) else np.float64
            out[name] = np.array([list(_columns(p, f[canon], separator))[j][1] for f in fin], dtype=dt).reshape(-1)
    return out


def property_table(labels, properties=('label', 'bbox'), intensity_image=None, spacing=None, separator='-', iter_channels=True,
                   mutant=None):
    """Label image [H, W] or [H, W, C] -> (OrderedDict column -> array over all channels, channel of every row, index of every
    row as the reference's per-channel concatenation numbers it)."""
    labels = np.asarray(labels)
    if labels.ndim == 2:
        labels = labels[..., None]
    elif not iter_channels:
        raise NotImplementedError('restatement: iter_channels=False on 2-D images only')
    parts = [regionprops_table(labels[..., z], intensity_image, properties, separator=separator, spacing=spacing, mutant=mutant)
             for z in range(labels.shape[2])]
    cols = OrderedDict((k, np.concatenate([p[k] for p in parts])) for k in parts[0])
    counts = [len(next(iter(p.values()))) if p else 0 for p in parts]
    channel = np.concatenate([np.full(n, z, np.int64) for z, n in enumerate(counts)])
    index = np.concatenate([np.arange(n, dtype=np.int64) for n in counts])
    if mutant == 'sort_across_channels' and 'label' in properties:
        order = np.argsort(cols['label'], kind='stable')
        cols = OrderedDict((k, v[order]) for k, v in cols.items())
        channel = channel[order]
    return cols, channel, index


def ulp_distance(a, b):
    """Distance of two fp64 arrays in units in the last place (0 for equal bit patterns, +0 / -0 included)."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    assert a.shape == b.shape and not np.isnan(a).any() and not np.isnan(b).any()

    def ordered(x):  # bit pattern -> integers that are monotonic in the value
        i = x.view(np.int64).astype(object)
        return np.where(i < 0, -(i & 0x7fffffffffffffff), i)
    d = np.abs(ordered(a) - ordered(b))
    return int(d.max()) if d.size else 0
