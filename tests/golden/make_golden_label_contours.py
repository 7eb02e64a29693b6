"""Golden-vector generator of the label-image contours (build container only: needs the reference checkout that
``oracle/ref_shim.py`` points to, which never travels).

Imports the read-only Python reference through ``oracle/ref_shim.py`` and runs its own ``labels2contours`` /
``labels2contour_list`` (celldetection/data/cpn.py:93-144) and ``resample_contours`` (celldetection/data/misc.py:371-405) on small
cases; writes ``label_contours.npz`` next to this file: per case the inputs, the keywords and the reference's result.  Arrays only.

What this pins and what it does not.  ``resample_contours`` is pure numpy in the reference: fully pinned.  ``labels2contours``
calls ``skimage.measure.regionprops`` and ``cv2.findContours``; both are absent here, so stand-ins are put onto the stub modules at
run time: ``regionprops`` giving ``label``, ``image`` and ``bbox`` (ascending labels > 0, the boolean crop of the bounding box) and,
for ``cv2.findContours``, the tracer of ``tests/label_contours_oracle.py``.  The border following is therefore third-party,
restated and UNPINNED, as the polygon fill and the dilation are elsewhere; what the fixture pins is the reference's wrapper: the
channel loop, the crop offsets, the order of the dictionary, the doubling of one-point contours, the overwrite across channels
and the handling of fragmented objects.

Every mutant of ``tests/label_contours_oracle.py`` has to differ from the reference's result on at least one case (asserted below).

Run:  python tests/golden/make_golden_label_contours.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')

import ref_shim  # noqa: E402

ref_shim.import_reference()
import cv2  # noqa: E402  (the stub module of ref_shim)
import celldetection.data.cpn as ref_cpn  # noqa: E402
import celldetection.data.misc as ref_misc  # noqa: E402
import label_contours_oracle as oracle  # noqa: E402
from test_instance_eval import disc_labels  # noqa: E402


class Region:
    def __init__(self, label, image, bbox):
        self.label, self.image, self.bbox = label, image, bbox


def regionprops(label_image):
    """skimage.measure.regionprops as far as the reference touches it: one region per value > 0, ascending, with the bounding
    box (min of every axis, then max + 1 of every axis) and the boolean crop of that box."""
    a = np.asarray(label_image)
    out = []
    for v in np.unique(a[a > 0]).tolist():
        idx = np.nonzero(a == v)
        lo, hi = [int(i.min()) for i in idx], [int(i.max()) + 1 for i in idx]
        out.append(Region(v, a[tuple(slice(l, h) for l, h in zip(lo, hi))] == v, tuple(lo) + tuple(hi)))
    return out


def cv2_findContours(image, mode=None, method=None, offset=(0, 0)):
    image = np.asarray(image)
    assert image.dtype == np.uint8
    return tuple(oracle.find_contours(image.reshape(image.shape[:2]), offset)), None


cv2.findContours = cv2_findContours
ref_cpn.regionprops = regionprops


def put(img, value, pixels, c=0):
    for x, y in pixels:
        img[y, x, c] = value
    return img


def rect(x0, y0, x1, y1):
    return [(x, y) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1)]


def label_cases():
    """name -> (labels int32 [H, W, C], keywords)."""
    z = lambda h, w, c=1: np.zeros((h, w, c), np.int32)
    out = {
        'anchor_square': (put(z(5, 6), 1, rect(2, 1, 3, 2)), {}),
        'anchor_row': (put(z(3, 5), 1, rect(1, 1, 3, 1)), {}),
        'anchor_plus': (put(z(3, 3), 1, [(1, 0), (0, 1), (2, 1), (1, 2)]), {}),
        'anchor_single': (put(z(3, 4), 7, [(2, 1)]), {}),
    }
    b = z(12, 14)
    put(b, 1, [(0, 0), (1, 0), (0, 1)]); put(b, 2, rect(12, 0, 13, 1)); put(b, 3, [(0, 11), (1, 11), (1, 10)])
    put(b, 4, [(13, 11)]); put(b, 5, rect(5, 0, 8, 1)); put(b, 6, rect(12, 4, 13, 7)); put(b, 7, rect(4, 10, 9, 11) + [(6, 9)])
    put(b, 8, rect(0, 4, 0, 8) + [(1, 6)]); put(b, 9, rect(4, 4, 8, 7)); put(b, 0, [(6, 5), (6, 6)])  # a hole
    put(b, -3, [(10, 3)])  # negative: ignored
    out['borders'] = (b, {})
    t = z(10, 12, 2)
    put(t, 3, rect(1, 1, 3, 3)); put(t, 3, rect(6, 5, 10, 8), 1)  # both intact: the higher channel is returned
    put(t, 5, rect(6, 1, 8, 2)); put(t, 5, [(1, 6), (3, 6)], 1)   # intact in 0, fragmented in 1: channel 0 is returned
    put(t, 2, rect(1, 8, 2, 8), 1); put(t, 9, rect(10, 0, 11, 0))
    out['two_channels_skip'] = (t, dict(raise_fragmented=False))
    out['two_channels_flag'] = (t.copy(), dict(flag_fragmented_inplace=True, constant=-7))
    out['two_channels_raise'] = (t.copy(), {})
    f = z(9, 11)
    put(f, 4, rect(1, 1, 2, 2) + rect(5, 1, 6, 2)); put(f, 6, rect(1, 5, 4, 7))  # 4: two components
    put(f, 8, rect(6, 4, 10, 8)); put(f, 2, [(8, 6)])  # a ring of 8 with an island of 2
    out['fragmented_flag'] = (f, dict(flag_fragmented_inplace=True))
    out['fragmented_skip'] = (f.copy(), dict(flag_fragmented_inplace=False, raise_fragmented=False))
    out['fragmented_raise'] = (f.copy(), {})
    for c, (h, w, n, seed) in {1: (40, 52, 12, 3), 3: (44, 48, 30, 5), 4: (36, 40, 40, 8)}.items():
        out[f'discs_c{c}'] = (disc_labels(h, w, n, c, seed), {})
    r = z(23, 23)
    r[oracle.ragged_object(np.random.default_rng(21), 23, 23, 160), 0] = 11
    out['ragged'] = (r, {})
    return out


def run_labels(labels, kw):
    """The reference on a copy -> (ids, offsets, points, labels afterwards), or None when it raises ValueError."""
    a = labels.copy()
    try:
        d = ref_cpn.labels2contours(a, **kw)
    except ValueError as e:
        assert 'multiple connected components' in str(e)
        return None
    lst = ref_cpn.labels2contour_list(labels.copy(), **kw)
    assert len(lst) == len(d) and all(np.array_equal(x, y[:, 0]) for x, y in zip(lst, d.values()))
    ids = np.asarray(list(d), np.int32)
    pts = [np.asarray(v, np.int32).reshape(-1, 2) for v in d.values()]
    offsets = np.cumsum([0] + [len(p) for p in pts]).astype(np.int64)
    return ids, offsets, np.concatenate(pts) if pts else np.zeros((0, 2), np.int32), a


def resample_cases(traced):
    """name -> (contours: a list of [n, 2] arrays or an array [..., n, 2], num, close, epsilon)."""
    rng = np.random.default_rng(17)
    out = {}
    c = max(traced, key=len)
    n = len(c)
    for tag, num in (('below', n // 2), ('at', n), ('above', 2 * n + 3)):
        out[f'traced_{tag}'] = ([c], num, True, 1e-6)
    out['traced_list'] = (list(traced), 32, True, 1e-6)
    out['traced_open'] = (list(traced[:5]), 9, False, 1e-6)
    out['doubled_point'] = ([np.array([[4, 2], [4, 2]], np.int32)], 4, True, 1e-6)
    for close in (True, False):
        f = rng.uniform(-5, 40, (12, 2))
        for tag, num in (('below', 5), ('at', 12), ('above', 29)):
            out[f'float_{"closed" if close else "open"}_{tag}'] = ([f], num, close, 1e-6)
    out['float_epsilon'] = ([rng.uniform(0, 9, (7, 2))], 10, True, .25)
    out['batch'] = (rng.uniform(0, 30, (2, 3, 9, 2)), 7, True, 1e-6)
    out['one_sample'] = ([rng.uniform(0, 9, (5, 2))], 1, True, 1e-6)
    return out


def tie_case():
    """A contour on which samples fall exactly onto points (t_j == cumsum[i]) and ``<`` for ``<=`` changes the result: equal steps,
    num a divisor of the segment count.  Searched, since it depends on how the running sum rounds."""
    for w in range(2, 12):
        for h in range(2, 12):
            c = oracle.labels2contour_list(np.ones((h, w), np.int32))[0]
            for num in (len(c), len(c) // 2, 2 * len(c)):
                for eps in (1e-6, 1e-3, .1):
                    ref = ref_misc.resample_contours(c, num=num, close=True, epsilon=eps)
                    if not np.array_equal(oracle.resample_contour(c, num, True, eps, mutant='search_lt'), ref):
                        return [c], num, True, eps
    raise AssertionError('no tie case found')


def main():
    out = {}
    seen = {m: 0 for m in oracle.MUTANTS}
    cases = label_cases()
    out['label_cases'] = np.asarray(list(cases))
    traced = []
    for name, (labels, kw) in cases.items():
        ref = run_labels(labels, kw)
        out[f'{name}.labels'] = labels
        out[f'{name}.flag'] = np.asarray(kw.get('flag_fragmented_inplace', False))
        out[f'{name}.raise'] = np.asarray(kw.get('raise_fragmented', True))
        out[f'{name}.constant'] = np.asarray(kw.get('constant', -1), np.int64)
        out[f'{name}.raises'] = np.asarray(ref is None)
        mine = None
        try:
            a = labels.copy()
            mine = oracle.labels2contours_packed(a, **kw) + (a,)
        except ValueError:
            pass
        assert (ref is None) == (mine is None), name
        if ref is not None:
            assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(mine, ref)), name
            out[f'{name}.ids'], out[f'{name}.offsets'], out[f'{name}.points'], out[f'{name}.labels_after'] = ref
            if name == 'discs_c3':
                traced = [ref[2][a:b] for a, b in zip(ref[1][:-1], ref[1][1:])]
        for m in oracle.CONTOUR_MUTANTS:
            try:
                a = labels.copy()
                got = oracle.labels2contours_packed(a, mutant=m, **kw) + (a,)
            except ValueError:
                got = None
            same = (got is None) == (ref is None) and (ref is None or all(np.array_equal(x, y) for x, y in zip(got, ref)))
            seen[m] += not same
        print(f'{name}: {labels.shape}, {"raises" if ref is None else f"{len(ref[0])} contours, {len(ref[2])} points"}')
    assert out['two_channels_raise.raises'] and out['fragmented_raise.raises']
    assert (out['fragmented_flag.labels_after'] != out['fragmented_flag.labels']).any()
    assert len(traced) >= 15 and len({len(c) for c in traced}) > 5
    cases = resample_cases(traced)
    cases['ties'] = tie_case()
    out['resample_cases'] = np.asarray(list(cases))
    for name, (contours, num, close, eps) in cases.items():
        given = [c.copy() for c in contours] if isinstance(contours, list) else contours.copy()
        ref = ref_misc.resample_contours(given, num=num, close=close, epsilon=eps)
        mine = oracle.resample_contours(contours, num, close, eps)
        ref_a, mine_a = np.asarray(ref, np.float64), np.asarray(mine, np.float64)
        assert ref_a.shape == mine_a.shape and np.array_equal(ref_a, mine_a), (name, np.abs(ref_a - mine_a).max())
        for m in oracle.RESAMPLE_MUTANTS:
            got = np.asarray(oracle.resample_contours(contours, num, close, eps, mutant=m), np.float64)
            seen[m] += not np.array_equal(got, ref_a, equal_nan=True)
        is_list = isinstance(contours, list)
        flat = contours if is_list else list(contours.reshape((-1,) + contours.shape[-2:]))
        out[f'{name}.points'] = np.concatenate(flat)
        out[f'{name}.lengths'] = np.asarray([len(c) for c in flat], np.int64)
        out[f'{name}.lead'] = np.asarray([-1] if is_list else contours.shape[:-2], np.int64)
        out[f'{name}.num'], out[f'{name}.close'], out[f'{name}.epsilon'] = np.asarray(num, np.int64), np.asarray(close), np.asarray(eps)
        out[f'{name}.result'] = ref_a.reshape(-1, num, 2)
        print(f'{name}: {len(flat)} contours of {sorted({len(c) for c in flat})} points, num {num}, close {close}, epsilon {eps}')
    print('cases that differ from the reference per mutant:', seen)
    assert all(seen.values()), seen
    path = os.path.join(HERE, 'label_contours.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
