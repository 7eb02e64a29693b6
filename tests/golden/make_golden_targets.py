"""Golden-vector generator of the CPN training targets (build container only: needs the reference checkout that
``oracle/ref_shim.py`` points to, which never travels).

Imports the read-only Python reference through ``oracle/ref_shim.py`` and runs its own ``labels2distances``,
``mask_labels_by_distance_`` (celldetection/data/cpn.py:424-497), ``filter_instances_`` (celldetection/data/segmentation.py:67-103)
and ``CPNTargetGenerator`` (data/cpn.py:500-644) on small label images; writes ``targets.npz`` next to this file.  Arrays only.

What this pins and what it does not.  The reference calls ``cv2.distanceTransform``, ``skimage.measure.regionprops`` and
``cv2.findContours``; all are absent here, so stand-ins are put onto the stub modules at run time.  ``cv2.distanceTransform`` is
the two-pass 3 x 3 algorithm of OpenCV's published source, pixel by pixel (``targets_oracle.chamfer_literal``); ``regionprops``
follows skimage's documentation (``label``, ``bbox``, ``image``, ``coords`` of every value > 0, ascending, on arrays of any rank);
``cv2.findContours`` is the tracer of ``tests/label_contours_oracle.py``.  Third-party arithmetic, restated and UNPINNED.  What
the fixture pins is the reference's own code around them: owner and overlap rule, padding, protected size, the order of
normalisation and clipping, the masking, the filter and the order of operations in ``CPNTargetGenerator.feed``.

The two disc images must tell wrong rules apart: every distance and mask mutant of ``tests/targets_oracle.py`` has to differ
from the reference's result on both; the seeds are advanced until they do (asserted below).  The filter mutant (counting per
channel) cannot differ on an image whose labels each live in one channel; it is asserted on the two-channel filter case.

Run:  python tests/golden/make_golden_targets.py
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
import celldetection.data.segmentation as ref_seg  # noqa: E402
import label_contours_oracle  # noqa: E402
import targets_oracle as oracle  # noqa: E402
from test_instance_eval import disc_labels  # noqa: E402  (the synthetic images are the tests' own, not the reference's)


class Region:
    def __init__(self, label, image, bbox, coords):
        self.label, self.image, self.bbox, self.coords = label, image, bbox, coords


def regionprops(label_image):
    """skimage.measure.regionprops as far as the reference touches it: one region per value > 0, ascending, with the bounding
    box (min of every axis, then max + 1 of every axis), the boolean crop of that box and the coordinates of its elements."""
    a = np.asarray(label_image)
    out = []
    for v in np.unique(a[a > 0]).tolist():
        idx = np.nonzero(a == v)
        lo, hi = [int(i.min()) for i in idx], [int(i.max()) + 1 for i in idx]
        out.append(Region(v, a[tuple(slice(l, h) for l, h in zip(lo, hi))] == v, tuple(lo) + tuple(hi), np.stack(idx, 1)))
    return out


def cv2_distanceTransform(src, distanceType, maskSize):
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2 and maskSize == 3
    return oracle.to_float(oracle.chamfer_literal(src, distanceType))


def cv2_findContours(image, mode=None, method=None, offset=(0, 0)):
    image = np.asarray(image)
    assert image.dtype == np.uint8
    return tuple(label_contours_oracle.find_contours(image.reshape(image.shape[:2]), offset)), None


cv2.distanceTransform = cv2_distanceTransform
cv2.findContours = cv2_findContours
cv2.DIST_L1, cv2.DIST_L2, cv2.DIST_C = 1, 2, 3
ref_cpn.regionprops = regionprops

BG, FG = .5, .75  # the thresholds of CPNTargetGenerator's defaults


def disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[:h, :w]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def anchors():
    """name -> labels int32 [H, W, C]."""
    z = lambda h, w, c=1: np.zeros((h, w, c), np.int32)
    out = {}
    a = z(5, 5); a[2, 2] = 1
    out['one_pixel'] = a
    a = z(10, 11); a[2:8, 3:9] = 1  # 36 pixels: not normalised
    out['square_6x6'] = a
    a = z(10, 11); a[1:8, 3:9] = 1  # 42 pixels: normalised
    out['rect_7x6'] = a
    a = z(12, 13); a[:5, :6] = 1; a[4:11, 9:] = 2; a[10:, 2:7] = 3  # corner, right border, bottom border
    out['border_corner'] = a
    a = z(24, 30, 2); a[disc(24, 30, 11, 10, 8), 0] = 1; a[disc(24, 30, 12, 19, 7), 1] = 2
    out['two_discs_overlap'] = a
    a = z(16, 20, 2); a[2:9, 2:9, 0] = 4; a[8:15, 11:19, 1] = 4; a[5:8, 7:12, 1] = 4; a[10:14, 2:6, 0] = 2  # 4 twice at (5:8, 7:9)
    out['one_label_two_channels'] = a
    a = z(14, 18); a[1:8, 1:8] = 3; a[6:13, 10:17] = 3; a[9:13, 2:6] = 5
    out['two_pieces'] = a
    a = z(12, 14, 2); a[2:9, 2:9, 0] = 1; a[4:7, 4:7, 1] = -1; a[2:9, 9:12, 0] = -1; a[9:11, 3:8, 1] = 2; a[0, :, 1] = -2
    out['negatives'] = a
    return out


def disc_images():
    """The two disc images, re-seeded until every distance and mask mutant of the oracle differs from the reference's result."""
    out = {}
    for name, (h, w, n, c, seed, rmax) in (('discs_c3', (96, 130, 70, 3, 0, 11.)), ('discs_c2', (112, 144, 60, 2, 1, 14.))):
        while True:
            a = disc_labels(h, w, n, c, seed=seed, rmax=rmax)
            diff = {}
            for inst, mutants in ((True, oracle.DISTANCE_MUTANTS), (False, oracle.FG_MUTANTS)):
                ref, lab = ref_cpn.labels2distances(a, distance_type=2, per_instance=inst)
                assert np.array_equal(oracle.labels2distances(a, per_instance=inst)[0], ref)
                for m in mutants:
                    diff[m, inst] = int((oracle.labels2distances(a, per_instance=inst, mutant=m)[0] != ref).sum())
                if inst:
                    masked = lab.copy()
                    ref_cpn.mask_labels_by_distance_(masked, ref, BG, FG)
                    for m in oracle.MASK_MUTANTS:
                        diff[m, inst] = int((oracle.mask_labels_by_distance(lab, ref, BG, FG, mutant=m)[0] != masked).sum())
            if all(diff.values()):
                break
            seed += 1
            print(f'{name}: a mutant agrees, re-seeding -> {seed}')
        print(f'{name}: seed {seed}, pixels that differ from the reference per (mutant, per_instance): {diff}')
        out[name] = a
    return out


def filter_cases():
    """name -> (labels, keywords)."""
    out = {}
    d = disc_labels(64, 80, 30, 2, seed=5, rmax=9.)
    full = oracle.filter_instances(d, partials=False, min_area=None, continuous=True)  # gap-free: nothing moves below
    sizes = np.bincount(full[full > 0])
    mid = int(np.sort(sizes[1:])[len(sizes) // 2])
    out['gap_free_defaults'] = (full, dict(partials=False))
    for b in (0, 1, 3):
        out[f'partials_border{b}'] = (full, dict(partials=True, partials_border=b, continuous=False))
    out['min_area_at'] = (full, dict(partials=False, min_area=mid, continuous=False))
    out['min_area_above'] = (full, dict(partials=False, min_area=mid + 1, continuous=False))
    out['max_area_at'] = (full, dict(partials=False, min_area=None, max_area=mid, continuous=False))
    out['max_area_below'] = (full, dict(partials=False, min_area=None, max_area=mid - 1, continuous=False))
    out['constant_7'] = (full, dict(partials=True, partials_border=2, constant=-7, continuous=False))
    out['gaps'] = (d * 3, dict(partials=True, partials_border=1, min_area=30))
    out['gaps_flat'] = (d.max(2) * 2, dict(partials=False, min_area=None))
    a = np.zeros((8, 12, 2), np.int32)  # label 1: 3 + 3 elements in two channels, label 2: 5 in one, label 3: 7
    a[1, 1:4, 0], a[3, 1:4, 1], a[5, 1:6, 0], a[6, 3:10, 1] = 1, 1, 2, 3
    out['two_channel_counts'] = (a, dict(partials=False, min_area=6, continuous=False))
    b = a.copy()
    b[0, 8:, 0] = -1  # negatives: the reference drops the first unique value, which is -1 here; 0 has enough elements
    out['negatives'] = (b, dict(partials=False, min_area=4, continuous=False))
    return out


def generator_cases(discs, anch):
    """name -> (labels fed, constructor keywords, feed keywords, np.random seed, exact)."""
    gap_free = lambda a: oracle.filter_instances(a, partials=False, min_area=None, continuous=True)
    big = lambda a: oracle.filter_instances(a, partials=True, partials_border=1, min_area=12, continuous=True)
    return {
        'gen_discs_c3': (big(discs['discs_c3']), dict(samples=16, order=5), dict(), 3, True),
        'gen_discs_c2_linear': (big(discs['discs_c2']), dict(samples=12, order=3, random_sampling=False, min_fg_dist=.8,
                                                             max_bg_dist=.4), dict(min_area=20), 4, True),
        'gen_two_pieces_flag': (gap_free(anch['two_pieces']), dict(samples=8, order=4), dict(), 5, True),
        'gen_two_pieces_keep': (gap_free(anch['two_pieces']), dict(samples=8, order=4, flag_fragmented=False), dict(), 6, True),
        'gen_partials_flat': (big(discs['discs_c2']).max(2), dict(samples=8, order=2, remove_partials=True), dict(border=2), 7, True),
        'gen_gaps': (discs['discs_c3'] * 2, dict(samples=8, order=3), dict(min_area=10), 8, False),
    }


def main():
    out = {}
    anch, discs = anchors(), disc_images()
    names = []
    for name, a in dict(anch, **discs).items():
        for inst in (True, False):
            for dt in ((1, 2, 3) if name in discs else (2,)):
                for prot in ((36, 0) if name == 'square_6x6' and inst else (36,)):
                    key = f'{name}.{"inst" if inst else "fg"}.d{dt}.p{prot}'
                    kw = dict(protected_size=prot) if inst else {}
                    ref, lab = ref_cpn.labels2distances(a.copy(), distance_type=dt, per_instance=inst, **kw)
                    assert ref.dtype == np.float32 and ref.shape == a.shape[:2] and lab.shape == a.shape
                    masked = lab.copy()
                    ref_cpn.mask_labels_by_distance_(masked, ref, BG, FG)
                    names.append(key)
                    out[f'{key}.labels'] = a
                    out[f'{key}.params'] = np.asarray([dt, int(inst), prot], np.int64)
                    out[f'{key}.distances'], out[f'{key}.labels_out'] = ref, lab
                    out[f'{key}.masked'], out[f'{key}.reduced'] = masked, masked.max(2)
                    want, _ = oracle.labels2distances(a, dt, per_instance=inst, protected_size=prot)
                    print(f'{key}: {a.shape}, owner pixels {int((ref > 0).sum())}, oracle differs at {int((want != ref).sum())}')
    out['distance_cases'] = np.asarray(names)

    names = []
    for name, (a, kw) in filter_cases().items():
        got = a.copy()
        ref_seg.filter_instances_(got, **kw)
        names.append(name)
        out[f'filter.{name}.labels'], out[f'filter.{name}.result'] = a, got
        full = dict(partials=True, partials_border=1, min_area=4, max_area=None, constant=-1, continuous=True)
        full.update(kw)
        out[f'filter.{name}.params'] = np.asarray([int(full['partials']), full['partials_border'],
                                                  -1 if full['min_area'] is None else full['min_area'],
                                                  -1 if full['max_area'] is None else full['max_area'], full['constant'],
                                                  int(full['continuous'])], np.int64)
        want = oracle.filter_instances(a, **kw)
        print(f'filter.{name}: {a.shape}, labels {len(np.unique(a[a > 0]))} -> {len(np.unique(got[got > 0]))}, oracle equal '
              f'{np.array_equal(want, got)}, same partition {oracle.same_partition(want, got)}')
    a, kw = filter_cases()['two_channel_counts']
    assert not np.array_equal(oracle.filter_instances(a, mutant='count_per_channel', **kw), out['filter.two_channel_counts.result'])
    out['filter_cases'] = np.asarray(names)

    names = []
    for name, (a, ckw, fkw, seed, exact) in generator_cases(discs, anch).items():
        gen = ref_cpn.CPNTargetGenerator(**ckw)
        fed = a.copy()
        gen.feed(fed, distance_type=2, **fkw)
        np.random.seed(seed)
        names.append(name)
        p = f'gen.{name}'
        out[f'{p}.input'] = a
        full = dict(random_sampling=True, remove_partials=False, min_fg_dist=.75, max_bg_dist=.5, flag_fragmented=True,
                    flag_fragmented_constant=-1)
        full.update(ckw)
        feed = dict(border=1, min_area=1, max_area=None)
        feed.update(fkw)
        out[f'{p}.ints'] = np.asarray([full['samples'], full['order'], int(full['random_sampling']), int(full['remove_partials']),
                                       int(full['flag_fragmented']), full['flag_fragmented_constant'], feed['border'],
                                       feed['min_area'], -1 if feed['max_area'] is None else feed['max_area'], seed, int(exact)],
                                      np.int64)
        out[f'{p}.floats'] = np.asarray([full['min_fg_dist'], full['max_bg_dist']], np.float64)
        out[f'{p}.reduced_labels'] = gen.reduced_labels
        out[f'{p}.labels'], out[f'{p}.distances'], out[f'{p}.labels_red'] = gen.labels, gen.distances, gen.labels_red
        out[f'{p}.sampling'] = gen.sampling
        con = gen.contours
        out[f'{p}.contour_ids'] = np.asarray(list(con), np.int64)
        out[f'{p}.contour_offsets'] = np.cumsum([0] + [len(c) for c in con.values()]).astype(np.int64)
        out[f'{p}.contour_points'] = np.concatenate([np.asarray(c).reshape(-1, 2) for c in con.values()]).astype(np.int32) \
            if len(con) else np.zeros((0, 2), np.int32)
        out[f'{p}.fourier'], out[f'{p}.locations'] = gen.fourier, gen.locations
        out[f'{p}.sampled_contours'] = np.asarray(gen.sampled_contours)
        out[f'{p}.resampled_contours'] = np.asarray(gen.resampled_contours)
        out[f'{p}.sampled_sizes'] = np.asarray(gen.sampled_sizes)
        print(f'{p}: {a.shape}, contours {len(con)}, fourier {gen.fourier.shape} {gen.fourier.dtype}, sampled '
              f'{out[f"{p}.sampled_contours"].shape} {out[f"{p}.sampled_contours"].dtype}')
    out['generator_cases'] = np.asarray(names)

    path = os.path.join(HERE, 'targets.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
