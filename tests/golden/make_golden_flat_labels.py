"""Golden-vector generator of the flat label images (build container only: needs the reference checkout that
``oracle/ref_shim.py`` points to, which never travels).

Imports the read-only Python reference through ``oracle/ref_shim.py`` and runs its own ``resolve_label_channels``
(celldetection/data/cpn.py:361-399) on small label images; writes ``flat_labels.npz`` next to this file: per case the input
image, ``max_iter``, the kernel (an empty array = the default ``(3, 3)``) and the reference's result.  Arrays only.

The reference calls ``cv2.getStructuringElement`` and ``cv2.dilate``; OpenCV is absent here, so stand-ins written from OpenCV's
documentation are put onto the stub ``cv2`` module at run time (shape 1 = MORPH_CROSS; dilate = maximum over the non-zero
kernel entries anchored at the centre, neighbours outside the image taking no part, which is what the default border value
amounts to).  Third-party arithmetic, restated and unpinned; what the fixture pins is the reference's code around it.

The disc cases must tell wrong rules apart: every mutant of ``tests/flat_labels_oracle.py`` has to differ from the reference's
result on both; the seeds are advanced until they do (asserted below).

Run:  python tests/golden/make_golden_flat_labels.py          (writes the fixture)
      python tests/golden/make_golden_flat_labels.py time     (times the reference's function on larger images)
"""
import os
import sys
import time
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
from celldetection.data.cpn import resolve_label_channels  # noqa: E402
from flat_labels_oracle import MUTANTS, resolve_label_channels as oracle  # noqa: E402
from test_instance_eval import disc_labels  # noqa: E402  (the synthetic images are the tests' own, not the reference's)


def cv2_getStructuringElement(shape, ksize, anchor=(-1, -1)):
    """cv2.getStructuringElement for 3 x 3: 0 = MORPH_RECT, 1 = MORPH_CROSS (centre row and centre column)."""
    if tuple(ksize) != (3, 3) or tuple(anchor) != (-1, -1):
        raise NotImplementedError('stand-in: 3 x 3 kernels with the default anchor only')
    if shape == 0:
        return np.ones((3, 3), np.uint8)
    if shape == 1:
        return np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
    raise NotImplementedError(f'stand-in: shape {shape}')


def cv2_dilate(src, kernel, dst=None, anchor=(-1, -1), iterations=1, borderType=None, borderValue=None):
    """cv2.dilate with its defaults on a 2-D array: dst(y, x) = max of src(y + i - 1, x + j - 1) over the non-zero kernel(i, j)
    that fall inside the image (the default border value is the lowest value of the type: it never wins)."""
    src, kernel = np.asarray(src), np.asarray(kernel)
    if src.ndim != 2 or kernel.shape != (3, 3) or iterations != 1 or tuple(anchor) != (-1, -1) or borderType is not None:
        raise NotImplementedError('stand-in: one iteration of a 3 x 3 kernel with default anchor and border on a 2-D array')
    h, w = src.shape
    pad = np.full((h + 2, w + 2), -np.inf if src.dtype.kind == 'f' else np.iinfo(src.dtype).min, src.dtype)
    pad[1:-1, 1:-1] = src
    out = np.full_like(src, pad[0, 0])
    for i in range(3):
        for j in range(3):
            if kernel[i, j]:
                out = np.maximum(out, pad[i:i + h, j:j + w])
    return out


cv2.getStructuringElement = cv2_getStructuringElement
cv2.dilate = cv2_dilate
cv2.MORPH_RECT, cv2.MORPH_CROSS = 0, 1

DEFAULT = np.zeros((0,), np.uint8)  # stands for kernel=(3, 3)
EIGHT = np.ones((3, 3), np.uint8)


def hand_made():
    """name -> (labels, max_iter, kernel)."""
    out = {}
    a = np.zeros((12, 14, 2), np.int32)  # two identical squares: the overlap is unreachable and vanishes
    a[3:9, 4:10, 0], a[3:9, 4:10, 1] = 1, 2
    out['identical_squares'] = (a, 999, DEFAULT)
    a = np.zeros((6, 7, 2), np.int32)  # no overlap: the plain maximum, negative values included
    a[1:3, 1:3, 0], a[3:5, 4:6, 1] = 5, 6
    a[0, 0], a[5, 6] = (-1, -2), (-1, 3)
    out['no_overlap_negatives'] = (a, 999, DEFAULT)
    b = a.copy()  # the same plus one isolated overlap pixel: negatives become 0, the overlap pixel stays 0
    b[5, 0] = (4, 5)
    out['one_overlap_negatives'] = (b, 999, DEFAULT)
    a = np.zeros((9, 11, 2), np.int32)  # overlaps on the image border and in a corner
    a[0:4, 0:5, 0], a[0:3, 3:9, 1] = 1, 2  # top border, corner object
    a[5:9, 7:11, 0], a[6:9, 8:11, 1] = 3, 4  # bottom right corner
    a[4:9, 0:3, 1], a[6:9, 0:2, 0] = 5, 6  # left border / bottom left corner
    out['border_corner'] = (a, 999, DEFAULT)
    a = np.zeros((5, 9, 2), np.int32)  # one overlap pixel between cores 7 and 9: the larger label wins
    a[2, 1:5, 0], a[2, 4:8, 1] = 7, 9
    out['larger_wins'] = (a, 999, DEFAULT)
    a = np.zeros((5, 9, 2), np.int32)
    a[2, 1:5, 1], a[2, 4:8, 0] = 9, 7
    out['larger_wins_swapped'] = (a, 999, DEFAULT)
    out['one_channel'] = (disc_labels(40, 50, 12, 1, seed=3), 999, DEFAULT)
    return out


def disc_cases():
    """The two disc images, re-seeded until every mutant of the oracle differs from the reference's result."""
    out = {}
    for name, (h, w, n, c, seed, rmax) in (('discs_c3', (160, 200, 120, 3, 0, 11.)), ('discs_c4', (96, 130, 60, 4, 1, 20.))):
        while True:
            a = disc_labels(h, w, n, c, seed=seed, rmax=rmax)
            ref = resolve_label_channels(a)
            diff = {m: int((oracle(a, mutant=m) != ref).sum()) for m in MUTANTS}
            if all(diff.values()) and np.array_equal(oracle(a), ref):
                break
            seed += 1
            print(f'{name}: a mutant agrees, re-seeding -> {seed}')
        print(f'{name}: seed {seed}, pixels that differ from the reference per mutant: {diff}')
        out[name] = (a, 999, DEFAULT)
        for it in (1, 2, 5):
            out[f'{name}_iter{it}'] = (a, it, DEFAULT)
        out[f'{name}_eight'] = (a, 999, EIGHT)
    return out


def main():
    cases = dict(disc_cases(), **hand_made())
    out = dict(cases=np.asarray(list(cases)))
    for name, (a, max_iter, kernel) in cases.items():
        ref = resolve_label_channels(a, max_iter=max_iter, kernel=(3, 3) if kernel.size == 0 else kernel)
        assert ref.dtype == a.dtype and ref.shape == a.shape[:2]
        out[f'{name}.labels'], out[f'{name}.max_iter'], out[f'{name}.kernel'] = a, np.asarray(max_iter, np.int64), kernel
        out[f'{name}.result'] = ref
        over = (a > 0).sum(-1) > 1
        print(f'{name}: {a.shape}, max_iter {max_iter}, overlap pixels {int(over.sum())}, of them 0 in the result '
              f'{int((ref[over] == 0).sum())}, labels {len(np.unique(ref[ref > 0]))}')
    path = os.path.join(HERE, 'flat_labels.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


def time_reference():
    """Wall time of the reference's function (with the numpy stand-in of cv2.dilate) on growing images, one run each."""
    for size, n in ((512, 600), (1024, 2500), (2048, 10000)):
        a = disc_labels(size, size, n, 4, seed=1, rmax=20.)
        t0 = time.perf_counter()
        ref = resolve_label_channels(a)
        dt = time.perf_counter() - t0
        print(f'reference resolve_label_channels {size} x {size} x 4, overlap pixels {int(((a > 0).sum(-1) > 1).sum())}: '
              f'{dt:.2f} s, labels {len(np.unique(ref[ref > 0]))}', flush=True)


if __name__ == '__main__':
    time_reference() if sys.argv[1:] == ['time'] else main()
