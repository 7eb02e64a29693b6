"""Golden-vector generator of component labelling (build container only: needs the reference checkout that
``oracle/ref_shim.py`` points to, which never travels).

Imports the read-only Python reference through ``oracle/ref_shim.py`` and runs its own ``relabel_``, ``stack_labels``,
``unary_masks2labels`` (celldetection/data/segmentation.py:106-167), ``masks2labels`` (celldetection/data/cpn.py:147-176) and
``rgb_to_scalar`` (celldetection/data/misc.py:264-280) on small cases; writes ``components.npz`` next to this file: per case the
inputs, the keywords and the reference's result.  Arrays only.

What this pins and what it does not.  ``unary_masks2labels`` and ``rgb_to_scalar`` are pure numpy in the reference: fully pinned.
``relabel_`` calls ``skimage.morphology.label`` and ``masks2labels`` calls ``cv2.connectedComponents``; both are absent here, so
stand-ins are put onto the stub modules at run time.  They are built on ``scipy.ndimage.label`` -- per distinct value for
skimage's equal-value rule, on ``mask != 0`` for OpenCV -- and number the components by their first raster pixel (asserted below
for every call).  They share no code with ``tests/components_oracle.py`` (a sequential union-find), so each checks the other.
Third-party arithmetic, restated and UNPINNED: in particular OpenCV's 8-way default algorithm may number the components of one
mask in another order.  What the fixture pins is the reference's own code around them: the channel loop, the running ``cur_max``,
the skipping of components with negative pixels, the ascending iteration of ``set(np.unique(...))`` (a channel of more than 1000
components), the stacking and dtype handling of ``stack_labels`` and the ``cnt`` arithmetic of ``masks2labels`` with its two
quirks.

Run:  python tests/golden/make_golden_components.py
"""
import os
import sys
import warnings

import numpy as np
from scipy import ndimage as ndi

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
import celldetection.data.segmentation as ref_seg  # noqa: E402
import components_oracle as oracle  # noqa: E402
from test_instance_eval import disc_labels  # noqa: E402  (the synthetic images are the tests' own, not the reference's)

FULL, CROSS = np.ones((3, 3), int), ndi.generate_binary_structure(2, 1)


def _ranked(parts, shape):
    """parts: list of (mask of the elements, scipy labels of them, n) -> labels 1, 2, ... by first raster pixel."""
    firsts, owner = [], []
    for k, (_, lab, n) in enumerate(parts):
        u, idx = np.unique(lab.reshape(-1), return_index=True)
        keep = u > 0
        assert keep.sum() == n and (np.diff(idx[keep]) > 0).all()  # scipy numbers by first raster pixel
        firsts += idx[keep].tolist()
        owner += [(k, int(v)) for v in u[keep]]
    out = np.zeros(shape, np.int64)
    luts = [np.zeros(n + 1, np.int64) for _, _, n in parts]
    for rank, j in enumerate(np.argsort(np.asarray(firsts, np.int64), kind='stable').tolist()):
        k, v = owner[j]
        luts[k][v] = rank + 1
    for (sel, lab, _), lut in zip(parts, luts):
        out[sel] = lut[lab[sel]]
    return out


def skimage_label(label_image, background=None, return_num=False, connectivity=None):
    """skimage.morphology.label as the reference calls it: background 0, full connectivity, equal values of any sign link."""
    a = np.asarray(label_image)
    assert a.ndim == 2 and background in (None, 0) and connectivity in (None, 2) and not return_num
    parts = []
    for v in np.unique(a[a != 0]).tolist():
        sel = a == v
        lab, n = ndi.label(sel, structure=FULL)
        parts.append((sel, lab, n))
    return _ranked(parts, a.shape)


def cv2_connectedComponents(image, labels=None, connectivity=8, ltype=None):
    """cv2.connectedComponents: (number of labels with the background, int32 labels of the non-zero pixels)."""
    m = np.asarray(image)
    assert m.ndim == 2 and connectivity in (4, 8) and labels is None and ltype is None
    sel = m != 0
    lab, n = ndi.label(sel, structure=FULL if connectivity == 8 else CROSS)
    return n + 1, _ranked([(sel, lab, n)], m.shape).astype(np.int32)


ref_seg.morphology.label = skimage_label
cv2.connectedComponents = cv2_connectedComponents


def relabel_cases():
    """name -> int32 [H, W, C], C = 1 .. 4."""
    z = lambda h, w, c=1: np.zeros((h, w, c), np.int32)
    out = {}
    a = z(7, 9)
    a[0, 5:8] = 9; a[1:4, 0:2] = 9          # one value in two places; the second starts further left, one row down
    a[5, 0] = a[6, 1] = 4; a[5, 3] = 4      # a diagonal-only contact, and a third piece two columns on
    a[2, 4] = 3; a[3, 5] = 3; a[3, 7] = 2   # the lower value 2 comes after the higher ones
    out['one_channel'] = a
    a = z(8, 10, 2)
    a[1:3, 1:4, 0] = 5; a[5:7, 6:9, 0] = 5; a[1:3, 6:9, 1] = 5; a[5:7, 1:4, 1] = 7; a[0, 0, 1] = 5
    a[3:5, 4:6, 0] = -1; a[7, :, 1] = -3; a[0, 9, 0] = -1; a[1, 8, 0] = -1
    out['two_channels_negatives'] = a
    a = z(9, 9, 3)
    a[0:3, 6:9, 0] = 2; a[4:9, 0:3, 0] = 1; a[2, 2, 0] = 2; a[3, 3, 0] = 1  # different values touching, also diagonally
    a[:, :, 1] = 6                                                          # one value over the whole channel
    a[::2, ::2, 2] = 8; a[1::2, 1::2, 2] = 8                                # a checkerboard: one component at 8, 41 at 4
    out['three_channels'] = a
    a = z(6, 12, 4)
    a[1:3, 1:5, 0] = 3; a[1:3, 5:9, 0] = -2; a[1:3, 9:11, 0] = 3; a[4, 2:10, 1] = 1; a[0, 0, 3] = 2 ** 31 - 1; a[5, 11, 3] = 1
    out['four_channels_one_empty'] = a
    a = z(72, 70, 2)
    a[::2, ::2, 0] = 1                      # 36 * 35 = 1260 single pixels of one value: more than 1000 components
    a[10:20, 10:30, 1] = 1; a[40:50, 10:30, 1] = 1
    out['many_components'] = a
    d = disc_labels(48, 64, 40, 3, seed=11, rmax=8.)
    d[20:24] = 0                            # a cut through the discs: objects in two pieces
    d[d == 7] = -1
    out['discs_cut'] = (d % 9).astype(np.int32) * (d > 0) + d * (d < 0)  # values recur in many places
    return out


def mask_cases():
    """name -> (uint8 [N, H, W], keywords)."""
    rng = np.random.default_rng(3)
    h, w = 12, 14
    blobs = (rng.random((5, h, w)) < .45).astype(np.uint8)
    blobs[1] = 0                            # no foreground in the middle of the stack
    blobs[3] = 1                            # no background in the middle of the stack
    diag = np.zeros((2, 6, 6), np.uint8)
    diag[0][np.arange(6), np.arange(6)] = 255; diag[1, 0, 5] = diag[1, 1, 4] = diag[1, 3, 3] = 1
    d = disc_labels(40, 44, 25, 3, seed=4, rmax=7.)
    discs = (d.transpose(2, 0, 1) > 0).astype(np.uint8)
    out = {}
    for conn in (8, 4):
        out[f'blobs_c{conn}'] = (blobs, dict(connectivity=conn, count=True))
        out[f'blobs_c{conn}_stack0'] = (blobs, dict(connectivity=conn, label_axis=0, reduce=None, count=True))
        out[f'diag_c{conn}'] = (diag, dict(connectivity=conn, reduce=None, count=True))
    out['discs_flat'] = (discs, dict(keepdims=False, count=True))
    out['first_empty'] = (np.stack([blobs[1], blobs[0]]), dict(count=True, reduce=None))
    out['first_full'] = (np.stack([blobs[3], blobs[0], blobs[2]]), dict(count=True, reduce=None, connectivity=4))
    return out


def main():
    out = {}
    names = []
    for name, a in relabel_cases().items():
        got = a.copy()
        ref_seg.relabel_(got)
        names.append(name)
        out[f'relabel.{name}.labels'], out[f'relabel.{name}.result'] = a, got
        again = got.copy()
        ref_seg.relabel_(again)
        assert np.array_equal(again, got)
        print(f'relabel.{name}: {a.shape}, components {int(got.max())}, oracle equal {np.array_equal(oracle.relabel(a), got)}')
    out['relabel_cases'] = np.asarray(names)

    rng = np.random.default_rng(5)
    gray = disc_labels(30, 36, 14, 1, seed=2, rmax=6.)[:, :, 0]
    gray[14:16] = 0
    rgb = np.zeros((30, 36, 3), np.uint8)
    colours = rng.integers(0, 256, (6, 3)).astype(np.uint8)
    for k, col in enumerate(colours):
        rgb[3 + 4 * k:6 + 4 * k, 2 + 3 * k:12 + 3 * k] = col
    rgb[20:26, 20:30] = colours[0]          # one colour in two places
    small = (gray % 4).astype(np.uint8)
    names = []
    for name, maps, kw in (('gray_rgb', (gray, rgb), {}), ('rgb_gray_small', (rgb, small, gray), {}),
                           ('not_relabelled', (gray, rgb), dict(relabel=False)), ('int64', (small, rgb), dict(dtype='int64'))):
        got = ref_seg.stack_labels(*[m.copy() for m in maps], **kw)
        names.append(name)
        for i, m in enumerate(maps):
            out[f'stack.{name}.map{i}'] = m
        out[f'stack.{name}.params'] = np.asarray([len(maps), int(kw.get('relabel', True))], np.int64)
        out[f'stack.{name}.dtype'] = np.asarray(kw.get('dtype', 'int32'))
        out[f'stack.{name}.result'] = got
        print(f'stack.{name}: {got.shape} {got.dtype}, max {int(got.max())}')
    out['stack_cases'] = np.asarray(names)
    out['rgb.input'], out['rgb.result'] = rgb, ref_misc.rgb_to_scalar(rgb)
    out['rgb.result_int64'] = ref_misc.rgb_to_scalar(rgb, dtype='int64')

    names = []
    for name, (masks, kw) in mask_cases().items():
        labels, cnt = ref_cpn.masks2labels(masks.copy(), **kw)
        full = dict(connectivity=8, label_axis=2, reduce='max', keepdims=True)
        full.update(kw)
        names.append(name)
        out[f'masks.{name}.masks'] = masks
        out[f'masks.{name}.params'] = np.asarray([full['connectivity'], full['label_axis'], int(full['reduce'] is not None),
                                                 int(full['keepdims'])], np.int64)
        out[f'masks.{name}.result'], out[f'masks.{name}.count'] = labels, np.asarray(cnt, np.int64)
        print(f'masks.{name}: {masks.shape} -> {labels.shape} {labels.dtype}, count {cnt}')
    out['mask_cases'] = np.asarray(names)

    unary = (disc_labels(20, 24, 9, 4, seed=6, rmax=5.).transpose(2, 0, 1) > 0).astype(np.uint8) * np.uint8(3)
    out['unary.masks'] = unary
    out['unary.transposed'], out['unary.plain'] = ref_seg.unary_masks2labels(unary), ref_seg.unary_masks2labels(unary, transpose=False)

    path = os.path.join(HERE, 'components.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 100 << 10


if __name__ == '__main__':
    main()
