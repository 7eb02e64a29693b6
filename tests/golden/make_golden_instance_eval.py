"""Golden-vector generator of the instance evaluation (build container only: needs the reference checkout that
``oracle/ref_shim.py`` points to, which never travels).

Imports the read-only Python reference through ``oracle/ref_shim.py``, runs its own ``cd.data.LabelMatcher`` /
``LabelMatcherList`` (celldetection/data/instance_eval.py) on small synthetic label images and writes
``instance_eval.npz`` next to this file: the label images and, per case, ``matches``, ``intersections``, ``unions``, ``ious``,
the label lists and areas, and per threshold in (None, 0.3, 0.5, 0.75, 0.9) the selection mask, TP / FP / FN and the five
scores; the list-level values of one ``LabelMatcherList`` of three cases.  Arrays and numbers only.

Ties: the reference walks the pairs in the order of numpy's unstable ``argsort``, so its answer is only defined when no two
pairs with IoU >= threshold have EQUAL IoU and share a label.  Every case is re-seeded until that holds for every threshold
(asserted below): all fixtures are tie-free.

Run:  python tests/golden/make_golden_instance_eval.py          (writes the fixture)
      python tests/golden/make_golden_instance_eval.py time     (times the reference's matcher on larger images)
"""
import os
import sys
import time
import warnings
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')

import ref_shim  # noqa: E402

ref_shim.import_reference()
from celldetection.data.instance_eval import LabelMatcher, LabelMatcherList  # noqa: E402
from test_instance_eval import disc_labels  # noqa: E402  (the synthetic images are the tests' own, not the reference's)

THRESHOLDS = (None, 0.3, 0.5, 0.75, 0.9)
SIZE = (160, 200)
SCORES = ('precision', 'recall', 'f1', 'jaccard', 'fowlkes_mallows')
LIST_VALUES = ('avg_f1', 'avg_jaccard', 'avg_fowlkes_mallows', 'avg_recall', 'avg_precision', 'f1', 'f1_np', 'jaccard_np',
               'fowlkes_mallows_np', 'precision', 'recall', 'true_positives', 'false_positives', 'false_negatives')
LIST_CASES = ('shifted', 'c3_c2', 'missing')


def make_case(name, seed):
    """-> (inputs, targets) int32 label images of the named case."""
    h, w = SIZE
    img = lambda s, c, n=60, **k: disc_labels(h, w, n, c, seed=s, **k)
    if name == 'identical':
        a = img(seed, 3)
        return a, a.copy()
    if name == 'shifted':
        a = img(seed, 2)
        return a, np.roll(a, (2, 3), (0, 1))
    if name == 'independent':
        return img(seed, 1), img(seed + 1000, 1)
    if name == 'c1_c2':
        return img(seed, 1), img(seed, 2, jitter=2.)
    if name == 'c3_c2':
        return img(seed, 3), img(seed, 2, jitter=1.5)
    if name == 'c2_c3':
        return img(seed, 2), img(seed + 1, 3)
    if name == 'repeated':  # a value in two channels of one pixel: counted twice in the area, once in a pair
        a, b = img(seed, 2), img(seed, 2, jitter=1.)
        a[40:120, 50:150, 1] = a[40:120, 50:150, 0]
        b[:80, :, 0] = b[:80, :, 1]
        return a, b
    if name == 'missing':  # objects missing on either side
        a, b = img(seed, 2), img(seed, 2, jitter=1.)
        a[np.isin(a, (3, 17, 29))] = 0
        b[np.isin(b, (5, 8, 41, 42))] = 0
        return a, b
    if name == 'empty_input':
        return np.zeros((h, w, 1), np.int32), img(seed, 1, n=1)
    if name == 'empty_target':
        return img(seed, 1, n=1), np.zeros((h, w, 2), np.int32)
    if name == 'both_empty':
        return np.zeros((h, w, 1), np.int32), np.zeros((h, w, 1), np.int32)
    if name == 'gaps_large':  # labels with gaps and values > 2 ** 20
        a, b = img(seed, 2), img(seed, 3, jitter=1.5)
        a = np.where(a > 0, a * 7919 + (1 << 20) + 5, 0).astype(np.int32)
        b = np.where(b > 0, b * 3 + (1 << 24), 0).astype(np.int32)
        return a, b
    if name == 'two_d':
        return img(seed, 1)[:, :, 0], img(seed, 1, jitter=2.)[:, :, 0]
    if name == 'two_d_c3':
        return img(seed, 1)[:, :, 0], img(seed, 3, jitter=1.)
    if name == 'at_threshold':  # IoU exactly 0.5 and 0.75: tells '>=' from '>'
        a, b = np.zeros((h, w, 1), np.int32), np.zeros((h, w, 1), np.int32)
        a[10:14, 10:20], b[10:14, 10:15] = 1, 1  # 20 / 40
        a[30:34, 10:20], b[30:33, 10:20] = 2, 2  # 30 / 40
        a[50:60, 50:60], b[52:60, 50:60] = 3 + seed, 3  # 80 / 100
        return a, b
    raise KeyError(name)


CASES = ('identical', 'shifted', 'independent', 'c1_c2', 'c3_c2', 'c2_c3', 'repeated', 'missing', 'empty_input', 'empty_target',
         'both_empty', 'gaps_large', 'two_d', 'two_d_c3', 'at_threshold')


def tie_free(m, thresh):
    """No two pairs with IoU >= thresh have equal IoU (as exact fractions) and share a label."""
    iou = [Fraction(int(i), int(u)) for i, u in zip(m.intersections, m.unions)]
    ok = [k for k in range(len(iou)) if m.ious[k] >= thresh]
    seen = {}
    for k in ok:
        for side in (0, 1):
            key = (side, int(m.matches[k, side]), iou[k])
            if key in seen:
                return False
            seen[key] = k
    return True


def record(out, name, m):
    out[f'{name}.matches'] = np.asarray(m.matches, np.int64).reshape(-1, 2)
    out[f'{name}.intersections'] = np.asarray(m.intersections, np.int64)
    out[f'{name}.unions'] = np.asarray(m.unions)
    out[f'{name}.ious'] = np.asarray(m.ious, np.float64)
    out[f'{name}.input_labels'] = np.asarray(m.input_labels, np.int64)
    out[f'{name}.target_labels'] = np.asarray(m.target_labels, np.int64)
    out[f'{name}.input_counts'] = np.asarray([m.input_counts[l] for l in m.input_labels], np.int64)
    out[f'{name}.target_counts'] = np.asarray([m.target_counts[l] for l in m.target_labels], np.int64)


def main():
    out = dict(thresholds=np.asarray([np.nan if t is None else t for t in THRESHOLDS], np.float64),
               cases=np.asarray(CASES), list_cases=np.asarray(LIST_CASES), score_names=np.asarray(SCORES),
               list_value_names=np.asarray(LIST_VALUES))
    matchers = {}
    for ci, name in enumerate(CASES):
        seed = 100 * ci
        while True:
            a, b = make_case(name, seed)
            m = LabelMatcher(a, b)
            if all(tie_free(m, 0. if t is None else t) for t in THRESHOLDS):
                break
            seed += 1
            print(f'{name}: tie, re-seeding -> {seed}')
        out[f'{name}.inputs'], out[f'{name}.targets'] = a.astype(np.int32), b.astype(np.int32)
        record(out, name, m)
        for k, t in enumerate(THRESHOLDS):
            m = LabelMatcher(a, b, iou_thresh=t)
            assert tie_free(m, 0. if t is None else t)
            sel = np.asarray(m._sel, bool).reshape(-1) if len(m.matches) else np.zeros(0, bool)
            out[f'{name}.t{k}.selected'] = sel
            out[f'{name}.t{k}.counts'] = np.asarray([m.true_positives, m.false_positives, m.false_negatives], np.int64)
            out[f'{name}.t{k}.scores'] = np.asarray([getattr(m, s) for s in SCORES], np.float64)
            # the setter gives what the constructor gives
            m2 = matchers.setdefault(name, LabelMatcher(a, b))
            m2.iou_thresh = 0. if t is None else t
            assert (m2.true_positives, m2.false_positives, m2.false_negatives) == tuple(out[f'{name}.t{k}.counts'])
        print(f'{name}: seed {seed}, {a.shape} vs {b.shape}, {len(m.input_labels)} / {len(m.target_labels)} labels, '
              f'{len(m.matches)} pairs, counts {[out[f"{name}.t{k}.counts"].tolist() for k in range(len(THRESHOLDS))]}')
    lml = LabelMatcherList([LabelMatcher(out[f'{n}.inputs'], out[f'{n}.targets']) for n in LIST_CASES])
    for k, t in enumerate(THRESHOLDS):
        lml.iou_thresh = 0. if t is None else t
        out[f'list.t{k}.values'] = np.asarray([getattr(lml, v) for v in LIST_VALUES], np.float64)
    path = os.path.join(HERE, 'instance_eval.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


def time_reference():
    """Wall time of the reference's numpy matcher on growing images (one run each)."""
    for size, n in ((512, 600), (1024, 2500), (2048, 10000)):
        a = disc_labels(size, size, n, 2, seed=1)
        b = disc_labels(size, size, n, 2, seed=1, jitter=1.5)
        t0 = time.perf_counter()
        m = LabelMatcher(a, b, iou_thresh=.5)
        dt = time.perf_counter() - t0
        print(f'reference LabelMatcher {size} x {size} x 2, {len(m.input_labels)} objects, {len(m.matches)} pairs: {dt:.2f} s, '
              f'f1 {m.f1:.4f}', flush=True)


if __name__ == '__main__':
    time_reference() if sys.argv[1:] == ['time'] else main()
