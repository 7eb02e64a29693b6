"""Instance evaluation (celldetection_amd.LabelMatcher / LabelMatcherList), CPU part.

``tests/golden/instance_eval.npz`` holds what the reference's own ``cd.data.LabelMatcher`` / ``LabelMatcherList`` computed on
small label images (``tests/golden/make_golden_instance_eval.py``; all cases tie-free, so the reference's answer does not
depend on numpy's sort).  This file restates the rules in plain numpy and shows that the restatement reproduces every
fixture value exactly; the GPU tests (``test_gpu_instance_eval.py``) then use the restatement on cases the reference would
take minutes for, and on ties, where only the package's documented rule defines the answer:

    larger IoU first, compared exactly as i1 * u2 against i2 * u1 in integers; among equal IoU the pair with the smaller
    (input label, target label) first.
"""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import celldetection_amd as cda
from celldetection_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'instance_eval.npz')
SCORES = ('precision', 'recall', 'f1', 'jaccard', 'fowlkes_mallows')


# ---- synthetic label images (the tests' own) ------------------------------------------------------------------------------
def disc_labels(h, w, n, channels, seed, jitter=0., rmin=4., rmax=11.):
    """int32 [h, w, channels]: n seeded discs, disc i with value i + 1 in the first channel it does not overlap anything in
    (dropped when every channel is taken).  ``jitter`` moves centres and radii of the SAME discs by seeded noise."""
    rng = np.random.default_rng(seed)
    cy, cx, r = rng.uniform(0, h, n), rng.uniform(0, w, n), rng.uniform(rmin, rmax, n)
    if jitter:
        rj = np.random.default_rng(seed + 777)
        cy, cx, r = cy + rj.normal(0, jitter, n), cx + rj.normal(0, jitter, n), np.maximum(r + rj.normal(0, jitter / 2, n), 2.)
    out = np.zeros((h, w, channels), np.int32)
    for i in range(n):
        y0, y1 = max(int(cy[i] - r[i]), 0), min(int(cy[i] + r[i]) + 2, h)
        x0, x1 = max(int(cx[i] - r[i]), 0), min(int(cx[i] + r[i]) + 2, w)
        if y0 >= y1 or x0 >= x1:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1]
        mask = (yy - cy[i]) ** 2 + (xx - cx[i]) ** 2 <= r[i] ** 2
        for c in range(channels):
            win = out[y0:y1, x0:x1, c]
            if not win[mask].any():
                win[mask] = i + 1
                break
    return out


# ---- the rules, restated in numpy -----------------------------------------------------------------------------------------
def _areas(x, per_pixel=False):
    """{label: count} over the positive values.  Elements over all channels count (``per_pixel``: a mutant)."""
    if per_pixel:
        pix = np.broadcast_to(np.arange(x.shape[0] * x.shape[1]).reshape(x.shape[0], x.shape[1], 1), x.shape)
        rows = np.unique(np.stack((pix[x > 0], x[x > 0]), 1), axis=0)
        vals = rows[:, 1]
    else:
        vals = x[x > 0]
    uni, cnt = np.unique(vals, return_counts=True)
    return {int(u): int(c) for u, c in zip(uni, cnt)}


def pair_table(inputs, targets, pair_per_channel=False, area_per_pixel=False):
    """-> dict(matches [P, 2], intersections, unions, ious, input_labels, target_labels, input_counts, target_counts)."""
    a = np.asarray(inputs).astype(np.int64)
    b = np.asarray(targets).astype(np.int64)
    a = a[:, :, None] if a.ndim == 2 else a
    b = b[:, :, None] if b.ndim == 2 else b
    pix = np.arange(a.shape[0] * a.shape[1]).reshape(a.shape[:2])
    rows = [np.zeros((0, 3), np.int64)]
    for i in range(a.shape[2]):
        for j in range(b.shape[2]):
            both = (a[:, :, i] > 0) & (b[:, :, j] > 0)
            rows.append(np.stack((pix[both], a[:, :, i][both], b[:, :, j][both]), 1))
    rows = np.concatenate(rows)
    if not pair_per_channel:  # a pixel contributes a pair once, however many channels repeat a value
        rows = np.unique(rows, axis=0)
    pairs = {}
    uni, cnt = np.unique(rows[:, 1:], axis=0, return_counts=True)
    for (i, t), c in zip(uni.tolist(), cnt.tolist()):
        pairs[(i, t)] = c
    in_area, t_area = _areas(a, area_per_pixel), _areas(b, area_per_pixel)
    matches = sorted(pairs)
    inter = np.asarray([pairs[m] for m in matches], np.int64)
    unions = np.asarray([in_area[i] + t_area[t] for i, t in matches], np.int64) - inter
    return dict(matches=np.asarray(matches, np.int64).reshape(-1, 2), intersections=inter, unions=unions,
                ious=inter / unions, input_labels=np.asarray(sorted(in_area), np.int64),
                target_labels=np.asarray(sorted(t_area), np.int64), input_counts=in_area, target_counts=t_area)


def select(table, iou_thresh, strict=False, exclusive=True):
    """Greedy one-to-one matching -> bool [P].  ``strict`` (> instead of >=) and ``exclusive=False`` are mutants."""
    thresh = 0. if iou_thresh is None else iou_thresh
    m, inter, unions, ious = table['matches'], table['intersections'], table['unions'], table['ious']
    order = sorted(range(len(m)), key=lambda k: (-Fraction(int(inter[k]), int(unions[k])), int(m[k, 0]), int(m[k, 1])))
    sel = np.zeros(len(m), bool)
    used_in, used_t = set(), set()
    for k in order:
        if not (ious[k] > thresh if strict else ious[k] >= thresh):
            continue
        i, t = int(m[k, 0]), int(m[k, 1])
        if exclusive and (i in used_in or t in used_t):
            continue
        sel[k] = True
        used_in.add(i)
        used_t.add(t)
    return sel


def counts(table, sel):
    tp = len(set(table['matches'][:, 0][sel].tolist()))
    return tp, len(set(table['input_labels'].tolist()) - set(table['matches'][:, 0][sel].tolist())), \
        len(set(table['target_labels'].tolist()) - set(table['matches'][:, 1][sel].tolist()))


def scores(tp, fp, fn, eps=1e-12):
    pr, rc = tp / (tp + fp + eps), tp / (tp + fn + eps)
    return dict(precision=pr, recall=rc, f1=(2 * pr * rc) / (pr + rc + eps), jaccard=tp / (tp + fn + fp + eps),
                fowlkes_mallows=tp / np.sqrt((tp + fp) * (tp + fn) + eps))


def list_values(per_item, eps=1e-12):
    """per_item: [(tp, fp, fn)] -> the values of a LabelMatcherList."""
    sc = [scores(*c, eps=eps) for c in per_item]
    avg = {k: np.sum([s[k] for s in sc]) / len(sc) for k in SCORES}
    tp, fp, fn = (np.sum([c[k] for c in per_item]) for k in range(3))
    rc, pr = avg['recall'], avg['precision']
    return dict(avg_f1=avg['f1'], avg_jaccard=avg['jaccard'], avg_fowlkes_mallows=avg['fowlkes_mallows'], avg_recall=rc,
                avg_precision=pr, f1=(2 * rc * pr) / (rc + pr + eps), f1_np=(2 * tp) / (2 * tp + fn + fp + eps),
                jaccard_np=tp / (tp + fn + fp + eps), fowlkes_mallows_np=tp / np.sqrt((tp + fp) * (tp + fn) + eps),
                precision=tp / (tp + fp + eps), recall=tp / (tp + fn + eps), true_positives=tp, false_positives=fp,
                false_negatives=fn)


# ---- fixture access -------------------------------------------------------------------------------------------------------
def load_fixture():
    g = np.load(GOLDEN)
    thresholds = [None if np.isnan(t) else float(t) for t in g['thresholds']]
    return g, [str(c) for c in g['cases']], thresholds


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def fixture_values(g, cases, thresholds, **mutant):
    """Everything the restatement computes for the fixture's images, keyed like the fixture."""
    table_kw = {k: v for k, v in mutant.items() if k in ('pair_per_channel', 'area_per_pixel')}
    select_kw = {k: v for k, v in mutant.items() if k in ('strict', 'exclusive')}
    out = {}
    for name in cases:
        t = pair_table(g[f'{name}.inputs'], g[f'{name}.targets'], **table_kw)
        for key in ('matches', 'intersections', 'unions', 'ious', 'input_labels', 'target_labels'):
            out[f'{name}.{key}'] = t[key]
        out[f'{name}.input_counts'] = np.asarray([t['input_counts'][l] for l in t['input_labels'].tolist()], np.int64)
        out[f'{name}.target_counts'] = np.asarray([t['target_counts'][l] for l in t['target_labels'].tolist()], np.int64)
        for k, thr in enumerate(thresholds):
            sel = select(t, thr, **select_kw)
            c = counts(t, sel)
            out[f'{name}.t{k}.selected'] = sel
            out[f'{name}.t{k}.counts'] = np.asarray(c, np.int64)
            out[f'{name}.t{k}.scores'] = np.asarray([scores(*c)[s] for s in SCORES], np.float64)
    return out


def differing_keys(g, values):
    bad = []
    for key, v in values.items():
        exp = g[key]
        ok = same_bits(v, exp) if (exp.dtype.kind == 'f' and exp.size) else \
            (np.asarray(v).shape == exp.shape and np.array_equal(np.asarray(v), exp))
        if not ok:
            bad.append(key)
    return bad


# ---- tests ----------------------------------------------------------------------------------------------------------------
def test_fixture_covers_the_cases():
    g, cases, thresholds = load_fixture()
    assert thresholds == [None, 0.3, 0.5, 0.75, 0.9]
    for name in ('identical', 'shifted', 'independent', 'c1_c2', 'c3_c2', 'c2_c3', 'repeated', 'missing', 'empty_input',
                 'empty_target', 'both_empty', 'gaps_large', 'two_d', 'at_threshold'):
        assert name in cases
    assert g['two_d.inputs'].ndim == 2 and g['c3_c2.inputs'].shape[2] == 3 and g['c3_c2.targets'].shape[2] == 2
    assert g['gaps_large.inputs'].max() > 2 ** 20 and g['gaps_large.targets'].max() > 2 ** 20
    a = g['repeated.inputs']
    assert ((a[:, :, 0] == a[:, :, 1]) & (a[:, :, 0] > 0)).any()
    assert len(g['missing.t2.counts']) == 3 and g['missing.t2.counts'][1] > 0 and g['missing.t2.counts'][2] > 0
    # what the reference does without labels on a side: no exception, empty pair list, F1 = 0
    for name, exp in (('empty_input', (0, 0, 1)), ('empty_target', (0, 1, 0)), ('both_empty', (0, 0, 0))):
        assert g[f'{name}.matches'].shape == (0, 2)
        assert tuple(g[f'{name}.t0.counts']) == exp and g[f'{name}.t0.scores'][2] == 0.
    for v in g.values():
        assert v.dtype.kind in 'iufbU'  # arrays and numbers only


def test_restatement_reproduces_the_reference_fixture():
    g, cases, thresholds = load_fixture()
    values = fixture_values(g, cases, thresholds)
    assert len(values) == len(cases) * (8 + 3 * len(thresholds))
    assert differing_keys(g, values) == []
    names = [str(n) for n in g['list_value_names']]
    for k, thr in enumerate(thresholds):
        per_item = [tuple(int(c) for c in g[f'{n}.t{k}.counts']) for n in g['list_cases']]
        lv = list_values(per_item)
        assert same_bits([lv[n] for n in names], g[f'list.t{k}.values']), (thr, lv)


def test_tie_rule_on_hand_built_cases():
    # input 1 overlaps targets 5 and 7 with IoU 2 / 4 each: the smaller (input, target) pair wins, target 7 is unmatched
    t = pair_table(np.array([[1, 1, 1, 1, 0, 0]]), np.array([[7, 7, 5, 5, 0, 0]]))
    assert t['matches'].tolist() == [[1, 5], [1, 7]] and t['intersections'].tolist() == [2, 2] and t['unions'].tolist() == [4, 4]
    sel = select(t, None)
    assert sel.tolist() == [True, False] and counts(t, sel) == (1, 0, 1)
    assert select(t, .5).tolist() == [True, False] and select(t, .51).tolist() == [False, False]
    # inputs 2 and 4 overlap target 6 with IoU 2 / 5 each: (2, 6) before (4, 6); input 4 is a false positive
    t = pair_table(np.array([[4, 4, 0, 2, 2]]), np.array([[6, 6, 6, 6, 6]]))
    assert t['matches'].tolist() == [[2, 6], [4, 6]] and t['unions'].tolist() == [5, 5]
    sel = select(t, None)
    assert sel.tolist() == [True, False] and counts(t, sel) == (1, 1, 0)
    # equal IoU from different numbers, 3 / 9 and 1 / 3, sharing target 4: a tie, decided by the labels
    t = dict(matches=np.array([[1, 4], [2, 4]]), intersections=np.array([3, 1]), unions=np.array([9, 3]),
             ious=np.array([3 / 9, 1 / 3]), input_labels=np.array([1, 2]), target_labels=np.array([4]))
    assert select(t, None).tolist() == [True, False]
    t['matches'] = np.array([[2, 4], [1, 4]])  # the same two pairs named the other way round: the other one wins
    assert select(t, None).tolist() == [False, True]
    # two quotients that differ by 2 ** -62 give the same float64: the integers decide, not the labels
    i1, u1, i2, u2 = 2 ** 30, 2 ** 31 + 1, 2 ** 30 - 1, 2 ** 31 - 1
    assert i1 * u2 - i2 * u1 == 1 and i1 / u1 == i2 / u2
    t = dict(matches=np.array([[2, 4], [1, 4]]), intersections=np.array([i1, i2]), unions=np.array([u1, u2]),
             ious=np.array([i1 / u1, i2 / u2]), input_labels=np.array([1, 2]), target_labels=np.array([4]))
    assert select(t, None).tolist() == [True, False]
    # exclusivity over a chain: (1, 5) and (2, 6) at 1 / 2 are taken, (2, 5) at 1 / 5 loses both its labels
    t = pair_table(np.array([[1, 1, 1, 2, 2, 2, 0]]), np.array([[0, 5, 5, 5, 6, 6, 6]]))
    assert t['matches'].tolist() == [[1, 5], [2, 5], [2, 6]] and t['unions'].tolist() == [4, 5, 4]
    assert select(t, None).tolist() == [True, False, True]


@pytest.mark.parametrize('mutant', [dict(pair_per_channel=True), dict(area_per_pixel=True), dict(strict=True),
                                    dict(exclusive=False)], ids=lambda m: next(iter(m)))
def test_fixture_sees_mutants_of_the_rules(mutant):
    g, cases, thresholds = load_fixture()
    assert differing_keys(g, fixture_values(g, cases, thresholds, **mutant)) != []


def test_abi_exports_the_eval_entry_points():
    lib = _lib.load()
    for name in ('cpn_eval_workspace_bytes', 'cpn_eval_pairs', 'cpn_eval_table_status', 'cpn_eval_compact', 'cpn_eval_unions',
                 'cpn_eval_select'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _lib.ABI_VERSION >= 15
    w = lib.cpn_eval_workspace_bytes
    assert w(1 << 12, 0, 0) >= (1 << 12) * 16
    assert w(1 << 13, 0, 0) - w(1 << 12, 0, 0) == (1 << 12) * 16
    assert w(0, 1000, 0) > w(0, 0, 0) and w(0, 1000, 500) > w(0, 1000, 0) and w(1 << 12, 1000, 500) > w(1 << 12, 0, 0)


def test_no_cpu_fallback():
    assert 'LabelMatcher' in cda.__all__ and 'LabelMatcherList' in cda.__all__
    g, _, _ = load_fixture()
    a, b = torch.as_tensor(g['shifted.inputs']), torch.as_tensor(g['shifted.targets'])
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.LabelMatcher(a, b)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.LabelMatcher().update(a, b, .5)
    with pytest.raises(ValueError, match='No labels'):
        cda.LabelMatcher().f1
    lml = cda.LabelMatcherList()
    assert len(lml) == 0 and lml.length == 0 and not lml.distributed and lml.avg_f1 == 0
