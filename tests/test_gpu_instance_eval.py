"""Instance evaluation on the MI355X: celldetection_amd.LabelMatcher / LabelMatcherList against the reference's recorded
results (tests/golden/instance_eval.npz) and against the numpy restatement of tests/test_instance_eval.py, which the CPU
tests pin to that fixture.  Everything is exact: counts are integers, scores float64 functions of them."""
import os

import numpy as np
import pytest
import torch

import celldetection_amd as cda
from test_instance_eval import (SCORES, counts, disc_labels, list_values, load_fixture, pair_table, same_bits, scores, select)

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def check_against_table(m, t, thresholds, what=''):
    """A LabelMatcher against the restatement's table ``t`` at every threshold."""
    assert np.array_equal(m.matches, t['matches']), what
    assert np.array_equal(m.intersections, t['intersections']), what
    assert np.array_equal(m.unions, t['unions']), what
    assert same_bits(m.ious, t['ious']), what
    assert np.array_equal(m.input_labels, t['input_labels']) and np.array_equal(m.target_labels, t['target_labels']), what
    assert m.input_counts == t['input_counts'] and m.target_counts == t['target_counts'], what
    for thr in thresholds:
        m.iou_thresh = 0. if thr is None else thr
        sel = select(t, thr)
        c = counts(t, sel)
        assert np.array_equal(m._sel, sel), (what, thr)
        assert (m.true_positives, m.false_positives, m.false_negatives) == c, (what, thr)
        exp = scores(*c)
        for s in SCORES:
            assert same_bits(getattr(m, s), exp[s]), (what, thr, s)
        assert m.true_positive_labels == set(t['matches'][:, 0][sel].tolist())
        assert m.false_positive_labels == set(t['input_labels'].tolist()) - set(t['matches'][:, 0][sel].tolist())
        assert m.false_negative_labels == set(t['target_labels'].tolist()) - set(t['matches'][:, 1][sel].tolist())


def test_fixture_cases_equal_the_reference():
    g, cases, thresholds = load_fixture()
    for name in cases:
        a, b = torch.as_tensor(g[f'{name}.inputs']).to(DEV), torch.as_tensor(g[f'{name}.targets']).to(DEV)
        for k, thr in enumerate(thresholds):
            m = cda.LabelMatcher(a, b, iou_thresh=thr)
            if k == 0:
                for key in ('matches', 'intersections', 'unions', 'input_labels', 'target_labels'):
                    assert np.array_equal(getattr(m, key), g[f'{name}.{key}']), (name, key)
                assert getattr(m, 'matches').shape == g[f'{name}.matches'].shape
                assert same_bits(m.ious, g[f'{name}.ious']), name
                assert [m.input_counts[l] for l in m.input_labels.tolist()] == g[f'{name}.input_counts'].tolist(), name
                assert [m.target_counts[l] for l in m.target_labels.tolist()] == g[f'{name}.target_counts'].tolist(), name
            assert np.array_equal(m._sel, g[f'{name}.t{k}.selected']), (name, thr)
            assert [m.true_positives, m.false_positives, m.false_negatives] == g[f'{name}.t{k}.counts'].tolist(), (name, thr)
            assert same_bits([getattr(m, s) for s in SCORES], g[f'{name}.t{k}.scores']), (name, thr)
        # numpy arrays are uploaded; the setter selects again from the stored table
        m = cda.LabelMatcher(g[f'{name}.inputs'], g[f'{name}.targets'])
        for k, thr in enumerate(thresholds):
            m.iou_thresh = 0. if thr is None else thr
            assert [m.true_positives, m.false_positives, m.false_negatives] == g[f'{name}.t{k}.counts'].tolist(), (name, thr)


def test_label_matcher_list_equals_the_reference():
    g, _, thresholds = load_fixture()
    names = [str(n) for n in g['list_value_names']]
    lml = cda.LabelMatcherList([cda.LabelMatcher(torch.as_tensor(g[f'{n}.inputs']).to(DEV), torch.as_tensor(g[f'{n}.targets']).to(DEV))
                                for n in g['list_cases']])
    assert lml.length == 3 and lml.iou_thresh == 0.
    for k, thr in enumerate(thresholds):
        lml.iou_thresh = 0. if thr is None else thr
        assert lml.iou_thresh == (0. if thr is None else thr)
        assert same_bits([getattr(lml, n) for n in names], g[f'list.t{k}.values']), thr
    lml.append(cda.LabelMatcher(torch.as_tensor(g['two_d.inputs']).to(DEV), torch.as_tensor(g['two_d.targets']).to(DEV), iou_thresh=.5))
    per_item = [(m.true_positives, m.false_positives, m.false_negatives) for m in lml]
    assert len(np.atleast_1d(lml.iou_thresh)) == 2
    lv = list_values(per_item)
    assert same_bits([getattr(lml, n) for n in names], [lv[n] for n in names])


def test_input_kinds():
    g, _, _ = load_fixture()
    a, b = g['c3_c2.inputs'], g['c3_c2.targets']
    exp = g['c3_c2.t2.counts'].tolist()
    for dt in (torch.int64, torch.int16):
        m = cda.LabelMatcher(torch.as_tensor(a).to(DEV).to(dt), torch.as_tensor(b).to(DEV).to(dt), iou_thresh=.5)
        assert [m.true_positives, m.false_positives, m.false_negatives] == exp
    # a view that is neither contiguous nor 16-byte aligned
    pad = torch.zeros((a.shape[0], a.shape[1] + 1, a.shape[2] + 1), dtype=torch.int32, device=DEV)
    pad[:, 1:, 1:] = torch.as_tensor(a).to(DEV)
    m = cda.LabelMatcher(pad[:, 1:, 1:], torch.as_tensor(b).to(DEV), iou_thresh=.5)
    assert [m.true_positives, m.false_positives, m.false_negatives] == exp
    # negative values are background
    neg = torch.as_tensor(a).to(DEV).clone()
    neg[neg == 0] = -3
    m = cda.LabelMatcher(neg, torch.as_tensor(b).to(DEV), iou_thresh=.5)
    assert [m.true_positives, m.false_positives, m.false_negatives] == exp
    big = torch.as_tensor(a).to(DEV).to(torch.int64)
    big[0, 0, 0] = 2 ** 31
    with pytest.raises(ValueError, match='int32'):
        cda.LabelMatcher(big, torch.as_tensor(b).to(DEV))
    with pytest.raises(ValueError, match='differ in size'):
        cda.LabelMatcher(torch.as_tensor(a[:-1]).to(DEV), torch.as_tensor(b).to(DEV))
    with pytest.raises(RuntimeError, match='8 channels'):
        cda.LabelMatcher(torch.zeros((8, 8, 9), dtype=torch.int32, device=DEV), torch.as_tensor(b[:8, :8]).to(DEV))


def test_more_than_four_channels():
    """5 to 8 channels a side take the kernel without register run-lengths: same table."""
    a = np.concatenate((disc_labels(96, 130, 40, 3, seed=5), disc_labels(96, 130, 40, 3, seed=6) * 100), 2)  # 6 channels
    b = np.concatenate([disc_labels(96, 130, 40, 2, seed=5 + k, jitter=1.) * (k + 1) for k in range(4)], 2)  # 8 channels
    a[:, :, 4] = np.where(a[:, :, 0] > 0, a[:, :, 0], a[:, :, 4])  # repeated values across channels
    t = pair_table(a, b)
    assert len(t['matches']) > 100
    check_against_table(cda.LabelMatcher(torch.as_tensor(a).to(DEV), torch.as_tensor(b).to(DEV)), t, (None, .5), '6 x 8')
    check_against_table(cda.LabelMatcher(torch.as_tensor(b).to(DEV), torch.as_tensor(a[:, :, :2]).to(DEV)), pair_table(b, a[:, :, :2]),
                        (None, .5), '8 x 2')


def test_large_seeded_case_against_the_restatement():
    a = disc_labels(2048, 2048, 10000, 3, seed=11)
    b = disc_labels(2048, 2048, 10000, 3, seed=11, jitter=1.5)
    t = pair_table(a, b)
    print(f'2048 x 2048 x 3: {len(t["input_labels"])} / {len(t["target_labels"])} objects, {len(t["matches"])} pairs')
    assert len(t['input_labels']) > 9000 and len(t['matches']) > 9000
    m = cda.LabelMatcher(torch.as_tensor(a).to(DEV), torch.as_tensor(b).to(DEV))
    check_against_table(m, t, (None, .5, .75), '2048')
    print('stats', m.stats)


def test_odd_sizes():
    for (h, w, ca, cb) in ((1023, 777, 2, 3), (1, 1, 1, 1), (3, 5, 1, 2), (257, 2049, 4, 1), (300, 333, 4, 4), (120, 77, 3, 4),
                           (64, 1000, 4, 3), (513, 255, 2, 4)):
        n = max(h * w // (400 if ca + cb < 7 else 120), 1)  # 4 channels a side: dense enough to fill them
        a = disc_labels(h, w, n, ca, seed=h)
        b = disc_labels(h, w, n, cb, seed=h, jitter=1.)
        if ca + cb >= 7:
            assert a[:, :, ca - 1].any() and b[:, :, cb - 1].any()
        if h == 1:
            a[:], b[:] = 7, 9
        check_against_table(cda.LabelMatcher(torch.as_tensor(a).to(DEV), torch.as_tensor(b).to(DEV)), pair_table(a, b),
                            (None, .5), f'{h} x {w}')


def test_table_grows_when_started_too_small():
    a = disc_labels(512, 512, 700, 2, seed=3)
    b = disc_labels(512, 512, 700, 2, seed=3, jitter=1.5)
    t = pair_table(a, b)
    entries = len(t['matches']) + len(t['input_labels']) + len(t['target_labels'])
    m = cda.LabelMatcher(torch.as_tensor(a).to(DEV), torch.as_tensor(b).to(DEV), table_capacity=64)
    assert m.stats['grown'] >= 1 and m.stats['table_capacity'] >= entries > 64 and m.stats['entries'] == entries
    check_against_table(m, t, (None, .5), 'grown table')


def test_tie_heavy_grid_under_the_documented_rule():
    """Equal squares on a regular grid against the same grid shifted by half a pitch: every input square meets four target
    squares at the same IoU.  Only the documented order (equal IoU: smaller (input, target) pair first) defines the result."""
    n, pitch, side = 24, 16, 12
    a = np.zeros((n * pitch + pitch, n * pitch + pitch, 1), np.int32)
    b = np.zeros_like(a)
    lab = np.random.default_rng(0).permutation(n * n) + 1  # target labels in no spatial order
    for i in range(n):
        for j in range(n):
            a[i * pitch:i * pitch + side, j * pitch:j * pitch + side, 0] = 1 + i * n + j
            y, x = i * pitch + pitch // 2, j * pitch + pitch // 2
            b[y:y + side, x:x + side, 0] = lab[i * n + j]
    t = pair_table(a, b)
    assert len(np.unique(t['ious'])) == 1 and len(t['matches']) > 3 * n * (n - 1)
    m = cda.LabelMatcher(torch.as_tensor(a).to(DEV), torch.as_tensor(b).to(DEV))
    check_against_table(m, t, (None, .1, .5), 'grid')
    print('tie-heavy grid: pairs', len(t['matches']), 'selection rounds', m.stats['selection_rounds'], 'tp', m.true_positives)


def test_two_calls_give_identical_tables():
    a = torch.as_tensor(disc_labels(1024, 1024, 2500, 3, seed=21)).to(DEV)
    b = torch.as_tensor(disc_labels(1024, 1024, 2500, 2, seed=21, jitter=2.)).to(DEV)
    t1 = cda.instance_eval.label_pair_table(a, b)
    t2 = cda.instance_eval.label_pair_table(a, b)
    assert t1.dtype == torch.int64 and t1.shape[1] == 2 and t1.shape[0] > 5000 and torch.equal(t1, t2)
    import celldetection_amd.torch_ops  # noqa: F401  (registers torch.ops.cpn_hip.label_pair_table)
    assert torch.equal(torch.ops.cpn_hip.label_pair_table(a, b), t1)
    m1, m2 = cda.LabelMatcher(a, b, iou_thresh=.5), cda.LabelMatcher(a, b, iou_thresh=.5)
    assert np.array_equal(m1._sel, m2._sel) and m1.f1 == m2.f1


def test_end_to_end_on_device_tensors(monkeypatch):
    """model -> contours2labels -> LabelMatcher in 'fp32' and 'bf16': runs on device tensors (the label images never visit the
    host), identical inputs give F1 = 1.  No quality threshold: nobody has measured one; the value is printed (on the CpnU22
    fixture input with synthetic weights: F1 0.875 = 28 matched, 3 only in bf16, 5 only in fp32, at IoU 0.5)."""
    from celldetection_amd.synth import synth_state_dict
    from model_specs import G, MODEL_SPECS
    spec = MODEL_SPECS['CpnU22']
    g = np.load(os.path.join(G, 'model_CpnU22.npz'))
    model = getattr(cda.models, spec['cls'])(**spec['kwargs'])
    overrides = {k[len('override.'):]: torch.as_tensor(g[k]) for k in g.files if k.startswith('override.')}
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=int(g['seed']) if 'seed' in g.files else 0, overrides=overrides))
    model = model.to(DEV)
    x = torch.as_tensor(g['x']).to(DEV)
    labels = {}
    for precision in ('fp32', 'bf16'):
        model.precision = precision
        y = model(x)
        labels[precision] = cda.contours2labels(y['contours'][0], x.shape[2:])
        assert labels[precision].is_cuda and labels[precision].dtype == torch.int32

    def no_host_copy(self, *a, **k):
        if self.numel() > 4096:
            raise AssertionError(f'a tensor of {self.numel()} elements was copied to the host')
        return orig_cpu(self, *a, **k)
    orig_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', no_host_copy)
    m = cda.LabelMatcher(labels['bf16'], labels['fp32'], iou_thresh=.5)
    print(f'bf16 labels against fp32 labels at IoU 0.5: F1 {m.f1:.4f} (tp {m.true_positives}, fp {m.false_positives}, '
          f'fn {m.false_negatives}; {labels["fp32"].shape[2]} / {labels["bf16"].shape[2]} channels)')
    assert m.true_positives + m.false_negatives == len(torch.unique(labels['fp32'][labels['fp32'] > 0]))
    same = cda.LabelMatcher(labels['fp32'], labels['fp32'], iou_thresh=.5)
    assert same.true_positives > 0 and same.false_positives == 0 and same.false_negatives == 0
    assert abs(same.f1 - 1.) < 1e-9 and same.f1 == scores(same.true_positives, 0, 0)['f1']
