"""Flat label images on the MI355X: celldetection_amd.resolve_label_channels against the reference's recorded results
(tests/golden/flat_labels.npz) and against the numpy restatement of tests/flat_labels_oracle.py, which the CPU tests pin to
that fixture.  Everything is exact: integers in, integers out, no tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

import celldetection_amd as cda
from celldetection_amd.flat_labels import MAX_STEPS
from flat_labels_oracle import resolve_label_channels as oracle
from test_flat_labels import load_fixture
from test_instance_eval import disc_labels

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def check_against_oracle(a, what='', **kw):
    """cda.resolve_label_channels on the device copy of ``a`` (numpy) against the oracle, stats included."""
    exp, est = oracle(a, return_stats=True, **kw)
    max_iter = kw.get('max_iter', 999)
    out, st = cda.resolve_label_channels(torch.as_tensor(a).to(DEV), return_stats=True, **kw)
    assert out.is_cuda and out.dtype == torch.as_tensor(a).dtype and tuple(out.shape) == a.shape[:2], what
    bad = int((out.cpu().numpy() != exp).sum())
    assert bad == 0, (what, f'{bad} pixels differ')
    assert st['overlap_pixels'] == est['overlap_pixels'] and st['unresolved_pixels'] == est['unresolved_pixels'], (what, st, est)
    # whole launches, and at most one launch of steps that change nothing after the last productive one
    assert est['steps'] <= st['steps'] <= min(max_iter, -(-est['steps'] // MAX_STEPS) * MAX_STEPS + MAX_STEPS), (what, st, est)
    assert len(st['active_tiles']) == st['launches'] == -(-st['steps'] // MAX_STEPS), (what, st)
    return st


def test_fixture_cases_equal_the_reference():
    for name, a, max_iter, kernel, ref in load_fixture():
        exp, est = oracle(a, max_iter=max_iter, kernel=kernel, return_stats=True)
        out, st = cda.resolve_label_channels(torch.as_tensor(a).to(DEV), max_iter=max_iter, kernel=kernel, return_stats=True)
        assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == ref.shape, name
        assert np.array_equal(out.cpu().numpy(), ref), name
        assert st['overlap_pixels'] == est['overlap_pixels'], (name, st, est)
        assert st['unresolved_pixels'] == est['unresolved_pixels'], (name, st, est)
        assert st['steps'] <= max_iter, (name, st)
        # defaults; the kernel as a list and as a Tensor
        if max_iter == 999:
            k = [3, 3] if isinstance(kernel, tuple) else torch.as_tensor(kernel)
            assert np.array_equal(cda.resolve_label_channels(torch.as_tensor(a).to(DEV), kernel=k).cpu().numpy(), ref), name


def test_odd_sizes_and_channel_counts():
    for (h, w, c) in ((1, 1, 2), (3, 5, 1), (3, 5, 3), (1, 700, 2), (257, 2049, 4), (1023, 777, 3), (513, 255, 2), (513, 255, 5),
                      (120, 77, 6), (64, 128, 4), (65, 129, 3)):
        a = disc_labels(h, w, max(h * w // 150, 1), c, seed=h + c, rmax=14.)
        if h == 1:
            a[:] = 0
            a[0, : w // 2 + 1, 0], a[0, w // 4:, c - 1] = 7, 9  # a row: two runs that share a stretch (1 x 1: one overlap pixel)
        st = check_against_oracle(a, f'{h} x {w} x {c}')
        if h * w > 1000 and c > 1:
            assert st['overlap_pixels'] > 0, (h, w, c)
    # more channels than the vector kernels cover, values in the last channels
    a = np.concatenate((disc_labels(90, 110, 60, 6, seed=2, rmax=14.), disc_labels(90, 110, 30, 5, seed=3, rmax=14.) * 1000), 2)
    assert a.shape[2] == 11 and a[:, :, 6:].any()
    check_against_oracle(a, '11 channels')


def test_input_kinds():
    a = disc_labels(96, 130, 60, 3, seed=4, rmax=16.)
    exp = oracle(a)
    for dt in (torch.int64, torch.int16, torch.uint8):
        x = torch.as_tensor(a).to(DEV).to(dt)
        out = cda.resolve_label_channels(x)
        assert out.dtype == dt and out.is_cuda and torch.equal(out.cpu(), torch.as_tensor(exp).to(dt)), dt
    # a view that is neither contiguous nor 16-byte aligned
    pad = torch.zeros((a.shape[0], a.shape[1] + 1, a.shape[2] + 1), dtype=torch.int32, device=DEV)
    pad[:, 1:, 1:] = torch.as_tensor(a).to(DEV)
    view = pad[:, 1:, 1:]
    assert not view.is_contiguous() and view.data_ptr() % 16
    assert np.array_equal(cda.resolve_label_channels(view).cpu().numpy(), exp)
    # negative values are background on the overlap path and survive the plain maximum without overlap
    neg = a.copy()
    neg[neg == 0] = -3
    check_against_oracle(neg, 'negative background')
    one = neg[:, :, :1].copy()
    assert (oracle(one) == -3).any()
    check_against_oracle(one, 'negative background, no overlap')
    big = torch.as_tensor(a).to(DEV).to(torch.int64)
    big[0, 0, 0] = 2 ** 31
    with pytest.raises(ValueError, match='int32'):
        cda.resolve_label_channels(big)
    with pytest.raises(ValueError, match=r'\[H, W, C\]'):
        cda.resolve_label_channels(torch.as_tensor(a[:, :, 0]).to(DEV))
    with pytest.raises(ValueError, match='Invalid method'):
        cda.resolve_label_channels(torch.as_tensor(a).to(DEV), method='voronoi')
    with pytest.raises(NotImplementedError):
        cda.resolve_label_channels(torch.as_tensor(a).to(DEV), kernel=(5, 5))
    # large label values
    check_against_oracle(np.where(a > 0, a * 7919 + (1 << 30), 0).astype(np.int32), 'large values')
    # max_iter = 0: every overlap pixel stays 0
    out, st = cda.resolve_label_channels(torch.as_tensor(a).to(DEV), max_iter=0, return_stats=True)
    assert np.array_equal(out.cpu().numpy(), oracle(a, max_iter=0)) and st['steps'] == 0 and st['unresolved_pixels'] == st['overlap_pixels']


def test_explicit_footprints():
    a = disc_labels(130, 150, 90, 3, seed=9, rmax=15.)
    for k in (np.ones((3, 3), np.uint8), np.array([[0, 1, 0], [0, 0, 0], [0, 0, 0]], np.uint8),  # all / only the pixel above
              np.array([[1, 0, 0], [0, 0, 1], [0, 1, 0]], np.uint8), np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)):
        check_against_oracle(a, f'footprint {k.tolist()}', kernel=k)
        check_against_oracle(a, f'footprint {k.tolist()} capped', kernel=k, max_iter=3)


def test_deep_overlap_over_many_launches():
    """Two rectangles that share a band 300 pixels wide: about 150 steps, fronts from both sides meeting in the middle; in
    full and with a cap that falls inside a launch group."""
    a = np.zeros((700, 900, 2), np.int32)
    a[50:650, 40:600, 0] = 3
    a[90:600, 300:860, 1] = 8
    a[200:260, 420:470, 0] = 0  # a hole in one rectangle inside the band: cores of label 8 in the middle of it
    full = check_against_oracle(a, 'deep overlap')
    assert full['steps'] >= 100 and full['launches'] >= 13 and full['unresolved_pixels'] == 0
    capped = check_against_oracle(a, 'deep overlap, max_iter 37', max_iter=37)
    assert capped['steps'] == 37 and capped['unresolved_pixels'] > 0
    for it in (1, 8, 9, 16, 33):
        check_against_oracle(a, f'deep overlap, max_iter {it}', max_iter=it)


def test_large_seeded_case_against_the_oracle():
    a = disc_labels(2048, 2048, 10000, 4, seed=11, rmax=20.)
    st = check_against_oracle(a, '2048')
    print('2048 x 2048 x 4:', st)
    assert st['overlap_pixels'] > 100000


def test_two_calls_give_identical_results():
    a = torch.as_tensor(disc_labels(1024, 1024, 2500, 3, seed=21, rmax=18.)).to(DEV)
    r1, s1 = cda.resolve_label_channels(a, return_stats=True)
    r2, s2 = cda.resolve_label_channels(a, return_stats=True)
    assert s1 == s2 and s1['overlap_pixels'] > 10000 and torch.equal(r1, r2)
    import celldetection_amd.torch_ops  # noqa: F401  (registers torch.ops.cpn_hip.resolve_label_channels)
    assert torch.equal(torch.ops.cpn_hip.resolve_label_channels(a, 999), r1)
    assert torch.equal(torch.ops.cpn_hip.resolve_label_channels(a, 2), cda.resolve_label_channels(a, max_iter=2))
    assert not torch.equal(cda.resolve_label_channels(a, max_iter=2), r1)


def test_end_to_end_on_device_tensors(monkeypatch):
    """model -> contours2labels -> resolve_label_channels -> LabelMatcher(flat, flat): device tensors all the way."""
    from celldetection_amd.synth import synth_state_dict
    from model_specs import G, MODEL_SPECS
    spec = MODEL_SPECS['CpnU22']
    g = np.load(os.path.join(G, 'model_CpnU22.npz'))
    model = getattr(cda.models, spec['cls'])(**spec['kwargs'])
    overrides = {k[len('override.'):]: torch.as_tensor(g[k]) for k in g.files if k.startswith('override.')}
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=int(g['seed']) if 'seed' in g.files else 0, overrides=overrides))
    model = model.to(DEV)
    x = torch.as_tensor(g['x']).to(DEV)
    model.precision = 'fp32'
    y = model(x)
    labels = cda.contours2labels(y['contours'][0], x.shape[2:])

    def no_host_copy(self, *a, **k):
        if self.numel() > 4096:
            raise AssertionError(f'a tensor of {self.numel()} elements was copied to the host')
        return orig_cpu(self, *a, **k)
    orig_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', no_host_copy)
    flat, st = cda.resolve_label_channels(labels, return_stats=True)
    assert flat.is_cuda and flat.dtype == torch.int32 and tuple(flat.shape) == tuple(labels.shape[:2])
    count = (labels > 0).sum(-1)
    core = count == 1
    assert bool(core.any()) and torch.equal(flat[core], labels.max(-1).values[core])  # every core pixel keeps its label
    assert bool((flat[count == 0] == 0).all())
    assert st['overlap_pixels'] == int((count > 1).sum())
    same = cda.LabelMatcher(flat, flat, iou_thresh=.5)
    assert same.true_positives > 0 and same.false_positives == 0 and same.false_negatives == 0 and abs(same.f1 - 1.) < 1e-9
    monkeypatch.setattr(torch.Tensor, 'cpu', orig_cpu)
    print(f'{tuple(labels.shape)} -> flat, {st}, objects {same.true_positives}')
    assert np.array_equal(flat.cpu().numpy(), oracle(labels.cpu().numpy()))
