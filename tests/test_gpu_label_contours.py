"""Contours of label images on the GPU (celldetection_amd.labels2contours / resample_contours): every comparison with the numpy
restatement (``tests/label_contours_oracle.py``) and with the reference's fixture (``tests/golden/label_contours.npz``) is exact.
The resampling is compared bit by bit: fp64 ``sqrt`` and ``/`` are correctly rounded on the device and contraction is off, so
the kernel performs the reference's operations in the reference's order."""
import os

import numpy as np
import pytest
import torch

import celldetection_amd as cda
import label_contours_oracle as oracle
from celldetection_amd import label_contours as lc
from labels_oracle import fill_polygon
from test_instance_eval import disc_labels
from test_label_contours import load_label_fixture, load_resample_fixture

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
T = lc.TILE
DISC_SIZES = ((1, 1, 1), (1, 7, 2), (7, 1, 3), (31, 33, 1), (33, 31, 4), (64, 65, 5), (67, 129, 7), (130, 257, 11), (130, 257, 3))
TILE_EDGES = tuple((h, w) for h in (T - 1, T, T + 1, 2 * T + 1) for w in (T - 1, T, T + 1, 2 * T + 1))
TRACED = {}  # contours traced by the tests of this file: resampled in test_resampling_of_traced_contours


def run_gpu(labels, dtype=torch.int32, **kw):
    """-> (ids, offsets, points, labels afterwards) as numpy, from the device copy of ``labels`` (numpy [H, W, C])."""
    t = torch.as_tensor(labels).to(dtype).to(DEV)
    ids, offsets, points = lc.labels2contours_packed(t, **kw)
    assert ids.is_cuda and offsets.is_cuda and points.is_cuda
    assert ids.dtype == torch.int32 and offsets.dtype == torch.int64 and points.dtype == torch.int32
    assert ids.ndim == 1 and tuple(offsets.shape) == (ids.shape[0] + 1,) and points.ndim == 2 and points.shape[1] == 2
    return ids.cpu().numpy(), offsets.cpu().numpy(), points.cpu().numpy(), t.cpu().numpy()


def check(labels, what='', keep=None, **kw):
    """The GPU result against the oracle's, exactly; returns the oracle's (ids, offsets, points)."""
    a = np.array(labels)
    exp = oracle.labels2contours_packed(a, **kw)
    got = run_gpu(labels, **kw)
    for name, g, e in zip(('ids', 'offsets', 'points'), got, exp):
        assert g.shape == e.shape and np.array_equal(g, e), (what, name, g.shape, e.shape)
    assert np.array_equal(got[3], a), (what, 'labels afterwards')
    if keep:
        TRACED[keep] = [exp[2][a:b] for a, b in zip(exp[1][:-1], exp[1][1:])]
    return exp


def test_fixture_cases_equal_the_reference():
    for name, labels, kw, ref in load_label_fixture():
        if ref is None:
            with pytest.raises(ValueError, match='multiple connected components'):
                run_gpu(labels, **kw)
            continue
        got = run_gpu(labels, **kw)
        for g, e in zip(got, ref):
            assert g.shape == e.shape and np.array_equal(g, e), name
        t = torch.as_tensor(labels).to(DEV)
        d = lc.labels2contours(t.clone(), **kw)
        assert list(d) == ref[0].tolist() and all(v.dtype == torch.int32 and v.shape[1:] == (1, 2) for v in d.values()), name
        lst = cda.labels2contours(t.clone(), **kw)
        for c, v, a, b in zip(lst, d.values(), ref[1][:-1], ref[1][1:]):
            assert np.array_equal(c.cpu().numpy(), ref[2][a:b]) and torch.equal(c, v[:, 0]), name
        if len(lst) > 1:  # views of one points tensor: no copies
            assert lst[1].data_ptr() == lst[0].data_ptr() + lst[0].numel() * 4, name
        if labels.shape[2] == 1:  # [H, W] is accepted by the list form
            flat = cda.labels2contours(t[:, :, 0].clone(), **kw)
            assert len(flat) == len(lst) and all(torch.equal(x, y) for x, y in zip(flat, lst)), name


@pytest.mark.parametrize('size', DISC_SIZES, ids=lambda s: 'x'.join(str(i) for i in s))
def test_random_disc_images_against_the_oracle(size):
    h, w, c = size
    labels = disc_labels(h, w, max(1, h * w // 150), c, seed=h * 1000 + w + c, rmin=1.5 if min(h, w) < 10 else 4.)
    if h * w == 1:
        labels[:] = 3
    exp = check(labels, str(size), keep=f'discs{size}' if (h, w) == (67, 129) else None, raise_fragmented=False)
    assert len(exp[0]) > 0 or h * w < 10


def test_tile_edges():
    """T - 1, T, T + 1 and 2 T + 1 in both dimensions: discs, and one object that covers the image but for its corners."""
    for h, w in TILE_EDGES:
        check(disc_labels(h, w, 12, 2, seed=h * 100 + w), f'discs {h} x {w}', raise_fragmented=False)
        full = np.full((h, w, 1), 9, np.int32)
        full[0, 0] = full[-1, -1] = 4  # two pixels of another value: fragmented, skipped
        exp = check(full, f'full {h} x {w}', raise_fragmented=False)
        assert exp[0].tolist() == [9]


def serpentine(h, w):
    """Value 1: a one-pixel-wide path along every even row, joined alternately at the right and the left end; value 2 on the
    odd rows between."""
    a = np.zeros((h, w), np.int32)
    a[0::2] = 1
    a[1::2, 1:-1] = 2
    a[1::4, -1] = 1
    a[3::4, 0] = 1
    return a


def spiral(h, w):
    """Value 1: a one-pixel-wide rectangular spiral from the corner inwards; value 2: the path between its arms."""
    a = np.full((h, w), 2, np.int32)
    y0, x0, y1, x1 = 0, 0, h - 1, w - 1
    first = True
    while x1 - x0 >= 2 and y1 - y0 >= 2:
        a[y0, x0 if first else max(x0 - 1, 0):x1 + 1] = 1
        a[y0:y1 + 1, x1] = 1
        a[y1, x0:x1 + 1] = 1
        a[y0 + 2:y1 + 1, x0] = 1
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
        first = False
    return a


def comb(h, w):
    """Value 1: the top row and the even columns down to the last row but one; value 2: the bottom row and the odd columns."""
    a = np.zeros((h, w), np.int32)
    a[:-1, 0::2] = 1
    a[1:, 1::2] = 2
    a[0] = 1
    a[-1] = 2
    return a


def test_seams():
    h, w = 130, 257
    yy, xx = np.mgrid[:h, :w]
    cases = {'serpentine': serpentine(h, w), 'spiral': spiral(h, w), 'checkerboard': np.where((xx + yy) % 2 == 0, 1, 2).astype(np.int32),
             'full': np.full((h, w), 7, np.int32), 'comb': comb(h, w)}
    for name, a in cases.items():
        n = {v: len(oracle.components((a == v).astype(np.int64))) for v in np.unique(a[a > 0]).tolist()}
        exp = check(a[:, :, None], name, keep=name if name in ('serpentine', 'comb') else None, raise_fragmented=False)
        print(name, 'components per value', n, 'contours', exp[0].tolist(), 'points', np.diff(exp[1]).tolist())
        assert n[1 if name != 'full' else 7] == 1 and len(exp[0]) >= 1, name  # the first value is ONE component across all tiles
        if name in ('checkerboard', 'comb', 'spiral'):
            assert n[2] == 1 and exp[0].tolist() == [1, 2], name
    # all of them as channels of one image (values made distinct per channel)
    stack = np.stack([np.where(a > 0, a + 10 * i, 0) for i, a in enumerate(cases.values())], -1)
    check(stack, 'channels', raise_fragmented=False)


def ring(h, w, y0, x0, size, thick, value):
    a = np.zeros((h, w), np.int32)
    a[y0:y0 + size, x0:x0 + size] = value
    a[y0 + thick:y0 + size - thick, x0 + thick:x0 + size - thick] = 0
    return a


def test_values():
    a = ring(70, 80, 10, 20, 45, 3, 5)
    a[30:34, 40:45] = 8  # an island of another value
    exp = check(a[:, :, None], 'ring, island of another value')
    assert exp[0].tolist() == [5, 8]
    b = a.copy()
    b[b == 8] = 5  # an island of the same value: fragmented by the rule of this package
    with pytest.raises(ValueError, match='multiple connected components'):
        run_gpu(b[:, :, None])
    assert check(b[:, :, None], 'ring, island of the same value', raise_fragmented=False)[0].tolist() == []
    big = np.zeros((40, 70, 2), np.int64)
    big[3:20, 5:40, 0] = 2 ** 31 - 1
    big[25:38, 30:66, 0] = 2 ** 31 - 2
    big[10:30, 20:50, 1] = 2 ** 31 - 1
    big[0, 0, 1] = 1
    for dtype in (torch.int32, torch.int64):
        got = run_gpu(big, dtype)
        exp = oracle.labels2contours_packed(big.copy())
        assert exp[0].tolist() == [1, 2 ** 31 - 2, 2 ** 31 - 1] and all(np.array_equal(g, e) for g, e in zip(got, exp))
    with pytest.raises(ValueError, match='int32'):
        run_gpu(big * 2, torch.int64)
    neg = disc_labels(50, 60, 14, 2, seed=4)
    neg[neg == 3] = -3
    neg[neg == 5] = -2 ** 31
    neg[40:45, 3:30, 1] = -1
    exp = check(neg, 'negatives')
    assert 3 not in exp[0] and 5 not in exp[0] and len(exp[0]) > 4
    small = disc_labels(40, 45, 9, 2, seed=6)
    exp = oracle.labels2contours_packed(small.copy(), raise_fragmented=False)
    for dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        got = run_gpu(small, dtype, raise_fragmented=False)
        assert all(np.array_equal(g, e) for g, e in zip(got, exp)), dtype


def test_twenty_thousand_small_objects():
    """20 000 objects of one to four pixels in 512 x 512 (cells of 3 x 3 pixels), values in random order: the scans and the sort."""
    rng = np.random.default_rng(12)
    n, side = 20000, 512 // 3
    cells = rng.permutation(side * side)[:n]
    values = rng.permutation(n) + 1
    a = np.zeros((512, 512), np.int32)
    shapes = ([(0, 0)], [(0, 0), (0, 1)], [(0, 0), (1, 1)], [(0, 1), (1, 0), (1, 1)], [(0, 0), (0, 1), (1, 0), (1, 1)], [(0, 1), (1, 0)])
    for cell, v, s in zip(cells.tolist(), values.tolist(), rng.integers(0, len(shapes), n).tolist()):
        for dy, dx in shapes[s]:
            a[3 * (cell // side) + dy, 3 * (cell % side) + dx] = v
    exp = check(a[:, :, None], '20000 objects')
    assert exp[0].tolist() == list(range(1, n + 1)) and np.diff(exp[1]).min() == 2


def test_fragmented_objects():
    base = disc_labels(90, 100, 40, 2, seed=9)
    frag = int(base[:, :, 0].max()) + 1
    base[2:5, 2:6, 1] = frag
    base[80:84, 90:97, 1] = frag  # two components, in different tiles
    base[50:53, 3:8, 0] = frag  # and one component in the other channel: that contour is returned
    others = oracle.labels2contours_packed(np.where(base == frag, 0, base))
    with pytest.raises(ValueError, match='multiple connected components'):
        run_gpu(base)
    skipped = check(base, 'skipped', raise_fragmented=False)
    flagged = check(base, 'flagged', flag_fragmented_inplace=True, constant=-4)
    t = torch.as_tensor(base).to(DEV)
    lc.labels2contours_packed(t, flag_fragmented_inplace=True, constant=-4)
    after = t.cpu().numpy()
    assert (after[base == frag] == -4).all() and (after == -4).sum() == (base == frag).sum() == 12 + 28 + 15
    assert np.array_equal(after[base != frag], base[base != frag]) and (after[:, :, 0] == -4).any() and (after[:, :, 1] == -4).any()
    for res in (skipped, flagged):  # the other objects are what they are without the fragmented one
        keep = res[0] != frag
        assert np.array_equal(res[0][keep], others[0]) and np.array_equal(np.diff(res[1])[keep], np.diff(others[1]))
        pts = np.concatenate([res[2][a:b] for a, b, k in zip(res[1][:-1], res[1][1:], keep) if k])
        assert np.array_equal(pts, others[2])
    flat = torch.as_tensor(base[:, :, 1].copy()).to(DEV)  # [H, W]: flagging reaches the caller's tensor
    cda.labels2contours(flat, flag_fragmented_inplace=True)
    assert int((flat == -1).sum()) == 12 + 28


def ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0


def test_resampling_of_the_fixture_cases():
    worst = 0
    for name, contours, num, close, eps, ref in load_resample_fixture():
        given = [torch.as_tensor(c).to(DEV) for c in contours] if isinstance(contours, list) else torch.as_tensor(contours).to(DEV)
        out = cda.resample_contours(given, num, close=close, epsilon=eps)
        if isinstance(contours, list):
            assert isinstance(out, list) and len(out) == len(contours)
            assert all(o.is_cuda and o.dtype == torch.float64 and tuple(o.shape) == (num, 2) for o in out), name
            got = torch.stack(out).cpu().numpy()
            assert isinstance(cda.resample_contours(tuple(given), num, close=close, epsilon=eps), tuple)
        else:
            assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == contours.shape[:-2] + (num, 2), name
            got = out.cpu().numpy().reshape(-1, num, 2)
        d = ulps(got, ref)
        worst = max(worst, d)
        print(f'{name}: largest distance {d} ulp')
        assert np.array_equal(got, ref), (name, d)
        out32 = cda.resample_contours(given, num, close=close, epsilon=eps, dtype=torch.float32)
        got32 = (torch.stack(out32) if isinstance(contours, list) else out32).cpu().numpy().reshape(-1, num, 2)
        assert got32.dtype == np.float32 and np.array_equal(got32, ref.astype(np.float32)), name  # the fp64 result rounded once
    assert worst == 0


def test_resampling_of_traced_contours():
    """The contours traced by the tests above (run alone, this test traces them itself), of 2 to tens of thousands of points."""
    if not TRACED:
        TRACED['discs'] = oracle.labels2contour_list(disc_labels(67, 129, 57, 7, seed=67 * 1000 + 129 + 7, rmin=4.), raise_fragmented=False)
        TRACED['serpentine'] = oracle.labels2contour_list(serpentine(130, 257), raise_fragmented=False)
    for name, contours in TRACED.items():
        given = [torch.as_tensor(c).to(DEV) for c in contours]
        for num, close in ((16, True), (200, True), (33, False)):
            exp = np.stack(oracle.resample_contours(contours, num, close))
            got = torch.stack(cda.resample_contours(given, num, close=close)).cpu().numpy()
            d = ulps(got, exp)
            print(f'{name}: {len(contours)} contours of {min(map(len, contours))} to {max(map(len, contours))} points, num {num}, '
                  f'close {close}: largest distance {d} ulp')
            assert np.array_equal(got, exp), (name, num, close, d)
        offsets = torch.as_tensor(np.cumsum([0] + [len(c) for c in contours])).to(DEV)
        packed = lc.resample_contours_packed(torch.cat(given), offsets, 16)
        assert np.array_equal(packed.cpu().numpy(), np.stack(oracle.resample_contours(contours, 16)))


def test_two_calls_give_identical_bytes_and_torch_ops():
    import celldetection_amd.torch_ops  # noqa: F401  (registers the ops)
    labels = torch.as_tensor(disc_labels(130, 257, 120, 3, seed=31)).to(DEV)
    a = lc.labels2contours_packed(labels, raise_fragmented=False)
    b = lc.labels2contours_packed(labels, raise_fragmented=False)
    c = torch.ops.celldetection_amd.labels2contours_packed(labels, False)
    assert len(a[0]) > 20 and all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))
    r1 = lc.resample_contours_packed(a[2], a[1], 24)
    r2 = lc.resample_contours_packed(a[2], a[1], 24)
    r3 = torch.ops.celldetection_amd.resample_contours(a[2], a[1], 24, True, 1e-6)
    assert tuple(r1.shape) == (len(a[0]), 24, 2) and torch.equal(r1, r2) and torch.equal(r1, r3)
    lst = cda.resample_contours(list(torch.split(a[2], (a[1][1:] - a[1][:-1]).tolist())), 24)
    assert torch.equal(torch.stack(lst), r1)  # the list form goes through the packed form
    with pytest.raises(ValueError, match='at least 2'):
        cda.resample_contours([a[2][:1]], 4, close=False)
    with pytest.raises(ValueError, match='multiple connected components'):
        torch.ops.celldetection_amd.labels2contours_packed(torch.as_tensor(np.eye(5, dtype=np.int32)[:, ::2, None].copy()).to(DEV), True)


def test_end_to_end_on_device_tensors():
    """model -> contours2labels -> resolve_label_channels -> labels2contours -> resample_contours -> contours2labels."""
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
    size = tuple(x.shape[2:])
    contours = y['contours'][0]
    assert contours.is_cuda and contours.shape[0] > 0
    flat = cda.resolve_label_channels(cda.contours2labels(contours, size))
    work = flat.clone()  # the dilation step can split an object: flag on a copy
    traced = cda.labels2contours(work, flag_fragmented_inplace=True)
    a = flat.cpu().numpy().copy()
    exp = oracle.labels2contour_list(a, flag_fragmented_inplace=True)
    assert np.array_equal(work.cpu().numpy(), a)
    assert len(traced) == len(exp) > 0 and all(t.is_cuda and np.array_equal(t.cpu().numpy(), e) for t, e in zip(traced, exp))
    ids = np.unique(a[a > 0])
    assert len(ids) == len(exp)
    for v, c in zip(ids.tolist(), exp):  # the round trip: the filled contour is the object with its holes filled (in its box)
        ys, xs = np.nonzero(a == v)
        y0, x0, y1, x1 = ys.min(), xs.min(), ys.max() + 1, xs.max() + 1
        assert np.array_equal(fill_polygon(c, x0, y0, x1 - x0, y1 - y0), oracle.fill_holes(a[y0:y1, x0:x1] == v)), v
    res = cda.resample_contours(traced, num=model.samples, dtype=torch.float32)
    stacked = torch.stack(res)
    assert stacked.is_cuda and stacked.dtype == contours.dtype and tuple(stacked.shape) == (len(traced), model.samples, 2)
    again = cda.contours2labels(stacked, size)
    assert again.is_cuda and again.dtype == torch.int32 and tuple(again.shape[:2]) == size and int(again.max()) == len(traced)
    print(f'{tuple(contours.shape)} contours on {size}: {len(traced)} flat objects, {int((work == -1).sum())} pixels flagged')
