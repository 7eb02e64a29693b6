"""Elliptic Fourier descriptors of contours on the GPU (celldetection_amd.efd / efd_packed / contours2fourier / labels2fourier).

Results are judged against ``fourier_oracle.truth`` (mpmath, 40 digits) in the unit ``U = 2^-53 N T`` of each contour, with the
constants that ``tests/test_fourier.py`` measured (``tests/golden/fourier_measured.json``: 4 x the reference's own largest error):
``|coefficient - truth| <= c_f U``, ``|location - truth| <= c_l U + 2^-53 |truth|``; contours with ``N <= 1`` are exact.
"""
import os

import numpy as np
import pytest
import torch

import celldetection_amd as cda
import fourier_oracle as oracle
from celldetection_amd import fourier as fo
from celldetection_amd import label_contours as lc
from test_fourier import (constants, fixture_contours, generator_cases, load_c2f_fixture, load_efd_fixture, segments, truths, within)
from test_instance_eval import disc_labels

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
C = fo.CHUNK
ORDERS = (1, 5, fo.MAX_ORDER)


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def pack(contours, dtype=None):
    """list of arrays [n, 2] -> (points tensor, offsets tensor) on the GPU."""
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in contours])]).astype(np.int64)
    points = np.concatenate(contours)
    return gpu(points if dtype is None else points.astype(dtype)), gpu(offsets)


def judge(coeff, loc, contour, append, ref, what):
    """One contour's float64 result against its truth; N <= 1 exactly."""
    N = segments(contour, append)
    coeff, loc = np.asarray(coeff), np.asarray(loc)
    if N == 0:
        assert (coeff == 0).all() and np.isnan(loc).all(), what
    elif N == 1:
        assert (coeff == 0).all() and loc.tolist() == np.asarray(contour[0], np.float64).tolist(), what
    else:
        return within(coeff, loc, ref, what)


def test_fixture_cases_are_within_the_bound():
    """Through ``efd`` (dense: the whole-tensor closing rule; a list: per contour), ``efd_packed`` and ``contours2fourier``;
    float32 output equals the float64 output rounded once."""
    per_contour = {}
    for name, c, a, order, eps, _, _ in fixture_contours():
        per_contour.setdefault(name.split('[')[0], []).append((name, c, a))
    worst = [0., 0.]
    for name, contours, order, eps, autoclose, ref_coeff, ref_loc in load_efd_fixture():
        arg = [gpu(c) for c in contours] if isinstance(contours, list) else gpu(contours)
        coeff, loc = cda.efd(arg, order=order, epsilon=eps, autoclose=autoclose)
        assert coeff.is_cuda and coeff.dtype == loc.dtype == torch.float64
        lead = (len(contours),) if isinstance(contours, list) else contours.shape[:-2]
        assert tuple(coeff.shape) == lead + (order, 4) and tuple(loc.shape) == lead + (2,), name
        coeff, loc = coeff.reshape(-1, order, 4).cpu().numpy(), loc.reshape(-1, 2).cpu().numpy()
        members = per_contour[name]
        for i, (full, c, a) in enumerate(members):
            r = judge(coeff[i], loc[i], c, a, truths()[full], f'{full}, {segments(c, a)} segments, order {order}')
            if r:
                worst = [max(worst[0], r[0]), max(worst[1], r[1])]
        if all(a == (not oracle.is_closed(c)) for _, c, a in members):  # the per-contour decision gives the same: efd_packed
            pts, off = pack([c for _, c, _ in members])
            pc, pl = fo.efd_packed(pts, off, order, eps)
            assert np.array_equal(pc.cpu().numpy(), coeff) and np.array_equal(pl.cpu().numpy(), loc, equal_nan=True), name
            c32, l32 = fo.efd_packed(pts, off, order, eps, dtype=torch.float32)
            assert c32.dtype == torch.float32 and torch.equal(c32, pc.float()) and torch.equal(l32.nan_to_num(-1), pl.float().nan_to_num(-1))
        else:
            assert name == 'dense_one_open'  # the closed members got the point appended as well
            pts, off = pack([c for _, c, _ in members])
            pc, _ = fo.efd_packed(pts, off, order, eps)
            assert not np.array_equal(pc.cpu().numpy()[0], coeff[0]) and np.array_equal(pc.cpu().numpy()[1], coeff[1])
    print(f'fixture: worst {worst[0]:.3g} U (coefficients), {worst[1]:.3g} U (locations); bound {constants()}')
    for name, contours, order, f64, l64, f32, l32 in load_c2f_fixture():
        if not contours:
            a, b = cda.contours2fourier({}, order=order)
            assert tuple(a.shape) == (0, order, 4) and tuple(b.shape) == (0, 2) and a.is_cuda and a.dtype == torch.float32
            continue
        dev = {k: gpu(v) for k, v in contours.items()}
        a64, b64 = cda.contours2fourier(dev, order=order, dtype=torch.float64)
        a32, b32 = cda.contours2fourier(dev, order=order)
        assert a32.dtype == b32.dtype == torch.float32 and tuple(a64.shape) == f64.shape and tuple(b64.shape) == l64.shape
        assert torch.equal(a32, a64.float()) and torch.equal(b32, b64.float())
        filled = np.zeros(len(f64), bool)
        for key, c in contours.items():
            c = c.reshape(-1, 2)
            a = not oracle.is_closed(c)
            judge(a64[key - 1].cpu().numpy(), b64[key - 1].cpu().numpy(), c, a, oracle.truth(c, order, 1e-6, a), f'{name} label {key}')
            filled[key - 1] = True
        assert not a64.cpu().numpy()[~filled].any() and not b64.cpu().numpy()[~filled].any()


def edge_batch():
    contours = oracle.edge_contours()
    assert [segments(c, not oracle.is_closed(c)) for c in contours] == \
        [1, 2, 3, 63, 64, 65, C - 1, C, C + 1, 2 * C, 2 * C + 1, 5 * C + 7]
    return contours


@pytest.mark.parametrize('order', ORDERS)
def test_chunk_edges(order):
    contours = edge_batch()
    pts, off = pack(contours)
    timings = {}
    coeff, loc = fo.efd_packed(pts, off, order, timings=timings)
    assert timings['chunks'] == 2 + 2 + 3 + 6  # C + 1, 2 C, 2 C + 1 and 5 C + 7 segments; C segments are one chunk
    coeff, loc = coeff.cpu().numpy(), loc.cpu().numpy()
    for i, c in enumerate(contours):
        a = not oracle.is_closed(c)
        N = segments(c, a)
        r = judge(coeff[i], loc[i], c, a, truths().get(f'edge{N}.order{order}'), f'{N} segments, order {order}')
        if r:
            print(f'{N} segments, order {order}: {r[0]:.3g} U, {r[1]:.3g} U')


def test_a_contour_does_not_depend_on_its_neighbours_or_the_run():
    contours = edge_batch()
    order = 5
    run = lambda cs: tuple(t.cpu().numpy() for t in fo.efd_packed(*pack(cs), order))
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    coeff, loc = run(contours)
    again = run(contours)
    assert same(coeff, again[0]) and same(loc, again[1])  # two runs: the same bytes
    for i, c in enumerate(contours):
        alone = run([c])
        assert same(alone[0][0], coeff[i]) and same(alone[1][0], loc[i]), len(c)
    rev = run(contours[::-1])
    assert same(rev[0][::-1], coeff) and same(rev[1][::-1], loc)
    front = run([oracle.ragged_walk(5 * C, 77)] + contours)
    assert same(front[0][1:], coeff) and same(front[1][1:], loc)


def test_input_dtypes():
    contours = edge_batch()
    base = [t.cpu().numpy() for t in fo.efd_packed(*pack(contours, np.int32), 5)]
    assert pack(contours)[0].dtype == torch.int32
    for dtype in (np.float64, np.float32, np.int64, np.int16):  # float64 is read as it is, the others are converted by the host
        out = fo.efd_packed(*pack(contours, dtype), 5)
        assert np.array_equal(out[0].cpu().numpy(), base[0]) and np.array_equal(out[1].cpu().numpy(), base[1]), dtype
    lst = cda.efd([gpu(c) for c in contours], 5)  # a list of int32 tensors
    assert np.array_equal(lst[0].cpu().numpy(), base[0]) and np.array_equal(lst[1].cpu().numpy(), base[1])


def test_one_long_contour_is_spread_over_chunks():
    c = oracle.long_contour()
    assert len(c) == 20 * C
    timings = {}
    coeff, loc = fo.efd_packed(gpu(c), gpu(np.asarray([0, len(c)], np.int64)), 3, timings=timings)
    assert timings['chunks'] == 20  # one wave each
    r = within(coeff[0].cpu().numpy(), loc[0].cpu().numpy(), truths()['long'], f'{len(c)} segments, order 3')
    print(f'{len(c)} points: {r[0]:.3g} U, {r[1]:.3g} U')
    # the length that the contour trace documents as its limit: many waves, no more work than its chunks
    n = 32796
    big = oracle.ragged_walk(n, 3, center=(9000, 9000))
    fo.efd_packed(gpu(big), gpu(np.asarray([0, n], np.int64)), 5, timings=timings)
    assert timings['chunks'] == -(-n // C) == 129


def test_no_contour_and_twenty_thousand_tiny_contours():
    e = fo.efd_packed(torch.zeros((0, 2), dtype=torch.int32, device=DEV), torch.zeros((1,), dtype=torch.int64, device=DEV), 5)
    assert tuple(e[0].shape) == (0, 5, 4) and tuple(e[1].shape) == (0, 2) and e[0].is_cuda
    points, offsets = oracle.tiny_contours()
    K = len(offsets) - 1
    assert K == 20000
    coeff, loc = (t.cpu().numpy() for t in fo.efd_packed(gpu(points), gpu(offsets), 5))
    c_f, c_l = constants()
    # all of them against the restatement (vectorised over the contours of one length): the bound plus the reference's own
    # error, which is c / 4 by the definition of c.  Both location results carry the rounding of their own last addition
    # (first point + mean), the 2^-53 |truth| of the bound, so two such terms stand between them
    lengths = np.diff(offsets)
    checked = 0
    for n in np.unique(lengths).tolist():
        ks = np.nonzero(lengths == n)[0]
        batch = points[offsets[ks][:, None] + np.arange(n)[None]]
        closed = np.asarray([oracle.is_closed(b) for b in batch])
        for sel in (closed, ~closed):
            if not sel.any():
                continue
            rc, rl = oracle.efd(batch[sel], 5, 1e-6)
            pts = oracle.close(batch[sel])
            d = np.diff(pts, axis=-2)
            T = (np.sqrt((d * d).sum(-1)) + 1e-6).sum(-1)
            U = 2. ** -53 * d.shape[-2] * T
            ef = np.abs(coeff[ks[sel]] - rc).max((1, 2)) / U
            el = np.maximum(np.abs(loc[ks[sel]] - rl) - 2 * 2. ** -53 * np.abs(rl), 0).max(1) / U
            assert ef.max() <= c_f + c_f / 4 and el.max() <= c_l + c_l / 4, (n, ef.max(), el.max())
            checked += int(sel.sum())
    assert checked == K
    for k in oracle.tiny_sample().tolist():
        c = points[offsets[k]:offsets[k + 1]]
        within(coeff[k], loc[k], truths()[f'tiny{k}'], f'tiny contour {k}, {len(c)} points, order 5')


def test_errors_found_on_the_device():
    pts = gpu(oracle.ragged_walk(20, 1))
    for offsets in ([1, 20], [0, 19], [0, 12, 8, 20], [0, 8, 8, 20], [0, 25, 20], [0, -3, 20]):
        with pytest.raises(ValueError, match='offsets'):
            fo.efd_packed(pts, gpu(np.asarray(offsets, np.int64)), 5)
    with pytest.raises(ValueError, match='explicitly closed'):
        fo.efd_packed(pts, gpu(np.asarray([0, 20], np.int64)), 5, autoclose=False)
    with pytest.raises(ValueError, match='explicitly closed'):
        cda.efd(pts, 5, autoclose=False)
    closed = gpu(oracle.ragged_walk(20, 1, closed=True))
    a, b = cda.efd(closed, 5, autoclose=False), cda.efd(closed, 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ok = fo.efd_packed(pts, gpu(np.asarray([0, 20], np.int64)), 5)  # the library still works after the refusals
    assert torch.isfinite(ok[0]).all()


def test_labels2fourier():
    labels = disc_labels(67, 129, 40, 3, 5)
    dev = gpu(labels)
    kw = dict(raise_fragmented=False)
    ids, offsets, points = lc.labels2contours_packed(dev.clone(), **kw)
    i2, f, l = cda.labels2fourier(dev.clone(), order=5, dtype=torch.float64, **kw)
    assert torch.equal(i2, ids) and i2.dtype == torch.int32 and len(ids) > 10
    pc, pl = fo.efd_packed(points, offsets, 5)
    assert points.dtype == torch.int32 and torch.equal(f, pc) and torch.equal(l, pl)
    i3, f32, l32 = cda.labels2fourier(dev.clone(), **kw)
    assert f32.dtype == l32.dtype == torch.float32 and tuple(f32.shape) == (len(ids), 5, 4) and torch.equal(f32, pc.float())
    table = cda.contours2fourier(lc.labels2contours(dev.clone(), **kw), order=5, dtype=torch.float64)
    rows = ids.long() - 1
    assert tuple(table[0].shape) == (int(ids.max()), 5, 4) and torch.equal(table[0][rows], pc) and torch.equal(table[1][rows], pl)
    rest = torch.ones(int(ids.max()), dtype=torch.bool, device=DEV)
    rest[rows] = False
    assert not table[0][rest].any() and not table[1][rest].any()
    # a fragmented object: raised, flagged or skipped as labels2contours does
    frag = labels.copy()
    v = int(ids[0])
    frag[0, 0, 0], frag[0, 2, 0] = 1000, 1000
    with pytest.raises(ValueError, match='multiple connected components'):
        cda.labels2fourier(gpu(frag))
    skipped = cda.labels2fourier(gpu(frag), raise_fragmented=False)
    assert 1000 not in skipped[0].tolist() and v in skipped[0].tolist()
    work = gpu(frag)
    flagged = cda.labels2fourier(work, flag_fragmented_inplace=True, constant=-7)
    assert int((work == -7).sum()) == 2 and torch.equal(flagged[0], skipped[0]) and torch.equal(flagged[1], skipped[1])


def test_end_to_end_from_a_model():
    """model -> contours2labels -> flat -> labels2fourier(order = the model's) -> fouriers2contours -> contours2labels: shapes and
    dtypes are those of the model's entries; the F1 at IoU 0.5 of the decoded image against the flat image is printed and only
    asserted to be > 0 (orientation and (x, y) order); no accuracy is claimed."""
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
    fourier, locations = y['fourier'][0], y['locations'][0]
    order = int(fourier.shape[1])
    flat = cda.resolve_label_channels(cda.contours2labels(y['contours'][0], size))
    work = flat.clone()[..., None]
    ids, f, l = cda.labels2fourier(work, order=order, dtype=fourier.dtype, flag_fragmented_inplace=True)
    assert f.is_cuda and f.dtype == fourier.dtype and l.dtype == locations.dtype and len(ids) > 0
    assert tuple(f.shape) == (len(ids),) + tuple(fourier.shape[1:]) and tuple(l.shape) == (len(ids),) + tuple(locations.shape[1:])
    decoded, _ = cda.ops.fouriers2contours(f, l, samples=model.samples)
    again = cda.contours2labels(decoded, size)
    f1 = cda.LabelMatcher(cda.resolve_label_channels(again), work[..., 0].clamp(min=0), iou_thresh=.5).f1
    print(f'{len(ids)} objects at order {order}: F1 at IoU 0.5 of the decoded against the flat image = {f1:.3f}')
    assert f1 > 0
