"""Component labelling on the GPU (celldetection_amd.label_components / relabel_ / stack_labels / masks2labels / ...): every
comparison with the numpy restatement (``tests/components_oracle.py``), with the reference's fixture
(``tests/golden/components.npz``) and with closed forms is exact; there is no tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

import celldetection_amd as cda
import components_oracle as oracle
from celldetection_amd import _lib
from celldetection_amd._lib import ptr
from test_components import load_fixture, mask_cases, relabel_cases, stack_cases
from test_instance_eval import disc_labels

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
COMBOS = ((8, 'equal'), (4, 'equal'), (8, 'nonzero'), (4, 'nonzero'))
RANDOM_SIZES = ((1, 1, 1), (1, 9, 3), (9, 1, 2), (5, 7, 11), (31, 33, 4), (40, 64, 5), (64, 65, 3), (67, 129, 2))
EDGES = (31, 32, 33, 63, 64, 65)
BIG_H, BIG_W = 130, 257


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def check(a, conn, mode, what='', first=1):
    """label_components on the device copy of ``a`` (numpy [H, W, C]) against the oracle, out of place and in place."""
    a = np.asarray(a)
    exp, counts = oracle.label_components(a, conn, mode, first)
    t = dev(a)
    got, n = cda.label_components(t, conn, mode, first)
    assert got.is_cuda and n.is_cuda and got.dtype == t.dtype and n.dtype == torch.int32 and tuple(got.shape) == a.shape, what
    assert np.array_equal(t.cpu().numpy(), a), (what, 'the input changed')
    bad = int((got.cpu().numpy() != exp).sum())
    assert bad == 0 and n.cpu().tolist() == counts.tolist(), (what, conn, mode, f'{bad} pixels differ', n.cpu().tolist()[:8])
    same, n2 = cda.label_components(t, conn, mode, first, out=t)
    assert same is t and torch.equal(t, got) and torch.equal(n2, n), (what, 'in place')
    return exp, counts


def random_image(h, w, c, seed):
    """Blobs of a few values, zeros and negatives: many small components, values that recur, every kind of contact."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-1, 4, (h, w, c)).astype(np.int32)
    a[rng.random((h, w, c)) < .25] = 0
    return a


def test_fixture_cases_through_every_public_function():
    z = load_fixture()
    for name, a, want in relabel_cases(z):
        t = dev(a)
        assert cda.relabel_(t) is None and np.array_equal(t.cpu().numpy(), want), name
        cda.relabel_(t)  # of its own output: the identity
        assert np.array_equal(t.cpu().numpy(), want), name
        got, counts = cda.label_components(dev(a))
        assert np.array_equal(got.cpu().numpy(), want) and int(counts.sum()) == max(int(want.max()), 0), name
        out = torch.full(a.shape, -7, dtype=torch.int32, device=DEV)
        same, _ = cda.label_components(dev(a), out=out)
        assert same is out and np.array_equal(out.cpu().numpy(), want), name
        host = a.copy()
        cda.relabel_(host)  # a numpy array is uploaded, relabelled and written back
        assert np.array_equal(host, want), name
    for name, maps, kw, want in stack_cases(z):
        for up in (dev, lambda m: m):
            got = cda.stack_labels(*[up(m) for m in maps], **kw)
            assert got.is_cuda and got.dtype == getattr(torch, kw['dtype']) and np.array_equal(got.cpu().numpy(), want), name
    for dtype, key in (('int32', 'rgb.result'), ('int64', 'rgb.result_int64')):
        got = cda.rgb_to_scalar(dev(z['rgb.input']), dtype=dtype)
        assert got.dtype == getattr(torch, dtype) and np.array_equal(got.cpu().numpy(), z[key])
    for name, masks, kw, want, cnt in mask_cases(z):
        for up in (dev, lambda m: m, lambda m: [dev(x) for x in m], lambda m: dev(m).bool(), lambda m: dev(m).float() * .5):
            got, n = cda.masks2labels(up(masks), count=True, **kw)
            assert got.is_cuda and got.dtype == torch.int32 and n == cnt, name
            assert tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), name
        if kw['reduce']:
            assert torch.equal(cda.masks2labels(dev(masks), **dict(kw, reduce=np.max)), got), name
    for transpose, key in ((True, 'unary.transposed'), (False, 'unary.plain')):
        for up in (dev, lambda m: [dev(x) for x in m]):
            got = cda.unary_masks2labels(up(z['unary.masks']), transpose=transpose)
            assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), z[key])


@pytest.mark.parametrize('size', RANDOM_SIZES, ids=lambda s: 'x'.join(str(i) for i in s))
def test_random_images_against_the_oracle(size):
    h, w, c = size
    a = random_image(h, w, c, seed=h * 1000 + w + c)
    for conn, mode in COMBOS:
        _, counts = check(a, conn, mode, str(size))
    assert counts.sum() > 0 or h * w < 4


def test_every_size_around_the_tile_edges():
    """31 .. 33 and 63 .. 65 in each dimension: (8, 'equal') on every size, the other three rules in turn."""
    k = 0
    for h in EDGES:
        for w in EDGES:
            a = random_image(h, w, 1, seed=h * 100 + w)
            a[h // 2 - 2:h // 2 + 2, :, 0] = 2  # a bar across every vertical seam, and one along a horizontal seam
            a[:, min(w - 1, 32), 0] = np.where(np.arange(h) % 7 == 3, 0, 3)
            check(a, 8, 'equal', (h, w))
            check(a, *COMBOS[1 + k % 3], (h, w))
            k += 1


def patterns():
    """name -> int32 [130, 257]: shapes that cross many seams and tile corners."""
    H, W = BIG_H, BIG_W
    yy, xx = np.mgrid[:H, :W]
    out = {}
    s = np.zeros((H, W), np.int32)  # a serpentine: every second row, joined at alternating ends
    s[::2] = 5
    for i, y in enumerate(range(1, H, 2)):
        s[y, W - 1 if i % 2 == 0 else 0] = 5
    out['serpentine'] = s
    d = np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx))  # a spiral: every second ring, cut and joined to the next
    sp = np.where(d % 2 == 0, 4, 0).astype(np.int32)
    for k in range(0, d.max() - 1, 2):
        sp[k + 2, k + 1] = 4  # the bridge from ring k to ring k + 2 ...
        sp[k + 1, k] = 0      # ... and the cut of ring k above it
    out['spiral'] = sp
    c = np.zeros((H, W), np.int32)  # a comb: a spine in the last row, teeth in every second column
    c[:, ::2] = 7
    c[H - 1] = 7
    out['comb'] = c
    out['one_value'] = np.full((H, W), 2 ** 31 - 1, np.int32)
    g = np.zeros((H, W), np.int32)  # a diagonal through the tile corners (31, 31) -> (32, 32), ...
    n = min(H, W)
    g[np.arange(n), np.arange(n)] = 3
    out['diagonal'] = g
    out['stripes'] = ((yy + xx) // 2 % 2 + 1).astype(np.int32)  # diagonal stripes, two pixels wide, of two interleaved values
    r = np.where(np.maximum(np.abs(yy % 16 - 8), np.abs(xx % 16 - 8)) == 6, 9, 0).astype(np.int32)  # rings with islands
    r[(yy % 16 == 8) & (xx % 16 == 8)] = 9
    r[64:80, 128:144] = np.where(r[64:80, 128:144] > 0, 6, -1)
    out['rings'] = r
    return out


@pytest.mark.parametrize('name', ('serpentine', 'spiral', 'comb', 'one_value', 'diagonal', 'stripes', 'rings'))
def test_patterns_across_seams_and_corners(name):
    a = patterns()[name][:, :, None]
    _, c8 = check(a, 8, 'equal', name)
    _, c4 = check(a, 4, 'equal', name)
    want = dict(serpentine=(1, 1), comb=(1, 1), one_value=(1, 1), diagonal=(1, BIG_H), stripes=None, rings=None, spiral=(1, 1))[name]
    if want:
        assert (int(c8[0]), int(c4[0])) == want, name
    if name == 'stripes':
        assert int(c4[0]) == int(c8[0]) == (BIG_H + BIG_W - 2) // 2 + 1
        check(a, 4, 'nonzero', name)
    if name == 'rings':
        check(a, 8, 'nonzero', name)


def test_checkerboard_at_connectivity_4_ranks_inside_blocks():
    """Every block of 256 pixels is half roots: 16705 components, numbered along the raster (closed form, no oracle)."""
    yy, xx = np.mgrid[:BIG_H, :BIG_W]
    board = ((yy + xx) % 2 == 0)
    a = np.stack([board * 3, ~board * 5, board * -2], 2).astype(np.int32)
    n0, n1 = int(board.sum()), int((~board).sum())
    assert n0 == 16705
    exp = a.copy()
    exp[:, :, 0][board] = np.arange(1, n0 + 1)
    exp[:, :, 1][~board] = n0 + np.arange(1, n1 + 1)
    got, counts = cda.label_components(dev(a), connectivity=4)
    assert counts.tolist() == [n0, n1, 0] and np.array_equal(got.cpu().numpy(), exp)
    got, counts = cda.label_components(dev(a), connectivity=4, mode='nonzero', first=100)
    exp[:, :, 2][board] = 99 + n0 + n1 + np.arange(1, n0 + 1)
    exp[:, :, :2][a[:, :, :2] > 0] += 99
    assert counts.tolist() == [n0, n1, n0] and np.array_equal(got.cpu().numpy(), exp)
    got, counts = cda.label_components(dev(a), connectivity=8)
    assert counts.tolist() == [1, 1, 0] and np.array_equal(got.cpu().numpy()[:, :, :2], np.stack([board * 1, ~board * 2], 2))


def test_mask_stacks_are_read_through_strides():
    rng = np.random.default_rng(8)
    masks = (rng.random((7, 45, 70)) < .4).astype(np.uint8) * rng.integers(1, 255, (7, 45, 70)).astype(np.uint8)
    masks[2], masks[4] = 0, 200
    for conn in (8, 4):
        for kw in (dict(), dict(reduce=None), dict(label_axis=0, reduce=None), dict(label_axis=1, keepdims=False)):
            want, cnt = oracle.masks2labels(masks, conn, count=True, **dict(kw, reduce=None if 'reduce' in kw else np.max))
            got, n = cda.masks2labels(dev(masks), conn, count=True, **kw)
            assert n == cnt and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), (conn, kw)
    # the C ABI itself: a planar [N][H][W] input and a channel-interleaved [H][W][N] output, no transposing copy
    N, H, W = masks.shape
    x = dev(masks, torch.int32)
    out = torch.empty((H, W, N), dtype=torch.int32, device=DEV)
    counts = torch.empty((N,), dtype=torch.int32, device=DEV)
    lib = _lib.load()
    ws = torch.empty((int(lib.cpn_components_workspace_bytes(N, H, W)),), dtype=torch.uint8, device=DEV)
    _lib.check(lib.cpn_components_label(ptr(x), 1, H * W, N, H, W, 8, _lib.COMPONENTS_NONZERO, 1, ptr(out), N, 1, ptr(counts), ptr(ws),
                                        _lib.stream_ptr()), 'components_label')
    exp, n = oracle.label_components(masks.transpose(1, 2, 0).astype(np.int32), 8, 'nonzero', 1)
    assert np.array_equal(out.cpu().numpy(), exp) and counts.tolist() == n.tolist()
    assert np.array_equal(x.cpu().numpy(), masks)


def test_first_large_values_dtypes_and_overflow():
    a = random_image(40, 50, 3, seed=77)
    check(a, 8, 'equal', 'first', first=1000)
    big = np.where(a > 0, 2 ** 31 - 1 - a, a).astype(np.int32)  # values near 2^31 - 1 link like any other
    exp, counts = check(big, 8, 'equal', 'large values')
    assert np.array_equal(exp, oracle.label_components(a, 8, 'equal', 1)[0])
    total = int(counts.sum())
    check(a, 8, 'equal', 'first at the top', first=2 ** 31 - total)  # the last label is 2^31 - 1
    t = dev(a)
    with pytest.raises(RuntimeError, match='does not fit int32'):
        cda.label_components(t, first=2 ** 31 - total + 1, out=t)
    assert np.array_equal(t.cpu().numpy(), a)  # nothing was written
    # five integer dtypes in place
    small = np.where(a[:12, :12] > 0, a[:12, :12], 0).astype(np.int32)
    small[small == 1] = -1
    want = oracle.relabel(small)
    assert 0 < want.max() <= 127
    for dt in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
        src = np.where(small < 0, 0, small) if dt == torch.uint8 else small
        t = dev(src, dt)
        cda.relabel_(t)
        assert t.dtype == dt and np.array_equal(t.cpu().numpy().astype(np.int64), oracle.relabel(src)), dt
    t = dev(a, torch.int8)
    with pytest.raises(ValueError, match='does not fit torch.int8'):
        cda.relabel_(t)
    assert np.array_equal(t.cpu().numpy(), a)
    v = dev(a, torch.int64)
    v[0, 0, 0] = 2 ** 31
    with pytest.raises(ValueError, match='int32'):
        cda.relabel_(v)
    # a view that is not contiguous is relabelled through a copy and written back
    pad = torch.zeros((40, 51, 4), dtype=torch.int32, device=DEV)
    pad[:, 1:, 1:] = dev(a)
    view = pad[:, 1:, 1:]
    cda.relabel_(view)
    assert np.array_equal(view.cpu().numpy(), oracle.relabel(a)) and int(pad[:, 0].abs().sum()) == 0


def test_two_runs_are_bit_identical():
    a = dev(disc_labels(512, 768, 1500, 3, seed=5, rmax=14.) % 17)
    r1, c1 = cda.label_components(a, 8)
    r2, c2 = cda.label_components(a, 8)
    assert torch.equal(r1, r2) and torch.equal(c1, c2) and int(c1.sum()) > 500
    r3, c3 = cda.label_components(a, 4, 'nonzero')
    r4, c4 = cda.label_components(a, 4, 'nonzero')
    assert torch.equal(r3, r4) and torch.equal(c3, c4) and not torch.equal(r1, r3)


def test_single_pixels_on_2048_squared_closed_form():
    """2048 x 2048 x 5, single pixels of one value at (3i + 1, 3j + 1): label c * n + i * cols + j + 1.  More than 80000 blocks of
    256 pixels and the scan across them; the expected image is built on the device."""
    H = W = 2048
    C = 5
    rows = cols = (H - 2) // 3 + 1
    n = rows * cols
    a = torch.zeros((H, W, C), dtype=torch.int32, device=DEV)
    a[1::3, 1::3] = 7
    assert a[1::3, 1::3].shape[:2] == (rows, cols) and H * W * C // 256 > 80000
    exp = torch.zeros_like(a)
    ij = torch.arange(n, dtype=torch.int32, device=DEV).reshape(rows, cols, 1) + 1
    exp[1::3, 1::3] = ij + torch.arange(C, dtype=torch.int32, device=DEV) * n
    for conn in (8, 4):
        got, counts = cda.label_components(a, conn)
        assert counts.tolist() == [n] * C and torch.equal(got, exp), conn
    cda.relabel_(a)
    assert torch.equal(a, exp)


def test_fill_label_gaps_and_remove_partials():
    a = disc_labels(60, 70, 30, 2, seed=9, rmax=8.) * 3
    a[5:8, 30:40, 1] = -4
    t = dev(a)
    assert cda.fill_label_gaps_(t) is t
    got = t.cpu().numpy()
    u = np.unique(a[a > 0])
    assert np.array_equal(np.unique(got[got > 0]), np.arange(1, len(u) + 1)) and oracle.same_partition(got, a)
    assert np.array_equal(got[a <= 0], a[a <= 0])
    keep = u[u <= len(u)]
    assert all(np.array_equal(got == v, a == v) for v in keep.tolist())  # labels <= n stay
    for border, constant in ((1, -1), (3, -9)):
        t = dev(a)
        same, mask = cda.remove_partials_(t, border=border, constant=constant)
        bad = set(np.unique(a[:, :border])) | set(np.unique(a[:, -border:])) | set(np.unique(a[:border])) | set(np.unique(a[-border:]))
        want_mask = np.isin(a, list(bad - {0}))
        want = a.copy()
        want[want_mask] = constant
        assert same is t and mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), want_mask)
        assert want_mask.any() and np.array_equal(t.cpu().numpy(), want)
    t = dev(a)
    assert cda.remove_partials_(t, border=0) == (t, None) and np.array_equal(t.cpu().numpy(), a)


def test_relabel_makes_resolved_labels_traceable():
    """model -> contours2labels -> resolve_label_channels -> relabel_ -> labels2contours(raise_fragmented=True): no object is
    fragmented any more, there is one contour per component, and the image matches itself."""
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
    flat = cda.resolve_label_channels(labels)[..., None].contiguous()
    before = flat.clone()
    cda.relabel_(flat)
    total = int(flat.max())
    assert total > 0 and torch.equal(flat > 0, before > 0)
    contours = cda.labels2contours(flat, raise_fragmented=True)  # does not raise
    assert len(contours) == total == len(torch.unique(flat[flat > 0]))
    same = cda.LabelMatcher(flat[:, :, 0], flat[:, :, 0], iou_thresh=.5)
    assert same.true_positives == total and same.false_positives == 0 and same.false_negatives == 0 and abs(same.f1 - 1.) < 1e-9
    assert np.array_equal(flat.cpu().numpy(), oracle.relabel(before.cpu().numpy()))
    print(f'{tuple(labels.shape)}: {len(torch.unique(before[before > 0]))} resolved labels -> {total} components')
