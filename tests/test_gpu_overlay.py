"""Overlay images on the MI355X: celldetection_amd.contours2overlay and label_cmap against the reference's recorded results
(tests/golden/overlay.npz) and against the numpy restatement of tests/overlay_oracle.py, which the CPU tests pin to that
fixture.  Everything is exact: integers, and one float32 expression with a fixed order; no tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

import celldetection_amd as cda
import overlay_oracle as oracle
from celldetection_amd.overlay import TILE
from test_overlay import load_cmap_fixture, load_overlay_fixture

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SIZES = ((1, 1), (1, 7), (33, 65), (67, 129), (130, 257))  # partial tiles next to full ones for 32 and for 64 pixel tiles


def blobs(rng, n, size, s=24, spread=10., rmin=3., rmax=12., centres=None):
    """n closed contours as float32 [n, s, 2] (xy, fractional coordinates) around centres that also lie outside the image."""
    H, W = size
    out = np.zeros((n, s, 2), np.float32)
    for i in range(n):
        cx, cy = (rng.uniform(-spread, W + spread), rng.uniform(-spread, H + spread)) if centres is None else centres[i]
        t = np.linspace(0, 2 * np.pi, s, endpoint=False) + rng.uniform(0, 1)
        r = rng.uniform(rmin, rmax) * (1 + .25 * np.sin(3 * t + rng.uniform(0, 6)))
        out[i] = np.stack((cx + 1.3 * r * np.cos(t), cy + r * np.sin(t)), 1)
    return out


def colours(rng, k):
    return rng.integers(0, 256, (k, 3)).astype(np.uint8)


def check_overlay(contours, size, colors, what='', **kw):
    """cda.contours2overlay on the device copy of ``contours`` (numpy [K, S, 2]) against the oracle, stats included."""
    okw = {k: v for k, v in kw.items() if k != 'intermediate_dtype'}  # the oracle's sums do not overflow
    exp, n = oracle.contours2overlay(contours, size, colors, return_count=True, **okw)
    out, col, st = cda.contours2overlay(torch.as_tensor(contours).to(DEV), size, colors=colors, return_colors=True,
                                        return_stats=True, **kw)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == tuple(size) + (4,) and out.is_contiguous(), what
    bad = int((out.cpu().numpy() != exp).any(-1).sum())
    assert bad == 0, (what, f'{bad} pixels differ')
    assert col.is_cuda and np.array_equal(col.cpu().numpy(), colors), what
    assert st['max_overlap'] == int(n.max()) and st['tiles'] == -(-size[0] // TILE) * -(-size[1] // TILE), (what, st)
    return st, n


def test_fixture_cases_equal_the_reference():
    for name, contours, size, kw, colors, ref in load_overlay_fixture():
        out = cda.contours2overlay(contours, size, colors=colors if len(colors) else None, **kw)  # a list of arrays, or None
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == ref.shape, name
        assert np.array_equal(out.cpu().numpy(), ref), name
        if contours is not None:
            con = torch.as_tensor(oracle.pad_contours(contours)).to(DEV)
            out = cda.contours2overlay(con, size, colors=torch.as_tensor(colors).to(DEV), processes=8, **kw)
            assert np.array_equal(out.cpu().numpy(), ref), name
    for name, a, colors, cname, alpha, ref in load_cmap_fixture():
        x = torch.as_tensor(a).to(DEV)
        out = cda.label_cmap(x, colors=colors, alpha=alpha, ubyte=True)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == ref.shape, name
        assert np.array_equal(out.cpu().numpy(), ref), name
        if cname not in ('', 'rand'):  # the matplotlib map by its name
            assert np.array_equal(cda.label_cmap(x, colors=cname, alpha=alpha, ubyte=True).cpu().numpy(), ref), name
        if a.ndim == 3:
            assert np.array_equal(cda.label_cmap(x, colors=colors, alpha=alpha, reduce_axis=-1, ubyte=True).cpu().numpy(), ref), name


@pytest.mark.parametrize('size', SIZES)
def test_overlay_sizes_against_the_oracle(size):
    rng = np.random.default_rng(size[0] * 1000 + size[1])
    k = max(size[0] * size[1] // 120, 3)
    con = blobs(rng, k, size)
    st, n = check_overlay(con, size, colours(rng, k), f'{size}')
    if size[0] > 32:
        assert n.max() >= 3 and st['pairs'] > k, (size, st)  # overlaps, and contours that span several tiles
    check_overlay(con, size, colours(rng, k), f'{size} unrounded', rounded=False)


def test_overlay_edge_cases():
    rng = np.random.default_rng(5)
    size = (33, 65)
    # K = 0 and contours=None: zeros
    for con in (torch.zeros((0, 8, 2), device=DEV), None, []):
        out, col, st = cda.contours2overlay(con, size, return_colors=True, return_stats=True)
        assert out.is_cuda and tuple(out.shape) == size + (4,) and out.dtype == torch.uint8 and not bool(out.any())
        assert tuple(col.shape) == (0, 3) and st == dict(max_overlap=0, pairs=0, tiles=6)
    # S = 1, 2, 3: a point, a line, a triangle; S = 512: the maximum
    for s in (1, 2, 3):
        con = blobs(rng, 9, size, s=s)
        _, n = check_overlay(con, size, colours(rng, 9), f'S = {s}')
        assert n.any()
    con = blobs(rng, 3, (67, 129), s=512, rmin=10., rmax=30.)
    check_overlay(con, (67, 129), colours(rng, 3), 'S = 512')
    with pytest.raises(RuntimeError, match='512'):
        cda.contours2overlay(torch.zeros((1, 513, 2), device=DEV), size)
    # wholly outside: clipped onto a border line and onto a corner
    con = np.array([[[-30, 5], [-12, 9], [-20, 25]], [[70, 40], [90, 50], [80, 60]], [[10, -9], [30, -4], [20, -20]]], np.float32)
    _, n = check_overlay(con, size, colours(rng, 3), 'outside')
    assert n[5:26, 0].all() and n[32, 64] == 1 and n[0, 10:31].all() and n.sum() == 21 + 1 + 21
    # clip=False: inside is fine, outside raises, as contours2labels does
    inside = blobs(rng, 6, size, spread=0., rmin=2., rmax=4., centres=[(12 + 8 * i, 16) for i in range(6)])
    check_overlay(inside, size, colours(rng, 6), 'clip=False', clip=False)
    for bad in (con[:1], con[1:2]):
        with pytest.raises(ValueError, match='clip=True'):
            cda.contours2overlay(torch.as_tensor(bad).to(DEV), size, clip=False)
    with pytest.raises(ValueError, match='zero-length'):
        cda.contours2overlay(torch.zeros((2, 0, 2), device=DEV), size)
    with pytest.raises(ValueError, match=r'uint8 \[6, 3\]'):
        cda.contours2overlay(torch.as_tensor(inside).to(DEV), size, colors=np.zeros((5, 3), np.uint8))
    # default colours: one vectorised draw on the host, fixed by np.random.seed
    np.random.seed(4)
    o1, c1 = cda.contours2overlay(torch.as_tensor(inside).to(DEV), size, return_colors=True)
    np.random.seed(4)
    exp = cda.random_colors_hsv(6, ubyte=True)
    assert np.array_equal(c1.cpu().numpy(), exp) and np.array_equal(o1.cpu().numpy(), oracle.contours2overlay(inside, size, exp))
    c2 = cda.contours2overlay(torch.as_tensor(inside).to(DEV), size, hue_range=(60, 61), saturation_range=(255, 256),
                              return_colors=True)[1].cpu().numpy()
    assert (c2[:, 0] == 0).all() and (c2[:, 2] == 0).all() and (c2[:, 1] >= 180).all()


def test_overlay_many_tiles_per_contour_and_many_contours_per_tile():
    rng = np.random.default_rng(6)
    size = (130, 257)
    big = np.array([[[2, 1], [254, 3], [255, 127], [128, 129], [1, 126]]], np.float32)  # nearly the whole image: 8 x 5 tiles
    big = oracle.pad_contours(list(big) + list(blobs(rng, 60, size, rmin=2., rmax=6.)))
    st, n = check_overlay(big, size, colours(rng, 61), 'big + 60 small')
    assert st['pairs'] >= 40 + 60 and n.max() >= 2 and (n > 0).mean() > .9
    # 400 small contours inside ONE tile: the list is walked in chunks
    centres = [(40 + rng.uniform(0, 14), 38 + rng.uniform(0, 18)) for _ in range(400)]
    small = blobs(rng, 400, (67, 129), s=12, rmin=1.5, rmax=4., centres=centres)
    assert small[..., 0].min() > 32.5 and small[..., 0].max() < 63.4 and small[..., 1].min() > 32.5 and small[..., 1].max() < 63.4
    st, n = check_overlay(small, (67, 129), colours(rng, 400), '400 in one tile', intermediate_dtype='uint32')
    assert st['pairs'] == 400 and n.max() > 20


def test_overlay_overflow_limit():
    """Identical contours on 16 x 16: the reference's uint16 sums hold 257 of them (257 * 255 = 65535), not 258."""
    square = np.array([[3, 2], [12, 2], [12, 11], [3, 11]], np.float32)
    rng = np.random.default_rng(8)

    def run(k, dtype):
        con = torch.as_tensor(np.repeat(square[None], k, 0)).to(DEV)
        col = colours(rng, k)
        col[0] = 255
        out, st = cda.contours2overlay(con, (16, 16), colors=col, intermediate_dtype=dtype, return_stats=True)
        assert st['max_overlap'] == k
        mean = col.astype(np.int64).sum(0) // k
        assert out[5, 5].tolist() == mean.tolist() + [255] and out[0, 0].tolist() == [0, 0, 0, 0]

    run(257, 'uint16')
    with pytest.raises(ValueError, match='258 contours overlap'):
        run(258, 'uint16')
    run(258, 'uint32')
    run(1, 'uint8')
    with pytest.raises(ValueError, match='2 contours overlap'):
        run(2, 'uint8')
    with pytest.raises(NotImplementedError, match='intermediate_dtype'):
        run(2, 'float32')
    with pytest.raises(NotImplementedError, match='thickness'):
        cda.contours2overlay(torch.as_tensor(square[None]).to(DEV), (16, 16), thickness=1)


def test_two_calls_give_identical_bytes_and_torch_ops():
    rng = np.random.default_rng(9)
    size = (130, 257)
    con = torch.as_tensor(blobs(rng, 300, size)).to(DEV)
    col = torch.as_tensor(colours(rng, 300)).to(DEV)
    r1, s1 = cda.contours2overlay(con, size, colors=col, return_stats=True)
    r2, s2 = cda.contours2overlay(con, size, colors=col, return_stats=True)
    assert s1 == s2 and s1['max_overlap'] >= 4 and torch.equal(r1, r2)
    import celldetection_amd.torch_ops  # noqa: F401  (registers the ops)
    assert torch.equal(torch.ops.celldetection_amd.contours2overlay(con, col, size[0], size[1]), r1)
    lab = torch.as_tensor(rng.integers(0, 50, size + (3,)).astype(np.int32)).to(DEV)
    table = torch.as_tensor(rng.random((13, 3)))
    m1 = cda.label_cmap(lab, colors=table, ubyte=True)
    assert torch.equal(cda.label_cmap(lab, colors=table, ubyte=True), m1)
    assert torch.equal(torch.ops.celldetection_amd.label_cmap(lab, table.to(DEV)), m1)
    assert np.array_equal(m1.cpu().numpy(), oracle.label_cmap(lab.cpu().numpy(), table.numpy()))


@pytest.mark.parametrize('size', SIZES)
def test_label_cmap_sizes_channels_and_dtypes(size):
    rng = np.random.default_rng(size[0] * 7 + size[1])
    colors = rng.random((23, 3))
    for c in range(1, 12):
        a = rng.integers(1, 300, size + (c,)).astype(np.int32)
        a[rng.random(a.shape) < .5] = 0
        a[0, 0] = 299  # every channel occupied
        alpha = (None, .5, .3)[c % 3]
        exp = oracle.label_cmap(a, colors, alpha)
        for dt in (torch.int32, torch.int64, torch.uint8) if c in (1, 3, 11) else (torch.int32,):
            x = a % 256 if dt == torch.uint8 else a
            e = oracle.label_cmap(x, colors, alpha) if dt == torch.uint8 else exp
            out = cda.label_cmap(torch.as_tensor(x).to(DEV).to(dt), colors=colors, alpha=alpha, ubyte=True)
            assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == size + (4,) and out.is_contiguous()
            bad = int((out.cpu().numpy() != e).any(-1).sum())
            assert bad == 0, (size, c, dt, f'{bad} pixels differ')
    flat = rng.integers(0, 300, size).astype(np.int32)
    out = cda.label_cmap(torch.as_tensor(flat).to(DEV), colors=colors, ubyte=True, reduce_axis=None)
    assert np.array_equal(out.cpu().numpy(), oracle.label_cmap(flat, colors))
    # a view that is not contiguous
    wide = torch.as_tensor(rng.integers(0, 300, size + (4,)).astype(np.int32)).to(DEV)
    view = wide[:, :, 1:3]
    assert not view.is_contiguous() or size == (1, 1)
    assert np.array_equal(cda.label_cmap(view, colors=colors, ubyte=True).cpu().numpy(), oracle.label_cmap(view.cpu().numpy(), colors))


def test_label_cmap_negative_labels_and_random_colours():
    rng = np.random.default_rng(12)
    a = rng.integers(0, 40, (33, 65, 2)).astype(np.int32)
    a[20, 30, 1] = -1
    for x in (a, a[:, :, 1], a.astype(np.int64)):
        with pytest.raises(ValueError, match='negative'):
            cda.label_cmap(torch.as_tensor(x).to(DEV), ubyte=True)
    big = torch.as_tensor(a).to(DEV).to(torch.int64).abs()
    big[0, 0, 0] = 2 ** 31
    with pytest.raises(ValueError, match='int32'):
        cda.label_cmap(big, ubyte=True)
    # 'rand': min(9999, max) colours.  Beyond 9999 labels the colours repeat: v and v + 9999 share one
    lab = np.zeros((8, 16), np.int32)
    lab[0, :4] = (5, 5 + 9999, 20000, 20000 - 9999)
    lab[1, :3] = (1, 9999, 9999 + 9999)
    out = cda.label_cmap(torch.as_tensor(lab).to(DEV), ubyte=True).cpu().numpy()
    assert out[0, 0].tolist() == out[0, 1].tolist() and out[0, 2].tolist() == out[0, 3].tolist()
    assert out[1, 1].tolist() == out[1, 2].tolist() and out[0, 0, 3] == 255 and not out[2:].any()
    # the table is exactly the draw of n = min(9999, max) colours
    for top in (7, 9999, 12345):
        lab = rng.integers(0, top + 1, (20, 30, 3)).astype(np.int32)
        lab[0, 0, 0] = top
        np.random.seed(top)
        out = cda.label_cmap(torch.as_tensor(lab).to(DEV), alpha=.5, ubyte=True).cpu().numpy()
        np.random.seed(top)
        colors = cda.random_colors_hsv(min(9999, top))
        assert np.array_equal(out, oracle.label_cmap(lab, colors, .5)), top
    # a table too large for LDS is read through the cache
    colors = rng.random((20000, 4))
    lab = rng.integers(0, 60000, (33, 65, 3)).astype(np.int32)
    out = cda.label_cmap(torch.as_tensor(lab).to(DEV), colors=colors, ubyte=True).cpu().numpy()
    assert np.array_equal(out, oracle.label_cmap(lab, colors))


def test_end_to_end_on_device_tensors():
    """model -> contours2labels -> label_cmap, and model -> contours2overlay: device tensors all the way."""
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
    labels = cda.contours2labels(contours, size)
    np.random.seed(2)
    cmap = cda.label_cmap(labels, ubyte=True)
    np.random.seed(2)
    table = cda.random_colors_hsv(max(1, min(9999, int(labels.max()))))  # the draw of colors='rand'
    assert cmap.is_cuda and cmap.dtype == torch.uint8 and tuple(cmap.shape) == size + (4,)
    assert np.array_equal(cmap.cpu().numpy(), oracle.label_cmap(labels.cpu().numpy(), table))
    single = (labels != 0).sum(-1) == 1
    assert bool(single.any()) and bool((cmap[..., 3][single] == 255).all())  # one label on the pixel: weight exactly 1
    assert bool((cmap[(labels == 0).all(-1)] == 0).all())
    np.random.seed(1)
    overlay, colors, st = cda.contours2overlay(contours, size, return_colors=True, return_stats=True)
    assert overlay.is_cuda and overlay.dtype == torch.uint8 and tuple(overlay.shape) == size + (4,)
    exp, n = oracle.contours2overlay(contours.cpu().numpy(), size, colors.cpu().numpy(), return_count=True)
    assert np.array_equal(overlay.cpu().numpy()[..., 3], np.where(n > 0, 255, 0)) and st['max_overlap'] == n.max()
    assert np.array_equal(overlay.cpu().numpy(), exp)
    assert torch.equal(overlay[..., 3] == 255, (labels != 0).any(-1))  # both rasterise the same polygons
    print(f'{tuple(contours.shape)} contours on {size}: {st}')


def test_overlay_allocates_no_full_image_intermediate():
    """2048 x 2048, about 2000 contours: beyond the inputs the call may hold 1.5 x the 4 B per pixel of the output plus 16 MiB
    (the lists and the integer points).  The reference's 10 B per pixel, or a 16 B per pixel sum image, would not pass."""
    H = W = 2048
    rng = np.random.default_rng(13)
    con = torch.as_tensor(blobs(rng, 2000, (H, W), s=32, rmin=8., rmax=20.)).to(DEV)
    col = torch.as_tensor(colours(rng, 2000)).to(DEV)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out, st = cda.contours2overlay(con, (H, W), colors=col, return_stats=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f'peak {peak / 2 ** 20:.1f} MiB over the inputs, output {out.numel() / 2 ** 20:.1f} MiB, {st}')
    assert peak <= 1.5 * 4 * H * W + 16 * 2 ** 20
    assert st['max_overlap'] >= 2 and st['tiles'] == 4096 and st['pairs'] > 2000
    covered = int((out[..., 3] == 255).sum())
    assert 2000 * 150 < covered < 2000 * 2000 and bool(((out[..., 3] == 0) | (out[..., 3] == 255)).all())
    # a window of it against the oracle (the contours that touch the window)
    c = con.cpu().numpy()
    near = ((c[..., 0].max(1) >= 960) & (c[..., 0].min(1) < 1120) & (c[..., 1].max(1) >= 960) & (c[..., 1].min(1) < 1120))
    exp = oracle.contours2overlay(c[near] - 960, (160, 160), col.cpu().numpy()[near], clip=False)
    assert near.sum() > 5 and np.array_equal(out[976:1104, 976:1104].cpu().numpy(), exp[16:144, 16:144])
