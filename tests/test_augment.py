"""The augmentation warp without a GPU: the numpy statement of the rule (``tests/augment_oracle.py``) against numpy's own
rot90 / flip / transpose / slicing (exact) and against torch's float64 CPU ``grid_sample(align_corners=True)`` (nearest exact,
bilinear within the bound the oracle file derives from the roundings of the formula); the host side of ``cda.augment`` (maps,
tables, the random draw, every argument error); and the surface (header, build list, binding, ``__all__``)."""
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_oracle as oracle
import celldetection_amd as cda
from celldetection_amd import _header, _lib, build

aug = cda.augment
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 37, 53  # a non-square source
SPECIAL = (-1, 0, 2 ** 24 + 1, 2 ** 31 - 1)
DIHEDRAL = tuple(itertools.product((0, 1, 2, 3), (False, True)))  # (rot90, transpose): the eight; the flips repeat them


def source(K, C=2, seed=0, h=H, w=W, dtype=np.uint8):
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (h, w, K)).astype(np.uint8) if dtype == np.uint8 else \
        rng.uniform(-3, 3, (h, w, K)).astype(np.float32)
    labels = rng.integers(-2 ** 31, 2 ** 31 - 1, (h, w, C)).astype(np.int32)
    flat = labels.reshape(-1)
    flat[rng.choice(flat.size, 4 * len(SPECIAL), replace=False)] = np.tile(np.array(SPECIAL, dtype=np.int32), 4)
    return image, labels


def numpy_dihedral(a, rot90, transpose, flip_h, flip_v):
    """[H, W, ...] -> flip_v(flip_h(rot90^k(transpose(a)))) with numpy's own functions."""
    if transpose:
        a = np.swapaxes(a, 0, 1)
    a = np.rot90(a, rot90, axes=(0, 1))
    if flip_h:
        a = np.flip(a, 1)
    if flip_v:
        a = np.flip(a, 0)
    return np.ascontiguousarray(a)


def oblique_maps(h, w, src=(H, W)):
    """A few oblique maps whose nearest coordinates stay clear of the half-integers (asserted where they are used)."""
    return [aug.affine_map(src, (h, w), angle=27., scale=1 / 1.3),
            aug.affine_map(src, (h, w), angle=-63.5, scale=1.7, shear=11., translate=(3.25, -2.5)),
            aug.affine_map(src, (h, w), rot90=1, flip_h=True, angle=8.1, scale=.61, translate=(-7.3, 4.9))]


def torch_grid_sample(t, m, size, mode, padding_mode):
    """float64 [H, W, K] through torch's CPU grid_sample(align_corners=True) at the positions of the map -> float64 [K, h, w]."""
    hs, ws = t.shape[:2]
    sx, sy = oracle.positions(m, size)
    grid = torch.from_numpy(np.stack([2 * sx / (ws - 1) - 1, 2 * sy / (hs - 1) - 1], axis=-1))[None]
    x = torch.from_numpy(np.ascontiguousarray(t.transpose(2, 0, 1)))[None]
    return F.grid_sample(x, grid, mode=mode, padding_mode=padding_mode, align_corners=True)[0].numpy()


@pytest.mark.parametrize('K', (1, 3, 4))
def test_oracle_reproduces_numpy_dihedral_maps_and_crops_exactly(K):
    image, labels = source(K)
    assert all((labels == v).any() for v in SPECIAL)
    for rot90, transpose in DIHEDRAL:
        for flip_h, flip_v in ((False, False), (True, False), (False, True)):
            want_l = numpy_dihedral(labels, rot90, transpose, flip_h, flip_v)
            want_i = numpy_dihedral(image, rot90, transpose, flip_h, flip_v).astype(np.float32).transpose(2, 0, 1)
            size = want_l.shape[:2]
            m = aug.affine_map((H, W), size, rot90=rot90, transpose=transpose, flip_h=flip_h, flip_v=flip_v)
            for border in ('constant', 'reflect'):
                got_l = oracle.warp_labels(labels, m, size, border, fill=7)
                got_i = oracle.warp_image(image, m, size, None, border, fill=-5.)
                assert got_l.dtype == np.int32 and np.array_equal(got_l, want_l), (rot90, transpose, flip_h, flip_v, border)
                assert got_i.dtype == np.float32 and np.array_equal(got_i, want_i), (rot90, transpose, flip_h, flip_v, border)
    m = aug.crop_map(5, 11)
    assert np.array_equal(oracle.warp_labels(labels, m, (20, 30)), labels[5:25, 11:41])
    assert np.array_equal(oracle.warp_image(image, m, (20, 30)), image[5:25, 11:41].astype(np.float32).transpose(2, 0, 1))


@pytest.mark.parametrize('border, padding_mode', (('constant', 'zeros'), ('reflect', 'reflection')))
def test_oracle_against_torch_grid_sample_in_float64(border, padding_mode):
    """torch's align_corners=True convention is this rule's: nearest exact, bilinear within the derived bound."""
    image, labels = source(3)
    small = (labels & 0xfffff).astype(np.int32)  # float64 holds any int32; this only keeps the printed numbers short
    tables = aug.intensity_table(3, scale=1.)  # T[v] = v: max |T| = 255
    bound = oracle.bilinear_bound(255.)
    shares, outside = [], 0
    for size in ((41, 47), (64, 29)):
        for m in oblique_maps(*size):
            sx, sy = oracle.positions(m, size)
            for s in (sx, sy):  # there torch rounds halves to even and this rule rounds them up: the maps avoid them
                assert np.abs((s + 0.5) - np.round(s + 0.5)).min() > 1e-9
            outside += int(((sx < -1) | (sx > W) | (sy < -1) | (sy > H)).sum())
            assert ((sx > 0) & (sx < W - 1) & (sy > 0) & (sy < H - 1)).any()
            got_l = oracle.warp_labels(small, m, size, border, fill=0)
            want_l = torch_grid_sample(small.astype(np.float64), m, size, 'nearest', padding_mode)
            assert np.array_equal(got_l.transpose(2, 0, 1).astype(np.float64), want_l)
            got = oracle.warp_image(image, m, size, tables, border, fill=0.)
            truth = oracle.truth(image, m, size, tables, border, fill=0.)
            want = torch_grid_sample(image.astype(np.float64), m, size, 'bilinear', padding_mode)
            assert np.abs(truth - want).max() < 1e-9  # two float64 statements of one convention
            err = np.abs(got.astype(np.float64) - want).max()
            shares.append(err / bound)
            assert err <= bound, (err, bound)
    print(f'bilinear, {border}: largest error {max(shares) * bound:.3e} = {max(shares):.2f} of the bound {bound:.3e}')
    assert max(shares) > 0.01 and outside > 500  # the bound is of the error's order, not a blanket; the border took part


def test_oracle_intensity_is_table_then_blend_and_float_images_scale_then_offset():
    image, _ = source(3)
    tables = aug.intensity_table(3, gamma=(.7, 1., 1.6), contrast=1.2, brightness=-.1, mean=(.4, .5, .6), std=.25)
    m = oblique_maps(33, 31)[0]
    got = oracle.warp_image(image, m, (33, 31), tables, 'reflect')
    truth = oracle.truth(image, m, (33, 31), tables, 'reflect')
    assert np.abs(got - truth).max() <= oracle.bilinear_bound(np.abs(tables).max())
    want = torch_grid_sample(np.stack([tables[k].astype(np.float64)[image[:, :, k]] for k in range(3)], axis=2), m, (33, 31),
                             'bilinear', 'reflection')
    assert np.abs(truth - want).max() < 1e-9
    fimage, _ = source(2, dtype=np.float32)
    so = aug.intensity_scale_offset(2, contrast=(1.5, .5), brightness=.25, mean=.1, std=(2., 4.))
    t = oracle.mapped(fimage, so)
    assert t.dtype == np.float32 and np.array_equal(t, (fimage * so[:, 0]).astype(np.float32) + so[:, 1])
    got = oracle.warp_image(fimage, m, (33, 31), so, 'constant', fill=1.5)
    assert np.abs(got - oracle.truth(fimage, m, (33, 31), so, 'constant', fill=1.5)).max() <= oracle.bilinear_bound(np.abs(t).max())
    assert np.array_equal(oracle.bf16_round(got), torch.from_numpy(got).to(torch.bfloat16).float().numpy())


def test_oracle_borders_halves_and_size_one():
    lab = np.arange(1, 6, dtype=np.int32).reshape(1, 5, 1)
    # reflect-101 several periods out: ... 3 2 | 1 2 3 4 5 | 4 3 2 1 2 ...
    m = aug.crop_map(0, -10)
    assert oracle.warp_labels(lab, m, (1, 26), 'reflect')[0, :, 0].tolist() == [3, 2, 1, 2, 3, 4, 5, 4, 3, 2, 1, 2, 3, 4, 5, 4, 3, 2, 1, 2,
                                                                                3, 4, 5, 4, 3, 2]
    assert oracle.warp_labels(lab, m, (1, 26), 'constant', fill=-9)[0, :, 0].tolist() == [-9] * 10 + [1, 2, 3, 4, 5] + [-9] * 11
    # exactly on -0.5 and on W - 0.5: halves round up, so -0.5 is pixel 0 and W - 0.5 is outside
    for x, want in ((-.5, 1), (-.5000001, -9), (4.4999, 5), (4.5, -9)):
        assert int(oracle.warp_labels(lab, aug.crop_map(0, x), (1, 1), 'constant', fill=-9)[0, 0, 0]) == want, x
    one = np.array([[[200]]], dtype=np.uint8)
    m = oblique_maps(4, 5, (1, 1))[1]  # a source of size 1: every tap is its one pixel; the weights need not sum to 1 in fp32
    assert np.abs(oracle.warp_image(one, m, (4, 5), None, 'reflect') - 200.).max() <= oracle.bilinear_bound(200.)
    assert np.array_equal(oracle.truth(one, m, (4, 5), None, 'reflect'), np.full((1, 4, 5), 200.))
    assert np.array_equal(oracle.warp_labels(one.astype(np.int32) - 500, m, (4, 5), 'reflect'), np.full((4, 5, 1), -300))
    img = np.array([[[10], [20]]], dtype=np.uint8)
    got = oracle.warp_image(img, aug.crop_map(0, -.25), (1, 3), None, 'constant', fill=4.)[0, 0]
    assert got.tolist() == [np.float32(.25) * 4 + np.float32(.75) * 10, np.float32(.25) * 10 + np.float32(.75) * 20, 20 * .25 + 4 * .75]


def test_affine_map_dihedral_entries_are_integers_and_the_centre_maps_to_the_centre():
    for rot90, transpose, flip_h, flip_v in itertools.product(range(4), (False, True), (False, True), (False, True)):
        size = (W, H) if (rot90 + transpose) % 2 else (H, W)
        m = aug.affine_map((H, W), size, rot90=rot90, transpose=transpose, flip_h=flip_h, flip_v=flip_v)
        assert m.dtype == np.float64 and m.shape == (6,) and not np.signbit(m[m == 0]).any()
        assert np.array_equal(m, np.round(m)) and sorted(np.abs(m[[0, 1, 3, 4]]).tolist()) == [0, 0, 1, 1]
        lab = np.arange(H * W, dtype=np.int32).reshape(H, W, 1)
        assert np.array_equal(oracle.warp_labels(lab, m, size), numpy_dihedral(lab, rot90, transpose, flip_h, flip_v))
    for kw in (dict(angle=27., scale=1 / 1.3), dict(angle=-140., shear=20., scale=2.5, rot90=3, transpose=True, flip_v=True),
               dict(translate=(4., -3.), angle=1e-3)):
        for size in ((41, 47), (8, 9)):
            m = aug.affine_map((H, W), size, **kw)
            t = kw.get('translate', (0., 0.))
            cx, cy = (size[1] - 1) / 2 + t[0], (size[0] - 1) / 2 + t[1]
            assert abs(m[0] * cx + m[1] * cy + m[2] - (W - 1) / 2) < 1e-12 and abs(m[3] * cx + m[4] * cy + m[5] - (H - 1) / 2) < 1e-12


def forward_matrix(src, dst, rot90=0, transpose=False, flip_h=False, flip_v=False, angle=0., scale=1., shear=0., translate=(0., 0.)):
    """The forward map, written independently: 3 x 3, source (x, y, 1) -> destination, step by step as the text of affine_map."""
    (hs, ws), (hd, wd) = src, dst

    def shift(x, y):
        return np.array([[1., 0., x], [0., 1., y], [0., 0., 1.]])

    def lin(a, b, c, d):
        return np.array([[a, b, 0.], [c, d, 0.], [0., 0., 1.]])

    f = shift(-(ws - 1) / 2, -(hs - 1) / 2)
    if transpose:
        f = lin(0, 1, 1, 0) @ f
    for _ in range(rot90 % 4):
        f = lin(0, 1, -1, 0) @ f  # np.rot90: counter-clockwise as displayed, (x, y) -> (y, -x) about the centre
    if flip_h:
        f = lin(-1, 0, 0, 1) @ f
    if flip_v:
        f = lin(1, 0, 0, -1) @ f
    f = lin(scale, 0, 0, scale) @ f
    f = lin(1, math.tan(math.radians(shear)), 0, 1) @ f
    c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    f = lin(c, s, -s, c) @ f
    return shift((wd - 1) / 2 + translate[0], (hd - 1) / 2 + translate[1]) @ f


def test_affine_map_is_the_inverse_of_the_forward_transform():
    cases = [dict(angle=27., scale=1 / 1.3), dict(angle=-140., shear=20., scale=2.5, rot90=3, transpose=True, flip_v=True),
             dict(rot90=1, flip_h=True, shear=-33., translate=(12.5, -40.)), dict(scale=.37, angle=90.), dict(rot90=2, transpose=True)]
    for kw in cases:
        m = aug.affine_map((H, W), (41, 47), **kw)
        inv = np.array([[m[0], m[1], m[2]], [m[3], m[4], m[5]], [0., 0., 1.]])
        prod = inv @ forward_matrix((H, W), (41, 47), **kw)
        assert np.abs(prod - np.eye(3)).max() < 1e-12 * max(1., np.abs(inv).max()), (kw, prod)
    # the crop map is slicing
    _, labels = source(1)
    assert np.array_equal(aug.crop_map(3, 9), [1, 0, 9, 0, 1, 3]) and aug.crop_map(3, 9).dtype == np.float64
    assert np.array_equal(oracle.warp_labels(labels, aug.crop_map(3, 9), (30, 40)), labels[3:33, 9:49])
    with pytest.raises(ValueError, match='scale'):
        aug.affine_map((H, W), (4, 4), scale=0.)
    with pytest.raises(ValueError, match='src_size'):
        aug.affine_map((0, W), (4, 4))


def test_intensity_table_identity_gamma_and_per_channel_arguments():
    t = aug.intensity_table(3, scale=1.)
    assert t.dtype == np.float32 and t.shape == (3, 256) and np.array_equal(t, np.broadcast_to(np.arange(256, dtype=np.float32), (3, 256)))
    assert np.array_equal(aug.intensity_table(1), (np.arange(256, dtype=np.float64) * (1 / 255)).astype(np.float32)[None])
    for gamma in (.5, 1.7):
        want = np.arange(0, 256. / 255, 1. / 255) ** gamma * 255  # the table expression of preprocess, before its truncation
        assert np.array_equal(aug.intensity_table(1, gamma=gamma, scale=1.)[0], want.astype(np.float32))
    t = aug.intensity_table(3, gamma=(1., .5, 2.), contrast=(1., 1.5, 1.), brightness=(0., 0., .2), mean=(0., .5, .1), std=(1., .25, 2.))
    i = np.arange(256, dtype=np.float64)
    assert np.array_equal(t[0], (i * (1 / 255)).astype(np.float32))
    g = np.arange(0, 256. / 255, 1. / 255) ** .5 * 255
    assert np.array_equal(t[1], ((np.clip(g * 1.5, 0, 255) * (1 / 255) - .5) / .25).astype(np.float32))
    g = np.arange(0, 256. / 255, 1. / 255) ** 2. * 255
    assert np.array_equal(t[2], ((np.clip(g + 255 * .2, 0, 255) * (1 / 255) - .1) / 2.).astype(np.float32))
    so = aug.intensity_scale_offset(2, contrast=2., brightness=(0., 1.), mean=.5, std=(1., 4.))
    assert so.dtype == np.float32 and np.array_equal(so, np.array([[2., -.5], [.5, .125]], dtype=np.float32))
    for bad in (dict(K=5), dict(K=0), dict(K=3, gamma=(1., 2.)), dict(K=2, std=0.), dict(K=2, gamma=-1.), dict(K=1, mean=float('nan'))):
        with pytest.raises(ValueError, match='intensity_table'):
            aug.intensity_table(**bad)


def test_random_affine_draws_reproducibly_in_the_documented_order():
    r = aug.RandomAffine((24, 32), angle=(-30, 60), scale=(.5, 2.), shear=(-10, 5), translate=(6, 3), gamma=(.6, 1.5), contrast=(.8, 1.3),
                         brightness=(-.2, .1), mean=(.4, .5, .6), std=.25)
    B = 64
    p = r.draw(B, (H, W), K=3, generator=torch.Generator().manual_seed(5))
    q = r.draw(B, (H, W), K=3, generator=torch.Generator().manual_seed(5))
    assert sorted(p) == sorted(q) and all(np.array_equal(p[k], q[k]) for k in p)
    other = r.draw(B, (H, W), K=3, generator=torch.Generator().manual_seed(6))
    assert not np.array_equal(p['maps'], other['maps'])
    torch.manual_seed(11)
    a = r.draw(2, (H, W), K=3)
    torch.manual_seed(11)
    assert np.array_equal(a['maps'], r.draw(2, (H, W), K=3)['maps'])  # the default generator: reproducible under manual_seed
    # the draw order: ONE torch.rand(B, 12, float64); row = sample, columns = DRAWS
    assert aug.DRAWS == ('rot90', 'transpose', 'flip_h', 'flip_v', 'angle', 'scale', 'shear', 'translate_x', 'translate_y', 'gamma',
                         'contrast', 'brightness')
    u = torch.rand(B, 12, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).numpy()
    assert np.array_equal(p['uniform'], u)
    assert np.array_equal(p['rot90'], np.floor(4 * u[:, 0])) and np.array_equal(p['transpose'], u[:, 1] < .5)
    assert np.array_equal(p['flip_h'], u[:, 2] < .5) and np.array_equal(p['flip_v'], u[:, 3] < .5)
    assert np.array_equal(p['angle'], -30 + u[:, 4] * 90) and np.array_equal(p['shear'], -10 + u[:, 6] * 15)
    assert np.allclose(p['scale'], .5 * 4 ** u[:, 5], rtol=1e-14, atol=0)
    assert np.array_equal(p['translate'], np.stack([np.round(-6 + u[:, 7] * 12), np.round(-3 + u[:, 8] * 6)], 1) + 0.)
    assert np.array_equal(p['gamma'], .6 + u[:, 9] * (1.5 - .6)) and np.array_equal(p['contrast'], .8 + u[:, 10] * (1.3 - .8))
    assert np.array_equal(p['brightness'], -.2 + u[:, 11] * (.1 - -.2))
    # ranges
    assert set(p['rot90'].tolist()) == {0, 1, 2, 3} and p['transpose'].any() and not p['transpose'].all()
    for name, lo, hi in (('angle', -30, 60), ('scale', .5, 2.), ('shear', -10, 5), ('gamma', .6, 1.5), ('contrast', .8, 1.3),
                         ('brightness', -.2, .1)):
        assert (p[name] >= lo).all() and (p[name] <= hi).all() and p[name].max() - p[name].min() > .5 * (hi - lo), name
    assert (np.abs(p['translate']) <= (6, 3)).all() and np.array_equal(p['translate'], np.round(p['translate']))
    # maps and tables are composed by the two public functions
    assert p['maps'].shape == (B, 6) and p['tables'].shape == (B, 3, 256) and p['tables'].dtype == np.float32
    for b in (0, 17, 63):
        assert np.array_equal(p['maps'][b], aug.affine_map((H, W), (24, 32), int(p['rot90'][b]), bool(p['transpose'][b]), bool(p['flip_h'][b]),
                                                           bool(p['flip_v'][b]), p['angle'][b], p['scale'][b], p['shear'][b], p['translate'][b]))
        assert np.array_equal(p['tables'][b], aug.intensity_table(3, p['gamma'][b], p['contrast'][b], p['brightness'][b], 1 / 255,
                                                                  (.4, .5, .6), .25))
    # defaults: the dihedral part alone; every map entry an integer, the tables the plain scaling
    d = aug.RandomAffine((H, H)).draw(32, (H, H), K=1, generator=torch.Generator().manual_seed(0))
    assert np.array_equal(d['maps'], np.round(d['maps'])) and np.array_equal(d['tables'][3], aug.intensity_table(1))
    off = aug.RandomAffine((H, H), rot90=False, transpose=False, flip=False).draw(8, (H, H), generator=torch.Generator().manual_seed(0))
    assert np.array_equal(off['maps'], np.broadcast_to(aug.crop_map(0, 0), (8, 6))) and off['tables'] is None
    f = aug.RandomAffine((8, 8), contrast=(.5, 2.), brightness=(-1, 1), mean=.5, std=2.).draw(4, (9, 9), K=2, u8=False,
                                                                                                 generator=torch.Generator().manual_seed(0))
    assert f['tables'].shape == (4, 2, 2) and np.array_equal(f['tables'][1], aug.intensity_scale_offset(2, f['contrast'][1], f['brightness'][1], 1., .5, 2.))
    with pytest.raises(NotImplementedError, match='gamma'):
        aug.RandomAffine((8, 8), gamma=(.5, 2.)).draw(1, (9, 9), K=1, u8=False)
    for bad in (dict(size=(0, 4)), dict(size=5), dict(size=(4, 4), angle=(3, 1)), dict(size=(4, 4), scale=(0, 1)),
                dict(size=(4, 4), gamma=(-1, 1)), dict(size=(4, 4), border='wrap'), dict(size=(4, 4), shear=(0, float('inf')))):
        with pytest.raises(ValueError, match='RandomAffine'):
            aug.RandomAffine(**bad)


def test_every_argument_error_of_warp_is_named():
    """Everything but the device is checked on the host, before the device: CPU tensors get as far as the last check."""
    img = torch.zeros(2, 5, 6, 3, dtype=torch.uint8)
    lab = torch.zeros(2, 5, 6, 2, dtype=torch.int64)
    m = np.broadcast_to(aug.crop_map(0, 0), (2, 6)).copy()

    def raises(kind, word, *args, **kwargs):
        with pytest.raises(kind) as e:
            aug.warp(*args, **kwargs)
        assert 'warp' in str(e.value) and word in str(e.value), (word, str(e.value))

    raises(ValueError, 'both None', None, None, m, (4, 4))
    raises(TypeError, 'image', img.numpy(), lab, m, (4, 4))
    raises(TypeError, 'labels', img, lab.numpy(), m, (4, 4))
    raises(TypeError, 'image', img.to(torch.float64), lab, m, (4, 4))
    raises(TypeError, 'labels', img, lab.float(), m, (4, 4))
    raises(TypeError, 'labels', img, lab.bool(), m, (4, 4))
    raises(ValueError, 'image', img[0, 0, 0], lab, m, (4, 4))
    raises(ValueError, 'labels', img, lab[None], m, (4, 4))
    raises(ValueError, 'both be batched', img, lab[0], m, (4, 4))
    raises(ValueError, 'share', img, lab[:1], m, (4, 4))
    raises(ValueError, 'share', img, lab[:, :4], m, (4, 4))
    raises(NotImplementedError, 'channels', torch.zeros(2, 5, 6, 5, dtype=torch.uint8), lab, m, (4, 4))
    raises(ValueError, 'no channel', img, lab[..., :0], m, (4, 4))
    raises(ValueError, 'empty', img[:, :0], None, m, (4, 4))
    raises(ValueError, 'size', img, lab, m, (4,))
    raises(ValueError, 'size', img, lab, m, (0, 4))
    raises(ValueError, 'size', img, lab, m, 4)
    raises(ValueError, 'border', img, lab, m, (4, 4), border='wrap')
    raises(NotImplementedError, 'out_dtype', img, lab, m, (4, 4), out_dtype=torch.float16)
    raises(ValueError, 'label_fill', img, lab, m, (4, 4), label_fill=2 ** 31)
    raises(ValueError, 'label_fill', img, lab, m, (4, 4), label_fill=1.5)
    raises(ValueError, 'image_fill', img, lab, m, (4, 4), image_fill=float('nan'))
    raises(ValueError, 'image_fill', img, lab, m, (4, 4), image_fill=1e39)
    raises(TypeError, 'maps', img, lab, m.astype(np.float32), (4, 4))
    raises(ValueError, 'maps', img, lab, m[:1], (4, 4))
    raises(ValueError, 'maps', img, lab, m[:, :5], (4, 4))
    for bad in (float('nan'), float('inf'), -float('inf')):
        for entry in (0, 2, 4):
            n = m.copy()
            n[1, entry] = bad
            raises(ValueError, 'non-finite', img, lab, n, (4, 4))
    far = m.copy()
    far[0, 2] = 2. ** 30 + 1  # the first corner itself
    raises(ValueError, '2 ** 30', img, lab, far, (4, 4))
    far = m.copy()
    far[1, 4] = 2. ** 29  # only the last row gets there
    raises(ValueError, '2 ** 30', img, lab, far, (4, 4))
    far[1, 4] = 1e308  # overflows in the corner product
    raises(ValueError, '2 ** 30', img, lab, far, (4, 4))
    raises(TypeError, 'tables', img, lab, m, (4, 4), tables=np.zeros((3, 256)))
    raises(ValueError, 'tables', img, lab, m, (4, 4), tables=np.zeros((2, 256), np.float32))
    raises(ValueError, 'tables', img, lab, m, (4, 4), tables=np.zeros((3, 2), np.float32))
    raises(ValueError, 'tables', img.float(), lab, m, (4, 4), tables=np.zeros((3, 256), np.float32))
    raises(ValueError, 'tables', img, lab, m, (4, 4), tables=np.full((3, 256), np.inf, np.float32))
    raises(ValueError, 'tables', None, lab, m, (4, 4), tables=np.zeros((3, 256), np.float32))
    raises(ValueError, 'int32', None, lab + 2 ** 31, m, (4, 4))
    # what is left is the device
    raises(RuntimeError, 'MI355X', img, lab, m, (4, 4))
    raises(RuntimeError, 'MI355X', img[0], None, m[0], (4, 4))
    raises(RuntimeError, 'MI355X', None, lab[0, :, :, 0], torch.from_numpy(m[0]), (4, 4), border='reflect')


def test_c_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    one = 1 << 20  # an aligned non-null address that is never read: every call below fails validation first

    def call(image=one, image_dtype=0, labels=one, B=1, H=4, W=4, K=3, C=2, maps=one, tables=one, border=0, image_fill=0., label_fill=0,
             image_out=one, out_dtype=0, labels_out=one, h=4, w=4):
        return lib.cpn_augment_warp(image, image_dtype, labels, B, H, W, K, C, maps, tables, border, image_fill, label_fill, image_out,
                                    out_dtype, labels_out, h, w, None)

    inv, uns = _lib.E_INVALID, _lib.E_UNSUPPORTED
    assert call(image=None, labels=None) == inv and b'both null' in lib.cpn_last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=-1), dict(h=0), dict(w=0), dict(K=0), dict(K=5), dict(C=0), dict(C=65536), dict(border=2),
               dict(border=-1), dict(image_dtype=2), dict(out_dtype=2), dict(image_fill=float('inf')), dict(image_fill=float('nan')),
               dict(maps=None), dict(maps=one + 4), dict(tables=None), dict(tables=one + 2), dict(image_out=None), dict(labels_out=None),
               dict(labels=one + 2), dict(labels_out=one + 1), dict(image_out=one + 2), dict(out_dtype=1, image_out=one + 1),
               dict(image_dtype=1, image=one + 2)):
        assert call(**kw) == inv and b'cpn_augment_warp' in lib.cpn_last_error(), kw
    for kw in (dict(H=65536, W=32768), dict(h=46341, w=46341), dict(B=65536), dict(h=2 ** 31), dict(W=2 ** 40)):
        assert call(**kw) == uns, kw
    assert call(image=None, K=9, tables=None, image_out=None, C=0) == inv  # a labels-only call still checks C
    assert call(labels=None, C=0, labels_out=None, K=5) == inv


def test_surface_header_build_list_binding_and_exports():
    text = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    assert '---- Augmentation warp ----' in text and 'third-party, unpinned' in text[text.index('---- Augmentation warp'):]
    h = _header.header()
    names = list(h.prototypes)  # declared behind every older prototype but the optimizer's, whose section a test keeps last
    assert [n for n in names if n.startswith('cpn_augment_')] == ['cpn_augment_warp']
    assert names.index('cpn_augment_warp') > names.index('cpn_bilinear_sum_f32')
    assert all(n.startswith('cpn_optim_') for n in names[names.index('cpn_augment_warp') + 1:])
    restype, argtypes = h.prototypes['cpn_augment_warp']
    from ctypes import c_double, c_float, c_int32, c_int64, c_void_p
    assert restype is c_int32 and argtypes == [c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                                                c_int32, c_float, c_int32, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_void_p]
    assert c_double and 'cpn_augment_warp' in _lib.EXPORTED_SYMBOLS and _lib.load().cpn_augment_warp.argtypes == argtypes
    assert (_lib.AUGMENT_TILE, _lib.AUGMENT_IMAGE_U8, _lib.AUGMENT_IMAGE_F32, _lib.AUGMENT_BORDER_CONSTANT, _lib.AUGMENT_BORDER_REFLECT,
            _lib.AUGMENT_MAX_CHANNELS) == (32, 0, 1, 0, 1, 65535) and _lib.AUGMENT_MAX_CHANNELS == cda.components.MAX_CHANNELS
    assert _lib.ABI_VERSION == 22
    assert build.SOURCES['augment.hip'] == ['-ffp-contract=off'] and 'warp_rule.h' in build.HEADERS
    assert os.path.isfile(os.path.join(build.CSRC, 'warp_rule.h')) and os.path.isfile(os.path.join(build.CSRC, 'augment.hip'))
    assert cda.augment is aug and 'augment' in cda.__all__ and 'RandomAffine' in cda.__all__ and cda.RandomAffine is aug.RandomAffine
    assert aug.__all__ == ['warp', 'affine_map', 'crop_map', 'intensity_table', 'intensity_scale_offset', 'RandomAffine']
    assert all(callable(getattr(aug, n)) for n in aug.__all__)
    for word in ('relabel_', 'anti-aliasing', 'table-then-blend', 'share the source', 'affine maps only'):
        assert word in aug.__doc__, word
    assert re.search(r'augment', open(os.path.join(ROOT, 'README.md')).read())


def test_host_build_of_the_warp_rule_agrees_with_brute_force(tmp_path):
    """``csrc/warp_rule.h`` compiled for the host only, with AddressSanitizer and UBSan on the host code, by
    ``tests/warp_rule_host.cpp`` (a program of its own, nothing preloaded): indices stay in range for every double, NaN and
    infinities included, and agree with integer brute force."""
    import subprocess
    hipcc = build._hipcc()
    exe = str(tmp_path / 'warp_rule_host')
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', os.path.join(ROOT, 'tests', 'warp_rule_host.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r'ok \d+', run.stdout.strip()), run.stdout[-500:] + run.stderr[-2000:]
    assert int(run.stdout.split()[1]) > 100000
