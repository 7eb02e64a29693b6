"""The augmentation warp on the GPU (celldetection_amd.augment.warp / RandomAffine): every comparison with the numpy statement of
the rule (``tests/augment_oracle.py``) and with torch's own rot90 / flip / transpose / slicing is bit for bit, for the image and the
labels; the rule fixes every rounding, so there is no tolerance anywhere in this file."""
import itertools

import numpy as np
import pytest
import torch

import augment_oracle as oracle
import celldetection_amd as cda
from test_augment import SPECIAL, source

pytestmark = pytest.mark.gpu

aug = cda.augment
DEV = 'cuda:0'
H, W = 97, 131
TILE, VEC = 32, 4


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the shared sources are read-only)


def bits(a):
    """float32 array -> its bit patterns (so that -0.0 != 0.0 and NaN == NaN)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(image, labels, maps, size, tables=None, border='constant', image_fill=0., label_fill=0, out_dtype=torch.float32, what=''):
    """warp on the device copies of a batch (numpy [B, H, W, K] / [B, H, W, C], either may be None) against the oracle, sample by
    sample, bit for bit; the inputs must come back unchanged."""
    maps = np.asarray(maps, dtype=np.float64)
    first = image if image is not None else labels
    B = first.shape[0]
    timg, tlab = (None if image is None else dev(image)), (None if labels is None else dev(labels))
    out, lab = aug.warp(timg, tlab, maps, size, tables, border, image_fill, label_fill, out_dtype)
    torch.cuda.synchronize()
    m = np.broadcast_to(maps, (B, 6))
    if image is None:
        assert out is None
    else:
        K = image.shape[3]
        assert out.is_cuda and out.dtype == out_dtype and tuple(out.shape) == (B, K) + tuple(size) and out.is_contiguous(), what
        assert np.array_equal(timg.cpu().numpy(), image), (what, 'the image changed')
        got = out.float().cpu().numpy()
        for b in range(B):
            t = None if tables is None else (tables if np.ndim(tables) == 2 else tables[b])
            exp = oracle.warp_image(image[b], m[b], size, t, border, image_fill, bf16=out_dtype == torch.bfloat16)
            bad = int((bits(got[b]) != bits(exp)).sum())
            assert bad == 0, (what, b, f'{bad} image elements differ', float(np.abs(got[b] - exp).max()))
    if labels is None:
        assert lab is None
    else:
        C = labels.shape[3]
        assert lab.is_cuda and lab.dtype == torch.int32 and tuple(lab.shape) == (B,) + tuple(size) + (C,) and lab.is_contiguous(), what
        assert np.array_equal(tlab.cpu().numpy(), labels), (what, 'the labels changed')
        got = lab.cpu().numpy()
        for b in range(B):
            bad = int((got[b] != oracle.warp_labels(labels[b], m[b], size, border, label_fill)).sum())
            assert bad == 0, (what, b, f'{bad} labels differ')
    return out, lab


@pytest.fixture(scope='module')
def batch():
    """Three samples, K = 3 uint8, C = 2 with the special labels; never written."""
    pairs = [source(3, 2, seed, H, W) for seed in (1, 2, 3)]
    image, labels = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    assert all((labels == v).any() for v in SPECIAL)
    image.setflags(write=False), labels.setflags(write=False)
    return image, labels


def obliques(size, src=(H, W)):
    """rotation, scale up, scale down, shear"""
    return {'rotation': aug.affine_map(src, size, angle=27.),
            'up': aug.affine_map(src, size, angle=-12., scale=2.3, translate=(1.5, -.75)),
            'down': aug.affine_map(src, size, angle=63.5, scale=.41, rot90=1, flip_h=True),
            'shear': aug.affine_map(src, size, shear=24., scale=1 / 1.3, transpose=True, translate=(-3.3, 2.2))}


@pytest.mark.parametrize('K', (1, 3, 4))
def test_dihedral_maps_and_crops_are_torchs_own_rot90_flip_transpose_and_slicing(K):
    image, labels = source(K, 2, 7, H, W)
    timg, tlab = dev(image), dev(labels)
    for rot90, transpose, flip_h, flip_v in itertools.product(range(4), (False, True), (False, True), (False, True)):
        wi, wl = (timg.transpose(0, 1), tlab.transpose(0, 1)) if transpose else (timg, tlab)
        wi, wl = torch.rot90(wi, rot90, (0, 1)), torch.rot90(wl, rot90, (0, 1))
        dims = [d for d, f in ((1, flip_h), (0, flip_v)) if f]
        wi, wl = (torch.flip(wi, dims), torch.flip(wl, dims)) if dims else (wi, wl)
        size = tuple(wl.shape[:2])
        m = aug.affine_map((H, W), size, rot90=rot90, transpose=transpose, flip_h=flip_h, flip_v=flip_v)
        for border in ('constant', 'reflect'):
            out, lab = aug.warp(timg, tlab, m, size, border=border, image_fill=-3., label_fill=9)
            assert torch.equal(lab, wl) and torch.equal(out, wi.permute(2, 0, 1).float()), (rot90, transpose, flip_h, flip_v, border)
    for (y, x), size in (((0, 0), (H, W)), ((5, 11), (64, 96)), ((H - 1, W - 1), (1, 1)), ((40, 3), (33, 127))):
        out, lab = aug.warp(timg, tlab, aug.crop_map(y, x), size)
        assert torch.equal(lab, tlab[y:y + size[0], x:x + size[1]])
        assert torch.equal(out, timg[y:y + size[0], x:x + size[1]].permute(2, 0, 1).float())


@pytest.mark.parametrize('size', ((1, 1), (TILE - 1, TILE + 1), (TILE + 1, TILE - 1), (TILE, 2 * TILE), (2 * TILE + 1, 3 * TILE + VEC + 1),
                                  (45, 70), (5, 3)))
def test_oblique_maps_at_the_tile_and_vector_edges(batch, size):
    """1 x 1, one pixel less and one more than a tile in each axis, whole tiles, widths that are no multiple of the lane's four
    columns, more than one tile in both axes; three samples with three different maps and tables."""
    image, labels = batch
    maps = obliques(size)
    tables = np.stack([aug.intensity_table(3, gamma=(.6, 1., 1.8), mean=.5, std=.25), aug.intensity_table(3, contrast=1.4, brightness=-.1),
                       aug.intensity_table(3, scale=1.)])
    for border in ('constant', 'reflect'):
        check(image, labels, np.stack([maps['rotation'], maps['up'], maps['down']]), size, tables, border, image_fill=-2.5, label_fill=-7,
              what=(size, border))
    check(image, labels, np.stack([maps['shear'], maps['down'], maps['rotation']]), size, tables[::-1].copy(), 'reflect', what=(size, 'shear'))


@pytest.mark.parametrize('K, C', ((1, 5), (3, 1), (4, 2)))
@pytest.mark.parametrize('dtype', (np.uint8, np.float32))
def test_channel_counts_dtypes_and_partial_calls(K, C, dtype):
    pairs = [source(K, C, seed, 61, 45, dtype) for seed in (4, 5)]
    image, labels = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    size = (TILE + 7, 2 * TILE + 6)
    m = obliques(size, (61, 45))
    maps = np.stack([m['rotation'], m['down']])
    if dtype == np.uint8:
        tables = np.stack([aug.intensity_table(K, gamma=1.3, mean=.4, std=.3), aug.intensity_table(K, contrast=.7, brightness=.2)])
    else:
        tables = np.stack([aug.intensity_scale_offset(K, 1.3, -.2, 1., .4, .3), aug.intensity_scale_offset(K, .7, .1, 2., 0., 1.)])
    for out_dtype in (torch.float32, torch.bfloat16):
        for border in ('constant', 'reflect'):
            check(image, labels, maps, size, tables, border, image_fill=.625, label_fill=3, out_dtype=out_dtype, what=(K, C, border, out_dtype))
    both = check(image, labels, maps, size, None, 'reflect')
    only_image = check(image, None, maps, size, None, 'reflect')
    only_labels = check(None, labels, maps, size, None, 'reflect')
    assert torch.equal(both[0], only_image[0]) and torch.equal(both[1], only_labels[1])
    # an output width that makes the vector store impossible: element by element, the same values
    odd = (TILE + 7, 2 * TILE + 5)
    check(image, labels, np.stack([aug.affine_map((61, 45), odd, angle=27.)] * 2), odd, tables, 'constant', out_dtype=torch.bfloat16)
    # unbatched arguments come back unbatched
    out, lab = aug.warp(dev(image[0]), dev(labels[0]), maps[0], size, tables[0])
    assert tuple(out.shape) == (K,) + size and tuple(lab.shape) == size + (C,)
    assert torch.equal(out, aug.warp(dev(image[:1]), None, maps[:1], size, tables[:1])[0][0])
    out, lab = aug.warp(dev(image[0, :, :, 0]), dev(labels[0, :, :, 0].astype(np.int64)), maps[0], size)
    assert tuple(out.shape) == (1,) + size and tuple(lab.shape) == size and lab.dtype == torch.int32
    assert np.array_equal(lab.cpu().numpy(), oracle.warp_labels(labels[0, :, :, :1], maps[0], size)[:, :, 0])


def test_tiny_sources(batch):
    image, labels = batch
    one_i, one_l = np.ascontiguousarray(image[:, 50:51, 60:61]), np.ascontiguousarray(labels[:, 50:51, 60:61])
    size = (TILE + 3, TILE + 2)
    m = obliques(size, (1, 1))
    maps = np.stack([m['rotation'], m['up'], m['shear']])
    for border in ('constant', 'reflect'):
        check(one_i, one_l, maps, size, None, border, image_fill=1., label_fill=-1, what=('1 x 1 source', border))
    out, lab = aug.warp(dev(one_i), dev(one_l), maps, size, border='reflect')
    assert torch.equal(lab, dev(one_l).expand(3, size[0], size[1], 2))  # reflect on a source of size 1: its one pixel everywhere
    small_i, small_l = np.ascontiguousarray(image[:, :5, :3]), np.ascontiguousarray(labels[:, :5, :3])
    m = obliques((70, 41), (5, 3))
    for border in ('constant', 'reflect'):
        check(small_i, small_l, np.stack([m['rotation'], m['down'], m['up']]), (70, 41), None, border, what=('5 x 3 source', border))
    line_i, line_l = np.ascontiguousarray(image[:, :1]), np.ascontiguousarray(labels[:, :1])  # 1 x W: one axis of size 1
    m = obliques((9, 140), (1, W))
    check(line_i, line_l, np.stack([m['rotation'], m['up'], m['shear']]), (9, 140), None, 'reflect', what='1 x W source')


def test_borders_far_outside_and_on_the_half_pixel(batch):
    image, labels = batch
    size = (40, 52)
    part = aug.affine_map((H, W), size, angle=31., translate=(-38., 25.))          # part of the output outside
    far = aug.affine_map((H, W), size, angle=31., scale=1.1, translate=(420., -350.))  # all of it a few hundred pixels outside
    maps = np.stack([part, far, aug.affine_map((H, W), size, angle=-75., scale=.2, translate=(60., 7.))])
    sx, sy = oracle.positions(far, size)
    assert (sx < -100).all() | (sx > W + 100).all() | (sy < -100).all() | (sy > H + 100).all()
    tables = aug.intensity_table(3, mean=.5, std=.25)
    out, lab = check(image, labels, maps, size, tables, 'constant', image_fill=-1.75, label_fill=-5, what='constant')
    assert bool((out[1] == -1.75).all()) and bool((lab[1] == -5).all())  # exactly the fills
    assert bool((out[0] == -1.75).any()) and bool((out[0] != -1.75).any()) and bool((lab[0] == -5).any())
    out, lab = check(image, labels, maps, size, tables, 'constant', out_dtype=torch.bfloat16, image_fill=.3, what='constant, bf16')
    assert bool((out[1] == torch.tensor(.3).bfloat16()).all())
    # reflect several periods out: every label is a label of the sample
    out, lab = check(image, labels, maps, size, tables, 'reflect', what='reflect')
    assert np.isin(lab[1].cpu().numpy(), labels[1]).all()
    periods = np.stack([aug.crop_map(-5 * (H - 1) + .25, 7 * (W - 1) - .5), aug.crop_map(2 * (H - 1), -2 * (W - 1)), aug.crop_map(-H, W)])
    out, lab = check(image, labels, periods, size, None, 'reflect', what='reflect, whole periods')
    assert torch.equal(lab[1], dev(labels[1, :size[0], :size[1]]))  # two whole periods away: the source itself
    # a coordinate exactly on -0.5 (halves round up: pixel 0) and exactly on W - 0.5 (outside / reflected to W - 2)
    edge = np.stack([aug.crop_map(-.5, -.5), aug.crop_map(H - 10.5, W - 10.5), aug.crop_map(.5, W - 1.5)])
    assert oracle.positions(edge[1], size)[0][0, 10] == W - .5
    for border in ('constant', 'reflect'):
        out, lab = check(image, labels, edge, size, None, border, image_fill=9., label_fill=-9, what=('halves', border))
    lab = aug.warp(None, dev(labels), edge, size, label_fill=-9)[1]
    assert torch.equal(lab[0, 0, 0], dev(labels[0, 0, 0])) and bool((lab[1, :, 10] == -9).all()) and bool((lab[1, 10] == -9).all())
    assert torch.equal(lab[1, :10, :10], dev(labels[1, H - 10:, W - 10:]))


def test_inputs_unchanged_repeatable_and_independent_of_the_batch_position(batch):
    image, labels = batch
    size = (2 * TILE + 3, TILE + 9)
    m = obliques(size)
    maps = np.stack([m['rotation'], m['up'], m['shear']])
    tables = np.stack([aug.intensity_table(3, gamma=g) for g in (.7, 1., 1.6)])
    timg, tlab = dev(image), dev(labels)
    a = aug.warp(timg, tlab, maps, size, tables, 'reflect')
    b = aug.warp(timg, tlab, maps, size, tables, 'reflect')
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(timg, dev(image)) and torch.equal(tlab, dev(labels))
    order = [2, 0, 1]
    c = aug.warp(timg[order], tlab[order], maps[order], size, tables[order], 'reflect')
    assert torch.equal(c[0], a[0][order]) and torch.equal(c[1], a[1][order])
    for i in range(3):  # alone, and as an unbatched call
        d = aug.warp(timg[i:i + 1], tlab[i:i + 1], maps[i:i + 1], size, tables[i:i + 1], 'reflect')
        e = aug.warp(timg[i], tlab[i], maps[i], size, tables[i], 'reflect')
        assert torch.equal(d[0][0], a[0][i]) and torch.equal(d[1][0], a[1][i]) and torch.equal(e[0], a[0][i]) and torch.equal(e[1], a[1][i])
    # a non-contiguous image view and int64 labels are taken as they are
    f = aug.warp(dev(np.ascontiguousarray(image.transpose(0, 3, 1, 2))).permute(0, 2, 3, 1), tlab.long(), maps, size, tables, 'reflect')
    assert torch.equal(f[0], a[0]) and torch.equal(f[1], a[1])


def discs(h, w):
    """A few discs in two channels, overlapping across the channels."""
    yy, xx = np.mgrid[:h, :w]
    lab = np.zeros((h, w, 2), dtype=np.int32)
    for n, (cy, cx, r, c) in enumerate(((20, 22, 11, 0), (24, 36, 9, 1), (55, 80, 14, 0), (60, 100, 12, 1), (75, 30, 8, 0), (40, 70, 6, 1)), 1):
        lab[:, :, c][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = n
    return lab


def test_the_recipe_random_affine_relabel_feed_equals_feeding_the_oracles_warp():
    labels = np.stack([discs(H, W), discs(H, W)[::-1, ::-1].copy()])
    image = np.stack([source(3, 2, s, H, W)[0] for s in (8, 9)])
    r = aug.RandomAffine((72, 88), angle=(-180, 180), scale=(.8, 1.25), shear=(-8, 8), translate=(10, 6), gamma=(.7, 1.4), mean=.5, std=.25,
                         border='reflect')
    inputs, lab = r(dev(image), dev(labels), generator=torch.Generator().manual_seed(3))
    p = r.last_params
    assert tuple(inputs.shape) == (2, 3, 72, 88) and tuple(lab.shape) == (2, 72, 88, 2) and p['maps'].shape == (2, 6)
    again = aug.warp(dev(image), dev(labels), p['maps'], (72, 88), p['tables'], 'reflect')  # a replay from last_params
    assert torch.equal(again[0], inputs) and torch.equal(again[1], lab)
    for b in range(2):
        assert (bits(inputs[b].cpu().numpy()) == bits(oracle.warp_image(image[b], p['maps'][b], (72, 88), p['tables'][b], 'reflect'))).all()
        want = dev(oracle.warp_labels(labels[b], p['maps'][b], (72, 88), 'reflect'))
        assert torch.equal(lab[b], want) and int(want.max()) > 0
        cda.relabel_(lab[b])  # in place on the view of the batch
        cda.relabel_(want)
        assert torch.equal(lab[b], want)
        gens = [cda.CPNTargetGenerator(samples=32, order=5, random_sampling=False) for _ in range(2)]
        gens[0].feed(lab[b])
        gens[1].feed(want)
        assert torch.equal(gens[0].labels, gens[1].labels) and torch.equal(gens[0].distances, gens[1].distances)
        assert torch.equal(gens[0].labels_red, gens[1].labels_red) and gens[0].distances.shape == (72, 88)
        assert float(gens[0].distances.max()) > 0
