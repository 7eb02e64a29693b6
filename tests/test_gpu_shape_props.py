"""Shape property tables on the MI355X: celldetection_amd.shape_properties / labels2property_table against the numpy statement
of the contract (tests/shape_props_oracle.py, which the CPU tests hold against independent restatements).

Acceptance: every integer column equal; every float column bit-identical (both sides IEEE fp64, the same order of operations,
no contraction; only + * / and constants are involved).  No case is skipped or filtered out of a comparison.  The tile of the
shape pass is 32 rows x 64 columns of the (H + 1) x (W + 1) grid, its LDS table takes 64 keys."""
import os

import numpy as np
import pytest
import torch

import celldetection_amd as cda
from property_table_oracle import property_table
from shape_props_oracle import SUPPORTED, shape_table
from test_instance_eval import disc_labels

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ALL = SUPPORTED + ('convex_area',)
TILE_H, TILE_W = 32, 64


def to_dev(x):
    return torch.as_tensor(x).to(DEV)


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and \
        np.array_equal(got.view(np.int64) if got.dtype == np.float64 else got, want.view(np.int64) if want.dtype == np.float64 else want)


def compare(cols, exp, what):
    assert list(cols) == list(exp), (what, list(cols), list(exp))
    for name, t in cols.items():
        assert t.is_cuda and t.ndim == 1, (what, name)
        got, want = t.cpu().numpy(), exp[name]
        if not same(got, want):
            bad = np.nonzero(got != want)[0][:6] if got.shape == want.shape else []
            raise AssertionError((what, name, got.dtype, want.dtype, got.shape, want.shape, list(bad), got[bad], want[bad]))


def check(a, properties=ALL, what='', table_capacity=None, **kw):
    """cda.shape_properties on the device copy of ``a`` against the oracle; -> (columns, stats)."""
    exp, channel = shape_table(a, properties, **kw)
    cols, st = cda.shape_properties(to_dev(a), properties, table_capacity=table_capacity, return_stats=True, **kw)
    compare(cols, exp, what or str(a.shape))
    assert st['rows'] == len(channel)
    return cols, st


@pytest.mark.parametrize('shape', [(1, 1), (7, 131), (67, 129)])
def test_odd_sizes_and_channel_counts(shape):
    h, w = shape
    for c in (1, 2, 3, 5, 11):
        a = disc_labels(h, w, max(h * w // 60, 1), c, seed=h + c, rmax=9.)
        if h == 1:
            a[0, 0, c - 1] = 3
        a[h - 1, w - 1, 0] = 77
        a[0, w - 1, c - 1] = 78
        _, st = check(a, what=f'{h} x {w} x {c}')
        assert st['rows'] >= 1


@pytest.mark.parametrize('h', [TILE_H - 1, TILE_H, TILE_H + 1])
def test_sizes_around_the_tile(h):
    for w in (TILE_W - 1, TILE_W, TILE_W + 1):
        a = disc_labels(h, w, 12, 2, seed=h * w, rmax=7.)
        a[:, :, 1][a[:, :, 1] == 0] = 500  # the background of channel 1 is an object with holes that touches every border
        a[h - 1, w - 1, 0], a[h - 1, 0, 0], a[0, w - 1, 0] = 91, 92, 93
        check(a, what=f'{h} x {w}')


def test_borders_and_a_frame_around_the_image():
    a = np.zeros((2 * TILE_H, 2 * TILE_W, 3), np.int32)  # the windows of row H and column W lie in tiles without a pixel
    a[0:5, 10:30, 0], a[20:64, 0:3, 0], a[60:64, 100:128, 0], a[30:40, 120:128, 0] = 1, 2, 3, 4
    a[0, :, 1] = a[-1, :, 1] = a[:, 0, 1] = a[:, -1, 1] = 9  # a one-pixel frame: one hole, every window row and column
    a[:, :, 2] = 5
    a[1:-1, 1:-1, 2] = 6  # the frame again, now with another label inside it
    cols, _ = check(a, what='frame')
    assert cols['euler_number'].tolist() == [1, 1, 1, 1, 0, 0, 1]
    assert cols['solidity'][6] == 1. and cols['area_convex'][4] == 64. * 128.


def test_staircase_through_a_tile_corner():
    a = np.zeros((2 * TILE_H, 2 * TILE_W), np.int32)
    for i in range(-20, 20):  # a diagonal staircase through (32, 64): the 5 x 5 dependency of a pixel spans four tiles
        a[TILE_H + i, TILE_W + i] = 3
        if i % 3:
            a[TILE_H + i, TILE_W + i - 1] = 3
    a[TILE_H - 3:TILE_H + 3, 10:16] = 4
    a[TILE_H - 1, 12] = a[TILE_H, 13] = 0  # two diagonal holes on the tile edge
    b = a[:, ::-1].copy()
    check(np.stack([a, b, np.roll(a, 1, 0)], -1), what='staircase')


def test_interleaved_labels_and_checkerboards():
    h, w = 45, 77
    yy, xx = np.mgrid[:h, :w]
    inter = np.where((yy + xx) % 2 == 0, 5, 6).astype(np.int32)  # two labels pixel by pixel: the predicate is SAME LABEL
    board = ((yy + xx) % 2 == 0).astype(np.int32) * 7            # one label, h * w / 2 pixels that touch only diagonally
    stripes = (yy % 2 == 0).astype(np.int32) * 8                 # many components
    holes = np.full((h, w), 9, np.int32)
    holes[1:-1:2, 1:-1:2] = 0                                    # many holes: strongly negative
    cols, _ = check(np.stack([inter, board, stripes, holes], -1), what='interleaved')
    e = cols['euler_number'].tolist()
    assert e[3] == 23 and e[4] == 1 - 22 * 38 and e[0] < -100 and e[1] < -100 and e[2] < -100


def test_rings_with_islands():
    a = np.zeros((80, 150, 2), np.int32)
    yy, xx = np.mgrid[:80, :150]
    for k, (cy, cx) in enumerate(((30, 40), (45, 100), (33, 64))):
        r2 = (yy - cy) ** 2 + (xx - cx) ** 2
        a[:, :, 0][(r2 <= 28 ** 2) & (r2 >= 20 ** 2)] = 10 + k   # ring (later rings overwrite earlier ones)
        a[:, :, 0][r2 <= 8 ** 2] = 10 + k                       # island of the same label inside it
        a[:, :, 1][(r2 <= 15 ** 2) & (r2 >= 9 ** 2)] = 20 + k
        a[:, :, 1][r2 <= 4] = 30 + k                            # island of another label
    cols, _ = check(a, what='rings')
    assert cols['euler_number'][2] == 1  # the last ring is whole: ring (0) + island (1)


def test_one_object_over_all_tiles():
    a = np.full((130, 257), 4, np.int32)
    cols, st = check(a, what='full image')
    assert cols['area_convex'][0] == 130 * 257 and cols['perimeter'][0] == 2 * 128 + 2 * 255 + 4. and st['hull_rows'] == 130
    a[::9, 3::11] = 0
    a[64:66, :] = 0  # two pieces
    a[65, 100] = 4
    check(a, what='full image with holes')


def test_more_objects_in_a_tile_than_lds_slots_and_a_table_that_grows():
    a = np.arange(1, 34 * 66 + 1, dtype=np.int32).reshape(34, 66)  # every pixel its own label: 2048 keys in the first tile
    cols, st = check(a, what='grow', table_capacity=16)
    assert st['grown'] >= 8 and st['rows'] == 34 * 66 and st['hull_rows'] == 34 * 66
    assert cols['euler_number'].eq(1).all() and cols['perimeter'].eq(0).all()
    b = (np.arange(34 * 66, dtype=np.int32).reshape(34, 66) // 3 + 1)  # runs of three: 680 keys a tile
    check(np.stack([b, b.reshape(66, 34).T.copy()], -1), what='runs of three')


def test_label_values():
    a = np.zeros((40, 50, 2), np.int32)
    a[2:9, 3:11, 0], a[12:20, 30:45, 0], a[25:31, 5:9, 0] = 1, 2 ** 31 - 1, 65537
    a[14:18, 33:40, 0] = 2 ** 31 - 2  # a label inside another one, both near 2^31
    a[3:8, 20:26, 1], a[30:39, 12:44, 1], a[0, 0, 1], a[10:12, 0:2, 1] = 1000000, 7, -5, -(2 ** 31)
    a[3:8, 3:11, 1] = 65537           # the same label in two channels: two rows
    cols, _ = check(a, what='label values')
    assert cols['label'].tolist() == [1, 65537, 2 ** 31 - 2, 2 ** 31 - 1, 7, 65537, 1000000]
    assert cols['euler_number'].tolist() == [1, 1, 1, 0, 1, 1, 1]
    for empty in (np.zeros((20, 30, 3), np.int32), np.full((5, 5), -1, np.int32), np.zeros((0, 7, 2), np.int32)):
        cols, st = check(empty, what='no positive label')
        assert st['rows'] == 0 and len(cols) == len(ALL) and all(v.numel() == 0 for v in cols.values())
        assert cols['euler_number'].dtype == torch.int64 and cols['perimeter'].dtype == torch.float64


def hull_shapes():
    a = np.zeros((140, 200, 2), np.int32)
    a[2:12, 3:30, 0] = 1                                   # rectangles
    a[20:21, 5:60, 0] = 2
    for i in range(25):                                    # a diagonal line, and one with slope 1 / 2
        a[30 + i, 70 + i, 0] = 3
        a[30 + i // 2, 110 + i, 0] = 4
    a[60:90, 5:9, 0], a[86:90, 5:40, 0] = 5, 5              # L
    a[60:90, 50:54, 0], a[60:64, 50:80, 0], a[86:90, 50:80, 0] = 6, 6, 6   # C
    yy, xx = np.mgrid[:140, :200]
    star = (np.abs(yy - 75) + np.abs(xx - 140) <= 4) | ((np.abs(yy - 75) <= 1) & (np.abs(xx - 140) <= 28)) | \
        ((np.abs(xx - 140) <= 1) & (np.abs(yy - 75) <= 14)) | (np.abs(yy - 75) == np.abs(xx - 140)) & (np.abs(yy - 75) <= 12)
    a[:, :, 0][star] = 7
    a[5:135, 190, 0] = 8                                   # a column of one pixel over 130 rows: five tiles
    rng = np.random.default_rng(2)                         # a fragmented label with empty rows
    rr, cc = rng.integers(0, 70, 40) * 2, rng.integers(0, 200, 40)
    a[rr, cc, 1] = 9
    a[0, 0, 1] = a[139, 199, 1] = a[0, 199, 1] = 11        # three corners of the image: lattice points on the long edge
    return a


def test_hull_shapes():
    cols, st = check(hull_shapes(), what='hull shapes')
    assert cols['area_convex'][:2].tolist() == [270., 55.] and cols['solidity'][:2].tolist() == [1., 1.]
    assert cols['num_pixels'][7] == 130 and cols['area_convex'][7] == 130. and st['hull_rows'] > 300


def test_2048_small_objects():
    rng = np.random.default_rng(7)
    a = np.zeros((256, 512), np.int32)
    for k in range(2048):
        r0, c0 = (k // 64) * 8, (k % 64) * 8
        n = int(rng.integers(1, 41))
        idx = rng.choice(64, n, replace=False)
        a[r0 + idx // 8, c0 + idx % 8] = k + 1
    cols, st = check(a, what='2048 objects')
    assert st['rows'] == 2048 and int(cols['num_pixels'].min()) == 1 and int(cols['num_pixels'].max()) == 40


def test_spacing():
    a = disc_labels(90, 120, 50, 2, seed=4, rmax=12.)
    check(a, what='spacing scalar', spacing=0.25)
    check(a, what='spacing pair', spacing=(1.1, 1.1))
    check(a, ('label', 'euler_number', 'area_convex', 'solidity', 'num_pixels'), what='anisotropic without lengths', spacing=(0.5, 2.0))
    with pytest.raises(NotImplementedError, match='isotropic spacings only'):
        cda.shape_properties(to_dev(a), ('perimeter_crofton',), spacing=(0.5, 2.0))


def test_two_calls_give_identical_results():
    a = to_dev(disc_labels(1024, 1024, 2500, 3, seed=21, rmax=18.))
    c1, s1 = cda.shape_properties(a, ALL, return_stats=True)
    c2, s2 = cda.shape_properties(a, ALL, return_stats=True)
    assert s1 == s2 and s1['rows'] > 2000 and list(c1) == list(c2)
    for k in c1:
        assert torch.equal(c1[k].view(torch.int64), c2[k].view(torch.int64)), k
    assert float(c1['solidity'].min()) > 0 and float(c1['solidity'].max()) <= 1 and int(c1['euler_number'].max()) >= 1


def test_property_table_with_old_and_new_names_mixed():
    import pandas as pd
    a = disc_labels(67, 129, 40, 3, seed=9, rmax=10.)
    a[:, :, 2][a[:, :, 2] > 0] = 3  # one fragmented label in the last channel
    props = ['solidity', 'label', 'bbox', 'perimeter', 'area', 'euler_number', 'centroid', 'convex_area', 'num_pixels', 'perimeter_crofton',
             'extent', 'area_convex']
    region = [p for p in props if p in ('label', 'bbox', 'area', 'centroid', 'num_pixels', 'extent')]
    shape = [p for p in props if p not in region]
    want = dict(property_table(a, region, spacing=(.5, .5))[0])
    want.update(shape_table(a, shape, spacing=(.5, .5))[0])
    tab = cda.labels2property_table(to_dev(a), *props, spacing=(.5, .5))
    assert isinstance(tab, pd.DataFrame)
    assert [str(c) for c in tab.columns] == ['solidity', 'label', 'bbox-0', 'bbox-1', 'bbox-2', 'bbox-3', 'perimeter', 'area', 'euler_number',
                                             'centroid-0', 'centroid-1', 'convex_area', 'num_pixels', 'perimeter_crofton', 'extent',
                                             'area_convex']
    for name in tab.columns:
        assert same(tab[name].to_numpy(), want[name]), name
    assert tab['euler_number'].dtype == np.int64 and tab['perimeter'].dtype == np.float64 and len(tab) > 20
    index = property_table(a, region)[2]
    assert np.array_equal(np.asarray(tab.index, np.int64), index)
    # the call of the issue, in list form, and shape names alone
    tab = cda.labels2property_table(to_dev(a), ['label', 'area', 'perimeter', 'solidity'])
    exp = shape_table(a, ('label', 'perimeter', 'solidity'))[0]
    assert list(tab.columns) == ['label', 'area', 'perimeter', 'solidity']
    assert all(same(tab[k].to_numpy(), exp[k]) for k in exp) and same(tab['area'].to_numpy(), property_table(a, ('area',))[0]['area'])
    tab = cda.labels2property_table(to_dev(a), 'perimeter')
    assert list(tab.columns) == ['perimeter'] and same(tab['perimeter'].to_numpy(), exp['perimeter'])
    with pytest.raises(NotImplementedError, match='supported: label, bbox, num_pixels'):
        cda.region_properties(to_dev(a), ('label', 'perimeter'))


def test_end_to_end_on_device_tensors(monkeypatch):
    """model -> contours2labels -> resolve_label_channels -> table with perimeter and solidity, without a host copy of an image."""
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
    flat = cda.resolve_label_channels(labels)

    def no_host_copy(self, *a, **k):
        if self.numel() > 4096:
            raise AssertionError(f'a tensor of {self.numel()} elements was copied to the host')
        return orig_cpu(self, *a, **k)
    orig_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', no_host_copy)
    tab = cda.labels2property_table(flat, 'label', 'area', 'perimeter', 'solidity')
    cols, st = cda.shape_properties(labels, ALL, return_stats=True)
    monkeypatch.setattr(torch.Tensor, 'cpu', orig_cpu)
    assert st['rows'] > 0 and len(tab) > 0 and all(v.is_cuda for v in cols.values())
    print(f'{tuple(labels.shape)}: {st}, flat rows {len(tab)}')
    compare(cols, shape_table(labels.cpu().numpy(), ALL)[0], 'model, channels')
    exp = shape_table(flat.cpu().numpy(), ('label', 'perimeter', 'solidity'))[0]
    assert all(same(tab[k].to_numpy(), exp[k]) for k in exp)
