"""Region property tables on the MI355X: celldetection_amd.region_properties / labels2property_table against the numpy
statement of the contract (tests/property_table_oracle.py, which the CPU tests check against exact rationals) and against
the recorded tables of the reference's own wrapper (tests/golden/property_table.npz).

Acceptance: integer columns equal; float columns built from + - * / only bit-identical (both sides IEEE fp64, same order of
operations, no contraction); columns through sqrt within 1 ulp (OCML's fp64 sqrt is specified correctly rounded; the 1 ulp is
a margin for not having measured it); orientation within 8 ulp (the OpenCL bound of 6 ulp for fp64 atan2 that OCML follows,
plus 1 for the host libm; the halving is exact).  No case is skipped or filtered out of a comparison."""
import os

import numpy as np
import pytest
import torch

import celldetection_amd as cda
from property_table_oracle import ALIASES, ALL_GEOMETRY, EXACT, SQRT, SUPPORTED, property_table, ulp_distance
from test_instance_eval import disc_labels
from test_property_table import load_fixture, oracle_kwargs

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SQRT_ULP, ORIENTATION_ULP = 1, 8
worst = dict(sqrt=0, orientation=0)  # largest distances seen in this session, printed by the last test


def canonical(column, sep='-'):
    for p in sorted(tuple(SUPPORTED) + tuple(ALIASES), key=len, reverse=True):
        if column == p or column.startswith(p + sep):
            return ALIASES.get(p, p)
    raise AssertionError(column)


def compare(cols, exp, what, sep='-'):
    """GPU columns (name -> Tensor) against oracle columns (name -> array) under the acceptance rules."""
    assert list(cols) == list(exp), (what, list(cols), list(exp))
    for name, t in cols.items():
        assert t.is_cuda and t.ndim == 1, (what, name)
        got, want = t.cpu().numpy(), exp[name]
        assert got.shape == want.shape and got.dtype == want.dtype, (what, name, got.shape, want.shape, got.dtype, want.dtype)
        prop = canonical(name, sep)
        if prop in EXACT:
            same = np.array_equal(got.view(np.int64), want.view(np.int64)) if got.dtype == np.float64 else np.array_equal(got, want)
            assert same, (what, name, got[:8], want[:8])
        else:
            d = ulp_distance(got, want)
            kind = 'sqrt' if prop in SQRT else 'orientation'
            assert prop in SQRT or prop == 'orientation'
            worst[kind] = max(worst[kind], d)
            assert d <= (SQRT_ULP if prop in SQRT else ORIENTATION_ULP), (what, name, f'{d} ulp')


def to_dev(x):
    return None if x is None else torch.as_tensor(x).to(DEV)


def check(a, properties=ALL_GEOMETRY, what='', intensity_image=None, table_capacity=None, **kw):
    """cda.region_properties on the device copy of ``a`` against the oracle; -> (columns, stats)."""
    exp, channel, index = property_table(a, properties, intensity_image=intensity_image, **kw)
    cols, st = cda.region_properties(to_dev(a), properties, intensity_image=to_dev(intensity_image), table_capacity=table_capacity,
                                     return_stats=True, **kw)
    compare(cols, exp, what or str(a.shape), kw.get('separator', '-'))
    assert st['rows'] == len(channel)
    return cols, st


def test_fixture_cases_equal_the_reference_wrapper():
    import pandas as pd
    for c in load_fixture():
        a, props, kw = c['labels'], c['properties'], dict(c['kwargs'])
        if 'intensity_image' in kw:
            kw['intensity_image'] = to_dev(kw['intensity_image'])
        tab = cda.labels2property_table(to_dev(a), list(props), **kw) if c['list_form'] else \
            cda.labels2property_table(to_dev(a), *props, **kw)
        assert isinstance(tab, pd.DataFrame) and [str(x) for x in tab.columns] == c['columns'], c['name']
        assert np.array_equal(np.asarray(tab.index, np.int64), c['index']), c['name']
        sep = kw.get('separator', '-')
        for name in c['columns']:
            got, want = tab[name].to_numpy(), c['values'][name]
            assert got.dtype == want.dtype and got.shape == want.shape, (c['name'], name, got.dtype, want.dtype)
            prop = canonical(name, sep)
            if prop in EXACT:
                assert np.array_equal(got, want), (c['name'], name)
            else:
                d = ulp_distance(got, want)
                worst['sqrt' if prop in SQRT else 'orientation'] = max(worst['sqrt' if prop in SQRT else 'orientation'], d)
                assert d <= (SQRT_ULP if prop in SQRT else ORIENTATION_ULP), (c['name'], name, d)
        # the same through region_properties, against the oracle
        check(a, props, c['name'], **oracle_kwargs(c['kwargs']))


@pytest.mark.parametrize('shape', [(1, 1), (7, 131), (67, 129)])
def test_odd_sizes_and_channel_counts(shape):
    h, w = shape
    for c in (1, 2, 3, 4, 5, 11):
        a = disc_labels(h, w, max(h * w // 60, 1), c, seed=h + c, rmax=9.)
        if h == 1:
            a[0, 0, c - 1] = 3
        a[h - 1, w - 1, 0] = 77  # the last element of the image, in a partial strip
        a[0, w - 1, c - 1] = 78
        cols, st = check(a, what=f'{h} x {w} x {c}')
        assert st['rows'] >= 1


def test_objects_over_many_tiles_and_large_sums():
    a = np.zeros((300, 700, 2), np.int32)
    yy, xx = np.mgrid[:300, :700]
    a[:, :, 0][(yy - 150) ** 2 / 140. ** 2 + (xx - 350 - .4 * (yy - 150)) ** 2 / 300. ** 2 <= 1] = 12  # a tilted ellipse over ~50 tiles
    a[5:290:3, 3:690, 1] = 4  # stripes: one object of many runs
    cols, _ = check(a, what='many tiles')
    assert int(cols['num_pixels'][0]) > 100000
    full = np.full((512, 512), 9, np.int32)  # one object filling the image
    cols, _ = check(full, what='full image')
    assert int(cols['num_pixels'][0]) == 512 * 512 and cols['bbox-2'][0] == 512
    far = np.zeros((2048, 2048), np.int32)  # 40 x 40 blocks in the bottom right corner: sum r^2 per object exceeds 2^32
    for i in range(3):
        for j in range(3):
            far[1920 + 42 * i:1960 + 42 * i, 1915 + 44 * j:1955 + 44 * j] = 1 + i * 3 + j
    assert int((np.nonzero(far == 1)[0].astype(np.int64) ** 2).sum()) > 2 ** 32
    check(far, what='far corner')


def test_label_values():
    a = np.zeros((40, 50, 2), np.int32)
    a[2:9, 3:11, 0], a[12:20, 30:45, 0], a[25:31, 5:9, 0] = 1, 2 ** 31 - 1, 65537
    a[3:8, 20:26, 1], a[30:39, 12:44, 1], a[0, 0, 1], a[10:12, 0:2, 1] = 1000000, 7, -5, -(2 ** 31)
    cols, _ = check(a, what='label values')
    assert cols['label'].tolist() == [1, 65537, 2 ** 31 - 1, 7, 1000000]
    # the same label in two channels: two rows
    b = a.copy()
    b[3:8, 20:26, 1] = 65537
    cols, _ = check(b, ('label', 'bbox', 'centroid'), what='same label in two channels')
    assert cols['label'].tolist().count(65537) == 2
    # int64 labels that fit, uint8 labels
    x = to_dev(a).to(torch.int64)
    assert cda.region_properties(x, ('label',))['label'].tolist() == [1, 65537, 2 ** 31 - 1, 7, 1000000]
    x[0, 0, 0] = 2 ** 31
    with pytest.raises(ValueError, match='int32'):
        cda.region_properties(x)
    assert cda.region_properties(to_dev(a).clamp(0, 200).to(torch.uint8), ('label',))['label'].tolist() == [1, 200, 7, 200]


def test_single_pixels_and_empty_images():
    a = np.zeros((9, 13, 2), np.int32)
    a[0, 0, 0], a[8, 12, 0], a[4, 6, 1], a[4, 7, 1], a[5, 7, 1] = 5, 3, 8, 9, 9
    cols, _ = check(a, what='single pixels')
    assert cols['inertia_tensor_eigvals-0'][:3].tolist() == [0., 0., 0.] and cols['eccentricity'][:3].tolist() == [0., 0., 0.]
    assert cols['orientation'][:3].tolist() == [-np.pi / 4] * 3 and cols['axis_major_length'][0] == 0
    for empty in (np.zeros((20, 30, 3), np.int32), np.full((5, 5), -1, np.int32), np.zeros((0, 7, 2), np.int32)):
        cols, st = check(empty, SUPPORTED[:15] + ('bbox_area',), what='no positive label')
        assert st['rows'] == 0 and len(cols) == 25 and all(v.numel() == 0 for v in cols.values())
        assert cols['label'].dtype == torch.int64 and cols['area'].dtype == torch.float64
    tab = cda.labels2property_table(to_dev(np.zeros((6, 6, 2), np.int32)), 'label', 'centroid')
    assert len(tab) == 0 and list(tab.columns) == ['label', 'centroid-0', 'centroid-1']


def test_table_grows():
    a = np.arange(1, 100 * 100 + 1, dtype=np.int32).reshape(100, 100)  # every pixel its own label: more keys than LDS slots
    cols, st = check(a, ('label', 'bbox', 'num_pixels', 'centroid', 'orientation'), what='grow', table_capacity=16)
    assert st['grown'] >= 10 and st['table_capacity'] >= 16384 and st['rows'] == 10000
    assert torch.equal(cols['label'].cpu(), torch.arange(1, 10001))
    with pytest.raises(ValueError, match='power of two'):
        cda.region_properties(to_dev(a), table_capacity=100)


def test_intensity_images():
    a = disc_labels(67, 129, 60, 3, seed=8, rmax=9.)
    rng = np.random.default_rng(5)
    props = ('label', 'intensity_mean', 'intensity_min', 'max_intensity', 'mean_intensity', 'area')
    for dt, lo, hi in ((np.uint8, 0, 256), (np.int16, -32768, 32768), (np.int32, -2 ** 31, 2 ** 31)):
        for k in (1, 3):
            img = rng.integers(lo, hi, (67, 129, k)).astype(dt)
            img[0, 0], img[-1, -1] = lo, hi - 1
            cols, _ = check(a, props, f'{dt.__name__} K={k}', intensity_image=img)
            assert cols['intensity_min' if k == 1 else 'intensity_min-0'].dtype == torch.as_tensor(img).dtype
        check(a[:, :, 0], props, f'{dt.__name__} 2-D', intensity_image=rng.integers(lo, hi, (67, 129)).astype(dt))
    # uint16 arrives as a numpy array and is converted on the way up
    img = rng.integers(0, 65536, (67, 129)).astype(np.uint16)
    exp, _, _ = property_table(a, ('label', 'intensity_mean'), intensity_image=img)
    got = cda.region_properties(to_dev(a), ('label', 'intensity_mean'), intensity_image=img)
    assert np.array_equal(got['intensity_mean'].cpu().numpy(), exp['intensity_mean'])
    with pytest.raises(TypeError, match='float'):
        cda.region_properties(to_dev(a), ('intensity_mean',), intensity_image=to_dev(img.astype(np.float32)))
    with pytest.raises(AttributeError, match='intensity_image'):
        cda.region_properties(to_dev(a), ('intensity_mean',))
    with pytest.raises(NotImplementedError, match='intensity channels'):
        cda.region_properties(to_dev(a), ('label',), intensity_image=to_dev(np.zeros((67, 129, 5), np.uint8)))


def test_spacing_and_separator():
    a = disc_labels(90, 120, 50, 2, seed=4, rmax=12.)
    check(a, what='spacing pair', spacing=(0.5, 2.0))
    check(a, what='spacing scalar', spacing=0.25)
    check(a, what='spacing odd', spacing=(1.1, 0.3))
    cols, _ = check(a, ('inertia_tensor', 'centroid', 'area'), what='separator', separator='.')
    assert list(cols)[:5] == ['inertia_tensor.0.0', 'inertia_tensor.0.1', 'inertia_tensor.1.0', 'inertia_tensor.1.1', 'centroid.0']


def test_two_calls_give_identical_results():
    a = to_dev(disc_labels(1024, 1024, 2500, 3, seed=21, rmax=18.))
    img = torch.randint(0, 255, (1024, 1024, 2), dtype=torch.uint8, device=DEV)
    props = ALL_GEOMETRY + ('intensity_mean', 'intensity_max')
    c1, s1 = cda.region_properties(a, props, intensity_image=img, return_stats=True)
    c2, s2 = cda.region_properties(a, props, intensity_image=img, return_stats=True)
    assert s1 == s2 and s1['rows'] > 2000 and list(c1) == list(c2)
    for k in c1:
        assert torch.equal(c1[k].view(torch.int64) if c1[k].dtype == torch.float64 else c1[k],
                           c2[k].view(torch.int64) if c2[k].dtype == torch.float64 else c2[k]), k
    import celldetection_amd.torch_ops  # noqa: F401  (registers torch.ops.cpn_hip.region_properties)
    t = torch.ops.cpn_hip.region_properties(a, 'label,area,centroid', 1., 1.)
    assert t.dtype == torch.float64 and tuple(t.shape) == (s1['rows'], 4)
    assert torch.equal(t[:, 0], c1['label'].double()) and torch.equal(t[:, 3], c1['centroid-1'])


def test_end_to_end_on_device_tensors(monkeypatch):
    """model -> contours2labels -> resolve_label_channels -> table, for the channel image and the flat image."""
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
    props = ('label', 'bbox', 'area', 'centroid', 'orientation', 'axis_major_length', 'axis_minor_length')
    cols, st = cda.region_properties(labels, props, return_stats=True)
    fcols, fst = cda.region_properties(flat, props, return_stats=True)
    monkeypatch.setattr(torch.Tensor, 'cpu', orig_cpu)
    assert st['rows'] > 0 and fst['rows'] > 0 and all(v.is_cuda for v in cols.values())
    print(f'{tuple(labels.shape)}: {st}, flat {fst}')
    compare(cols, property_table(labels.cpu().numpy(), props)[0], 'model, channels')
    compare(fcols, property_table(flat.cpu().numpy(), props)[0], 'model, flat')
    tab = cda.labels2property_table(labels, props)
    assert len(tab) == st['rows'] and np.array_equal(tab['label'].to_numpy(), cols['label'].cpu().numpy())


def test_report_largest_distances():
    """Runs last in this file: the largest ulp distances the comparisons above met."""
    print(f'largest ulp distance: sqrt columns {worst["sqrt"]}, orientation {worst["orientation"]}')
    assert worst['sqrt'] <= SQRT_ULP and worst['orientation'] <= ORIENTATION_ULP
