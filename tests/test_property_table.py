"""Region property tables (celldetection_amd.region_properties / labels2property_table), CPU part.

``tests/golden/property_table.npz`` holds what the reference's own ``labels2property_table`` (celldetection/data/misc.py:320-347)
returned on small label images with ``tests/property_table_oracle.regionprops_table`` standing in for scikit-image's function
(``tests/golden/make_golden_property_table.py``): it pins the wrapper (call forms, channel loop, concatenation, index), not the
property arithmetic, which is this package's contract and is checked here against exact rational arithmetic.  The GPU tests
(``test_gpu_property_table.py``) compare the HIP path with the oracle and the fixture.
"""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import celldetection_amd as cda
from celldetection_amd import _lib, region_props
from property_table_oracle import (ALIASES, ALL_GEOMETRY, MUTANTS, SUPPORTED, accumulate, finalise, property_table, ulp_distance)
from test_instance_eval import disc_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'property_table.npz')


def load_fixture():
    """-> [dict(name, labels, properties, list_form, kwargs, columns, index, values)]."""
    g = np.load(GOLDEN)
    out = []
    for name in (str(c) for c in g['cases']):
        kw = {}
        if str(g[f'{name}.separator']) != '-':
            kw['separator'] = str(g[f'{name}.separator'])
        if g[f'{name}.spacing'].size:
            kw['spacing'] = tuple(float(s) for s in g[f'{name}.spacing'])
        if g[f'{name}.intensity_image'].size:
            kw['intensity_image'] = g[f'{name}.intensity_image']
        if str(g[f'{name}.df_dtype']):
            kw['df_kwargs'] = dict(dtype=np.dtype(str(g[f'{name}.df_dtype'])))
        cols = [str(c) for c in g[f'{name}.columns']]
        out.append(dict(name=name, labels=g[f'{name}.labels'], properties=[str(p) for p in g[f'{name}.properties']],
                        list_form=bool(g[f'{name}.list_form']), kwargs=kw, columns=cols, index=g[f'{name}.index'],
                        values={c: g[f'{name}.col.{c}'] for c in cols}))
    return out


def extra_cases():
    """Cases beside the fixture that the mutants need: (name, labels, properties, kwargs)."""
    tall = np.zeros((65536, 2), np.int32)  # two pixels far down: the sum of r^2 exceeds 2^32
    tall[65000:65002, 1] = 5
    low = disc_labels(30, 40, 8, 2, seed=1)
    low[low == 2] = -2
    return [('tall', tall, ALL_GEOMETRY, {}), ('nonpositive', low, ALL_GEOMETRY, dict(spacing=(3., .25)))]


def oracle_kwargs(kw):
    return {k: v for k, v in kw.items() if k != 'df_kwargs'}


def tables_equal(a, b):
    (ca, cha, ia), (cb, chb, ib) = a, b
    if list(ca) != list(cb) or not np.array_equal(cha, chb) or not np.array_equal(ia, ib):
        return False
    return all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x,
                                                                          y.view(np.int64) if y.dtype == np.float64 else y)
               for x, y in zip(ca.values(), cb.values()))


def test_fixture_reloads_and_matches_the_oracle():
    cases = {c['name']: c for c in load_fixture()}
    for name in ('image_2d', 'channels_repeated_label', 'list_form', 'df_kwargs', 'separator_spacing_intensity', 'empty_channel'):
        assert name in cases
    assert cases['image_2d']['labels'].ndim == 2 and 65537 in cases['image_2d']['values']['label']
    rep = cases['channels_repeated_label']
    lab = rep['values']['label']
    assert rep['labels'].shape[2] == 3 and len(set(lab.tolist())) == len(lab) - 1  # one label has two rows
    assert (np.diff(rep['index']) < 0).sum() == 2 and rep['index'][0] == 0  # the index restarts in every channel
    assert cases['list_form']['list_form'] and cases['list_form']['columns'][2] == 'local_centroid-0'  # old names are kept
    assert cases['df_kwargs']['values']['label'].dtype == np.float64
    assert 'max_intensity_1' in cases['separator_spacing_intensity']['columns']
    assert cases['empty_channel']['index'].tolist() == [0]
    for v in np.load(GOLDEN).values():
        assert v.dtype.kind in 'iufU'  # arrays and name lists only
    for c in load_fixture():
        cols, channel, index = property_table(c['labels'], c['properties'], **oracle_kwargs(c['kwargs']))
        assert list(cols) == c['columns'], c['name']
        assert np.array_equal(index, c['index']), c['name']
        for k, v in cols.items():
            ref = c['values'][k]
            if 'df_kwargs' in c['kwargs']:
                v = v.astype(c['kwargs']['df_kwargs']['dtype'])
            assert ref.dtype == v.dtype and np.array_equal(ref, v), (c['name'], k)


def brute_force(labels2d, v, img=None):
    """Exact rationals of one object from its pixels in bounding-box coordinates (spacing 1): the columns that are integers or a
    single rounding of an exact value, and the exact inertia tensor."""
    rs, cs = np.nonzero(labels2d == v)
    rs, cs = [int(r) for r in rs], [int(c) for c in cs]
    n, r0, c0, r1, c1 = len(rs), min(rs), min(cs), max(rs) + 1, max(cs) + 1
    lr, lc = [r - r0 for r in rs], [c - c0 for c in cs]
    mr, mc = Fraction(sum(lr), n), Fraction(sum(lc), n)
    exact = dict(label=v, bbox=(r0, c0, r1, c1), num_pixels=n, area=Fraction(n), area_bbox=Fraction((r1 - r0) * (c1 - c0)),
                 extent=Fraction(n, (r1 - r0) * (c1 - c0)), centroid=(Fraction(sum(rs), n), Fraction(sum(cs), n)),
                 centroid_local=(mr, mc))
    tensor = (sum((c - mc) ** 2 for c in lc) / n, -sum((r - mr) * (c - mc) for r, c in zip(lr, lc)) / n,
              sum((r - mr) ** 2 for r in lr) / n)
    if img is not None:
        px = [int(i) for i in img[rs, cs]]
        exact.update(intensity_mean=Fraction(sum(px), n), intensity_min=min(px), intensity_max=max(px))
    return exact, tensor, (sum(c * c for c in lc), sum(r * r for r in lr))


def test_oracle_agrees_with_exact_rationals():
    """Integer columns equal; area, area_bbox, extent, centroid, centroid_local, intensity_mean are ONE rounding of the exact
    value (spacing 1: every other step of their chains is exact), so they equal float(Fraction).  The inertia tensor takes
    three roundings of terms no larger than scc / n (srr / n, their mixed bound): within 4 * 2^-53 of that magnitude."""
    a = disc_labels(70, 90, 25, 2, seed=12, rmax=13.)
    a[:, :, 1] += (a[:, :, 1] > 0) * 70000
    a[60:, 80:, 0] = 2 ** 31 - 1
    img = np.random.default_rng(0).integers(-3000, 3000, a.shape[:2]).astype(np.int16)
    seen = 0
    for z in range(2):
        rows = accumulate(a[:, :, z], img)
        assert [r['label'] for r in rows] == sorted(set(a[:, :, z][a[:, :, z] > 0].tolist()))
        for row in rows:
            got = finalise(row)
            exact, (ta, tb, tc), (scc, srr) = brute_force(a[:, :, z], row['label'], img)
            for k, v in exact.items():
                want = tuple(float(x) if isinstance(x, Fraction) else x for x in v) if isinstance(v, tuple) else \
                    float(v) if isinstance(v, Fraction) else v
                assert got[k] == want, (z, row['label'], k, got[k], want)
            (ga, gb), (gb2, gc) = got['inertia_tensor']
            n = row['n']
            assert gb == gb2
            assert abs(Fraction(ga) - ta) <= Fraction(4, 2 ** 53) * Fraction(max(scc, 1), n)
            assert abs(Fraction(gc) - tc) <= Fraction(4, 2 ** 53) * Fraction(max(srr, 1), n)
            assert abs(Fraction(gb) - tb) <= Fraction(4, 2 ** 53) * Fraction(max(srr, scc, 1), n)
            seen += 1
    assert seen >= 12
    # a single pixel: zero tensor, eccentricity 0, the -pi / 4 rule; a horizontal and a vertical bar: orientation +-pi / 2 and 0
    one = finalise(accumulate(np.array([[0, 0], [0, 7]]))[0])
    assert one['inertia_tensor_eigvals'] == (0., 0.) and one['eccentricity'] == 0. and one['orientation'] == -np.pi / 4
    assert one['axis_major_length'] == 0. and one['bbox'] == (1, 1, 2, 2) and one['centroid'] == (1., 1.)
    bar = np.zeros((5, 9), int)
    bar[2, 1:8] = 1
    assert abs(abs(finalise(accumulate(bar)[0])['orientation']) - np.pi / 2) < 1e-12
    assert finalise(accumulate(bar.T)[0])['orientation'] == 0.
    assert finalise(accumulate(bar)[0])['eccentricity'] == 1.


@pytest.mark.parametrize('mutant', MUTANTS)
def test_cases_see_mutants_of_the_rule(mutant):
    assert set(MUTANTS) == {'swap_ac', 'sign_b', 'closed_bbox', 'spacing_once', 'centroid_no_spacing', 'sort_across_channels',
                            'count_nonpositive', 'sum32'}
    cases = [(c['name'], c['labels'], c['properties'], oracle_kwargs(c['kwargs'])) for c in load_fixture()] + extra_cases()
    differ = [name for name, a, props, kw in cases
              if not tables_equal(property_table(a, props, **kw), property_table(a, props, mutant=mutant, **kw))]
    print(f'mutant {mutant} differs on {differ}')
    assert differ


def test_header_binding_and_oracle_name_the_same_properties():
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r'#define\s+CPN_PROP_([A-Z0-9_]+)\s+(\d+)', hdr)}
    count = codes.pop('count')
    assert count == len(codes) == len(_lib.PROP_NAMES)
    assert codes == _lib.PROP_CODES and tuple(sorted(codes, key=codes.get)) == _lib.PROP_NAMES == SUPPORTED == region_props.SUPPORTED
    assert ALIASES == region_props.ALIASES
    dts = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+CPN_PROPS_([A-Z0-9]+)\s+(\d+)', hdr)}
    assert dts == dict(U8=_lib.PROPS_U8, I16=_lib.PROPS_I16, I32=_lib.PROPS_I32)
    assert _lib.ABI_VERSION >= 17
    lib = _lib.load()
    for name in ('cpn_props_workspace_bytes', 'cpn_props_columns', 'cpn_props_accumulate', 'cpn_props_table_status',
                 'cpn_props_compact_sort', 'cpn_props_finalise'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    # the column count of a property list is the binding's
    for props, K in ((('label', 'bbox'), 0), (SUPPORTED[:15], 0), (SUPPORTED, 1), (SUPPORTED, 3), (('inertia_tensor',), 0)):
        arr = (ctypes.c_int32 * len(props))(*[_lib.PROP_CODES[p] for p in props])
        names, kinds = region_props._column_names(region_props._resolve(props), '-', K)
        assert lib.cpn_props_columns(arr, len(props), K) == len(names) == len(kinds)
    arr = (ctypes.c_int32 * 1)(_lib.PROP_CODES['intensity_mean'])
    assert lib.cpn_props_columns(arr, 1, 0) == -1  # an intensity property without an intensity image
    arr = (ctypes.c_int32 * 1)(count)
    assert lib.cpn_props_columns(arr, 1, 0) == -1
    w = lib.cpn_props_workspace_bytes
    assert w(1024, 0) >= 64 + 1024 * 72 + 1024 * 8 and w(1024, 4) == w(1024, 0) + 1024 * 64 and w(4096, 0) > w(1024, 0)
    assert w(1000, 0) == 0 and w(1024, 5) == 0 and w(1 << 29, 0) == 0
    # argument checks answer before anything touches a device
    ws = ctypes.create_string_buffer(64)  # never dereferenced: the calls below fail on their arguments
    assert lib.cpn_props_accumulate(None, 65537, 1, 1, None, 0, 0, 1024, ws, 0, None) == _lib.E_UNSUPPORTED
    assert b'65536' in lib.cpn_last_error()
    assert lib.cpn_props_accumulate(None, 65536, 65536, 1, None, 0, 0, 1024, ws, 0, None) == _lib.E_UNSUPPORTED
    assert lib.cpn_props_accumulate(None, 8, 8, 12, None, 0, 0, 1024, ws, 0, None) == _lib.E_UNSUPPORTED
    assert lib.cpn_props_accumulate(None, 8, 8, 1, None, 0, 0, 1000, ws, 0, None) == _lib.E_INVALID
    assert lib.cpn_props_accumulate(None, 8, 8, 1, None, 0, 0, 1024, ws, 0, None) == _lib.E_WORKSPACE


def test_column_names():
    names = region_props._column_names
    res = region_props._resolve
    assert names(res(('label', 'bbox')), '-', 0)[0] == ['label', 'bbox-0', 'bbox-1', 'bbox-2', 'bbox-3']
    assert names(res(('inertia_tensor', 'local_centroid')), '_', 0)[0] == \
        ['inertia_tensor_0_0', 'inertia_tensor_0_1', 'inertia_tensor_1_0', 'inertia_tensor_1_1', 'local_centroid_0', 'local_centroid_1']
    assert names(res(('mean_intensity', 'intensity_max')), '-', 1) == (['mean_intensity', 'intensity_max'], ['f', 'v'])
    assert names(res(('mean_intensity', 'intensity_max')), '-', 2)[0] == ['mean_intensity-0', 'mean_intensity-1', 'intensity_max-0',
                                                                         'intensity_max-1']
    assert names(res('area'), '-', 0) == (['area'], ['f'])
    for old, new in ALIASES.items():
        assert res((old,)) == [(old, new)]


def test_no_cpu_fallback_and_argument_errors():
    assert 'region_properties' in cda.__all__ and 'labels2property_table' in cda.__all__
    a = torch.zeros((8, 9, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.region_properties(a)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.labels2property_table(a, 'label', 'area', spacing=(1., 2.))
    with pytest.raises(TypeError, match='integers'):
        cda.region_properties(a.float())
    with pytest.raises(TypeError, match='integers'):
        cda.labels2property_table(a.double(), ['label'])
    for bad in ('perimeter', 'image', 'coords', 'convex_area', 'solidity', 'euler_number', 'feret_diameter_max', 'moments_hu',
                'area_filled', 'perimeter_crofton', 'no_such_property'):
        with pytest.raises(NotImplementedError, match='supported: label, bbox, num_pixels') as e:
            cda.region_properties(a, ('label', bad))
        assert all(p in str(e.value) for p in SUPPORTED) and repr(bad) in str(e.value)
    with pytest.raises(NotImplementedError, match='iter_channels'):
        cda.region_properties(a, iter_channels=False)
    with pytest.raises(NotImplementedError, match='iter_channels'):
        cda.labels2property_table(a, 'label', iter_channels=False)
    with pytest.raises(NotImplementedError, match='65536'):
        cda.region_properties(torch.zeros((1, 65537), dtype=torch.int8))
    with pytest.raises(NotImplementedError, match=r'2 \*\* 31 - 1'):
        cda.region_properties(torch.zeros((1, 1), dtype=torch.int8).expand(65536, 32768))
    with pytest.raises(NotImplementedError, match='11 label channels'):
        cda.region_properties(torch.zeros((2, 2, 12), dtype=torch.int32))
    with pytest.raises(ValueError, match=r'\[H, W\]'):
        cda.region_properties(torch.zeros((2, 2, 2, 2), dtype=torch.int32))
    with pytest.raises(TypeError, match='unexpected keyword'):
        cda.labels2property_table(a, 'label', cachee=True)


def test_ulp_distance():
    x = np.array([1., -1., 0., 3.5])
    assert ulp_distance(x, x) == 0 and ulp_distance([0.], [-0.]) == 0
    assert ulp_distance([1.], [np.nextafter(1., 2.)]) == 1 and ulp_distance([-1.], [np.nextafter(-1., -2.)]) == 1
    assert ulp_distance([np.nextafter(0., 1.)], [-np.nextafter(0., 1.)]) == 2
    assert ulp_distance([1., 2.], [1., np.nextafter(np.nextafter(2., 3.), 3.)]) == 2
