"""Shape property tables (celldetection_amd.shape_properties / labels2property_table), CPU part.

scikit-image is not available: the contract is the "Shape property tables" block of include/cpn_hip.h, stated in numpy by
``tests/shape_props_oracle.py``.  Here that oracle is held against independent restatements (scikit-image's histogram forms of
the two perimeters with scipy.ndimage, 8-connected components minus 4-connected holes, scipy.spatial.ConvexHull with an exact
rational point test), against anchors computed by hand, and against its own mutants; ``csrc/hull_count.h`` (the routine every
lane of the hull kernel runs) is built for the host with sanitizers and run against brute force.  The GPU tests
(``test_gpu_shape_props.py``) compare the HIP path with the oracle.
"""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi
from scipy.spatial import ConvexHull

import celldetection_amd as cda
from celldetection_amd import _lib, region_props, shape_props
from property_table_oracle import ulp_distance
from shape_props_oracle import (ALIASES, MUTANTS, SUPPORTED, counts, crop, finalise, hull_lattice_count, object_properties,
                                shape_table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIMETER_ULP = 64  # at most 17 positive terms, each product and sum rounded once, in two different orders


def padded(mask, margin=3):
    return np.pad(np.asarray(mask, bool), margin)


def random_masks(count=300, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        h, w = rng.integers(1, 14, 2)
        m = rng.random((h, w)) < rng.choice([.2, .5, .8])
        if i % 3 == 0:
            m = ndi.binary_dilation(m, iterations=int(rng.integers(1, 3)))
        if not m.any():
            m[rng.integers(h), rng.integers(w)] = True
        out.append(m)
    return out


# restatements of scikit-image's own forms -------------------------------------------------------------------------------------
def skimage_perimeter(mask):
    """skimage.measure.perimeter(image, neighborhood=4): erosion, border image, weighted histogram of a 3 x 3 convolution."""
    image = np.asarray(mask).astype(np.uint8)
    strel = ndi.generate_binary_structure(2, 1)
    eroded = ndi.binary_erosion(image, strel, border_value=0)
    border = image - eroded
    weights = np.zeros(50, dtype=np.float64)
    weights[[5, 7, 15, 17, 25, 27]] = 1
    weights[[21, 33]] = np.sqrt(2)
    weights[[13, 23]] = (1 + np.sqrt(2)) / 2
    conv = ndi.convolve(border, np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]]), mode='constant', cval=0)
    hist = np.bincount(conv.ravel(), minlength=50)
    return float(hist[:50] @ weights)


def skimage_perimeter_crofton(mask):
    """skimage.measure.perimeter_crofton(image, directions=4): 16-bin histogram of the 2 x 2 configurations."""
    image = np.pad(np.asarray(mask).astype(np.uint8), 1)
    conv = ndi.convolve(image, np.array([[0, 0, 0], [0, 1, 4], [0, 2, 8]]), mode='constant', cval=0)
    hist = np.bincount(conv.ravel(), minlength=16)
    s2 = np.sqrt(2)
    coefs = np.array([0, np.pi / 4 * (1 + 1 / s2), np.pi / (4 * s2), np.pi / (2 * s2), 0, np.pi / 4 * (1 + 1 / s2), 0,
                      np.pi / (4 * s2), np.pi / 4, np.pi / 2, np.pi / (4 * s2), np.pi / (4 * s2), np.pi / 4, np.pi / 2, 0, 0])
    return float(coefs @ hist)


def euler_by_components(mask):
    """8-connected components minus 4-connected holes."""
    m = np.pad(np.asarray(mask, bool), 1)
    comps = ndi.label(m, structure=np.ones((3, 3)))[1]
    holes = ndi.label(~m, structure=ndi.generate_binary_structure(2, 1))[1] - 1  # the outside is no hole
    return comps - holes


def hull_by_scipy(mask, closed=True):
    """Lattice points in the hull that scipy.spatial.ConvexHull finds for the diamond points, decided with rationals."""
    rs, cs = np.nonzero(mask)
    pts = sorted({(Fraction(2 * r + dr, 2), Fraction(2 * c + dc, 2)) for r, c in zip(rs.tolist(), cs.tolist())
                  for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1))})
    hull = ConvexHull(np.array([[float(y), float(x)] for y, x in pts]))
    poly = [pts[i] for i in hull.vertices]
    n = 0
    for r in range(int(rs.min()) - 1, int(rs.max()) + 2):
        for c in range(int(cs.min()) - 1, int(cs.max()) + 2):
            cr = [(b[0] - a[0]) * (c - a[1]) - (b[1] - a[1]) * (r - a[0]) for a, b in zip(poly, poly[1:] + poly[:1])]
            n += all(x >= 0 for x in cr) or all(x <= 0 for x in cr) if closed else all(x > 0 for x in cr) or all(x < 0 for x in cr)
    return n


def test_oracle_agrees_with_the_restatements():
    worst = dict(perimeter=0, crofton=0)
    masks = random_masks()
    for i, m in enumerate(masks):
        variants = (m, m[::-1], m[:, ::-1], m.T) if i % 4 == 0 else (m,)
        for v in variants:
            cnt = counts(padded(v))
            got = finalise(cnt, hull_lattice_count(padded(v)))
            worst['perimeter'] = max(worst['perimeter'], ulp_distance([got['perimeter']], [skimage_perimeter(v)]))
            worst['crofton'] = max(worst['crofton'], ulp_distance([got['perimeter_crofton']], [skimage_perimeter_crofton(v)]))
            assert got['euler_number'] == euler_by_components(v), i
            assert cnt['q1'] - cnt['q3'] - 2 * cnt['qd'] == 4 * got['euler_number']
        if i < 120:
            assert hull_lattice_count(padded(m)) == hull_by_scipy(m), i
    print(f'largest distance from the histogram forms: perimeter {worst["perimeter"]} ulp, crofton {worst["crofton"]} ulp')
    assert worst['perimeter'] <= PERIMETER_ULP and worst['crofton'] <= PERIMETER_ULP


def disk(radius):
    yy, xx = np.mgrid[-radius - 2:radius + 3, -radius - 2:radius + 3]
    return yy ** 2 + xx ** 2 <= radius ** 2


def anchor(mask):
    mask = np.asarray(mask, bool)
    return finalise(counts(padded(mask)), hull_lattice_count(padded(mask)))


def test_hand_computed_anchors():
    s2, pi = np.sqrt(2.0), np.pi
    one = anchor([[1]])
    assert one['perimeter'] == 0. and one['euler_number'] == 1 and one['area_convex'] == 1. and one['solidity'] == 1.
    assert one['perimeter_crofton'] == (2. + 2. / s2) * (pi / 4.)
    sq = anchor(np.ones((2, 2)))
    assert sq['perimeter'] == 4. and sq['euler_number'] == 1 and sq['area_convex'] == 4.
    ring = np.ones((5, 5), int)
    ring[2, 2] = 0
    rg = anchor(ring)
    assert rg['perimeter'] == 16. and rg['euler_number'] == 0 and rg['area_convex'] == 25. and rg['solidity'] == 24. / 25.
    dg = anchor(np.eye(3))
    assert dg['perimeter'] == 1. * s2 and dg['euler_number'] == 1 and dg['area_convex'] == 3.
    corners = np.zeros((3, 3), int)
    corners[::2, ::2] = 1
    cn = anchor(corners)
    assert cn['euler_number'] == 4 and cn['area_convex'] == 9.
    ell = np.array([[1, 0, 0], [1, 0, 0], [1, 1, 1]])
    assert anchor(ell)['area_convex'] == 6.
    d = anchor(disk(100))
    circ = 2 * pi * 100
    assert abs(d['perimeter'] / circ - 1.0532) < 5e-4, d['perimeter'] / circ
    assert abs(d['perimeter_crofton'] / circ - 1.0028) < 5e-4, d['perimeter_crofton'] / circ
    assert d['euler_number'] == 1
    # the predicate is SAME LABEL: a pixel enclosed by another label is a full object, and the enclosing ring has a hole
    a = np.full((5, 5), 7)
    a[2, 2] = 9
    inner, outer = object_properties(a, 9), object_properties(a, 7)
    assert inner == anchor([[1]]) and outer['euler_number'] == 0 and outer['perimeter'] == 16.
    # a lattice point exactly on a hull edge that is no pixel of the object: the closed hull counts it
    two = np.zeros((3, 3), int)
    two[0, 0] = two[2, 2] = 1
    assert anchor(two)['area_convex'] == 3. and anchor(two)['num_pixels'] == 2
    # spacing: lengths scale with s, areas with sy * sx, the Euler number not at all
    sp = finalise(counts(padded(ring)), 25, (0.5, 0.5))
    assert sp['perimeter'] == 8. and sp['area_convex'] == 6.25 and sp['euler_number'] == 0 and sp['solidity'] == 24. / 25.


def mutant_cases():
    """(name, label image, spacing)"""
    rng = np.random.default_rng(3)
    touching = np.zeros((9, 12), np.int32)
    touching[1:8, 1:6], touching[2:7, 6:11] = 1, 2  # two labels side by side
    border = np.zeros((6, 7), np.int32)
    border[0:4, 0:3], border[2:6, 4:7] = 3, 5       # objects on the image border
    noise = (rng.random((12, 15)) < .55).astype(np.int32) * 4
    cross = np.zeros((7, 7), np.int32)
    cross[3, :], cross[:, 3] = 6, 6
    cross[0, 0] = cross[6, 6] = 6
    checker = (np.indices((6, 6)).sum(0) % 2).astype(np.int32) * 8
    return [('touching', touching, (1., 1.)), ('border', border, (1., 1.)), ('noise', noise, (1., 1.)), ('cross', cross, (1., 1.)),
            ('checker', checker, (1., 1.)), ('spacing', touching, (.5, .5)), ('line', np.eye(5, dtype=np.int32), (1., 1.))]


@pytest.mark.parametrize('mutant', MUTANTS)
def test_cases_see_mutants_of_the_rule(mutant):
    assert set(MUTANTS) >= {'foreground', 'erosion8', 'border_inside', 'euler_plus_qd', 'crofton_two', 'open_hull', 'hull_centres',
                            'spacing_ignored', 'spacing_squared'}
    differ = []
    for name, a, spacing in mutant_cases():
        good, _ = shape_table(a, SUPPORTED, spacing)
        bad, _ = shape_table(a, SUPPORTED, spacing, mutant=mutant)
        if any(not np.array_equal(good[k], bad[k], equal_nan=True) for k in good):
            differ.append(name)
    print(f'mutant {mutant} differs on {differ}')
    assert differ


def host_masks():
    rng = np.random.default_rng(11)
    masks = []
    for i in range(160):
        h, w = (int(v) for v in rng.integers(1, 41, 2))
        m = np.zeros((h, w), np.int32)
        k = int(rng.integers(1, 120))
        m[rng.integers(0, h, k), rng.integers(0, w, k)] = 1  # sparse: fragmented, with empty rows
        masks.append(m)
    for i in range(40):
        h, w = (int(v) for v in rng.integers(3, 41, 2))
        yy, xx = np.mgrid[:h, :w]
        cy, cx, ry, rx = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1, h / 2 + 1), rng.uniform(1, w / 2 + 1)
        m = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1).astype(np.int32)
        if not m.any():
            m[h // 2, w // 2] = 1
        masks.append(m)
    # collinear cases: lattice points exactly on a hull edge that are no pixels of the object
    for n, step in ((9, 2), (13, 3), (21, 4)):
        m = np.zeros((n, n), np.int32)
        m[::step, ::step] = np.eye(len(range(0, n, step)), dtype=np.int32)
        masks += [m, m[::-1].copy()]
    m = np.zeros((5, 9), np.int32)
    m[0, 0] = m[4, 8] = m[0, 8] = 1  # slope 2: the edge passes through (1, 2), (2, 4), (3, 6)
    masks += [m, m.T.copy(), np.ones((1, 40), np.int32), np.ones((40, 1), np.int32), np.ones((40, 40), np.int32)]
    return masks


def test_host_build_of_the_hull_count_agrees_with_brute_force(tmp_path):
    """``csrc/hull_count.h`` compiled for the host only, with AddressSanitizer and UBSan on the host code, by ``tests/hull_count_host.cpp`` (a program of
    its own, nothing preloaded): all 65536 masks of 4 x 4 against brute force inside the program, and the masks written here
    against brute force and against the oracle."""
    from celldetection_amd.build import _hipcc
    exe, data = str(tmp_path / 'hull_count_host'), str(tmp_path / 'masks.txt')
    hipcc = _hipcc()
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(ROOT, 'tests', 'hull_count_host.cpp'), '-o', exe])
    run = subprocess.run([exe, 'all4x4'], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == 'ok 65536', run.stdout[-500:] + run.stderr[-2000:]
    masks = host_masks()
    with open(data, 'w') as f:
        f.write(f'{len(masks)}\n')
        for m in masks:
            f.write(f'{m.shape[0]} {m.shape[1]}\n' + ' '.join(str(int(v)) for v in m.reshape(-1)) + '\n')
    run = subprocess.run([exe, 'file', data], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-500:] + run.stderr[-2000:]
    lines = run.stdout.split('\n')[:-1]
    assert len(lines) == len(masks) > 200
    brute = 0
    for i, (line, m) in enumerate(zip(lines, masks)):
        got, bf = (int(v) for v in line.split())
        assert got == hull_lattice_count(padded(m)), (i, m.shape, got)
        if bf >= 0:
            assert got == bf, (i, m.shape, got, bf)
            brute += 1
    assert brute >= 200


def test_header_binding_and_exports_agree():
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r'#define\s+CPN_SHAPE_([A-Z0-9_]+)\s+(\d+)', hdr)}
    count = codes.pop('count')
    assert count == len(codes) == len(_lib.SHAPE_NAMES)
    assert codes == _lib.SHAPE_CODES and tuple(sorted(codes, key=codes.get)) == _lib.SHAPE_NAMES == SUPPORTED == shape_props.SUPPORTED
    assert ALIASES == shape_props.ALIASES == dict(convex_area='area_convex')
    assert _lib.ABI_VERSION >= 22
    lib = _lib.load()
    for name in ('cpn_shape_workspace_bytes', 'cpn_shape_columns', 'cpn_shape_heights', 'cpn_shape_accumulate',
                 'cpn_shape_hull_scratch_bytes', 'cpn_shape_hull', 'cpn_shape_finalise'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    arr = (ctypes.c_int32 * 7)(*range(7))
    assert lib.cpn_shape_columns(arr, 7) == 7 and lib.cpn_shape_columns(arr, 0) == 0 and lib.cpn_shape_columns(None, 1) == -1
    assert lib.cpn_shape_columns((ctypes.c_int32 * 1)(count), 1) == -1 and lib.cpn_shape_columns((ctypes.c_int32 * 1)(-1), 1) == -1
    w = lib.cpn_shape_workspace_bytes
    assert w(1024) >= 1024 * (7 * 4 + 8) and w(4096) > w(1024) and w(1000) == 0 and w(1 << 29) == 0
    assert lib.cpn_shape_hull_scratch_bytes(3, 10) >= 4 * 2 * (2 * 10 + 3) and lib.cpn_shape_hull_scratch_bytes(-1, 0) == 0
    # the existing table keeps its layout
    assert lib.cpn_props_workspace_bytes(1024, 0) == 64 + 1024 * 72 + 1024 * 8
    # argument checks answer before anything touches a device (the buffers are never dereferenced)
    ws = ctypes.create_string_buffer(64)
    acc = lib.cpn_shape_accumulate
    assert acc(None, 65537, 1, 1, ws, 1024, 0, 0, ws, 0, None, None, 0, None) == _lib.E_UNSUPPORTED
    assert b'65536' in lib.cpn_last_error()
    assert acc(None, 8, 8, 12, ws, 1024, 0, 0, ws, 0, None, None, 0, None) == _lib.E_UNSUPPORTED
    assert acc(None, 8, 8, 1, ws, 1000, 0, 0, ws, 0, None, None, 0, None) == _lib.E_INVALID
    assert acc(None, 8, 8, 1, None, 1024, 0, 0, ws, 0, None, None, 0, None) == _lib.E_INVALID
    assert acc(None, 8, 8, 1, ws, 1024, 0, 2000, ws, 0, None, None, 0, None) == _lib.E_INVALID
    assert acc(None, 8, 8, 1, ws, 1024, 0, 0, ws, 0, None, None, 0, None) == _lib.E_WORKSPACE
    assert lib.cpn_shape_heights(None, 1024, 0, 1, ws, None) == _lib.E_INVALID
    assert lib.cpn_shape_hull(1, ws, ws, 5, ws, 8, ws, None) == _lib.E_WORKSPACE
    assert lib.cpn_shape_hull(-1, ws, ws, 5, ws, 8, ws, None) == _lib.E_INVALID
    fin = lib.cpn_shape_finalise
    one = (ctypes.c_int32 * 1)(_lib.SHAPE_CODES['perimeter'])
    assert fin(ws, 1024, 0, 1, ws, None, one, 1, 1., 2., ws, 2, None) == _lib.E_UNSUPPORTED
    assert b'isotropic' in lib.cpn_last_error()
    assert fin(ws, 1024, 0, 1, ws, None, one, 1, 1., 1., ws, 3, None) == _lib.E_INVALID
    assert fin(ws, 1024, 0, 1, ws, None, (ctypes.c_int32 * 1)(count), 1, 1., 1., ws, 2, None) == _lib.E_INVALID
    hull = (ctypes.c_int32 * 1)(_lib.SHAPE_CODES['solidity'])
    assert fin(ws, 1024, 0, 1, ws, None, hull, 1, 1., 2., ws, 2, None) == _lib.E_INVALID  # no hull counts
    assert b'cpn_shape_hull' in lib.cpn_last_error()


def test_no_cpu_fallback_and_argument_errors():
    assert 'shape_properties' in cda.__all__ and 'shape_props' in cda.__all__
    a = torch.zeros((8, 9, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.shape_properties(a)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.shape_properties(a, SUPPORTED + ('convex_area',), spacing=.5)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.labels2property_table(a, 'label', 'area', 'perimeter', 'solidity')
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.labels2property_table(a, 'euler_number', 'convex_area', 'centroid', spacing=(1., 2.))  # no length: any spacing
    with pytest.raises(TypeError, match='integers'):
        cda.shape_properties(a.float())
    # anisotropic spacing is refused for the two perimeters, as scikit-image refuses it
    for name in ('perimeter', 'perimeter_crofton'):
        with pytest.raises(NotImplementedError, match='isotropic spacings only'):
            cda.shape_properties(a, ('label', name), spacing=(1., 2.))
        with pytest.raises(NotImplementedError, match='isotropic spacings only'):
            cda.labels2property_table(a, 'label', 'area', name, spacing=(1., 2.))
    # names refused everywhere
    for bad in ('feret_diameter_max', 'area_filled', 'moments', 'moments_hu', 'moments_central', 'image', 'image_convex', 'coords',
                'no_such_property'):
        with pytest.raises(NotImplementedError, match='supported: label, num_pixels, perimeter') as e:
            cda.shape_properties(a, ('label', bad))
        assert all(p in str(e.value) for p in SUPPORTED) and repr(bad) in str(e.value)
        with pytest.raises(NotImplementedError, match='supported: label, bbox, num_pixels'):
            cda.labels2property_table(a, 'label', 'perimeter', bad)
        with pytest.raises(NotImplementedError, match='supported: label, bbox, num_pixels'):
            cda.region_properties(a, ('label', bad))
    with pytest.raises(TypeError):
        cda.shape_properties(a, ('perimeter',), neighborhood=8)
    # region_properties keeps refusing the shape names, and says where they are
    for name in SUPPORTED[2:] + ('convex_area',):
        with pytest.raises(NotImplementedError, match='supported: label, bbox, num_pixels') as e:
            cda.region_properties(a, ('label', name))
        assert 'shape_properties' in str(e.value)
    with pytest.raises(NotImplementedError, match='area'):
        cda.shape_properties(a, ('label', 'area'))


def test_column_names_and_dtypes():
    res = shape_props._resolve
    assert shape_props._column_names(res(SUPPORTED)) == (list(SUPPORTED), ['i', 'i', 'f', 'f', 'i', 'f', 'f'])
    assert shape_props._column_names(res(('convex_area', 'label'))) == (['convex_area', 'label'], ['f', 'i'])
    assert res('perimeter') == [('perimeter', 'perimeter')] and res(('convex_area',)) == [('convex_area', 'area_convex')]
    assert [shape_props.shape_only(p) for p in ('label', 'num_pixels', 'area', 'perimeter', 'convex_area', 'solidity', 'bbox')] == \
        [False, False, False, True, True, True, False]
    assert not set(SUPPORTED[2:]) & set(region_props.SUPPORTED) and not set(ALIASES) & set(region_props.ALIASES)
    cols, channel = shape_table(np.array([[1, 1, 0], [0, 2, 2]]), SUPPORTED + ('convex_area',))
    assert list(cols) == list(SUPPORTED) + ['convex_area'] and channel.tolist() == [0, 0]
    assert [cols[k].dtype for k in cols] == [np.int64, np.int64, np.float64, np.float64, np.int64, np.float64, np.float64, np.float64]
    assert cols['label'].tolist() == [1, 2] and cols['euler_number'].tolist() == [1, 1] and cols['area_convex'].tolist() == [2., 2.]
