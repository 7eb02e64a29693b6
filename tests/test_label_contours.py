"""Contours of label images (celldetection_amd.labels2contours / resample_contours), CPU part.

``tests/golden/label_contours.npz`` holds what the reference's own ``labels2contours`` / ``labels2contour_list``
(celldetection/data/cpn.py:93-144) and ``resample_contours`` (celldetection/data/misc.py:371-405) returned on small cases
(``tests/golden/make_golden_label_contours.py``; ``cv2.findContours`` and ``regionprops`` restated there, so the border following
is unpinned and the reference's wrapper and all of ``resample_contours`` are pinned).  This file shows that the numpy restatement
of both rules (``tests/label_contours_oracle.py``) reproduces every fixture value exactly, that the fixture tells wrong rules from
the right ones, that a filled contour restores its object, and that ``csrc/contour_trace.h``, compiled for the host, follows
borders like the restatement; the GPU tests (``test_gpu_label_contours.py``) then use the fixture and the restatement.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import celldetection_amd as cda
import label_contours_oracle as oracle
from celldetection_amd import _lib
from labels_oracle import fill_polygon
from test_instance_eval import disc_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'label_contours.npz')
LABEL_CASES = ('anchor_square', 'anchor_row', 'anchor_plus', 'anchor_single', 'borders', 'two_channels_skip', 'two_channels_flag',
               'two_channels_raise', 'fragmented_flag', 'fragmented_skip', 'fragmented_raise', 'discs_c1', 'discs_c3', 'discs_c4',
               'ragged')
RESAMPLE_CASES = ('traced_below', 'traced_at', 'traced_above', 'traced_list', 'traced_open', 'doubled_point',
                  'float_closed_below', 'float_closed_at', 'float_closed_above', 'float_open_below', 'float_open_at',
                  'float_open_above', 'float_epsilon', 'batch', 'one_sample', 'ties')
ANCHORS = {'anchor_square': [(2, 1), (2, 2), (3, 2), (3, 1)], 'anchor_row': [(1, 1), (2, 1), (3, 1), (2, 1)],
           'anchor_plus': [(1, 0), (0, 1), (1, 2), (2, 1)], 'anchor_single': [(2, 1), (2, 1)]}


def load_label_fixture():
    """-> [(name, labels [H, W, C], keywords, None (the reference raises) or (ids, offsets, points, labels afterwards))]."""
    g = np.load(GOLDEN)
    out = []
    for name in (str(c) for c in g['label_cases']):
        kw = dict(flag_fragmented_inplace=bool(g[f'{name}.flag']), raise_fragmented=bool(g[f'{name}.raise']),
                  constant=int(g[f'{name}.constant']))
        ref = None if bool(g[f'{name}.raises']) else tuple(g[f'{name}.{k}'] for k in ('ids', 'offsets', 'points', 'labels_after'))
        out.append((name, g[f'{name}.labels'], kw, ref))
    return out


def load_resample_fixture():
    """-> [(name, contours (a list of [n, 2] arrays, or an array [..., n, 2]), num, close, epsilon, result [K, num, 2])]."""
    g = np.load(GOLDEN)
    out = []
    for name in (str(c) for c in g['resample_cases']):
        ends = np.cumsum(g[f'{name}.lengths'])
        contours = [g[f'{name}.points'][e - n:e] for e, n in zip(ends, g[f'{name}.lengths'])]
        lead = tuple(int(i) for i in g[f'{name}.lead'])
        if lead != (-1,):
            contours = np.stack(contours).reshape(lead + contours[0].shape)
        out.append((name, contours, int(g[f'{name}.num']), bool(g[f'{name}.close']), float(g[f'{name}.epsilon']), g[f'{name}.result']))
    return out


def run_oracle(labels, kw, mutant=None):
    a = labels.copy()
    try:
        return oracle.labels2contours_packed(a, mutant=mutant, **kw) + (a,)
    except ValueError:
        return None


def test_fixture_covers_the_cases():
    lab = {c[0]: c for c in load_label_fixture()}
    assert tuple(lab) == LABEL_CASES
    for name in ('two_channels_raise', 'fragmented_raise'):
        assert lab[name][3] is None
    b = lab['borders'][1][:, :, 0]
    for corner in (b[0, 0], b[0, -1], b[-1, 0], b[-1, -1]):
        assert corner > 0
    for edge in (b[0, 1:-1], b[-1, 1:-1], b[1:-1, 0], b[1:-1, -1]):
        assert len(set(edge[edge > 0].tolist())) >= 2  # the corner objects reach along the border; one more object in between
    assert (b < 0).any() and len(lab['borders'][3][0]) == 9
    two = lab['two_channels_skip']
    both = set(two[1][:, :, 0][two[1][:, :, 0] > 0].tolist()) & set(two[1][:, :, 1][two[1][:, :, 1] > 0].tolist())
    assert both == {3, 5} and two[3][0].tolist() == [2, 3, 5, 9]
    flagged = lab['two_channels_flag']
    assert (flagged[3][3] == -7).sum() == (flagged[1] == 5).sum() and ((flagged[3][3] == -7) == (flagged[1] == 5)).all()
    assert [lab[f'discs_c{c}'][1].shape[2] for c in (1, 3, 4)] == [1, 3, 4]
    assert not np.array_equal(lab['discs_c3'][3][0], np.asarray(list(dict.fromkeys(  # ascending is not the order of appearance
        v for c in range(3) for v in np.unique(lab['discs_c3'][1][:, :, c]).tolist() if v > 0))))
    res = {c[0]: c for c in load_resample_fixture()}
    assert tuple(res) == RESAMPLE_CASES
    n = len(res['traced_at'][1][0])
    assert (res['traced_below'][2] < n, res['traced_at'][2] == n, res['traced_above'][2] > n) == (True, True, True)
    assert res['float_open_at'][3] is False and res['float_closed_at'][3] is True and res['float_open_at'][1][0].dtype == np.float64
    assert res['traced_list'][1][0].dtype == np.int32 and len({len(c) for c in res['traced_list'][1]}) > 5
    assert res['batch'][1].shape == (2, 3, 9, 2) and res['batch'][5].shape == (6, 7, 2)
    for v in np.load(GOLDEN).values():
        assert v.dtype.kind in 'iufbU'  # arrays only
    assert os.path.getsize(GOLDEN) <= 150 * 1024


def test_restatement_reproduces_the_reference_fixture():
    for name, labels, kw, ref in load_label_fixture():
        out = run_oracle(labels, kw)
        assert (out is None) == (ref is None), name
        if ref is not None:
            for a, b in zip(out, ref):
                assert a.dtype == b.dtype and np.array_equal(a, b), name
            lst = oracle.labels2contour_list(labels.copy(), **kw)
            assert all(np.array_equal(c, ref[2][a:b]) for c, a, b in zip(lst, ref[1][:-1], ref[1][1:])), name
    for name, contours, num, close, eps, ref in load_resample_fixture():
        out = np.asarray(oracle.resample_contours(contours, num, close, eps), np.float64).reshape(-1, num, 2)
        assert out.shape == ref.shape and np.array_equal(out, ref), name


@pytest.mark.parametrize('mutant', oracle.MUTANTS)
def test_fixture_sees_mutants_of_the_rules(mutant):
    """Contours: traced clockwise, a 4-connected search, the leftmost instead of the raster-first start pixel, thin parts visited
    once, a single point not doubled, result order by first appearance, fragmentation judged 4-connected.  Resampling: not
    closed, ``<`` for ``<=`` in the search, ``epsilon`` left out, ``t_j`` from ``num - 1`` intervals."""
    assert set(oracle.CONTOUR_MUTANTS) == {'clockwise', 'four_connected', 'wrong_start', 'thin_once', 'single_not_doubled',
                                           'first_appearance', 'frag_four'}
    assert set(oracle.RESAMPLE_MUTANTS) == {'resample_open', 'search_lt', 'no_epsilon', 't_num_minus_1'}
    n = 0
    if mutant in oracle.CONTOUR_MUTANTS:
        for name, labels, kw, ref in load_label_fixture():
            out = run_oracle(labels, kw, mutant)
            n += not ((out is None) == (ref is None) and (ref is None or all(np.array_equal(a, b) for a, b in zip(out, ref))))
    else:
        for name, contours, num, close, eps, ref in load_resample_fixture():
            out = np.asarray(oracle.resample_contours(contours, num, close, eps, mutant=mutant), np.float64).reshape(-1, num, 2)
            n += not np.array_equal(out, ref, equal_nan=True)
    print(f'mutant {mutant} differs on {n} cases')
    assert n > 0


def test_anchors():
    """The orderings worked out from the rule by hand; the first is the well-known one of cv2."""
    lab = {c[0]: c for c in load_label_fixture()}
    for name, pts in ANCHORS.items():
        ids, offsets, points, _ = lab[name][3]
        assert points.tolist() == [list(p) for p in pts] and offsets.tolist() == [0, len(pts)] and len(ids) == 1, name
        assert oracle.labels2contour_list(lab[name][1][:, :, 0])[0].tolist() == [list(p) for p in pts], name


def test_abi_header_bindings_and_exports_agree():
    names = ('cpn_contours_workspace_bytes', 'cpn_contours_components', 'cpn_contours_table', 'cpn_contours_count',
             'cpn_contours_write', 'cpn_resample_contours')
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    assert _lib.ABI_VERSION >= 20
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    assert int(re.search(r'#define\s+CPN_CONTOURS_TILE\s+(\d+)', hdr).group(1)) == cda.label_contours.TILE
    assert int(re.search(r'#define\s+CPN_E_INTERNAL\s+\((-\d+)\)', hdr).group(1)) == _lib.E_INTERNAL
    flat_hdr = re.sub(r'\s*\n \*\s*', ' ', hdr)
    for phrase in ('raster-first', 'clockwise on screen', 'counter-clockwise', 'starting after the pixel just left', 'fragmented',
                   'hole of another component'):  # the rule is stated in the header and in the module text
        assert phrase in flat_hdr and phrase in ' '.join(cda.label_contours.__doc__.split()), phrase
    assert {'label_contours', 'labels2contours', 'resample_contours'} <= set(cda.__all__)
    assert cda.labels2contours is cda.label_contours.labels2contour_list  # cd.data.labels2contours is that function
    assert cda.resample_contours is cda.label_contours.resample_contours
    import celldetection_amd.torch_ops  # noqa: F401  (registers the operators)
    assert torch.ops.celldetection_amd.labels2contours_packed.default and torch.ops.celldetection_amd.resample_contours.default
    # argument checks answer before anything touches a device (the buffers are never dereferenced)
    buf = ctypes.create_string_buffer(4096)
    status = (ctypes.c_int64 * 2)()
    assert lib.cpn_contours_workspace_bytes(0) >= 64 and lib.cpn_contours_workspace_bytes(1000) > 1000 * 48
    assert lib.cpn_contours_components(buf, 0, 8, 8, buf, buf, 4096, status, None) == _lib.E_INVALID
    assert lib.cpn_contours_components(buf, 1, 65536, 65536, buf, buf, 4096, status, None) == _lib.E_UNSUPPORTED
    assert b'2^31 - 1' in lib.cpn_last_error()
    assert lib.cpn_contours_components(buf, 1, 8, 8, buf, buf, 8, status, None) == _lib.E_WORKSPACE
    assert lib.cpn_contours_components(buf, 1, 0, 8, buf, buf, 4096, status, None) == 0 and status[0] == 0  # no pixel
    assert lib.cpn_contours_table(buf, 1, 8, 8, buf, -1, buf, buf, buf, 4096, status, None) == _lib.E_INVALID
    assert lib.cpn_contours_table(buf, 1, 8, 8, buf, 1000, buf, buf, buf, 4096, status, None) == _lib.E_WORKSPACE
    assert lib.cpn_contours_table(buf, 1, 8, 8, buf, 0, buf, buf, buf, 4096, status, None) == 0  # no component
    assert lib.cpn_contours_count(buf, 1, 8, 8, -1, buf, buf, buf, buf, buf, buf, 4096, status, None) == _lib.E_INVALID
    assert lib.cpn_contours_write(buf, 1, 8, 8, 1, buf, buf, buf, buf, None, buf, 4096, None) == _lib.E_INVALID
    assert lib.cpn_contours_write(buf, 1, 8, 8, 0, buf, buf, buf, buf, buf, buf, 4096, None) == 0
    assert lib.cpn_resample_contours(buf, buf, 1, 4, 0, 1, 1e-6, buf, buf, None) == _lib.E_INVALID
    assert lib.cpn_resample_contours(None, buf, 1, 4, 8, 1, 1e-6, buf, buf, None) == _lib.E_INVALID
    assert lib.cpn_resample_contours(buf, buf, 0, 0, 8, 1, 1e-6, buf, buf, None) == 0


def test_no_cpu_fallback_and_argument_errors():
    lab = torch.zeros((8, 9, 2), dtype=torch.int32)
    for fn in (cda.labels2contours, cda.label_contours.labels2contours, cda.label_contours.labels2contours_packed):
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(lab)
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(lab, flag_fragmented_inplace=True, raise_fragmented=False, constant=-2)
        with pytest.raises(TypeError, match='integers'):
            fn(lab.float())
        with pytest.raises(TypeError, match='integers'):
            fn(lab.bool())
        with pytest.raises(ValueError, match=r'\[H, W, C\]'):
            fn(lab[0, 0])
        with pytest.raises(TypeError, match='Tensor'):
            fn(lab.numpy())
        for kw in (dict(mode=1), dict(mode=2), dict(mode=3)):  # RETR_LIST, RETR_CCOMP, RETR_TREE
            with pytest.raises(NotImplementedError, match='RETR_EXTERNAL'):
                fn(lab, **kw)
        for kw in (dict(method=2), dict(method=3), dict(method=4)):  # CHAIN_APPROX_SIMPLE, TC89_L1, TC89_KCOS
            with pytest.raises(NotImplementedError, match='CHAIN_APPROX_NONE'):
                fn(lab, **kw)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.labels2contours(lab[:, :, 0])  # [H, W] is accepted by the list form ...
    with pytest.raises(ValueError, match=r'\[H, W, C\]'):
        cda.label_contours.labels2contours_packed(lab[:, :, 0])  # ... only
    con = torch.zeros((3, 8, 2))
    for num in (None, 2.5, 1.):
        with pytest.raises(NotImplementedError, match='num'):
            cda.resample_contours(con, num)
        with pytest.raises(NotImplementedError, match='num'):
            cda.resample_contours([con[0]], num=num)
    with pytest.raises(NotImplementedError, match='num'):
        cda.resample_contours(con)
    with pytest.raises(ValueError, match='positive'):
        cda.resample_contours(con, 0)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.resample_contours(con, 16)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.resample_contours([con[0], con[1, :5]], 16, close=False, epsilon=1e-3, dtype=torch.float32)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.label_contours.resample_contours_packed(con.reshape(-1, 2), torch.tensor([0, 8, 24]), 16)
    with pytest.raises(ValueError, match=r'\[\.\.\., n, 2\]'):
        cda.resample_contours(torch.zeros((3, 8, 3)), 16)
    with pytest.raises(ValueError, match=r'\[n, 2\]'):
        cda.resample_contours([torch.zeros((8, 3))], 16)
    with pytest.raises(TypeError, match='Tensor'):
        cda.resample_contours(np.zeros((8, 2)), 16)


def round_trip_objects():
    """-> (image int32 [H, W], value) of 8-connected objects on grids up to 23 x 23: at least 337 from seeded disc images (discs
    cut by the border and by each other) and 300 ragged random-walk objects."""
    out = []
    for seed in range(200):
        rng = np.random.default_rng(seed)
        h, w = int(rng.integers(5, 24)), int(rng.integers(5, 24))
        img = disc_labels(h, w, 8, 1, seed, rmin=1., rmax=6.)[:, :, 0]
        for v in np.unique(img[img > 0]).tolist():
            if len(oracle.components((img == v).astype(np.int64))) == 1:
                out.append((img, v))
    n_discs = len(out)
    for seed in range(300):
        rng = np.random.default_rng(1000 + seed)
        h, w = int(rng.integers(3, 24)), int(rng.integers(3, 24))
        out.append((oracle.ragged_object(rng, h, w, int(rng.integers(1, 120))).astype(np.int32) * 5, 5))
    return out, n_discs


def test_filled_contour_restores_the_object_with_its_holes_filled():
    objects, n_discs = round_trip_objects()
    assert n_discs >= 337 and len(objects) - n_discs == 300
    holes = wrong = 0
    for img, v in objects:
        mask = img == v
        contour = oracle.labels2contour_list(np.where(mask, img, 0))[0]
        full = oracle.fill_holes(mask)
        holes += bool((full != mask).any())
        wrong += not np.array_equal(fill_polygon(contour, 0, 0, img.shape[1], img.shape[0]), full)
    print(f'{len(objects)} objects, {holes} with holes, {wrong} mismatches')
    assert wrong == 0 and holes > 20


def host_images():
    """Images whose values > 0 are one component each: the fixture's single-channel cases without fragmented objects, objects on
    all four borders and in the corners, a full image, single rows and columns, and the round-trip objects."""
    imgs = [labels[:, :, 0] for name, labels, kw, ref in load_label_fixture()
            if labels.shape[2] == 1 and ref is not None and not name.startswith('fragmented')]
    imgs += [np.ones((1, 1), np.int32), np.ones((1, 7), np.int32), np.ones((7, 1), np.int32), np.ones((5, 6), np.int32) * 3,
             np.eye(6, dtype=np.int32) * 2, np.fliplr(np.eye(5, dtype=np.int32))]
    frame = np.ones((9, 8), np.int32)
    frame[1:-1, 1:-1] = 0  # a ring along all four borders
    imgs.append(frame)
    imgs += [np.where(img == v, img, 0) for img, v in round_trip_objects()[0][::7]]
    return imgs


def test_host_build_of_the_tracer_follows_borders_like_the_restatement(tmp_path):
    """``csrc/contour_trace.h`` (the code every lane of the trace kernel runs) compiled for the host by
    ``tests/contour_trace_host.cpp``, on images written here."""
    from celldetection_amd.build import _hipcc
    exe, data = str(tmp_path / 'contour_trace_host'), str(tmp_path / 'images.txt')
    hipcc = _hipcc()
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(ROOT, 'tests', 'contour_trace_host.cpp'), '-o', exe])
    imgs = host_images()
    with open(data, 'w') as f:
        f.write(f'{len(imgs)}\n')
        for img in imgs:
            f.write(f'{img.shape[0]} {img.shape[1]}\n' + ' '.join(str(int(v)) for v in img.reshape(-1)) + '\n')
    run = subprocess.run([exe, data], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-500:] + run.stderr[-500:]
    expected = []
    for i, img in enumerate(imgs):
        expected.append(f'image {i}')
        ids, offsets, points = oracle.labels2contours_packed(img[:, :, None].copy())
        for k, v in enumerate(ids.tolist()):
            expected.append(f'value {v} {offsets[k + 1] - offsets[k]}')
            expected += [f'{x} {y}' for x, y in points[offsets[k]:offsets[k + 1]].tolist()]
    got = run.stdout.split('\n')[:-1]
    assert len(imgs) > 100 and len(got) == len(expected) and got == expected
