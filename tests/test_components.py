"""Component labelling (celldetection_amd.components: label_components, relabel_, stack_labels, masks2labels, ...), CPU part.

``tests/golden/components.npz`` holds what the reference's own ``relabel_``, ``stack_labels``, ``masks2labels``,
``unary_masks2labels`` and ``rgb_to_scalar`` returned (``tests/golden/make_golden_components.py``: skimage's and OpenCV's labelling
replaced by stand-ins on scipy.ndimage).  Here ``tests/components_oracle.py`` -- a sequential union-find that shares no code with
those stand-ins -- is held against every recorded result and against its own mutants; the header, the binding and the argument
checks are held against each other; ``csrc/component_rank.h`` (the rank arithmetic of the numbering kernels) is built for the
host with sanitizers and run against brute force.  The GPU tests (``test_gpu_components.py``) compare the HIP path with the oracle
and the fixture.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import celldetection_amd as cda
import components_oracle as oracle
from celldetection_amd import _lib, build, components

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_fixture():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'components.npz'))


def relabel_cases(z=None):
    z = load_fixture() if z is None else z
    return [(str(n), z[f'relabel.{n}.labels'], z[f'relabel.{n}.result']) for n in z['relabel_cases']]


def stack_cases(z=None):
    z = load_fixture() if z is None else z
    out = []
    for n in z['stack_cases']:
        count, relabel = (int(v) for v in z[f'stack.{n}.params'])
        out.append((str(n), [z[f'stack.{n}.map{i}'] for i in range(count)], dict(relabel=bool(relabel), dtype=str(z[f'stack.{n}.dtype'])),
                    z[f'stack.{n}.result']))
    return out


def mask_cases(z=None):
    z = load_fixture() if z is None else z
    out = []
    for n in z['mask_cases']:
        conn, axis, reduce, keep = (int(v) for v in z[f'masks.{n}.params'])
        out.append((str(n), z[f'masks.{n}.masks'], dict(connectivity=conn, label_axis=axis, reduce='max' if reduce else None,
                                                        keepdims=bool(keep)), z[f'masks.{n}.result'], int(z[f'masks.{n}.count'])))
    return out


def test_fixture_has_the_cases_the_rule_needs():
    z = load_fixture()
    cases = relabel_cases(z)
    assert {a.shape[2] for _, a, _ in cases} == {1, 2, 3, 4}
    assert any((a < 0).any() and (a == 0).any() for _, a, _ in cases)
    many = dict((n, r) for n, _, r in cases)['many_components']
    assert len(np.unique(many[:, :, 0])) > 1000 and many.dtype == np.int32
    masks = dict((n, m) for n, m, _, _, _ in mask_cases(z))['blobs_c8']
    assert not masks[1].any() and masks[3].all() and masks[0].any() and masks[4].any()  # in the middle of the stack
    assert any(not kw['relabel'] for _, _, kw, _ in stack_cases(z)) and any(m.ndim == 3 for _, maps, _, _ in stack_cases(z) for m in maps)
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'components.npz')) < \
        os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'objective.npz')) / 2


def test_oracle_equals_every_recorded_result():
    z = load_fixture()
    for name, a, want in relabel_cases(z):
        assert np.array_equal(oracle.relabel(a), want), name                      # the reference's loop on the union-find
        got, counts = oracle.label_components(a, 8, 'equal', 1)                   # the rule
        assert np.array_equal(got, want) and got.dtype == want.dtype, name
        assert counts.sum() == (want.max() if (want > 0).any() else 0), name
        assert np.array_equal(got <= 0, a <= 0) and np.array_equal(got[a <= 0], a[a <= 0]), name
    for name, maps, kw, want in stack_cases(z):
        got = oracle.stack_labels(*maps, dtype=kw['dtype'], relabel_stack=kw['relabel'])
        assert np.array_equal(got, want) and got.dtype == want.dtype, name
    for name, masks, kw, want, cnt in mask_cases(z):
        got, n = oracle.masks2labels(masks, count=True, **dict(kw, reduce=np.max if kw['reduce'] else None))
        assert np.array_equal(got, want) and got.dtype == want.dtype == np.int32 and n == cnt, name
    assert np.array_equal(oracle.rgb_to_scalar(z['rgb.input']), z['rgb.result'])
    assert np.array_equal(oracle.rgb_to_scalar(z['rgb.input'], 'int64'), z['rgb.result_int64']) and z['rgb.result_int64'].dtype == np.int64
    for transpose, key in ((True, 'unary.transposed'), (False, 'unary.plain')):
        got = oracle.unary_masks2labels(z['unary.masks'], transpose)
        assert np.array_equal(got, z[key]) and got.dtype == z[key].dtype


def test_fixture_tells_wrong_rules_apart():
    z = load_fixture()
    differs = {m: [] for m in oracle.MUTANTS}
    for name, a, want in relabel_cases(z):
        for m in oracle.MUTANTS:
            if not m.startswith('cnt_') and not np.array_equal(oracle.label_components(a, 8, 'equal', 1, mutant=m)[0], want):
                differs[m].append(name)
    for name, masks, kw, want, cnt in mask_cases(z):
        for m in ('cnt_empty_repaired', 'cnt_full_repaired'):
            got, n = oracle.masks2labels(masks, count=True, mutant=m, **dict(kw, reduce=np.max if kw['reduce'] else None))
            if not np.array_equal(got, want):  # the labels, not only the count
                differs[m].append(name)
    print({m: len(v) for m, v in differs.items()})
    assert len(oracle.MUTANTS) >= 9 and all(differs.values()), differs


def test_relabel_is_idempotent_and_keeps_the_partition():
    for name, a, want in relabel_cases():
        assert np.array_equal(oracle.relabel(want), want), name
        got, _ = oracle.label_components(want, 8, 'equal', 1)
        assert np.array_equal(got, want), name
        for c in range(a.shape[2]):  # every new object is one component of one old value
            pos = want[:, :, c] > 0
            pairs = np.unique(np.stack([want[:, :, c][pos], a[:, :, c][pos]], 1), axis=0)
            assert len(pairs) == len(np.unique(pairs[:, 0])), name
    # first, connectivity and mode of the primitive
    a = np.array([[1, 0, 2], [0, 1, 0], [-3, 0, 1]], np.int32)[:, :, None]
    assert oracle.label_components(a, 8, 'equal', 5)[0][:, :, 0].tolist() == [[5, 0, 6], [0, 5, 0], [-3, 0, 5]]
    assert oracle.label_components(a, 4, 'equal', 1)[0][:, :, 0].tolist() == [[1, 0, 2], [0, 3, 0], [-3, 0, 4]]
    assert oracle.label_components(a, 8, 'nonzero', 1)[0][:, :, 0].tolist() == [[1, 0, 1], [0, 1, 0], [1, 0, 1]]
    assert oracle.label_components(a, 4, 'nonzero', 1)[1].tolist() == [5]


def test_abi_header_bindings_and_exports_agree():
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    lib = _lib.load()
    for name in ('cpn_components_workspace_bytes', 'cpn_components_label'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    modes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r'#define\s+CPN_COMPONENTS_([A-Z]+)\s+(\d+)', hdr)}
    assert modes == _lib.COMPONENTS_MODES == dict(equal=_lib.COMPONENTS_EQUAL, nonzero=_lib.COMPONENTS_NONZERO)
    flat_hdr = re.sub(r'\s*\n \*\s*', ' ', hdr)
    doc = ' '.join(components.__doc__.split())
    assert 'Component labelling' in flat_hdr
    for phrase in ('by channel ascending', 'raster index', 'keep their value', 'the order within a mask'):
        assert phrase in flat_hdr and phrase in doc, phrase
    assert 'components.hip' in build.SOURCES and {'components.h', 'component_rank.h'} <= set(build.HEADERS)
    names = {'label_components', 'relabel_', 'stack_labels', 'rgb_to_scalar', 'unary_masks2labels', 'masks2labels', 'fill_label_gaps_',
             'remove_partials_'}
    assert names | {'components'} <= set(cda.__all__) and names == set(components.__all__)
    for n in names:
        assert getattr(cda, n) is getattr(components, n)
    # the shared pass is one file: label_contours.hip holds no union-find of its own any more
    src = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'label_contours.hip')).read()
    assert '#include "components.h"' in src and 'uf_union' not in src and 'cc_components_pass<8, CC_EQUAL>' in src
    # argument checks answer before anything touches a device (the buffers are never dereferenced)
    w = lib.cpn_components_workspace_bytes
    assert w(3, 100, 100) >= 3 * 100 * 100 * 4 + 2 * 8 * 3 * 40 and w(1, 0, 0) > 0
    assert w(0, 8, 8) == w(65536, 8, 8) == w(1, -1, 8) == w(1, 65536, 65536) == 0
    buf = ctypes.create_string_buffer(4096)
    call = lambda *a: lib.cpn_components_label(*a)
    ok = dict(ps=3, cs=1, C=3, H=8, W=8, conn=8, mode=0, first=1, ops=3, ocs=1)

    def rc(**kw):
        a = dict(ok, **kw)
        return call(buf, a['ps'], a['cs'], a['C'], a['H'], a['W'], a['conn'], a['mode'], a['first'], buf, a['ops'], a['ocs'],
                    a.get('counts', buf), a.get('ws', buf), None)

    assert rc(C=0) == rc(C=65536) == rc(H=-1) == _lib.E_INVALID
    assert rc(C=1, H=65536, W=65536, ps=1, ops=1) == _lib.E_UNSUPPORTED and b'2^31 - 1' in lib.cpn_last_error()
    assert rc(conn=6) == rc(conn=0) == _lib.E_INVALID and b'connectivity' in lib.cpn_last_error()
    assert rc(mode=2) == rc(mode=-1) == _lib.E_INVALID and b'mode' in lib.cpn_last_error()
    assert rc(first=0) == rc(first=-5) == _lib.E_INVALID and b'first' in lib.cpn_last_error()
    assert rc(ps=2) == rc(cs=2) == rc(ps=1, cs=63) == rc(ops=2) == rc(ops=1, ocs=8) == _lib.E_INVALID
    assert b'strides' in lib.cpn_last_error()
    assert rc(counts=None) == rc(ws=None) == _lib.E_INVALID


def test_no_cpu_fallback_and_argument_errors():
    lab = torch.zeros((8, 9, 2), dtype=torch.int32)
    for fn in (cda.label_components, cda.relabel_, cda.fill_label_gaps_, cda.remove_partials_):
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(lab)
        with pytest.raises(TypeError, match='integers'):
            fn(lab.float())
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.masks2labels(lab.permute(2, 0, 1))
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.unary_masks2labels([lab[:, :, 0], lab[:, :, 1]])
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.stack_labels(lab[:, :, 0], lab[:, :, 1])
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.rgb_to_scalar(torch.zeros((4, 4, 3), dtype=torch.uint8))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='MI355X'):  # a numpy array is uploaded: that needs the GPU
            cda.relabel_(np.zeros((4, 4, 1), np.int32))
    for axis in (0, 1, -2, 3):
        with pytest.raises(NotImplementedError, match='only the last axis'):
            cda.relabel_(lab, axis=axis)
        with pytest.raises(NotImplementedError, match='only the last axis'):
            cda.stack_labels(lab[:, :, 0], axis=axis)
    with pytest.raises(ValueError, match=r'\[H, W, C\]'):
        cda.relabel_(lab[:, :, 0])
    for kw in (dict(connectivity=6), dict(connectivity=True), dict(connectivity='8')):
        with pytest.raises(ValueError, match='connectivity must be 4 or 8'):
            cda.label_components(lab, **kw)
        with pytest.raises(ValueError, match='connectivity must be 4 or 8'):
            cda.masks2labels(lab.permute(2, 0, 1), **kw)
    for mode in ('same', 0, None):
        with pytest.raises(ValueError, match="'equal' or 'nonzero'"):
            cda.label_components(lab, mode=mode)
    for first in (0, -1, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError, match='first must be'):
            cda.label_components(lab, first=first)
    with pytest.raises(ValueError, match='out must be'):
        cda.label_components(lab, out=torch.zeros((8, 9, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match='out must be'):
        cda.label_components(lab, out=torch.zeros((8, 9, 1), dtype=torch.int32))
    for reduce in (np.min, np.sum, max, 'min', lambda x, **kw: x):
        with pytest.raises(TypeError, match="'max', np.max or None"):
            cda.masks2labels(lab.permute(2, 0, 1), reduce=reduce)
    with pytest.raises(ValueError, match='label_axis'):
        cda.masks2labels(lab.permute(2, 0, 1), label_axis=3)
    with pytest.raises(ValueError, match=r'\[N, H, W\]'):
        cda.masks2labels(lab[:, :, 0])
    with pytest.raises(ValueError, match='at least one'):
        cda.masks2labels([])
    with pytest.raises(TypeError):
        cda.masks2labels(lab.permute(2, 0, 1), ltype=4)  # no keywords for cv2
    with pytest.raises(TypeError, match='integer dtype'):
        cda.stack_labels(lab[:, :, 0], dtype='float32')
    with pytest.raises(ValueError, match=r'\[H, W\] or \[H, W, 3\]'):
        cda.stack_labels(lab)
    with pytest.raises(ValueError, match='at least one'):
        cda.stack_labels()
    with pytest.raises(ValueError, match=r'\[\.\.\., 3\]'):
        cda.rgb_to_scalar(torch.zeros((4, 4, 2), dtype=torch.uint8))


def test_host_build_of_the_block_ranks_agrees_with_brute_force(tmp_path):
    """``csrc/component_rank.h`` compiled for the host only, with AddressSanitizer and UBSan on the host code, by
    ``tests/component_rank_host.cpp`` (a program of its own, nothing preloaded): all 65536 masks of 16 root flags spread over a
    block, 2000 random blocks and the rank encoding, against brute force inside the program."""
    hipcc = build._hipcc()
    exe = str(tmp_path / 'component_rank_host')
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(ROOT, 'tests', 'component_rank_host.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == 'ok 65536 2000', run.stdout[-500:] + run.stderr[-2000:]
