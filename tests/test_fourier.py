"""Elliptic Fourier descriptors of contours (celldetection_amd.efd / contours2fourier / labels2fourier), CPU part.

``tests/golden/fourier.npz`` holds what the reference's own ``efd`` and ``contours2fourier`` (celldetection/data/cpn.py:23-90, 213-227)
returned on small cases (``tests/golden/make_golden_fourier.py``; pure numpy, so fully pinned).  This file shows that the numpy
restatement (``tests/fourier_oracle.py``) reproduces every recorded value bit for bit, that ``truth`` (mpmath, 40 digits) agrees with
hand-worked anchors, MEASURES the constants of the bound, shows that the bound rejects wrong rules, and runs ``csrc/efd_chunks.h``
(the chunk decomposition of the kernels) on the host within the bound.

The bound.  numpy's sum is pairwise and its sin / cos are glibc's, so bit equality with the kernels is not possible.  Results are
judged against ``truth`` in the unit ``U = 2^-53 N T`` of each contour: every coefficient has ``|value - truth| <= c_f U``, every
location component ``|value - truth| <= c_l U + 2^-53 |truth|``; contours with ``N <= 1`` are exact.  ``c_f`` and ``c_l`` are 4 x the
largest ratio that the reference's own float64 result shows over all contours of the fixture and of the GPU test's generators
(margin 4: the kernel differs from the reference in summation order and in the sin / cos implementation, each of which may cost
about as much as the reference's own rounding; nothing else may differ).  ``python tests/test_fourier.py`` measures them and writes
``tests/golden/fourier_measured.json``; the test here measures again and holds the committed constants to the measurement.
"""
import ctypes
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import celldetection_amd as cda
import fourier_oracle as oracle
from celldetection_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'fourier.npz')
MEASURED = os.path.join(ROOT, 'tests', 'golden', 'fourier_measured.json')
EFD_CASES = ('open_int', 'closed_int', 'closed_no_autoclose', 'one_point', 'doubled_point', 'two_points', 'three_points',
             'dense_closed', 'dense_one_open', 'object_list', 'float_16000_loose', 'float_16000_apart', 'float_small', 'order_1',
             'order_5', 'order_10', 'order_25', 'epsilon_1e-3', 'two_chunks')
C2F_CASES = ('gaps', 'one', 'empty')
MARGIN = 4.


def load_efd_fixture():
    """-> [(name, contours (a list of [n, 2] arrays, or an array [..., n, 2]), order, epsilon, autoclose, coefficients [K, order,
    4], locations [K, 2])]."""
    g = np.load(GOLDEN)
    out = []
    for name in (str(c) for c in g['efd_cases']):
        ends = np.cumsum(g[f'efd.{name}.lengths'])
        contours = [g[f'efd.{name}.points'][e - n:e] for e, n in zip(ends, g[f'efd.{name}.lengths'])]
        lead = tuple(int(i) for i in g[f'efd.{name}.lead'])
        if lead != (-1,):
            contours = np.stack(contours).reshape(lead + contours[0].shape)
        out.append((name, contours, int(g[f'efd.{name}.order']), float(g[f'efd.{name}.epsilon']), bool(g[f'efd.{name}.autoclose']),
                    g[f'efd.{name}.coefficients'], g[f'efd.{name}.locations']))
    return out


def load_c2f_fixture():
    """-> [(name, dict label -> array [n, 1, 2] or [n, 2], order, fouriers f64, locations f64, fouriers f32, locations f32)]."""
    g = np.load(GOLDEN)
    out = []
    for name in (str(c) for c in g['c2f_cases']):
        ends = np.cumsum(g[f'c2f.{name}.lengths'])
        contours = {}
        for key, e, n, sq in zip(g[f'c2f.{name}.keys'].tolist(), ends, g[f'c2f.{name}.lengths'], g[f'c2f.{name}.squeeze']):
            c = g[f'c2f.{name}.points'][e - n:e]
            contours[key] = c[:, None] if sq else c
        out.append((name, contours, int(g[f'c2f.{name}.order'])) + tuple(g[f'c2f.{name}.{k}'] for k in
                                                                         ('fouriers', 'locations', 'fouriers_f32', 'locations_f32')))
    return out


def fixture_contours():
    """Every contour of the efd fixture on its own -> [(name, contour [n, 2], append, order, epsilon, coefficients, location)];
    ``append``: whether the reference appended the first point (a dense array decides once for all its members)."""
    out = []
    for name, contours, order, eps, autoclose, coeff, loc in load_efd_fixture():
        if isinstance(contours, list):
            members, appends = contours, [not oracle.is_closed(c) for c in contours]
        else:
            members = list(contours.reshape((-1,) + contours.shape[-2:]))
            appends = [not oracle.is_closed(contours)] * len(members)
        out += [(f'{name}[{i}]', c, a, order, eps, coeff[i], loc[i]) for i, (c, a) in enumerate(zip(members, appends))]
    return out


def segments(contour, append):
    return len(contour) - 1 + bool(append)


@functools.lru_cache(maxsize=None)
def generator_cases():
    """The contours of the GPU test's generators -> [(name, contour, append, order, epsilon)]."""
    out = []
    for c in oracle.edge_contours():
        a = not oracle.is_closed(c)
        out += [(f'edge{segments(c, a)}.order{o}', c, a, o, 1e-6) for o in (1, 5, oracle.MAX_ORDER)]
    out.append(('long', oracle.long_contour(), True, 3, 1e-6))
    points, offsets = oracle.tiny_contours()
    for k in oracle.tiny_sample().tolist():
        c = points[offsets[k]:offsets[k + 1]]
        out.append((f'tiny{k}', c, not oracle.is_closed(c), 5, 1e-6))
    return out


@functools.lru_cache(maxsize=None)
def truths():
    """name -> truth of every contour the bound is measured over (computed once, shared by the tests)."""
    out = {name: oracle.truth(c, order, eps, a) for name, c, a, order, eps, _, _ in fixture_contours()}
    out.update({name: oracle.truth(c, order, eps, a) for name, c, a, order, eps in generator_cases()})
    return out


@functools.lru_cache(maxsize=None)
def measure():
    """The reference's own float64 error over all those contours, in units of U -> {'c_f', 'c_l', 'cases': name -> ratios}."""
    cases = {}
    ref = truths()
    for name, c, a, order, eps, coeff, loc in fixture_contours():
        if segments(c, a) >= 2:
            rf, _, rl = oracle.ratios(coeff, loc, ref[name])  # the recorded reference result itself
            cases[name] = [rf, rl]
    for name, c, a, order, eps in generator_cases():
        if segments(c, a) >= 2:
            coeff, loc = oracle.efd(c, order, eps)  # bit-equal to the reference (test_restatement_...)
            rf, _, rl = oracle.ratios(coeff, loc, ref[name])
            cases[name] = [rf, rl]
    return {'c_f': MARGIN * max(v[0] for v in cases.values()), 'c_l': MARGIN * max(v[1] for v in cases.values()), 'cases': cases}


def constants():
    with open(MEASURED) as f:
        m = json.load(f)
    return float(m['c_f']), float(m['c_l'])


def within(coeff, loc, ref, what):
    """Asserts the bound for one contour; a failure names the contour, the order and the coefficient."""
    c_f, c_l = constants()
    rf, at, rl = oracle.ratios(coeff, loc, ref)
    assert rf <= c_f, f'{what}: coefficient k={at[0] + 1} j={at[1]} is {rf:.3g} U from the truth (bound {c_f:.3g} U)'
    assert rl <= c_l, f'{what}: location is {rl:.3g} U (+ 2^-53 |truth|) from the truth (bound {c_l:.3g} U)'
    return rf, rl


def test_fixture_covers_the_cases():
    efd = {c[0]: c for c in load_efd_fixture()}
    assert tuple(efd) == EFD_CASES and tuple(c[0] for c in load_c2f_fixture()) == C2F_CASES
    assert oracle.is_closed(efd['closed_int'][1]) and not oracle.is_closed(efd['open_int'][1])
    assert [len(efd[k][1]) for k in ('one_point', 'doubled_point', 'two_points', 'three_points')] == [1, 2, 2, 3]
    assert (efd['one_point'][5] == 0).all() and np.isnan(efd['one_point'][6]).all()
    assert (efd['doubled_point'][5] == 0).all() and efd['doubled_point'][6].tolist() == [[7., 9.]]
    one_open = efd['dense_one_open'][1]
    assert one_open.shape == (3, 9, 2) and [oracle.is_closed(c) for c in one_open] == [True, False, True]
    assert efd['dense_closed'][1].shape == (3, 1, 9, 2) and oracle.is_closed(efd['dense_closed'][1])
    assert isinstance(efd['object_list'][1], list) and len({len(c) for c in efd['object_list'][1]}) == 6
    loose, apart = efd['float_16000_loose'][1], efd['float_16000_apart'][1]
    assert loose.dtype == np.float64 and oracle.is_closed(loose) and not oracle.is_closed(apart)
    assert 0.05 < np.abs(loose[0] - loose[-1]).max() < 0.16 and loose.min() > 15900
    assert [efd[f'order_{o}'][2] for o in (1, 5, 10, 25)] == [1, 5, 10, 25] and efd['epsilon_1e-3'][3] == 1e-3
    assert len(efd['two_chunks'][1]) == oracle.CHUNK + 44 and efd['closed_no_autoclose'][4] is False
    gaps = load_c2f_fixture()[0]
    assert list(gaps[1]) == [2, 5, 9, 6] and gaps[3].shape == (9, 5, 4) and gaps[5].dtype == np.float32
    assert {v.ndim for v in gaps[1].values()} == {2, 3}
    for v in np.load(GOLDEN).values():
        assert v.dtype.kind in 'iufbU'  # arrays only
    assert os.path.getsize(GOLDEN) <= 100 * 1024


def test_restatement_reproduces_the_reference_fixture():
    for name, contours, order, eps, autoclose, coeff, loc in load_efd_fixture():
        with np.errstate(all='ignore'):
            c, l = oracle.efd(contours, order, eps, autoclose)
        assert np.array_equal(np.reshape(c, coeff.shape), coeff, equal_nan=True), name
        assert np.array_equal(np.reshape(l, loc.shape), loc, equal_nan=True), name
    for name, contours, order, f64, l64, f32, l32 in load_c2f_fixture():
        for dtype, f, l in ((np.float64, f64, l64), (np.float32, f32, l32)):
            out = oracle.contours2fourier(contours, order, dtype)
            assert out[0].dtype == dtype and np.array_equal(out[0], f) and np.array_equal(out[1], l), name
    with pytest.raises(AssertionError):
        oracle.efd(load_efd_fixture()[0][1], 5, 1e-6, autoclose=False)  # an open contour without autoclose


def test_truth_agrees_with_hand_worked_anchors():
    pi = np.pi
    # the unit square with epsilon = 0: T = 4, phi_(k,i) = k pi i / 2, one non-zero difference per segment
    square = np.asarray([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64)
    coeff, loc, U = oracle.truth(square, 6, 0.)
    for k in range(1, 7):
        c, s = (lambda i: np.cos(k * pi * i / 2)), (lambda i: np.sin(k * pi * i / 2))
        ck = 4 / (2 * k * k * pi * pi)
        want = [ck * ((c(1) - c(0)) - (c(3) - c(2))), ck * ((s(1) - s(0)) - (s(3) - s(2))),
                ck * ((c(2) - c(1)) - (c(4) - c(3))), ck * ((s(2) - s(1)) - (s(4) - s(3)))]
        assert np.allclose(coeff[k - 1], want, rtol=0, atol=1e-15), k
    assert np.allclose(coeff[0], [-4 / pi ** 2, 4 / pi ** 2, -4 / pi ** 2, -4 / pi ** 2], rtol=0, atol=1e-15)
    assert np.allclose(coeff[1], 0, atol=1e-15) and loc.tolist() == [0.5, 0.5] and U == 2. ** -53 * 4 * 4
    # a regular 64-gon: the polygon is the linear interpolation of 64 samples of a circle, whose first harmonic is the circle's
    # times sinc^2(pi / 64); the second harmonic vanishes.  (The float64 vertices are off the circle by ~1e-16 R.)
    M, R = 64, 10.
    theta = 2 * pi * np.arange(M) / M
    gon = np.stack([R * np.cos(theta), R * np.sin(theta)], -1)
    coeff, loc, _ = oracle.truth(gon, 2, 0.)
    first = R * (np.sin(pi / M) / (pi / M)) ** 2
    assert np.allclose(coeff[0], [first, 0, 0, first], rtol=0, atol=1e-13) and np.allclose(coeff[1], 0, atol=1e-13)
    assert np.allclose(loc, 0, atol=1e-13)
    # a translated copy moves only the location (integer points and shift: the differences are the same numbers)
    walk = oracle.ragged_walk(40, 9, center=(50, 60)).astype(np.float64)
    a, b = oracle.truth(walk, 5, 1e-6), oracle.truth(walk + (1000, -30), 5, 1e-6)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2] and np.allclose(b[1] - a[1], (1000, -30), rtol=0, atol=2e-13)
    # N <= 1
    assert np.isnan(oracle.truth(square[:1], 3, 1e-6)[1]).all()
    coeff, loc, _ = oracle.truth(np.asarray([[7, 9], [7, 9]]), 3, 1e-6)
    assert (coeff == 0).all() and loc.tolist() == [7., 9.]


def test_bound_constants_are_the_measured_ones():
    """Measures the reference's own error (4 x its largest ratio is the constant) and holds the committed file to it.  numpy's sum
    and sin / cos may round differently on another CPU, so the committed constants are compared with a factor, not bit for bit:
    the reference's largest ratio measured here has to lie within [1/4, 1] of the committed constant / 4 ... x 1."""
    m = measure()
    c_f, c_l = constants()
    worst_f, worst_l = m['c_f'] / MARGIN, m['c_l'] / MARGIN
    print(f'measured: c_f = {m["c_f"]:.4g}, c_l = {m["c_l"]:.4g} over {len(m["cases"])} contours; committed: {c_f:.4g}, {c_l:.4g}')
    assert len(m['cases']) > 250 and 0 < c_f < MARGIN and 0 < c_l < MARGIN  # (the issue expects c below 1 x margin)
    assert c_f / MARGIN / 4 <= worst_f <= c_f and c_l / MARGIN / 4 <= worst_l <= c_l
    with open(MEASURED) as f:
        assert set(json.load(f)['cases']) == set(m['cases'])


@pytest.mark.parametrize('mutant', oracle.MUTANTS)
def test_bound_rejects_mutants_of_the_rule(mutant):
    """float32 arithmetic, epsilon dropped from dt, no closing segment, T without the last segment, 1/k for 1/k^2, dcos and dsin
    swapped, location without the first point, X_(i-1) for X_i: each exceeds the bound on every fixture contour with N >= 3.
    (Evaluated at order >= 2: at order 1 the rules 1/k and 1/k^2 are the same rule.)"""
    c_f, c_l = constants()
    n = 0
    for name, c, a, order, eps, _, _ in fixture_contours():
        if segments(c, a) < 3:
            continue
        order = max(order, 2)
        ref = truths()[name] if order == truths()[name][0].shape[0] else oracle.truth(c, order, eps, a)
        pts = np.concatenate([c, c[:1]]) if a else c
        with np.errstate(all='ignore'):
            coeff, loc = oracle.efd(pts, order, eps, autoclose=False, mutant=mutant)
        rf, _, rl = oracle.ratios(coeff, loc, ref)
        assert rf > c_f or rl > c_l, f'{mutant} passes on {name}: {rf:.3g} U, {rl:.3g} U'
        n += 1
    assert n >= 20


def pack_for_host(contours, order, eps):
    lines = [f'{len(contours)} {order} {eps!r}']
    for c, a in contours:
        lines.append(f'{len(c)} {segments(c, a)}')
        lines.append(' '.join(repr(float(v)) for v in np.asarray(c, np.float64).reshape(-1)))
    return '\n'.join(lines) + '\n'


def test_host_build_of_the_chunk_decomposition_is_within_the_bound(tmp_path):
    """``csrc/efd_chunks.h`` (the decomposition, the order of summation and the per-segment arithmetic of the kernels) compiled for
    the host by ``tests/efd_chunks_host.cpp`` and run sequentially: contours of 1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK,
    2 CHUNK + 1 and 5 CHUNK + 7 segments within the bound, every one bit-identical at another position of the packed batch."""
    from celldetection_amd.build import _hipcc
    exe = str(tmp_path / 'efd_chunks_host')
    hipcc = _hipcc()
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-ffp-contract=off', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(ROOT, 'tests', 'efd_chunks_host.cpp'), '-o', exe])
    assert int(subprocess.run([exe, 'chunk'], capture_output=True, text=True).stdout) == oracle.CHUNK
    C = oracle.CHUNK
    wanted = [1, 2, 3, C - 1, C, C + 1, 2 * C, 2 * C + 1, 5 * C + 7]
    batch = [(c, not oracle.is_closed(c)) for c in oracle.edge_contours() if segments(c, not oracle.is_closed(c)) in wanted]
    assert [segments(c, a) for c, a in batch] == wanted
    batch.append((np.asarray([[4, 5]]), False))  # one point: N = 0
    order, eps = 5, 1e-6

    def run(contours):
        path = str(tmp_path / 'contours.txt')
        with open(path, 'w') as f:
            f.write(pack_for_host(contours, order, eps))
        r = subprocess.run([exe, 'efd', path], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-500:]
        return [[float.fromhex(v) for v in line.split()] for line in r.stdout.split('\n')[:-1]]

    out = run(batch)
    assert len(out) == len(batch)
    for (c, a), row in zip(batch, out):
        coeff, loc, N = np.asarray(row[:-2]).reshape(order, 4), np.asarray(row[-2:]), segments(c, a)
        if N == 0:
            assert (coeff == 0).all() and np.isnan(loc).all()
        elif N == 1:
            assert (coeff == 0).all() and loc.tolist() == c[0].tolist()
        else:
            rf, rl = within(coeff, loc, truths()[f'edge{N}.order5'], f'host, {N} segments, order {order}')
            print(f'host {N} segments: {rf:.3g} U, {rl:.3g} U')
    shuffled = [batch[i] for i in (9, 8, 3, 0, 7, 1, 6, 2, 5, 4)]
    again = run(shuffled)
    for i, j in enumerate((9, 8, 3, 0, 7, 1, 6, 2, 5, 4)):
        assert np.array_equal(np.asarray(again[i]), np.asarray(out[j]), equal_nan=True), j
    # the checks of offsets every index rests on
    for offsets, P, want in (([0, 3, 7], 7, 'ok'), ([1, 3, 7], 7, 'bad'), ([0, 3, 7], 8, 'bad'), ([0, 5, 3, 7], 7, 'bad'),
                             ([0, 3, 3, 7], 7, 'bad'), ([0, 9, 7], 7, 'bad'), ([0, -2, 7], 7, 'bad')):
        path = str(tmp_path / 'offsets.txt')
        with open(path, 'w') as f:
            f.write(f'{len(offsets) - 1} {P}\n' + ' '.join(str(o) for o in offsets) + '\n')
        assert subprocess.run([exe, 'offsets', path], capture_output=True, text=True).stdout.strip() == want, offsets


def test_abi_header_bindings_and_exports_agree():
    names = ('cpn_efd_workspace_bytes', 'cpn_efd')
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    assert _lib.ABI_VERSION >= 21
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    define = lambda what: int(re.search(r'#define\s+%s\s+(\d+)' % what, hdr).group(1))
    f = cda.fourier
    assert define('CPN_EFD_CHUNK') == f.CHUNK == oracle.CHUNK and f.CHUNK % 64 == 0
    assert define('CPN_EFD_MAX_ORDER') == f.MAX_ORDER == oracle.MAX_ORDER >= 64
    assert (define('CPN_EFD_POINTS_I32'), define('CPN_EFD_POINTS_F64')) == (f.POINTS_I32, f.POINTS_F64)
    assert (define('CPN_EFD_CLOSE_NONE'), define('CPN_EFD_CLOSE_ALL'), define('CPN_EFD_CLOSE_EACH')) == \
        (f.CLOSE_NONE, f.CLOSE_ALL, f.CLOSE_EACH)
    assert define('CPN_EFD_TIMED') == f.TIMED and define('CPN_EFD_STATUS_WORDS') == f.STATUS_WORDS
    chunks_h = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'efd_chunks.h')).read()
    assert int(re.search(r'#define\s+CPN_EFD_CHUNK\s+(\d+)', chunks_h).group(1)) == f.CHUNK
    kernel = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'contour_fourier.hip')).read()
    assert not re.search(r'atomic\w*\s*\(\s*[^,]*,\s*\(?\s*(double|float)', kernel) and 'unsafeAtomicAdd' not in kernel
    flat = lambda text: ' '.join(re.sub(r'\n\s*(\*|//)\s*', ' ', text).split())
    for phrase in ('1e-8 + 1e-5', 'sqrt(dx_i^2 + dy_i^2) + epsilon', '2 k^2 pi^2', 'location NaN'):  # the rule, restated
        for text in (hdr, chunks_h, kernel, f.__doc__):
            assert phrase in flat(text).replace('``', ''), phrase
    assert {'fourier', 'efd', 'contours2fourier', 'labels2fourier'} <= set(cda.__all__)
    assert cda.efd is f.efd and cda.contours2fourier is f.contours2fourier and cda.labels2fourier is f.labels2fourier
    # argument checks answer before anything touches a device (the buffers are never dereferenced)
    buf = ctypes.create_string_buffer(4096)
    status = (ctypes.c_int64 * f.STATUS_WORDS)()
    assert lib.cpn_efd_workspace_bytes(10, 100, 5) > 0 and lib.cpn_efd_workspace_bytes(10, 100, 0) == 0
    assert lib.cpn_efd_workspace_bytes(10, 100, f.MAX_ORDER + 1) == 0
    assert lib.cpn_efd_workspace_bytes(1000, 10 ** 6, 25) >= (10 ** 6 // f.CHUNK) * 102 * 8
    call = lambda dtype, K, P, order, eps, mode, nbytes: lib.cpn_efd(buf, dtype, buf, K, P, order, eps, mode, buf, nbytes, buf, buf,
                                                                     status, None)
    assert call(0, 1, 4, 0, 1e-6, 2, 4096) == _lib.E_INVALID and b'order' in lib.cpn_last_error()
    assert call(0, 1, 4, f.MAX_ORDER + 1, 1e-6, 2, 4096) == _lib.E_INVALID
    assert call(2, 1, 4, 5, 1e-6, 2, 4096) == _lib.E_INVALID and b'points_dtype' in lib.cpn_last_error()
    assert call(0, 1, 4, 5, 1e-6, 3, 4096) == _lib.E_INVALID and b'close_mode' in lib.cpn_last_error()
    assert call(0, 1, 4, 5, -1., 2, 4096) == _lib.E_INVALID and call(0, -1, 4, 5, 1e-6, 2, 4096) == _lib.E_INVALID
    assert call(0, 0, 4, 5, 1e-6, 2, 4096) == _lib.E_INVALID and b'offsets' in lib.cpn_last_error()  # K = 0 ends at P = 0
    assert call(0, 5, 4, 5, 1e-6, 2, 4096) == _lib.E_INVALID and b'at least one point' in lib.cpn_last_error()
    assert call(0, 1, 4, 5, 1e-6, 2, 8) == _lib.E_WORKSPACE
    assert call(1, 0, 0, 5, 1e-6, 2, 0) == 0 and list(status) == [0] * f.STATUS_WORDS


def test_no_cpu_fallback_and_argument_errors():
    con = torch.zeros((3, 8, 2))
    off = torch.tensor([0, 8, 24])
    f = cda.fourier
    for call in (lambda: cda.efd(con), lambda: cda.efd([con[0], con[1, :5]], order=3), lambda: cda.efd(con.int(), autoclose=False),
                 lambda: f.efd_packed(con.reshape(-1, 2), off), lambda: cda.contours2fourier({1: con[0][:, None], 4: con[1]}),
                 lambda: cda.labels2fourier(torch.zeros((8, 9, 1), dtype=torch.int32))):
        with pytest.raises(RuntimeError, match='MI355X'):
            call()
    for order in (0, -1, f.MAX_ORDER + 1, 2.5, True):
        for call in (lambda: cda.efd(con, order), lambda: f.efd_packed(con.reshape(-1, 2), off, order),
                     lambda: cda.contours2fourier({1: con[0]}, order), lambda: cda.labels2fourier(torch.zeros((8, 9, 1)), order)):
            with pytest.raises(ValueError, match='order'):
                call()
    with pytest.raises(TypeError, match='Tensor'):
        cda.efd(np.zeros((8, 2)))
    with pytest.raises(TypeError, match='dict'):
        cda.contours2fourier([con[0]])
    with pytest.raises(ValueError, match=r'\[n, 2\]'):
        cda.efd([torch.zeros((8, 3))])
    with pytest.raises(ValueError, match='empty'):
        cda.efd([])
    with pytest.raises(ValueError, match='labels start at 1'):
        cda.contours2fourier({0: con[0]})
    with pytest.raises(ValueError, match='labels start at 1'):
        cda.contours2fourier({3: con[0], -1: con[1]})
    with pytest.raises(ValueError, match=r'\[n, 1, 2\] or \[n, 2\]'):
        cda.contours2fourier({3: torch.zeros((8, 2, 2))})
    # shapes are checked before the device, so a CPU tensor of a wrong shape is told its shape
    with pytest.raises(ValueError, match=r'\[\.\.\., n, 2\]'):
        cda.efd(torch.zeros((3, 8, 3)))
    with pytest.raises(ValueError, match=r'\[\.\.\., n, 2\]'):
        cda.efd(torch.zeros((3, 0, 2)))
    with pytest.raises(ValueError, match=r'\[P, 2\]'):
        f.efd_packed(torch.zeros((8, 3)), off)
    with pytest.raises(ValueError, match=r'\[K \+ 1\]'):
        f.efd_packed(torch.zeros((8, 2)), torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match=r'\[K \+ 1\]'):
        f.efd_packed(torch.zeros((8, 2)), torch.tensor([0., 8.]))
    # offsets that do not run from 0 to P or decrease, and an open contour with autoclose=False, are found on the device
    # (tests/test_gpu_fourier.py); the rule of the offsets is the host-built efd_chunks.h above, the C entry point rejects here what
    # it can see without a device (test_abi_header_bindings_and_exports_agree)


if __name__ == '__main__':
    m = measure()
    with open(MEASURED, 'w') as fh:
        json.dump(m, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(f'c_f = {m["c_f"]:.6g}, c_l = {m["c_l"]:.6g} over {len(m["cases"])} contours -> {MEASURED}')
