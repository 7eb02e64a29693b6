"""Flat label images (celldetection_amd.resolve_label_channels), CPU part.

``tests/golden/flat_labels.npz`` holds what the reference's own ``resolve_label_channels`` (celldetection/data/cpn.py:361-399)
returned on small label images (``tests/golden/make_golden_flat_labels.py``; cv2's dilate restated there).  This file shows
that the numpy restatement of the rule (``tests/flat_labels_oracle.py``) reproduces every fixture value exactly and that the
fixture tells wrong rules from the right one; the GPU tests (``test_gpu_flat_labels.py``) then use the fixture and, on images
the reference would take long for, the restatement.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import celldetection_amd as cda
from celldetection_amd import _lib
from celldetection_amd.flat_labels import MAX_STEPS
from flat_labels_oracle import MUTANTS, resolve_label_channels as oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'flat_labels.npz')
DISC_CASES = ('discs_c3', 'discs_c4')


def load_fixture():
    """-> [(name, labels, max_iter, kernel, result)]; kernel is (3, 3) or a 3 x 3 array."""
    g = np.load(GOLDEN)
    out = []
    for name in (str(c) for c in g['cases']):
        k = g[f'{name}.kernel']
        out.append((name, g[f'{name}.labels'], int(g[f'{name}.max_iter']), (3, 3) if k.size == 0 else k, g[f'{name}.result']))
    return out


def test_fixture_covers_the_cases():
    cases = {c[0]: c for c in load_fixture()}
    for name in ('discs_c3', 'discs_c4', 'identical_squares', 'no_overlap_negatives', 'one_overlap_negatives', 'border_corner',
                 'larger_wins', 'larger_wins_swapped', 'one_channel') + tuple(f'{d}_iter{k}' for d in DISC_CASES for k in (1, 2, 5)) + \
            tuple(f'{d}_eight' for d in DISC_CASES):
        assert name in cases
    assert cases['discs_c3'][1].shape == (160, 200, 3) and cases['discs_c4'][1].shape == (96, 130, 4)
    for d in DISC_CASES:
        for k in (1, 2, 5):
            assert cases[f'{d}_iter{k}'][2] == k and np.array_equal(cases[f'{d}_iter{k}'][1], cases[d][1])
        assert np.array_equal(cases[f'{d}_eight'][3], np.ones((3, 3))) and cases[d][3] == (3, 3)
        # the cap matters: fewer steps leave more overlap pixels at 0
        left = [int((cases[f'{d}_iter{k}'][4] == 0).sum()) for k in (1, 2, 5)] + [int((cases[d][4] == 0).sum())]
        assert left[0] > left[1] > left[2] > left[3]
    _, a, _, _, r = cases['identical_squares']
    assert ((a > 0).sum(-1) > 1).sum() == 36 and not r.any()  # unreachable overlap -> 0
    _, a, _, _, r = cases['no_overlap_negatives']
    assert tuple(a[0, 0]) == (-1, -2) and tuple(a[5, 6]) == (-1, 3) and r[0, 0] == -1 and r[5, 6] == 3  # plain maximum
    _, a, _, _, r = cases['one_overlap_negatives']
    assert tuple(a[5, 0]) == (4, 5) and r[0, 0] == 0 and r[5, 6] == 3 and r[5, 0] == 0  # negatives -> 0, isolated overlap -> 0
    _, a, _, _, r = cases['border_corner']
    over = (a > 0).sum(-1) > 1
    assert over[0].any() and over[-1, -1] and over[-1, 0] and (r[over] > 0).all()
    for name, row in (('larger_wins', [0, 7, 7, 7, 9, 9, 9, 9, 0]), ('larger_wins_swapped', [0, 9, 9, 9, 9, 7, 7, 7, 0])):
        _, a, _, _, r = cases[name]
        assert ((a > 0).sum(-1) > 1).sum() == 1 and r[2].tolist() == row  # 9 wins from the right and from the left
    _, a, _, _, r = cases['one_channel']
    assert a.shape[2] == 1 and np.array_equal(r, a[:, :, 0])
    for v in np.load(GOLDEN).values():
        assert v.dtype.kind in 'iuU'  # arrays only


def test_restatement_reproduces_the_reference_fixture():
    for name, a, max_iter, kernel, ref in load_fixture():
        out, stats = oracle(a, max_iter=max_iter, kernel=kernel, return_stats=True)
        assert out.dtype == ref.dtype and np.array_equal(out, ref), name
        assert stats['steps'] <= max_iter and stats['overlap_pixels'] == int(((a > 0).sum(-1) > 1).sum()), name
        over = (a > 0).sum(-1) > 1
        if over.any():
            assert stats['unresolved_pixels'] == int((ref[over] == 0).sum()), name


@pytest.mark.parametrize('mutant', MUTANTS)
def test_fixture_sees_mutants_of_the_rule(mutant):
    """in-place raster sweep, smaller label wins, 8-neighbourhood, wrap-around border, first channel wins, plain channel
    maximum, one step only: each differs from the reference's result on both disc cases."""
    assert set(MUTANTS) == {'inplace', 'smaller', 'eight', 'wrap', 'first_channel', 'plain_max', 'one_step'}
    cases = {c[0]: c for c in load_fixture()}
    for d in DISC_CASES:
        _, a, max_iter, kernel, ref = cases[d]
        n = int((oracle(a, max_iter=max_iter, kernel=kernel, mutant=mutant) != ref).sum())
        print(f'{d}: mutant {mutant} differs on {n} pixels')
        assert n > 0, d


def test_abi_exports_the_flat_label_entry_points():
    lib = _lib.load()
    for name in ('cpn_flat_workspace_bytes', 'cpn_flat_classify', 'cpn_flat_step', 'cpn_flat_finish'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _lib.ABI_VERSION >= 16
    w = lib.cpn_flat_workspace_bytes
    assert w(100, 200) >= 100 * 200 * 4 + 4 * 7 * 4  # a second image + four flags per 32 x 32 tile
    assert w(1000, 1000) > w(100, 200) and w(-1, 5) == 0
    # the binding's steps per launch are the header's; argument checks answer before anything touches a device
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cpn_hip.h')).read()
    assert int(re.search(r'#define\s+CPN_FLAT_MAX_STEPS\s+(\d+)', hdr).group(1)) == MAX_STEPS
    ws = ctypes.create_string_buffer(64)  # never dereferenced: the calls below fail on their arguments
    assert lib.cpn_flat_step(None, 8, 8, MAX_STEPS + 1, 0o272, 0, ws, 0, None, None) == _lib.E_INVALID
    assert b'CPN_FLAT_MAX_STEPS' in lib.cpn_last_error()
    assert lib.cpn_flat_step(None, 8, 8, MAX_STEPS, 0o272, 0, ws, 0, None, None) == _lib.E_WORKSPACE  # steps accepted
    assert lib.cpn_flat_classify(None, 2, 65536, 65536, 0, None, 1, 0, None, None) == _lib.E_UNSUPPORTED
    assert b'2^31 - 1' in lib.cpn_last_error()


def test_no_cpu_fallback_and_argument_errors():
    assert 'resolve_label_channels' in cda.__all__
    a = torch.zeros((8, 9, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.resolve_label_channels(a)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.resolve_label_channels(a, kernel=np.ones((3, 3), np.uint8), max_iter=3, return_stats=True)
    with pytest.raises(ValueError, match='Invalid method: erosion'):
        cda.resolve_label_channels(a, method='erosion')
    with pytest.raises(NotImplementedError, match=r'\(5, 5\)'):
        cda.resolve_label_channels(a, kernel=(5, 5))
    with pytest.raises(NotImplementedError, match='3 x 3'):
        cda.resolve_label_channels(a, kernel=np.ones((5, 5), np.uint8))
    with pytest.raises(ValueError, match=r'\[H, W, C\]'):
        cda.resolve_label_channels(a[:, :, 0])
    with pytest.raises(TypeError, match='integers'):
        cda.resolve_label_channels(a.float())


def test_footprint_bits():
    from celldetection_amd.flat_labels import CROSS, _footprint
    assert _footprint((3, 3)) == _footprint([3, 3]) == CROSS == 0b010111010
    assert _footprint(np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])) == CROSS
    assert _footprint(np.ones((3, 3))) == 0b111111111 and _footprint(torch.ones(3, 3)) == 0b111111111
    assert _footprint(np.array([[0, 7, 0], [0, 0, 0], [0, 0, 0]])) == 0b10  # row 0, column 1: the pixel above
