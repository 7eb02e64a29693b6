"""Overlay images (celldetection_amd.contours2overlay / label_cmap / random_colors_hsv), CPU part.

``tests/golden/overlay.npz`` holds what the reference's own ``contours2overlay`` (celldetection/data/cpn.py:811-855) and
``label_cmap(..., ubyte=True)`` (celldetection/visualization/cmaps.py:21-77) returned on small cases, with the colours the
reference drew (``tests/golden/make_golden_overlay.py``; cv2's HSV conversion and polygon fill restated there).  This file shows
that the numpy restatement of both rules (``tests/overlay_oracle.py``) reproduces every fixture value exactly and that the
fixture tells wrong rules from the right ones; the GPU tests (``test_gpu_overlay.py``) then use the fixture and the restatement.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import celldetection_amd as cda
import overlay_oracle as oracle
from celldetection_amd import _lib
from celldetection_amd.overlay import TILE, hsv2rgb_ubyte

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'overlay.npz')
OVERLAY_CASES = ('main', 'lengths', 'unrounded', 'uint8', 'none')
CMAP_CASES = tuple(f'c{c}_alpha{a}' for c in (1, 2, 3, 5, 7, 11) for a in (None, .5, .3)) + \
    ('flat', 'explicit_rgb', 'explicit_rgba', 'tab10')


def load_overlay_fixture():
    """-> [(name, contours (list of [S_i, 2] arrays, or None), size, keywords, colors uint8 [K, 3], result)]."""
    g = np.load(GOLDEN)
    out = []
    for name in (str(c) for c in g['overlay_cases']):
        ends = np.cumsum(g[f'{name}.lengths'])
        contours = None if bool(g[f'{name}.none']) else [g[f'{name}.points'][e - n:e] for e, n in zip(ends, g[f'{name}.lengths'])]
        kw = dict(rounded=bool(g[f'{name}.rounded']), intermediate_dtype=str(g[f'{name}.intermediate_dtype']))
        out.append((name, contours, tuple(int(s) for s in g[f'{name}.size']), kw, g[f'{name}.colors'], g[f'{name}.result']))
    return out


def load_cmap_fixture():
    """-> [(name, labels, colours the reference used (float [n, 3 | 4]), name of the map or '', alpha or None, result)]."""
    g = np.load(GOLDEN)
    out = []
    for name in (str(c) for c in g['cmap_cases']):
        alpha = float(g[f'{name}.alpha'])
        out.append((name, g[f'{name}.labels'], g[f'{name}.colors'], str(g[f'{name}.colors_name']),
                    None if np.isnan(alpha) else alpha, g[f'{name}.result']))
    return out


def test_fixture_covers_the_cases():
    ov = {c[0]: c for c in load_overlay_fixture()}
    assert tuple(ov) == OVERLAY_CASES
    _, contours, size, kw, colors, ref = ov['main']
    n = oracle.contours2overlay(contours, size, colors, return_count=True)[1]
    assert len(contours) >= 40 and 55 <= size[0] <= 70 and 75 <= size[1] <= 90 and n.max() >= 5
    pts = np.concatenate(contours)
    assert pts[:, 0].min() < 0 and pts[:, 1].min() < 0 and pts[:, 0].max() > size[1] and pts[:, 1].max() > size[0]
    assert any((c[:, 0] < 0).all() for c in contours) and any(((c[:, 0] > size[1]) & (c[:, 1] > size[0])).all() for c in contours)
    assert len({len(c) for c in ov['lengths'][1]}) > 4 and {1, 2, 3} <= {len(c) for c in ov['lengths'][1]}
    assert ov['unrounded'][3]['rounded'] is False and ov['main'][3]['rounded'] is True
    assert ov['uint8'][3]['intermediate_dtype'] == 'uint8' and ov['main'][3]['intermediate_dtype'] == 'uint16'
    assert oracle.contours2overlay(ov['uint8'][1], ov['uint8'][2], ov['uint8'][4], return_count=True)[1].max() == 1
    assert ov['none'][1] is None and not ov['none'][5].any() and ov['none'][5].shape == ov['none'][2] + (4,)
    cm = {c[0]: c for c in load_cmap_fixture()}
    assert tuple(cm) == CMAP_CASES
    for c in (1, 2, 3, 5, 7, 11):
        a = cm[f'c{c}_alphaNone'][1]
        assert a.shape[2] == c and .4 < (a == 0).mean() < .6
        assert len(cm[f'c{c}_alphaNone'][2]) == min(9999, a.max()) and cm[f'c{c}_alphaNone'][3] == 'rand'
    assert (cm['c11_alphaNone'][5][..., 3] == 254).any()  # eleven occupied channels: truncation gives 254, not 255
    assert (oracle.color_table(cm['c11_alpha0.3'][2], .3)[1:, 3] == 76).all() and (cm['c11_alpha0.3'][5][..., 3] == 75).any()
    assert cm['flat'][1].ndim == 2 and cm['tab10'][3] == 'tab10' and len(cm['tab10'][2]) == 10
    assert cm['explicit_rgb'][2].shape == (7, 3) and cm['explicit_rgba'][2].shape == (5, 4)
    for v in np.load(GOLDEN).values():
        assert v.dtype.kind in 'iufbU'  # arrays only
    assert os.path.getsize(GOLDEN) <= 150 * 1024


def test_restatement_reproduces_the_reference_fixture():
    for name, contours, size, kw, colors, ref in load_overlay_fixture():
        out = oracle.contours2overlay(contours, size, colors, rounded=kw['rounded'])
        assert out.dtype == ref.dtype and np.array_equal(out, ref), name
        if contours is not None:  # a list padded by repeating the last point rasters identically
            assert np.array_equal(oracle.contours2overlay(oracle.pad_contours(contours), size, colors, rounded=kw['rounded']), ref), name
    for name, a, colors, _, alpha, ref in load_cmap_fixture():
        out = oracle.label_cmap(a, colors, alpha)
        assert out.dtype == ref.dtype and np.array_equal(out, ref), name


@pytest.mark.parametrize('mutant', oracle.MUTANTS)
def test_fixture_sees_mutants_of_the_rules(mutant):
    """Overlay: rounded instead of floored mean, last writer wins, no normalisation, sums kept in 8 bits, truncation instead
    of half-to-even on the points.  Colour map: final cast rounded instead of truncated, float64 accumulation, fused
    multiply-add, ``v % n`` without the ``+ 1``, half-up instead of half-to-even table rounding."""
    assert set(oracle.OVERLAY_MUTANTS) == {'rounded_mean', 'last_wins', 'no_normalisation', 'sums_8bit', 'truncated_points'}
    assert set(oracle.CMAP_MUTANTS) == {'rounded_cast', 'float64', 'fma', 'no_plus_one', 'half_up_table'}
    n = 0
    if mutant in oracle.OVERLAY_MUTANTS:
        for name, contours, size, kw, colors, ref in load_overlay_fixture():
            n += int((oracle.contours2overlay(contours, size, colors, rounded=kw['rounded'], mutant=mutant) != ref).sum())
    else:
        for name, a, colors, _, alpha, ref in load_cmap_fixture():
            n += int((oracle.label_cmap(a, colors, alpha, mutant=mutant) != ref).sum())
    print(f'mutant {mutant} differs on {n} values')
    assert n > 0


def test_abi_exports_the_overlay_entry_points():
    lib = _lib.load()
    for name in ('cpn_overlay_bin_count', 'cpn_overlay_bin_fill', 'cpn_overlay_paint', 'cpn_label_cmap'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cpn_hip.h')).read()
    assert _lib.ABI_VERSION >= 19
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    assert int(re.search(r'#define\s+CPN_OVERLAY_TILE\s+(\d+)', hdr).group(1)) == TILE
    # argument checks answer before anything touches a device (the buffers are never dereferenced)
    buf = ctypes.create_string_buffer(64)
    word = ctypes.c_uint32(0)
    flag = ctypes.c_int32(0)
    assert lib.cpn_overlay_bin_count(buf, -1, 8, 8, buf, None) == _lib.E_INVALID
    assert lib.cpn_overlay_bin_count(buf, 1, 0, 8, buf, None) == _lib.E_INVALID
    assert lib.cpn_overlay_bin_count(None, 1, 8, 8, buf, None) == _lib.E_INVALID
    assert lib.cpn_overlay_bin_count(buf, 1, 65536, 65536, buf, None) == _lib.E_UNSUPPORTED
    assert b'2^31 - 1' in lib.cpn_last_error()
    assert lib.cpn_overlay_bin_count(buf, 0, 8, 8, buf, None) == 0  # nothing to do
    assert lib.cpn_overlay_bin_fill(buf, 1, 8, 8, buf, buf, buf, -1, None) == _lib.E_INVALID
    assert lib.cpn_overlay_bin_fill(buf, 1, 8, 8, None, buf, buf, 1, None) == _lib.E_INVALID
    assert lib.cpn_overlay_paint(buf, buf, buf, 1, 0, 8, 8, buf, buf, buf, buf, word, None) == _lib.E_INVALID
    assert lib.cpn_overlay_paint(buf, buf, buf, 1, 513, 8, 8, buf, buf, buf, buf, word, None) == _lib.E_INVALID
    assert b'512' in lib.cpn_last_error()
    assert lib.cpn_overlay_paint(buf, buf, buf, 1, 4, 8, 8, None, buf, buf, buf, word, None) == _lib.E_INVALID
    assert lib.cpn_overlay_paint(buf, buf, buf, 1, 4, 8, -1, buf, buf, buf, buf, word, None) == _lib.E_INVALID
    assert lib.cpn_label_cmap(buf, 4, 0, 1, buf, 2, buf, buf, flag, None) == _lib.E_INVALID
    assert lib.cpn_label_cmap(buf, 4, 1, 1, buf, 1, buf, buf, flag, None) == _lib.E_INVALID  # no colour in the table
    assert lib.cpn_label_cmap(buf, 4, 3, 0, buf, 2, buf, buf, flag, None) == _lib.E_INVALID  # 3 channels need the reduction
    assert b'reduction' in lib.cpn_last_error()
    assert lib.cpn_label_cmap(buf, 2 ** 31, 1, 1, buf, 2, buf, buf, flag, None) == _lib.E_UNSUPPORTED
    assert lib.cpn_label_cmap(buf, 4, 1, 1, None, 2, buf, buf, flag, None) == _lib.E_INVALID


def test_row_form_of_the_fill_rule_equals_the_pixel_form(tmp_path):
    """``lb_filled_row32`` (one walk over the edges for 32 pixels of a row: the overlay kernel) against ``lb_filled`` (one pixel:
    the label kernel) of ``csrc/polygon_fill.h``, compiled for the host: window edges (a crossing on column 30, 31, 32 and left
    of the window), 1 and 2 points, repeated points, random polygons."""
    from celldetection_amd.build import _hipcc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'polygon_fill_host')
    hipcc = _hipcc()
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(root, 'tests', 'polygon_fill_host.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    m = re.search(r'checked (\d+) differ (\d+)', run.stdout)
    assert run.returncode == 0 and m and int(m.group(1)) > 10 ** 7 and int(m.group(2)) == 0, run.stdout[-500:]


def test_random_colors_hsv():
    assert {'contours2overlay', 'label_cmap', 'random_colors_hsv', 'overlay'} <= set(cda.__all__)
    # the six pure hues (H = degrees / 2), white and black
    hsv = [[0, 255, 255], [30, 255, 255], [60, 255, 255], [90, 255, 255], [120, 255, 255], [150, 255, 255], [77, 0, 255], [13, 255, 0]]
    rgb = [[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255], [255, 255, 255], [0, 0, 0]]
    assert hsv2rgb_ubyte(hsv).tolist() == rgb and hsv2rgb_ubyte(hsv).dtype == np.uint8
    assert hsv2rgb_ubyte([[15, 255, 255], [0, 128, 200], [60, 51, 100]]).tolist() == [[255, 128, 0], [200, 100, 100], [80, 100, 80]]
    # inside the requested ranges: max = V, min = V * (1 - S / 255) rounded, the hue decides the order of the channels
    np.random.seed(5)
    c = cda.random_colors_hsv(4000, ubyte=True)
    assert c.shape == (4000, 3) and c.dtype == np.uint8
    mx, mn = c.max(1).astype(int), c.min(1).astype(int)
    assert mx.min() >= 180 and mx.max() <= 255 and mx.min() < 185 and mx.max() > 250
    sat = 255. * (mx - mn) / mx
    assert sat.min() > 60 - 1.5 and sat.max() < 132 + 1.5 and sat.min() < 65 and sat.max() > 127
    c = cda.random_colors_hsv(500, hue_range=(60, 61), saturation_range=(255, 256), value_range=(100, 200), ubyte=True)
    assert (c[:, 0] == 0).all() and (c[:, 2] == 0).all() and c[:, 1].min() >= 100 and c[:, 1].max() <= 199  # pure green
    c = cda.random_colors_hsv(300, hue_range=(0, 30), saturation_range=(200, 256), value_range=(255, 256), ubyte=True)
    assert (c[:, 0] == 255).all() and (c[:, 1] >= c[:, 2]).all() and (c[:, 2] <= 55).all()  # red to yellow
    # three vectorised draws in the reference's order; a seed fixes them; floats are the bytes / 255
    np.random.seed(9)
    a = cda.random_colors_hsv(7, ubyte=True)
    np.random.seed(9)
    hsv = np.stack((np.random.randint(0, 180, 7), np.random.randint(60, 133, 7), np.random.randint(180, 256, 7)), 1)
    assert np.array_equal(a, hsv2rgb_ubyte(hsv))
    np.random.seed(9)
    f = cda.random_colors_hsv(7)
    assert f.dtype == np.float64 and np.array_equal(f, a / 255)


def test_color_table_of_label_cmap():
    from celldetection_amd.overlay import QUALITATIVE_MAPS, _color_table
    for name, a, colors, cname, alpha, _ in load_cmap_fixture():
        t = _color_table(colors, 1, alpha)
        assert t.dtype == np.uint8 and np.array_equal(t, oracle.color_table(colors, alpha)) and not t[0].any(), name
        if cname not in ('', 'rand'):
            assert np.array_equal(_color_table(cname, 1, alpha), t), name
    assert (_color_table(np.ones((3, 3)), 1, .3)[1:, 3] == 76).all()  # 76.5: half to even
    assert (_color_table(np.ones((3, 3)), 1, .5)[1:, 3] == 128).all()  # 127.5
    assert _color_table(torch.ones(3, 4) * .25, 1, None)[1:].tolist() == [[64] * 4] * 3  # 63.75
    np.random.seed(2)
    t = _color_table('rand', 17, None)
    assert t.shape == (18, 4) and (t[1:, 3] == 255).all() and t[1:, :3].max(1).min() >= 180
    assert 'tab10' in QUALITATIVE_MAPS and len(QUALITATIVE_MAPS) == 12
    with pytest.raises(ValueError, match=r'\[n, 3\]'):
        _color_table(np.ones((3, 5)), 1, None)
    with pytest.raises(ValueError, match='qualitative'):
        _color_table('viridis', 1, None)
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        _color_table(np.ones((3, 3)) * 2, 1, None)


def test_no_cpu_fallback_and_argument_errors():
    con = torch.zeros((3, 8, 2))
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.contours2overlay(con, (16, 16))
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.contours2overlay(con, (16, 16), colors=np.zeros((3, 3), np.uint8), return_colors=True, return_stats=True, processes=4)
    with pytest.raises(NotImplementedError, match='thickness'):
        cda.contours2overlay(con, (16, 16), thickness=2)
    with pytest.raises(NotImplementedError, match='intermediate_dtype'):
        cda.contours2overlay(con, (16, 16), intermediate_dtype='float32')
    with pytest.raises(ValueError, match='zero-length contour at position 1'):
        cda.contours2overlay([np.zeros((4, 2)), np.zeros((0, 2))], (16, 16))
    lab = torch.zeros((8, 9, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.label_cmap(lab, ubyte=True)
    with pytest.raises(RuntimeError, match='MI355X'):
        cda.label_cmap(lab[:, :, 0], colors='tab10', alpha=.5, ubyte=True)
    with pytest.raises(NotImplementedError, match='ubyte'):
        cda.label_cmap(lab)
    with pytest.raises(NotImplementedError, match='rgba'):
        cda.label_cmap(lab, rgba=False, ubyte=True)
    for axis in (0, 1, -2):
        with pytest.raises(NotImplementedError, match='reduce_axis'):
            cda.label_cmap(lab, reduce_axis=axis, ubyte=True)
    for zero_val in (None, 1., (0., 0., 0., 1.)):
        with pytest.raises(NotImplementedError, match='zero_val'):
            cda.label_cmap(lab, zero_val=zero_val, ubyte=True)
    with pytest.raises(TypeError, match='integers'):
        cda.label_cmap(lab.float(), ubyte=True)
    with pytest.raises(ValueError, match=r'\[H, W\]'):
        cda.label_cmap(lab[0, 0], ubyte=True)
