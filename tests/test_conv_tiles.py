"""The conv case table of tests/conv_tiles.py against the built library, without a GPU.

cpn_conv2d_kernel_info is the selection step of launch_conv itself (host arithmetic, no HIP call): it says which
conv_igemm_kernel<TH, BN, WM, WN, MODE> a call runs.  Checked here:

* every table entry runs the instantiation its key names and shows the tile edges listed in conv_tiles (the written exemptions
  are exactly the edges it does not show);
* the kernels exported by libcpn_hip.so (dynamic symbol names) are exactly the table's keys plus conv_tiles.UNREACHABLE, and a
  grid of descriptors driven through the query selects none of the unreachable ones;
* every existing single-conv case (CONV_CASES, S1F_CASES, S1Q_CASES, SUBPIXEL_CASES, FP8_CASES) runs the instantiation recorded
  for it, so a change of MIN_BLOCKS or lds_bytes that moves a case to another kernel fails here;
* the query rejects what the launch rejects, with the same code.
"""
import ctypes
import itertools

import pytest

import conv_tiles as ct
import test_gpu_conv_bridge as tb
import test_gpu_kernels as tk
from celldetection_amd import _lib

LIBRARY = ct.library_instantiations()


@pytest.mark.parametrize('key', list(ct.TABLE))
def test_table_entry_runs_its_instantiation_and_shows_its_edges(key):
    unit, mode, th, bn, _ = ct.parse_key(key)
    info = ct.query(key)
    assert info[:3] == (mode, th, bn), f'{key}: the library runs {ct.info_key(unit, info)}'
    assert info[3:] == LIBRARY[ct.instantiation(key)], f'{key}: launched wave grid {info[3:]} is not the exported kernel\'s'
    shown = ct.edges(key, info)
    assert set(shown) == set(ct.EDGES)
    missing = {e for e, ok in shown.items() if not ok}
    assert missing == ct.exempt(key), f'{key}: edges not shown {sorted(missing)}, written exemptions {sorted(ct.exempt(key))}'
    cfg = ct.TABLE[key]
    if mode == 'PW' and cfg.get('stride', 1) == 1 and not cfg.get('res_up'):
        # (cpn_conv2d flattens a plain 1x1 over N * H * W pixels when that is a multiple of 32: the tile edges above would be others)
        assert cfg['n'] * cfg['h'] * cfg['w'] % 32, f'{key}: flattened to [1, M / 32, 32]'


@pytest.mark.parametrize('key', [k for k in ct.TABLE if '/S1F/' in k or '/S1Q/' in k])
def test_switched_modes_follow_their_switches(key, monkeypatch):
    """MODE_S1F / MODE_S1Q entries under the switch values their tests set (read per call by the query as by the launch)."""
    cfg = ct.TABLE[key]
    if '/S1F/' in key:
        monkeypatch.setenv('CPN_S1F', '2')
        assert ct.query_conv(cfg)[:3] == ('S1F', 8, 128)
        monkeypatch.setenv('CPN_S1F', '0')
        assert ct.query_conv(cfg)[0] == 'S1'
        monkeypatch.delenv('CPN_S1F')
        assert ct.query_conv(cfg)[0] == 'S1', 'below 1024 blocks the mode is not the default'
    else:
        monkeypatch.delenv('CPN_S1Q', raising=False)
        assert ct.query_conv(cfg)[:3] == ('S1Q', 16, 64)
        monkeypatch.setenv('CPN_S1Q', '1')
        assert ct.query_conv(cfg)[:3] == ('S1Q', 16, 64)
        monkeypatch.setenv('CPN_S1Q', '0')
        assert ct.query_conv(cfg)[:3] == ('S1', 16, 64)


def test_library_holds_exactly_the_table_and_the_unreachable():
    """Symbol names only: a new instantiation without a case, or a case for a vanished one, fails."""
    keys = {ct.instantiation(k) for k in ct.TABLE}
    assert not keys & set(ct.UNREACHABLE)
    assert len(LIBRARY) == 75, sorted(LIBRARY)
    assert set(LIBRARY) == keys | set(ct.UNREACHABLE), \
        f'exported without a case: {sorted(set(LIBRARY) - keys - set(ct.UNREACHABLE))}; ' \
        f'cases without a kernel: {sorted((keys | set(ct.UNREACHABLE)) - set(LIBRARY))}'
    tiles = {(16, 64): (2, 2), (8, 256): (4, 2), (8, 128): (2, 2), (8, 64): (2, 2), (8, 32): (2, 1), (4, 256): (2, 2),
             (4, 128): (2, 2), (4, 64): (1, 2), (4, 32): (1, 1)}
    for key, waves in LIBRARY.items():
        _, mode, th, bn, _ = ct.parse_key(key)
        assert waves == ((4, 2) if mode == 'S1F' else tiles[th, bn]), key


def _raw_op(cin_b, cout_b, kh, kw, stride, pad, out, up0=0):
    op = _lib.OpDesc()
    op.op, op.src0, op.src1, op.res, op.dst = _lib.OP_CONV, 0, -1, -1, (1 if out == 'nhwc' else -1)
    op.up0, op.c0_used, op.kh, op.kw, op.stride, op.pad = up0, cin_b, kh, kw, stride, pad
    op.bundles, op.cin_b, op.cout_b, op.bias_offset, op.cout_real, op.out_index = 1, cin_b, cout_b, -1, cout_b, 0
    op.fuse_weight_offset = op.fuse_bias_offset = op.mult_offset = -1
    if out == 'fused':
        op.fuse_cout, op.fuse_weight_offset = 2, 0
    return op


def test_grid_of_descriptors_never_selects_an_unreachable_instantiation():
    """About 10^5 descriptors (n, h, w, cin, cout, kh x kw, stride, source resize, output mode; both units) through the query:
    every plain-mode instantiation of the table is selected by some of them, none of conv_tiles.UNREACHABLE by any."""
    lib = _lib.load()
    info = (ctypes.c_int32 * 5)()
    reached, calls = set(), 0
    kernels = [(1, 1), (2, 2), (3, 3), (5, 5), (7, 7), (1, 3), (3, 1), (1, 7)]
    for unit, prec, cins in (('bf16', _lib.PRECISION_BF16, (32, 64, 96, 256)), ('e4m3', _lib.PRECISION_FP8, (64, 128, 192))):
        for (kh, kw), stride, cin, cout, out, up0 in itertools.product(
                kernels, (1, 2), cins, (32, 64, 96, 128, 160, 256, 288, 512), ('nhwc', 'f32', 'fused'), (0, 2)):
            if up0 and (unit == 'e4m3' or stride == 2 or kh * kw == 1):
                continue  # (bilinear source: k x k stride-1 convs of the bf16 unit)
            if unit == 'e4m3' and out == 'nhwc' and cout % 64:
                continue
            pad = 0 if kh * kw == 1 else max(kh, kw) // 2
            op = _raw_op(cin, cout, kh, kw, stride, pad, out, up0)
            for n, h, w in itertools.product((1, 4, 32, 256), (4, 9, 16, 33, 64, 256), (16, 33, 64, 256)):
                calls += 1
                ds = 0 if out != 'nhwc' else cout
                if lib.cpn_conv2d_kernel_info(op, prec, cin, 0, 0, ds, n, h, w, info) == 0:
                    reached.add(f'{unit}/{_lib.CONV_MODE_NAMES[info[0]]}/{info[1]}x{info[2]}')
    assert calls > 50000
    assert not reached & set(ct.UNREACHABLE), sorted(reached & set(ct.UNREACHABLE))
    plain = {k for k in LIBRARY if ct.parse_key(k)[1] in ('PW', 'S1', 'S2', 'BL', 'N')} - set(ct.UNREACHABLE)
    assert plain <= reached, f'the grid does not reach {sorted(plain - reached)}: it proves nothing about them'


@pytest.mark.parametrize('name', list(tk.CONV_CASES))
def test_recorded_instantiation_conv_cases(name):
    assert set(ct.RECORDED_CONV) == set(tk.CONV_CASES)
    assert ct.info_key('bf16', ct.query_conv(tk.CONV_CASES[name])) == ct.RECORDED_CONV[name]


@pytest.mark.parametrize('name', list(tk.S1F_CASES))
def test_recorded_instantiation_s1f_cases(name, monkeypatch):
    assert set(ct.RECORDED_S1F) == set(tk.S1F_CASES)
    got = []
    for value in (None, '0', '2'):
        monkeypatch.delenv('CPN_S1F', raising=False) if value is None else monkeypatch.setenv('CPN_S1F', value)
        got.append(ct.info_key('bf16', ct.query_conv(tk.S1F_CASES[name])))
    assert tuple(got) == ct.RECORDED_S1F[name]


@pytest.mark.parametrize('name', list(tk.S1Q_CASES))
def test_recorded_instantiation_s1q_cases(name, monkeypatch):
    assert set(ct.RECORDED_S1Q) == set(tk.S1Q_CASES)
    got = []
    for value in (None, '0', '1'):
        monkeypatch.delenv('CPN_S1Q', raising=False) if value is None else monkeypatch.setenv('CPN_S1Q', value)
        got.append(ct.info_key('bf16', ct.query_conv(tk.S1Q_CASES[name])))
    assert tuple(got) == ct.RECORDED_S1Q[name]


@pytest.mark.parametrize('name', list(tk.SUBPIXEL_CASES))
def test_recorded_instantiation_subpixel_cases(name):
    assert set(ct.RECORDED_SUBPIXEL) == set(tk.SUBPIXEL_CASES)
    assert tuple(ct.info_key('bf16', i) for i in ct.query_subpixel(tk.SUBPIXEL_CASES[name])) == ct.RECORDED_SUBPIXEL[name]


@pytest.mark.parametrize('name', list(tk.FP8_CASES))
def test_recorded_instantiation_fp8_cases(name):
    assert set(ct.RECORDED_FP8) == set(tk.FP8_CASES)
    assert ct.info_key('e4m3', ct.query_conv_fp8(tk.FP8_CASES[name])) == ct.RECORDED_FP8[name]


@pytest.mark.parametrize('name', list(tb.CASES))
def test_bridge_cases_run_the_bridge_kernel(name):
    assert ct.query_bridge(ct.bridge_cfg(name)) == ('BR', 16, 64, 2, 2)


def test_named_tiles_are_what_runs():
    """The cases whose names state a tile."""
    assert ct.RECORDED_CONV['3x3_256_small_grid_4x64_tile'] == 'bf16/S1/4x64'
    assert ct.RECORDED_FP8['7x7_256_small_grid_4x64_tile'] == 'e4m3/S1/4x64'
    assert ct.RECORDED_CONV['3x3_256_flagship_tile'] == 'bf16/S1F/8x128'
    for name in ('3x3_256_flagship_concat_up', 'fused_head_256_flagship_tile', '1x1_flagship_tile', '1x1_flagship_tile_res'):
        assert ct.RECORDED_CONV[name].endswith('/8x256'), name
    for name in ('3x3_c64_th16_tile', '7x7_c64_th16_tile', 'c64_fused_head_th16', 'fused_head_64_tanh_th16'):
        assert ct.RECORDED_CONV[name].endswith('/16x64'), name


def test_query_rejects_what_the_launch_rejects():
    """Same argument building and validation as cpn_conv2d / cpn_conv2d_fp8, same codes: CPN_E_INVALID (-1) from the argument
    checks (test_conv_rejects_a_resized_source_of_no_pixels is the launch's side), hipErrorInvalidValue (1) from launch_conv."""
    with pytest.raises(RuntimeError, match=r'conv2d_kernel_info failed \(code -1\).*empty input'):
        ct.query_conv(dict(n=1, h=1, w=40, cin=32, cout=32, k=1, up0=True))
    lib = _lib.load()
    info = (ctypes.c_int32 * 5)(7, 7, 7, 7, 7)
    # a 3x3 conv at stride 3: launch_conv's own check
    assert lib.cpn_conv2d_kernel_info(_raw_op(32, 32, 3, 3, 3, 1, 'nhwc'), _lib.PRECISION_BF16, 32, 0, 0, 32, 2, 32, 32, info) == 1
    # a fused head whose block cannot own its 96 hidden channels
    assert lib.cpn_conv2d_kernel_info(_raw_op(32, 96, 3, 3, 1, 1, 'fused'), _lib.PRECISION_BF16, 32, 0, 0, 0, 2, 32, 32, info) == 1
    # e4m3: 32-channel strides, the fp32 verification path, null pointers
    assert lib.cpn_conv2d_kernel_info(_raw_op(64, 64, 3, 3, 1, 1, 'nhwc'), _lib.PRECISION_FP8, 32, 0, 0, 64, 2, 32, 32, info) == -1
    assert lib.cpn_conv2d_kernel_info(_raw_op(32, 32, 3, 3, 1, 1, 'nhwc'), _lib.PRECISION_F32, 32, 0, 0, 32, 2, 32, 32, info) == -1
    assert lib.cpn_conv2d_kernel_info(None, _lib.PRECISION_BF16, 32, 0, 0, 32, 2, 32, 32, info) == -1
    # a tensor too large for one launch: CPN_E_UNSUPPORTED (-2)
    assert lib.cpn_conv2d_kernel_info(_raw_op(32, 32, 3, 3, 1, 1, 'nhwc'), _lib.PRECISION_BF16, 32, 0, 0, 32, 4096, 1024, 1024, info) == -2
    assert list(info) == [7] * 5, 'a rejected call leaves info untouched'
    assert lib.cpn_conv2d_kernel_info(_raw_op(32, 32, 3, 3, 1, 1, 'nhwc'), _lib.PRECISION_BF16, 32, 0, 0, 32, 2, 32, 32, info) == 0
    assert list(info) == [1, 4, 32, 1, 1]
