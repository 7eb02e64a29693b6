"""CPU tests of the trainable concat convolution (celldetection_amd/nn/cat_conv.py, csrc/cat_conv_train.hip, csrc/nearest_adjoint.h): the
fp64 statements of tests/cat_conv_oracle.py against torch's own autograd of the stock expression, the wrong rules the cases tell
apart, the index arithmetic on the host under sanitizers, the host-side entry points, the Python surface and the decoder convert on
a stand-in decoder (tests/unet_standin.py) pinned to the oracle's restatement of the reference.  Nothing here needs a GPU."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import celldetection_amd as cda
import cat_conv_oracle as oracle
import cpn_oracle
import unet_standin
from celldetection_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nn = cda.nn

# (name, H, W, h, w, C0 (0: bridge), C1, Cout, k)
CASES = [('ceil_half', 5, 7, 3, 4, 32, 64, 32, 3), ('floor_half', 5, 7, 2, 3, 64, 32, 32, 3), ('ratio_3', 9, 10, 3, 3, 32, 32, 32, 1),
         ('ratio_1', 5, 7, 5, 7, 32, 32, 32, 3), ('one_pixel', 3, 6, 1, 1, 32, 32, 32, 3), ('bridge', 6, 10, 3, 5, 0, 32, 32, 3),
         ('float_rule', 46, 3, 14, 2, 32, 32, 32, 3)]


def _operands(name, H, W, h, w, c0, c1, cout, k, n=2):
    g = torch.Generator().manual_seed(H * 100 + W + k)
    lateral = torch.randn(n, c0, H, W, generator=g, dtype=torch.float64) if c0 else None
    top = torch.randn(n, c1, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, c0 + c1, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    dy = torch.randn(n, cout, H, W, generator=g, dtype=torch.float64)
    return lateral, top, wt, b, dy


def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0])
def test_statements_equal_torch_autograd(case):
    name, H, W, h, w, c0, c1, cout, k = case
    lateral, top, wt, b, dy = _operands(*case)
    y, dl, dt, dw, db = oracle.autograd64(lateral, top, wt, b, dy)
    _close(oracle.forward(lateral, top, wt, b), y)
    if c0:
        _close(oracle.d_lateral(dy, wt, c0), dl)
    t = oracle.top_gradient_at_lateral_size(dy, wt, c0)
    assert t.shape == (2, c1, H, W)
    got, S, count = oracle.d_top(t, (h, w))
    _close(got, dt)
    assert int(count.sum()) == H * W and bool((S >= got.abs() - 1e-9).all())
    got, S = oracle.wgrad(lateral, top, dy, k)
    _close(got, dw)
    _close(oracle.bgrad(dy)[0], db)
    if (h, w) == (H, W):
        assert torch.equal(oracle.resize(top, (H, W)), top) and bool((count == 1).all())
    if (h, w) == (1, 1):
        assert count.tolist() == [[H * W]]


def test_the_inner_conv_commutes_with_the_resize():
    """inner(resize(x)) == resize(inner(x)) per pixel, and the gradients of the latter are the footprint sum followed by the 1x1
    conv's own gradients at the low resolution."""
    g = torch.Generator().manual_seed(3)
    last = torch.randn(2, 8, 3, 4, generator=g, dtype=torch.float64, requires_grad=True)
    wi = torch.randn(4, 8, 1, 1, generator=g, dtype=torch.float64, requires_grad=True)
    bi = torch.randn(4, generator=g, dtype=torch.float64, requires_grad=True)
    stock = F.conv2d(F.interpolate(last, size=(5, 7), mode='nearest'), wi, bi)
    _close(oracle.inner_then_resize(last.detach(), wi.detach(), bi.detach(), (5, 7)), stock.detach())  # (torch's conv: own sum order)
    dtop = torch.randn(2, 4, 5, 7, generator=g, dtype=torch.float64)
    stock.backward(dtop)
    d_last, dw, db = oracle.inner_gradients(last.detach(), wi.detach(), dtop)
    _close(d_last, last.grad)
    _close(dw, wi.grad)
    _close(db, bi.grad)


def test_wrong_rules_are_told_apart():
    """Each rule of cat_conv_oracle.WRONG_RULES moves a result of the case named beside it by an amount of the order of the values
    themselves; the GPU tests accept about 1e-2 of that."""
    told = set()

    def differs(a, b):
        return float((a - b).abs().max()) > .1 * float(b.abs().mean())

    # round to nearest instead of floor: at ratio 3 dst 2 reads source 1 instead of 0
    case = CASES[2]
    lateral, top, wt, b, dy = _operands(*case)
    y, dl, dt, dw, db = oracle.autograd64(lateral, top, wt, b, dy)
    assert differs(oracle.forward(lateral, top, wt, b, 'round_to_nearest'), y)
    assert differs(oracle.d_top(oracle.top_gradient_at_lateral_size(dy, wt, 32), (3, 3), 'round_to_nearest')[0], dt)
    told.add('round_to_nearest')
    # top first in the concat
    case = CASES[0]
    lateral, top, wt, b, dy = _operands(*case)
    y, dl, dt, dw, db = oracle.autograd64(lateral, top, wt, b, dy)
    assert differs(oracle.forward(lateral, top[:, :32], wt[:, :64], b, 'top_first'),
                   oracle.forward(lateral, top[:, :32], wt[:, :64], b))  # (32 + 32 channels: both orders fit the weight)
    assert differs(oracle.d_lateral(dy, wt[:, :64], 32, 'top_first'), oracle.d_lateral(dy, wt[:, :64], 32))
    told.add('top_first')
    # the footprint by integer arithmetic: 14 <- 46 is the smallest source size at which floor(fl32(d) * fl32(14 / 46)) and
    # d * 14 // 46 differ
    assert not torch.equal(oracle.src_index(46, 14), oracle.src_index(46, 14, 'integer_footprint'))
    assert all(torch.equal(oracle.src_index(o, i), oracle.src_index(o, i, 'integer_footprint')) for o in range(1, 44) for i in range(1, o + 1))
    case = CASES[6]
    lateral, top, wt, b, dy = _operands(*case)
    y, dl, dt, dw, db = oracle.autograd64(lateral, top, wt, b, dy)
    assert differs(oracle.forward(lateral, top, wt, b, 'integer_footprint'), y)
    assert differs(oracle.d_top(oracle.top_gradient_at_lateral_size(dy, wt, 32), (14, 2), 'integer_footprint')[0], dt)
    told.add('integer_footprint')
    # the inner conv's gradient without the footprint sum in front of it
    g = torch.Generator().manual_seed(5)
    last = torch.randn(2, 8, 3, 4, generator=g, dtype=torch.float64)
    wi = torch.randn(4, 8, 1, 1, generator=g, dtype=torch.float64)
    dtop = torch.randn(2, 4, 5, 7, generator=g, dtype=torch.float64)
    right = oracle.inner_gradients(last, wi, dtop)
    wrong = oracle.inner_gradients(last, wi, dtop, 'inner_gradient_not_summed')
    assert all(differs(p, q) for p, q in zip(wrong, right))
    told.add('inner_gradient_not_summed')
    # unflipped taps
    case = CASES[1]
    lateral, top, wt, b, dy = _operands(*case)
    y, dl, dt, dw, db = oracle.autograd64(lateral, top, wt, b, dy)
    assert differs(oracle.d_lateral(dy, wt, 64, 'taps_not_flipped'), dl)
    assert differs(oracle.d_top(oracle.top_gradient_at_lateral_size(dy, wt, 64, 'taps_not_flipped'), (2, 3))[0], dt)
    told.add('taps_not_flipped')
    assert told == set(oracle.WRONG_RULES)


def test_host_build_of_the_index_arithmetic_agrees_with_brute_force(tmp_path):
    """``csrc/nearest_adjoint.h`` and the partition compiled for the host only, with AddressSanitizer and UBSan on the host code, by
    ``tests/nearest_adjoint_host.cpp`` (a program of its own, nothing preloaded): every dst pixel in exactly one footprint, the
    footprints contiguous, for all 1 <= in <= out <= 70, against brute force inside the program."""
    hipcc = build._hipcc()
    exe = str(tmp_path / 'nearest_adjoint_host')
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(ROOT, 'tests', 'nearest_adjoint_host.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r'ok \d+', run.stdout.strip()), run.stdout[-500:] + run.stderr[-2000:]
    assert int(run.stdout.split()[1]) > 100000


def test_the_statement_of_the_nearest_map_is_torch_and_has_contiguous_footprints():
    for out in range(1, 71):
        for inn in range(1, out + 1):
            want = F.interpolate(torch.arange(inn, dtype=torch.float32)[None, None, :, None], size=(out, 1), mode='nearest')
            assert torch.equal(oracle.src_index(out, inn), want.reshape(-1).long()), (inn, out)
            fp = oracle.footprints(out, inn)
            assert sum(hi - lo for lo, hi in fp) == out


def test_wgrad_info_and_every_launch_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    info = nn.cat_weight_grad_info
    for n, h, w, h1, w1 in ((2, 1, 1, 1, 1), (2, 5, 7, 3, 4), (2, 3, 40, 1, 1), (2, 17, 33, 9, 17), (8, 256, 256, 128, 128)):
        for slab_rows in (0, 1, 3):
            for c0, c1, cout, k in ((32, 32, 32, 1), (96, 32, 160, 3), (0, 64, 32, 3), (64, 256, 256, 7)):
                i = info(n, h, w, c0, c1, (h1, w1), cout, k, slab_rows)
                rows = n * h
                assert i['slabs'] == -(-rows // i['slab_rows']) and i['reduce_chain'] == i['slabs']
                assert slab_rows == 0 or i['slab_rows'] == min(slab_rows, rows)
                assert i['steps'] == -(-i['slab_rows'] * w // 16)
                assert i['steps'] + 2 + i['reduce_chain'] <= -(-n * h * w // 16) + 2 + i['slabs']
                assert i['bias_chain'] == -(-i['slab_rows'] * w // 8) + 8 + i['slabs']
                nbytes = lib.cpn_cat_conv_wgrad_workspace_bytes(n, h, w, c0, c1, h1, w1, cout, k, slab_rows)
                assert nbytes == i['slabs'] * ((c0 + c1) * cout * k * k + cout) * 4
                if c0:  # the partition is the dense conv's on C0 + C1 channels
                    assert i == nn.weight_grad_info(n, h, w, c0 + c1, cout, k, slab_rows)
    assert info(2, 4, 8, 32, 32, (2, 4), 32, 3, 4)['slabs'] == 2  # a slab boundary between the two images of the batch
    out = (ctypes.c_int32 * 5)()
    # (N, H, W, c0, c1, h1, w1, cout, k, slab_rows)
    for bad, what in (((0, 4, 4, 32, 32, 2, 2, 32, 3, 0), 'N, H and W'), ((2, 4, 4, 33, 32, 2, 2, 32, 3, 0), 'multiple'),
                      ((2, 4, 4, 32, 0, 2, 2, 32, 3, 0), 'multiple'), ((2, 4, 4, 32, 32, 2, 2, 48, 3, 0), 'multiple'),
                      ((2, 4, 4, 32, 32, 5, 2, 32, 3, 0), 'h1 and w1'), ((2, 4, 4, 32, 32, 2, 0, 32, 3, 0), 'h1 and w1'),
                      ((2, 4, 4, 32, 32, 2, 2, 32, 2, 0), 'k must be'), ((2, 4, 4, 32, 32, 2, 2, 32, 9, 0), 'k must be'),
                      ((2, 4, 4, 32, 32, 2, 2, 32, 3, -1), 'slab_rows'), ((65536, 65536, 1, 32, 32, 1, 1, 32, 3, 0), '2^31 - 1'),
                      ((1, 1, 1, 2 ** 20, 2 ** 20, 1, 1, 2 ** 20, 3, 0), '2^31 - 1')):
        rc = lib.cpn_cat_conv_wgrad_info(*bad, out)
        assert rc in (_lib.E_INVALID, _lib.E_UNSUPPORTED) and what in lib.cpn_last_error().decode(), (bad, lib.cpn_last_error())
        assert lib.cpn_cat_conv_wgrad_workspace_bytes(*bad) == 0
        # the launch rejects the same call before it touches a buffer (the pointers are never read)
        assert lib.cpn_cat_conv_wgrad(16, 16, 16, *bad, 16, 0, 16, 0, 16, 1 << 40, None) == rc
    ok = (2, 4, 4, 32, 32, 2, 2, 32, 3, 0)
    assert lib.cpn_cat_conv_wgrad_info(*ok, None) == _lib.E_INVALID
    assert lib.cpn_cat_conv_wgrad(16, 16, 16, *ok, 16, 0, 16, 0, 16, 16, None) == _lib.E_WORKSPACE
    assert lib.cpn_cat_conv_wgrad(None, 16, 16, *ok, 16, 0, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID  # c0 > 0 without x0
    assert lib.cpn_cat_conv_wgrad(16, 16, 16, 2, 4, 4, 0, 32, 2, 2, 32, 3, 0, 16, 0, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID
    assert lib.cpn_cat_conv_wgrad(16, 8, 16, *ok, 16, 0, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID and \
        'aligned' in lib.cpn_last_error().decode()
    assert lib.cpn_cat_conv_wgrad(16, 16, 16, *ok, 16, 2, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID  # dtype code
    assert lib.cpn_cat_conv_wgrad(16, 16, 16, *ok, None, 0, None, 0, 16, 1 << 40, None) == _lib.E_INVALID  # nothing to compute
    # (t, N, H, W, C, dst, h, w)
    for bad, code in (((16, 0, 4, 4, 32, 16, 2, 2), _lib.E_INVALID), ((16, 2, 4, 4, 12, 16, 2, 2), _lib.E_INVALID),
                      ((16, 2, 4, 4, 32, 16, 5, 2), _lib.E_INVALID), ((16, 2, 4, 4, 32, 16, 2, 0), _lib.E_INVALID),
                      ((16, 65536, 65536, 1, 32, 16, 1, 1), _lib.E_UNSUPPORTED), ((None, 2, 4, 4, 32, 16, 2, 2), _lib.E_INVALID),
                      ((16, 2, 4, 4, 32, 24, 2, 2), _lib.E_INVALID)):
        assert lib.cpn_nearest_sum(*bad, None) == code and 'cpn_nearest_sum' in lib.cpn_last_error().decode(), bad
    # cpn_conv2d_sized: the sizes are looked at before any pointer
    d = nn.cat_conv._cat_desc(32, 32, 32, 3, False)
    args = (ctypes.byref(d), 16, 32, 16, 32, None, 0, 16, 32, 2, 4, 4)
    assert lib.cpn_conv2d_sized(*args, None, 16, None, None) == _lib.E_INVALID
    for stored in ((4, 4, 0, 2, 4, 4), (4, 4, 2, 5, 4, 4), (4, 4, -1, -1, 4, 4)):
        assert lib.cpn_conv2d_sized(*args, (ctypes.c_int32 * 6)(*stored), 16, None, None) == _lib.E_INVALID, stored
        assert 'resized source' in lib.cpn_last_error().decode()
    assert lib.cpn_conv2d_sized(None, *args[1:], (ctypes.c_int32 * 6)(4, 4, 2, 2, 4, 4), 16, None, None) == _lib.E_INVALID
    assert lib.cpn_conv2d_sized(args[0], None, *args[2:], (ctypes.c_int32 * 6)(4, 4, 2, 2, 4, 4), 16, None, None) == _lib.E_INVALID


@pytest.mark.parametrize('k', nn.CAT_KERNEL_SIZES)
def test_the_conv_kernels_accept_the_two_source_descriptor(k):
    """``cpn_conv2d_kernel_info`` (host only) on the descriptor ``cat_conv2d`` hands over, at the shapes of the GPU tests: the family
    keeps a kernel size only if the selection takes it."""
    assert nn.CAT_KERNEL_SIZES == (1, 3, 5, 7)
    for H, W, c0, c1, cout in ((6, 8, 32, 32, 32), (5, 7, 32, 64, 64), (9, 10, 64, 32, 32), (3, 40, 32, 32, 64), (17, 33, 96, 32, 160),
                               (17, 33, 32, 96, 64)):
        d = nn.cat_conv._cat_desc(c0, c1, cout, k, True)
        assert (d.src1 >= 0, d.up1, d.up0, d.c0_used, d.cin_b) == (True, 1, 0, c0, c0 + c1)
        mode = _lib.conv_kernel_info(d, _lib.PRECISION_BF16, 2, H, W, c0, c1, 0, cout)[0]
        assert mode == ('PW' if k == 1 else 'S1')
    for h, w, c1, cout in ((1, 1, 32, 32), (3, 5, 64, 32), (17, 20, 32, 64)):
        d = nn.cat_conv._cat_desc(0, c1, cout, k, False)
        assert (d.src1, d.up0, d.up1, d.c0_used) == (-1, 1, 0, c1)
        _lib.conv_kernel_info(d, _lib.PRECISION_BF16, 2, 2 * h, 2 * w, c1, 0, 0, cout)


def test_header_binding_and_exports_agree():
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    lib = _lib.load()
    new = ('cpn_conv2d_sized', 'cpn_cat_conv_wgrad_info', 'cpn_cat_conv_wgrad_workspace_bytes', 'cpn_cat_conv_wgrad', 'cpn_nearest_sum')
    for name in new:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
        assert not name.startswith(('cpn_bn_', 'cpn_tail_'))
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    flat_hdr = re.sub(r'\s*\n \*\s*', ' ', hdr)
    assert 'Trainable concat convolution' in flat_hdr
    for phrase in ('Additions to ABI 22', 'the lateral) first', 'ascending row-major', 'an empty footprint gives an exact zero',
                   'exact adjoints at every size', 'never written', 'No floating-point atomics', 'ascending slab order',
                   'once per 128-pixel chunk'):
        assert phrase in flat_hdr, phrase
    assert 'cat_conv_train.hip' in build.SOURCES and 'nearest_adjoint.h' in build.HEADERS
    assert {'cat_conv2d', 'CatConv2d', 'UNetDecoder', 'convert_unet_decoder_', 'nearest_resize_backward'} <= set(nn.__all__)
    src = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'cat_conv_train.hip')).read()
    dense = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'wgrad_dense.h')).read()  # the slab kernel, compiled inside the unit
    assert '#include "wgrad_dense.h"' in src and 'wgrad_dense.h' in build.HEADERS
    for text in (src, dense):
        assert 'conv_igemm_kernel' not in text and 'atomic' not in text.replace('No floating-point atomics', '')
    frag = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'mfma_frag.h')).read()  # the fragment idiom, included by the header
    assert '#include "mfma_frag.h"' in dense and 'mfma_frag.h' in build.HEADERS and 'atomic' not in frag
    assert 'ds_read_tr16_b64' in frag and 'mf_operand(' in dense and 'mfma_f32_32x32x16_bf16' in dense and 'na_pixel_src' in src
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        assert 'cat_conv2d' in open(os.path.join(ROOT, doc)).read(), doc


def test_every_unsupported_argument_raises_naming_it():
    lat, top = torch.zeros(2, 32, 5, 7), torch.zeros(2, 32, 3, 4)
    w = torch.zeros(32, 64, 3, 3)
    for args, name in (((lat, top[0], w), 'top of 3 dimensions'), ((lat[0], top, w), 'lateral of 3 dimensions'),
                       ((lat, top, w[0]), 'weight of 3 dimensions'), ((lat, top, torch.zeros(32, 64, 3, 5)), 'kernel_size'),
                       ((lat, top, torch.zeros(32, 64, 2, 2)), 'kernel_size'), ((lat, top, torch.zeros(32, 64, 9, 9)), 'kernel_size'),
                       ((torch.zeros(2, 48, 5, 7), torch.zeros(2, 16, 3, 4), w), 'lateral of 48 channels'),
                       ((torch.zeros(2, 32, 5, 7), torch.zeros(2, 16, 3, 4), torch.zeros(32, 48, 3, 3)), 'top of 16 channels'),
                       ((lat, top, torch.zeros(20, 64, 3, 3)), 'out_channels 20'), ((lat, top, w.double()), 'weight dtype'),
                       ((lat.half(), top, w), 'lateral dtype'), ((lat, top.double(), w), 'top dtype'),
                       ((lat, top, w, torch.zeros(32).double()), 'bias'), ((lat, top, w, torch.zeros(16)), 'bias'),
                       ((lat, torch.zeros(2, 32, 6, 4), w), 'larger than the lateral'),
                       ((lat, torch.zeros(2, 32, 3, 8), w), 'larger than the lateral'),
                       ((lat, torch.zeros(2, 32, 0, 4), w), 'at least one pixel'), ((torch.zeros(0, 32, 5, 7), torch.zeros(0, 32, 3, 4), w), 'at least one pixel'),
                       ((None, torch.zeros(2, 48, 3, 4), torch.zeros(32, 48, 3, 3)), 'top of 48 channels')):
        with pytest.raises(NotImplementedError, match=name):
            nn.cat_conv2d(*args)
    with pytest.raises(ValueError, match='channels'):
        nn.cat_conv2d(lat, top, torch.zeros(32, 96, 3, 3))
    with pytest.raises(ValueError, match='images'):
        nn.cat_conv2d(lat, torch.zeros(3, 32, 3, 4), w)
    with pytest.raises(RuntimeError, match='MI355X'):  # supported arguments on the CPU: the usual device error, no fallback
        nn.cat_conv2d(lat, top, w)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.cat_conv2d(None, top, torch.zeros(32, 32, 3, 3))
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.CatConv2d(64, 32, 3)(lat, top)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.CatConv2d(64, 32, 3)(torch.zeros(2, 64, 5, 7))
    for t, size, name in ((torch.zeros(2, 12, 5, 7), (3, 4), '12 channels'), (torch.zeros(8, 5, 7), (3, 4), 'input of 3 dimensions'),
                          (torch.zeros(2, 8, 5, 7), (6, 4), 'size'), (torch.zeros(2, 8, 5, 7), (3, 0), 'size'),
                          (torch.zeros(2, 8, 5, 7).double(), (3, 4), 'input dtype')):
        with pytest.raises(NotImplementedError, match=name):
            nn.nearest_resize_backward(t, size)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.nearest_resize_backward(torch.zeros(2, 8, 5, 7), (3, 4))
    for kwargs, name in ((dict(stride=2), 'stride'), (dict(groups=2), 'groups'), (dict(dilation=2), 'dilation'),
                         (dict(padding=0), 'padding'), (dict(padding_mode='reflect'), 'padding_mode'), (dict(kernel_size=9), 'kernel_size'),
                         (dict(in_channels=48), 'in_channels'), (dict(out_channels=2), 'out_channels')):
        kw = dict(in_channels=64, out_channels=32, kernel_size=3)
        kw.update(kwargs)
        with pytest.raises(NotImplementedError, match=name):
            nn.CatConv2d(**kw)
    m = nn.CatConv2d(96, 64, 3, bias=False)
    stock = torch.nn.Conv2d(96, 64, 3, padding=1, bias=False)
    assert isinstance(m, torch.nn.Conv2d) and list(m.state_dict()) == list(stock.state_dict()) and m.padding == (1, 1)
    m.load_state_dict(stock.state_dict())
    stock.load_state_dict(m.state_dict())


# ---- the decoder

def _decoder64(seed=0):
    torch.manual_seed(seed)
    return unet_standin.randomise_(unet_standin.Decoder(), seed).double().eval()


@pytest.mark.parametrize('size', [(40, 56), (36, 52)], ids=['even', 'odd_laterals'])
def test_the_stand_in_decoder_is_the_oracles_generalized_unet(size):
    """float64, eval: within 1e-9 of the largest output magnitude -- orders above fp64 summation noise at these sizes, orders below
    any change of rule."""
    dec = _decoder64()
    feats = unet_standin.features(2, *size, dtype=torch.float64, seed=1)
    if size == (36, 52):
        assert [tuple(v.shape[2:]) for v in feats.values()] == [(18, 26), (9, 13), (5, 7)]
    with torch.no_grad():
        got = dec(feats, None)
        want = cpn_oracle._generalized_unet(feats, dec.state_dict(), '', dec.bridges)
    assert list(got) == ['out', '0', '1', '2', 'encoder.0', 'encoder.1', 'encoder.2'] and len(want) == 4
    for key, ref in (('out', want['0']), ('0', want['0']), ('1', want['1']), ('2', want['2'])):
        assert got[key].shape == ref.shape
        assert float((got[key] - ref).abs().max()) <= 1e-9 * float(ref.abs().max()), key
    assert tuple(got['0'].shape[2:]) == (2 * feats['0'].shape[2], 2 * feats['0'].shape[3])
    with torch.no_grad():
        resized = dec(feats, size)
    assert tuple(resized['out'].shape[2:]) == size and all(resized[f'encoder.{k}'] is feats[k] for k in feats)


def _signature(net):
    return [(name, type(m), getattr(m, 'activation', None), getattr(m, 'p', None)) for name, m in net.named_modules()]


class _Net(torch.nn.Module):
    def __init__(self, **flags):
        super().__init__()
        t = torch.nn
        self.unet = unet_standin.Decoder(**flags)
        self.head = t.Sequential(t.Conv2d(32, 32, 7, padding=3), t.BatchNorm2d(32), t.ReLU(), t.Dropout2d(.1), t.Conv2d(32, 2, 1))
        self.grouped = t.Conv2d(64, 64, 3, padding=1, groups=2)


def _expect_converted(dec):
    assert type(dec) is nn.UNetDecoder
    assert [type(m) for m in dec.inner_blocks] == [nn.Conv2d, torch.nn.Identity, nn.Conv2d]
    for blk in dec.layer_blocks:  # (the level keeps its class: a subclass of nn.Sequential, as in the reference, or nn.Sequential itself)
        assert type(blk) in (unet_standin.TwoConvNormRelu, torch.nn.Sequential) and type(blk[0]) is nn.CatConv2d


def test_convert_unet_decoder_replaces_the_decoder_in_place():
    net = _Net()
    net.unet.layer_blocks[1].eval()
    hook = net.unet.layer_blocks[2][0].register_forward_hook(lambda *a: None)
    params, buffers, keys = dict(net.named_parameters()), dict(net.named_buffers()), list(net.state_dict().keys())
    blocks, inner = list(net.unet.layer_blocks), net.unet.inner_blocks
    replaced, left = nn.convert_unet_decoder_(net)
    assert (replaced, left) == (['unet'], {})
    dec = net.unet
    _expect_converted(dec)
    assert all(a is b for a, b in zip(dec.layer_blocks, blocks)) and dec.inner_blocks is inner  # the containers stay the objects they are
    assert dec.layer_blocks[2][0]._forward_hooks and hook is not None
    assert dec.training and not dec.layer_blocks[1].training and not dec.layer_blocks[1][0].training and dec.layer_blocks[0][0].training
    assert [type(m) for m in dec.layer_blocks[0]][1:] == [torch.nn.BatchNorm2d, torch.nn.ReLU, torch.nn.Conv2d, torch.nn.BatchNorm2d,
                                                         torch.nn.ReLU]  # the other slots are the other converts' business
    after_p, after_b = dict(net.named_parameters()), dict(net.named_buffers())
    assert after_p.keys() == params.keys() and all(after_p[k] is params[k] for k in params)  # the same Parameter objects
    assert after_b.keys() == buffers.keys() and all(after_b[k] is buffers[k] for k in buffers)
    assert list(net.state_dict().keys()) == keys
    assert (dec.has_lat, dec.bridges, dec.depth, dec.keep_features) == ({0: False, 1: True, 2: True}, 1, 3, True)
    fresh = _Net()
    fresh.load_state_dict(net.state_dict())  # state dicts interchange, both ways
    net.load_state_dict(fresh.state_dict())
    assert nn.convert_unet_decoder_(net) == ([], {})  # a second call finds nothing to replace
    with pytest.raises(RuntimeError, match='MI355X'):  # the converted decoder runs this library's kernels: no CPU fallback
        dec(unet_standin.features(2, 16, 16), None)
    # the root module is reported as left, never replaced; a class listed in decoder_types is a candidate
    lone = unet_standin.Decoder()
    assert nn.convert_unet_decoder_(lone) == ([], {'': 'the root module cannot be replaced in place: convert its parent'})
    wrap = torch.nn.Sequential(unet_standin.SameNames())
    assert nn.convert_unet_decoder_(wrap) == ([], {}) and type(wrap[0]) is unet_standin.SameNames
    assert nn.convert_unet_decoder_(wrap, decoder_types=(unet_standin.SameNames,)) == (['0'], {})
    _expect_converted(wrap[0])
    # the levels of the reference are a SUBCLASS of nn.Sequential without a forward of its own; nn.Sequential itself is taken as well
    assert all(type(b) is unet_standin.TwoConvNormRelu and type(b) is not torch.nn.Sequential for b in dec.layer_blocks)
    assert unet_standin.TwoConvNormRelu.forward is torch.nn.Sequential.forward
    plain = unet_standin.Decoder()
    plain.layer_blocks[1] = torch.nn.Sequential(*plain.layer_blocks[1])
    wrap = torch.nn.Sequential(plain)
    assert nn.convert_unet_decoder_(wrap) == (['0'], {}) and type(wrap[0].layer_blocks[1]) is torch.nn.Sequential
    _expect_converted(wrap[0])
    twice = unet_standin.Decoder()
    both = torch.nn.ModuleList([twice, twice])
    assert nn.convert_unet_decoder_(both)[1] == {'0': 'the decoder sits in 2 slots', '1': 'the decoder sits in 2 slots'}


def test_the_module_builds_from_converted_pieces_only():
    t = torch.nn
    inner = t.ModuleList([nn.Conv2d(64, 32, 1), t.Identity()])
    layers = t.ModuleList([t.Sequential(nn.CatConv2d(32, 32, 3), nn.BatchNorm2d(32, activation='relu')),
                           t.Sequential(nn.CatConv2d(128, 64, 3), nn.BatchNorm2d(64, activation='relu'))])
    dec = nn.UNetDecoder(inner, layers, has_lat=[False, True], bridges=1)
    assert dec.has_lat == {0: False, 1: True} and dec.depth == 2 and dec.out_layer is None
    assert list(dec.state_dict())[:2] == ['inner_blocks.0.weight', 'inner_blocks.0.bias']
    layers[1][0] = t.Conv2d(128, 64, 3, padding=1)
    with pytest.raises(NotImplementedError, match=r'layer_blocks\.1\.0'):
        nn.UNetDecoder(inner, layers, has_lat=[False, True], bridges=1)
    layers[1][0] = nn.CatConv2d(128, 64, 3)
    inner[0] = t.Conv2d(64, 32, 1)  # a stock inner conv would run in stock torch without saying so
    with pytest.raises(NotImplementedError, match=r'inner_blocks\.0: Conv2d: not a Conv2d of this library'):
        nn.UNetDecoder(inner, layers, has_lat=[False, True], bridges=1)


def test_every_ineligible_decoder_is_left_with_its_reason():
    t = torch.nn

    def left_of(dec):
        keys = list(dec.state_dict().keys())
        sig = _signature(dec)
        replaced, left = nn.convert_unet_decoder_(t.ModuleList([dec]))
        assert replaced == [] and list(left) == ['0'] and _signature(dec) == sig and list(dec.state_dict().keys()) == keys
        return left['0']

    for flags, word in ((dict(interpolate='bilinear'), 'interpolate'), (dict(cat_order=1), 'cat_order'), (dict(block_cat=True), 'block_cat'),
                        (dict(block_interpolate=True), 'block_interpolate'), (dict(bridge_block_interpolate=True), 'bridge_block_interpolate'),
                        (dict(extra_blocks=t.Identity()), 'extra_blocks')):
        assert left_of(unet_standin.Decoder(**flags)).startswith(word + ':'), flags
    dec = unet_standin.Decoder()
    dec.inner_blocks[2] = t.Conv2d(128, 64, 3, padding=1)
    assert left_of(dec).startswith('inner_blocks.2: kernel_size')
    dec = unet_standin.Decoder()
    dec.inner_blocks[0] = t.Conv2d(64, 16, 1)
    assert left_of(dec).startswith('inner_blocks.0: out_channels 16')
    dec = unet_standin.Decoder()
    dec.inner_blocks[1] = t.ReLU()
    assert left_of(dec).startswith('inner_blocks.1: ReLU')
    dec = unet_standin.Decoder()
    dec.layer_blocks[1] = t.ModuleList(list(dec.layer_blocks[1]))
    assert left_of(dec).startswith('layer_blocks.1: ModuleList')
    dec = unet_standin.Decoder()
    dec.layer_blocks[1] = unet_standin.OwnForward(128, 64)  # a Sequential subclass whose forward is not the walk over its slots
    assert left_of(dec).startswith('layer_blocks.1: OwnForward')
    dec = unet_standin.Decoder()
    dec.layer_blocks[2][0] = t.Conv2d(128, 64, 3, stride=2, padding=1)
    assert left_of(dec).startswith('layer_blocks.2.0: stride')
    dec = unet_standin.Decoder()
    dec.layer_blocks[2][0] = t.BatchNorm2d(128)
    assert left_of(dec).startswith('layer_blocks.2.0: BatchNorm2d')
    dec = unet_standin.Decoder()
    dec.layer_blocks[1][0] = t.Conv2d(80, 64, 3, padding=1)  # 80 = 16 lateral + 64 top channels
    assert left_of(dec).startswith('layer_blocks.1.0: in_channels 80')
    dec = unet_standin.Decoder()
    dec.layer_blocks[0][0] = t.Conv2d(64, 32, 3, padding=1)  # a bridge level takes the top alone
    assert left_of(dec).startswith('layer_blocks.0.0: in_channels 64 on a bridge level')
    dec = unet_standin.Decoder()
    dec.inner_blocks.append(t.Identity())
    assert left_of(dec).startswith('layer_blocks: 3 blocks beside 4 inner blocks')
    dec = unet_standin.Decoder()
    del dec.cat_order
    assert left_of(dec).startswith('cat_order: the decoder has no such attribute')
    dec = unet_standin.Decoder()
    dec.has_lat = {1: True, 2: True}
    assert left_of(dec).startswith('has_lat:')


def test_any_order_with_the_other_converts_gives_the_same_modules():
    converts = {'conv': nn.convert_conv2d_, 'bn': nn.convert_batchnorm2d_, 'tail': nn.convert_readout_tail_,
                'grouped': nn.convert_grouped_conv2d_, 'bottleneck': nn.convert_bottleneck_, 'decoder': nn.convert_unet_decoder_}
    want = None
    for order in itertools.permutations(converts):
        net = _Net()
        params, keys = dict(net.named_parameters()), list(net.state_dict().keys())
        for name in order:
            out = converts[name](net)
            if name == 'decoder':
                assert out == (['unet'], {}), order
        sig = _signature(net)
        want = want or sig
        assert sig == want, order
        after = dict(net.named_parameters())
        assert after.keys() == params.keys() and all(after[k] is params[k] for k in params) and list(net.state_dict().keys()) == keys
    dec = net.unet
    _expect_converted(dec)
    for blk in dec.layer_blocks:
        assert [type(m) for m in blk] == [nn.CatConv2d, nn.BatchNorm2d, torch.nn.Identity, nn.Conv2d, nn.BatchNorm2d, torch.nn.Identity]
        assert blk[1].activation == blk[4].activation == 'relu'
    assert type(net.head[0]) is nn.Conv2d and type(net.head[4]) is nn.DropoutConv1x1 and type(net.grouped) is nn.GroupedConv2d
