"""CPU tests of the trainable bilinear resize (celldetection_amd/nn/resize.py, csrc/bilinear_train.hip, csrc/bilinear_adjoint.h): the fp64
statements of tests/bilinear_oracle.py against torch's own autograd of the stock expression, the taps against torch's on one-hot
inputs, the wrong rules the cases tell apart and the judges reject, the index arithmetic on the host under sanitizers, the host-side
entry points, the Python surface and the core convert on a stand-in core (tests/cpn_core_standin.py) pinned to the stock expression.
Nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bilinear_oracle as oracle
import celldetection_amd as cda
import conv_bounds as cb
import conv_train_oracle as dense
import cpn_core_standin as standin
from celldetection_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nn = cda.nn

# (name, N, H, W, h, w, Cin, Cout, k): exact x2; the ceil half and the floor half; 14 -> 46 and ratio 3; a 1 x 1 source; one axis at
# identity; non-square images with N = 3
CASES = [('exact_x2', 2, 16, 16, 8, 8, 4, 3, 3), ('ceil_and_floor_half', 2, 14, 13, 7, 7, 4, 3, 3), ('14_to_46_and_ratio_3', 2, 46, 9, 14, 3, 3, 2, 3),
         ('one_pixel', 2, 6, 10, 1, 1, 4, 3, 5), ('one_axis_identity', 2, 5, 14, 5, 7, 4, 3, 3), ('non_square', 3, 15, 27, 5, 9, 3, 4, 7)]


def _operands(name, n, H, W, h, w, cin, cout, k):
    g = torch.Generator().manual_seed(H * 100 + W + k)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    dy = torch.randn(n, cout, H, W, generator=g, dtype=torch.float64)
    return x, wt, b, dy


def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0])
def test_statements_equal_torch_autograd(case):
    """With the taps in float64 -- torch's own float64 rule -- the statements ARE torch's autograd of the stock expression."""
    name, n, H, W, h, w, cin, cout, k = case
    x, wt, b, dy = _operands(*case)
    f64 = dict(dtype=np.float64)
    y, dx, dw, db = oracle.autograd64(x, wt, b, dy, (H, W))
    _close(oracle.resize(x, (H, W), **f64), F.interpolate(x, size=(H, W), mode='bilinear', align_corners=False))
    _close(oracle.forward(x, wt, b, (H, W), **f64), y)
    t = oracle.top_gradient(dy, wt)
    assert t.shape == (n, cin, H, W)
    got, S, count = oracle.adjoint(t, (h, w), **f64)
    _close(got, dx)
    _close(oracle.d_input(dy, wt, (h, w), **f64), dx)
    assert bool((S >= got.abs() - 1e-9).all()) and count.shape == (h, w) and int(count.min()) >= 1
    _close(oracle.wgrad(x, dy, k, **f64)[0], dw)
    _close(oracle.bgrad(dy)[0], db)
    # the float32 taps of the kernels state the same function to float32 accuracy
    assert float((oracle.resize(x, (H, W)) - oracle.resize(x, (H, W), **f64)).abs().max()) < 1e-5
    if (h, w) == (1, 1):
        assert count.tolist() == [[H * W]] and torch.equal(oracle.resize(x, (H, W)), x.expand(n, cin, H, W))
    if h == H:
        assert torch.equal(oracle.weights(H, h), torch.eye(H, dtype=torch.float64))


def test_ba_tap_is_torchs_rule_on_one_hot_inputs():
    """For all 1 <= in <= out <= 70: torch-CPU's float32 resize of the identity matrix IS the matrix of weights -- the same index
    pairs, and every weight within one fp32 rounding -- and the footprints are contiguous, never empty, and cover every output twice
    except at the clamp.

    One rounding needs a word.  The source text leaves open how often the coordinate is rounded: split, the product
    p = scale * (dst + 0.5) and the difference p - 0.5 each on its own, or fused into one fma, as a compiler with contraction (and a
    torch build for a CPU with an fma) does.  ``ba_tap`` states both forms.  Torch's taps are bit for bit those of one of them, and
    the two differ by the rounding of p <= in alone: at most u p in lambda and in either weight, u = 2^-24 -- where that moves f
    across an integer k, the pair (k - 1, k) with lambda >= 1 - u p stands beside the pair (k, k + 1) with lambda <= u p: the same
    weights on the same source indices to within u p."""
    fused_somewhere = False
    for out in range(1, 71):
        for inn in range(1, out + 1):
            eye = torch.eye(inn, dtype=torch.float32).reshape(1, inn, inn, 1)
            want = F.interpolate(eye, size=(out, 1), mode='bilinear', align_corners=False).reshape(inn, out).t().double()
            split, fused = oracle.weights(out, inn, fused=False), oracle.weights(out, inn, fused=True)
            same = [torch.equal(m != 0, want != 0) and float((m - want).abs().max()) <= 2. ** -24 for m in (split, fused)]
            assert any(same), (inn, out)
            fused_somewhere |= not same[0]
            p = (torch.arange(out, dtype=torch.float64) + .5) * inn / out
            for m in (split, fused):
                assert bool(((m - want).abs().max(1).values <= 2. ** -24 * (p + 1.)).all()), (inn, out)
            assert bool(((split - fused).abs().max(1).values <= 2. ** -24 * (p + 1.)).all()), (inn, out)
    print('this torch build fuses the coordinate into one fma on the CPU:', fused_somewhere)
    for out in range(1, 71):
        for inn in range(1, out + 1):
            for fused in (False, True):
                i0, i1, lam = oracle.taps(out, inn, fused=fused)
                assert bool(((0 <= lam) & (lam < 1)).all()) and i0.min() >= 0 and i1.max() <= inn - 1, (inn, out)
                oracle.footprints(out, inn, fused)
    # the exact x2: 4 outputs per axis, 5 for source index 1 (the clamp at 0 gives index 0 a third output), 3 at the two ends; a
    # 1-pixel source: all of them
    widths = [hi - lo for lo, hi in oracle.footprints(512, 256)]
    assert widths[:3] == [3, 5, 4] and set(widths[2:-1]) == {4} and widths[-1] == 3
    assert max(hi - lo for lo, hi in oracle.footprints(512, 255)) == 5  # a ratio just above 2: 5 away from the border too
    assert oracle.footprints(4096, 1) == [(0, 4096)]
    i0, i1, lam = oracle.taps(16, 8)  # the exact x2: dyadic lambdas
    assert set(lam.tolist()) == {0., .25, .75} and i0.tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7]


def _differs(a, b):
    return float((a - b).abs().max()) > .05 * float(b.abs().mean())


def test_wrong_rules_are_told_apart_and_rejected_by_the_judges():
    """Each rule of bilinear_oracle.WRONG_RULES moves a result by an amount of the order of the values themselves; the judges of the
    GPU tests accept the CPU emulation of the stated arithmetic and reject the emulation of every wrong rule."""
    told = set()
    case = CASES[1]
    name, n, H, W, h, w, cin, cout, k = case
    x, wt, b, dy = _operands(*case)
    xq, wq, dyq = x.to(torch.bfloat16).double(), wt.to(torch.bfloat16).double(), dy.to(torch.bfloat16).double()
    y, dx, dw, db = oracle.autograd64(x, wt, b, dy, (H, W))
    t = oracle.top_gradient(dyq, wq).to(torch.bfloat16).double()

    # the judges accept the stated arithmetic
    blend = oracle.emulate_blend(xq, (H, W))
    oracle.check_blend('blend, fp32', oracle.emulate_blend(xq, (H, W), fused=False), xq, (H, W), stored='fp32')
    oracle.check_blend('blend, bf16', blend.to(torch.bfloat16), xq, (H, W))
    operand = blend.to(torch.bfloat16).double()
    ref, S, d = oracle.forward_bounds(xq, wq, b, (H, W))
    cb.check('forward', F.conv2d(operand, wq, b, 1, k // 2).float().to(torch.bfloat16), *cb.bf16_bounds(ref, d), ref, S)
    oracle.check_adjoint('adjoint, bf16', oracle.emulate_adjoint(t, (h, w)).to(torch.bfloat16), t, (h, w))
    oracle.check_adjoint('adjoint, fp32', oracle.emulate_adjoint(t, (h, w), fused=False), t, (h, w), stored='fp32')
    oracle.check_wgrad('dW', dense.wgrad(operand, dyq, k)[0].float(), xq, dyq, k, chain=40)

    for rule in ('align_corners', 'unclamped', 'i1_not_clamped'):
        assert _differs(oracle.forward(x, wt, b, (H, W), rule), y), rule
        wrong = oracle.emulate_blend(xq, (H, W), rule)
        with pytest.raises(cb.BoundError):
            oracle.check_blend(rule, wrong.to(torch.bfloat16), xq, (H, W))
        with pytest.raises(cb.BoundError):
            cb.check(rule, F.conv2d(wrong.to(torch.bfloat16).double(), wq, b, 1, k // 2).float().to(torch.bfloat16),
                     *cb.bf16_bounds(ref, d), ref, S)
        with pytest.raises(AssertionError):
            oracle.check_wgrad(rule, dense.wgrad(wrong.to(torch.bfloat16).double(), dyq, k)[0].float(), xq, dyq, k, chain=40)
        told.add(rule)
    for rule in ('adjoint_weights_swapped', 'adjoint_last_tap_single'):
        assert _differs(oracle.d_input(dy, wt, (h, w), rule), dx), rule
        with pytest.raises(cb.BoundError):
            oracle.check_adjoint(rule, oracle.emulate_adjoint(t, (h, w), rule).to(torch.bfloat16), t, (h, w))
        with pytest.raises(cb.BoundError):
            oracle.check_adjoint(rule, oracle.emulate_adjoint(t, (h, w), rule, fused=False), t, (h, w), stored='fp32')
        told.add(rule)
    assert _differs(oracle.wgrad(x, dy, k, 'dw_unresized')[0], dw)
    with pytest.raises(AssertionError):
        oracle.check_wgrad('dw_unresized', oracle.wgrad(xq, dyq, k, 'dw_unresized')[0].float(), xq, dyq, k, chain=40)
    told.add('dw_unresized')
    assert told == set(oracle.WRONG_RULES) and len(told) >= 6


def test_host_build_of_the_index_arithmetic_agrees_with_brute_force(tmp_path):
    """``csrc/bilinear_adjoint.h`` and the partition compiled for the host only, with AddressSanitizer and UBSan on the host code, by
    ``tests/bilinear_adjoint_host.cpp`` (a program of its own, nothing preloaded): ranges and weights against brute force for all
    1 <= in <= out <= 70 and a few large pairs."""
    hipcc = build._hipcc()
    exe = str(tmp_path / 'bilinear_adjoint_host')
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(ROOT, 'tests', 'bilinear_adjoint_host.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r'ok \d+', run.stdout.strip()), run.stdout[-500:] + run.stderr[-2000:]
    assert int(run.stdout.split()[1]) > 1000000


def _kernel_body(asm, name):
    """The instructions of the one kernel whose mangled name holds ``name``, from its label to its s_endpgm."""
    body = re.search(r'^_Z\w*%s\w*:.*?s_endpgm' % name, asm, re.S | re.M)
    assert body, name
    return body.group(0)


@pytest.mark.parametrize('source,kernel,fused', [('misc_kernels.hip', 'bilinear_kernel', True), ('decode_nms.hip', 'resize_f32_kernel', False)])
def test_the_forward_kernels_compile_the_coordinate_to_the_form_ba_tap_is_given(tmp_path, source, kernel, fused):
    """The form of the coordinate is the compiler's choice, so it is read off the compiled kernel, built with the flags of
    ``build.SOURCES``: ``bilinear_kernel`` subtracts the 0.5 inside a ``v_fma_f32`` (fused: what ``bl_sum_kernel`` and the weight
    gradient's staging pass to ``ba_tap``), ``resize_f32_kernel`` in a ``v_add_f32`` of its own (split: what ``bl_sum_planes_kernel``
    passes).  (The conv loader is compiled from csrc/conv_igemm.hip with the flags of ``bilinear_kernel``; it takes minutes to build and
    is held to the fused form by the one-hot operands of tests/test_gpu_bilinear_resize.py.)"""
    out = str(tmp_path / 'kernel.s')
    subprocess.check_call([build._hipcc(), f'--offload-arch={build.ARCH}', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                           os.path.join(build.CSRC, source), '-o', out] + build.SOURCES[source], stderr=subprocess.DEVNULL)
    body = _kernel_body(open(out).read(), kernel)
    fma = re.findall(r'v_fma(?:c|ak|mk)?_f32\w*\s[^\n]*-0\.5', body)
    add = re.findall(r'v_(?:add|sub|subrev)_f32\w*\s[^\n]*-0\.5', body)
    assert (bool(fma), bool(add)) == (fused, not fused), (kernel, fma[:2], add[:2])
    src = open(os.path.join(build.CSRC, 'bilinear_train.hip')).read()
    assert ('constexpr bool FUSED = true' in src.split('void bl_sum_kernel(')[1].split('__global__')[0]) and \
        ('constexpr bool FUSED = false' in src.split('void bl_sum_planes_kernel(')[1].split('__global__')[0])


def test_wgrad_info_and_every_launch_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    info = nn.resized_weight_grad_info
    for n, H, W, h, w in ((2, 1, 1, 1, 1), (2, 13, 14, 7, 7), (2, 6, 10, 1, 1), (2, 33, 70, 17, 35), (8, 512, 512, 256, 256)):
        for slab_rows in (0, 1, 3):
            for cin, cout, k in ((32, 32, 3), (96, 64, 3), (64, 32, 5), (64, 64, 7)):
                i = info(n, H, W, cin, (h, w), cout, k, slab_rows)
                rows = n * H
                assert i['slabs'] == -(-rows // i['slab_rows']) and i['reduce_chain'] == i['slabs']
                assert slab_rows == 0 or i['slab_rows'] == min(slab_rows, rows)
                assert i['steps'] == -(-i['slab_rows'] * W // 16)
                assert i['bias_chain'] == -(-i['slab_rows'] * W // 8) + 8 + i['slabs']
                assert lib.cpn_resized_conv_wgrad_workspace_bytes(n, H, W, cin, h, w, cout, k, slab_rows) == \
                    i['slabs'] * (cin * cout * k * k + cout) * 4
                assert i == nn.weight_grad_info(n, H, W, cin, cout, k, slab_rows)  # the partition is the dense conv's at H x W
    assert info(2, 4, 8, 32, (2, 4), 32, 3, 4)['slabs'] == 2  # a slab boundary between the two images of the batch
    out = (ctypes.c_int32 * 5)()
    # (N, H, W, cin, h, w, cout, k, slab_rows)
    for bad, what in (((0, 4, 4, 32, 2, 2, 32, 3, 0), 'N, H and W'), ((2, 4, 4, 33, 2, 2, 32, 3, 0), 'multiples'),
                      ((2, 4, 4, 0, 2, 2, 32, 3, 0), 'multiples'), ((2, 4, 4, 32, 2, 2, 48, 3, 0), 'multiples'),
                      ((2, 4, 4, 32, 5, 2, 32, 3, 0), 'h and w'), ((2, 4, 4, 32, 2, 0, 32, 3, 0), 'h and w'),
                      ((2, 4, 4, 32, 2, 2, 32, 1, 0), 'k must be'), ((2, 4, 4, 32, 2, 2, 32, 4, 0), 'k must be'),
                      ((2, 4, 4, 32, 2, 2, 32, 9, 0), 'k must be'), ((2, 4, 4, 32, 2, 2, 32, 3, -1), 'slab_rows'),
                      ((65536, 65536, 1, 32, 1, 1, 32, 3, 0), '2^31 - 1'), ((1, 1, 1, 2 ** 20, 1, 1, 2 ** 20, 3, 0), '2^31 - 1')):
        rc = lib.cpn_resized_conv_wgrad_info(*bad, out)
        assert rc in (_lib.E_INVALID, _lib.E_UNSUPPORTED) and what in lib.cpn_last_error().decode(), (bad, lib.cpn_last_error())
        assert lib.cpn_resized_conv_wgrad_workspace_bytes(*bad) == 0
        # the launch rejects the same call before it touches a buffer (the pointers are never read)
        assert lib.cpn_resized_conv_wgrad(16, 16, *bad, 16, 0, 16, 0, 16, 1 << 40, None) == rc
    ok = (2, 4, 4, 32, 2, 2, 32, 3, 0)
    assert lib.cpn_resized_conv_wgrad_info(*ok, None) == _lib.E_INVALID
    assert lib.cpn_resized_conv_wgrad(16, 16, *ok, 16, 0, 16, 0, 16, 16, None) == _lib.E_WORKSPACE
    assert lib.cpn_resized_conv_wgrad(None, 16, *ok, 16, 0, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID
    assert lib.cpn_resized_conv_wgrad(16, 8, *ok, 16, 0, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID and \
        'aligned' in lib.cpn_last_error().decode()
    assert lib.cpn_resized_conv_wgrad(16, 16, *ok, 16, 2, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID  # dtype code
    assert lib.cpn_resized_conv_wgrad(16, 16, *ok, None, 0, None, 0, 16, 1 << 40, None) == _lib.E_INVALID  # nothing to compute
    # (t, N, H, W, C, dst, h, w)
    for bad, code in (((16, 0, 4, 4, 32, 16, 2, 2), _lib.E_INVALID), ((16, 2, 4, 4, 12, 16, 2, 2), _lib.E_INVALID),
                      ((16, 2, 4, 4, 0, 16, 2, 2), _lib.E_INVALID), ((16, 2, 4, 4, 32, 16, 5, 2), _lib.E_INVALID),
                      ((16, 2, 4, 4, 32, 16, 2, 0), _lib.E_INVALID), ((16, 65536, 65536, 1, 32, 16, 1, 1), _lib.E_UNSUPPORTED),
                      ((16, 2, 65536, 65536, 32, 16, 1, 1), _lib.E_UNSUPPORTED), ((None, 2, 4, 4, 32, 16, 2, 2), _lib.E_INVALID),
                      ((16, 2, 4, 4, 32, None, 2, 2), _lib.E_INVALID), ((16, 2, 4, 4, 32, 24, 2, 2), _lib.E_INVALID)):
        assert lib.cpn_bilinear_sum(*bad, None) == code and 'cpn_bilinear_sum' in lib.cpn_last_error().decode(), bad
    # (t, planes, H, W, dst, h, w)
    for bad, code in (((16, 0, 4, 4, 16, 2, 2), _lib.E_INVALID), ((16, 3, 4, 4, 16, 5, 2), _lib.E_INVALID),
                      ((16, 3, 4, 4, 16, 2, 0), _lib.E_INVALID), ((16, 3, 0, 4, 16, 1, 1), _lib.E_INVALID),
                      ((16, 1 << 33, 4, 4, 16, 2, 2), _lib.E_UNSUPPORTED), ((16, 3, 65536, 65536, 16, 2, 2), _lib.E_UNSUPPORTED),
                      ((None, 3, 4, 4, 16, 2, 2), _lib.E_INVALID), ((16, 3, 4, 4, 18, 2, 2), _lib.E_INVALID)):
        assert lib.cpn_bilinear_sum_f32(*bad, None) == code and 'cpn_bilinear_sum_f32' in lib.cpn_last_error().decode(), bad
    # cpn_conv2d_sized with the bilinear descriptor: the sizes are looked at before any pointer
    d = nn.resize._resized_desc(32, 32, 3, False)
    args = (ctypes.byref(d), 16, 32, None, 0, None, 0, 16, 32, 2, 4, 4)
    for stored in ((0, 2, 4, 4, 4, 4), (2, 5, 4, 4, 4, 4), (-1, -1, 4, 4, 4, 4)):
        assert lib.cpn_conv2d_sized(*args, (ctypes.c_int32 * 6)(*stored), 16, None, None) == _lib.E_INVALID, stored
        assert 'resized source' in lib.cpn_last_error().decode()
    assert lib.cpn_conv2d_sized(*args, None, 16, None, None) == _lib.E_INVALID


@pytest.mark.parametrize('k', nn.RESIZED_KERNEL_SIZES)
def test_the_conv_kernels_accept_the_bilinear_descriptor(k):
    """``cpn_conv2d_kernel_info`` (host only) on the descriptor ``resized_conv2d`` hands over: the family keeps a kernel size only if
    the selection takes it, and it is the loader's bilinear mode that is selected."""
    assert nn.RESIZED_KERNEL_SIZES == (3, 5, 7)
    for H, W, cin, cout in ((16, 16, 32, 32), (14, 14, 64, 32), (6, 10, 32, 64), (34, 70, 96, 64), (512, 512, 64, 64)):
        d = nn.resize._resized_desc(cin, cout, k, True)
        assert (d.src1, d.up0, d.up1, d.c0_used, d.cin_b, d.stride, d.pad) == (-1, 2, 0, cin, cin, 1, k // 2)
        mode = _lib.conv_kernel_info(d, _lib.PRECISION_BF16, 2, H, W, cin, 0, 0, cout)[0]
        assert mode == 'BL', (mode, H, W, cin, cout)


def test_header_binding_and_exports_agree():
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    lib = _lib.load()
    new = ('cpn_resized_conv_wgrad_info', 'cpn_resized_conv_wgrad_workspace_bytes', 'cpn_resized_conv_wgrad', 'cpn_bilinear_sum',
           'cpn_bilinear_sum_f32')
    for name in new:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    flat_hdr = re.sub(r'\s*\n \*\s*', ' ', hdr)
    assert 'Trainable bilinear resize' in flat_hdr
    for phrase in ('Additions to ABI 22', 'fmaxf(scale * ((float) dst + 0.5f) - 0.5f, 0.f)', 'i1 = i0 + (i0 < in - 1)',
                   'ascending row-major', 'no fma', 'at the clamped last index both terms apply', 'never written',
                   'No floating-point atomics', 'ascending slab order', 'once per 128-pixel chunk',
                   'hy * (hx * x[y0][x0] + lx * x[y0][x1]) + ly * (hx * x[y1][x0] + lx * x[y1][x1])'):
        assert phrase in flat_hdr, phrase
    assert build.SOURCES['bilinear_train.hip'] == ['-ffp-contract=off'] and 'bilinear_adjoint.h' in build.HEADERS
    assert {'bilinear_resize', 'bilinear_resize_backward', 'resized_conv2d', 'ResizedConv2d', 'CPNCore', 'convert_cpn_core_',
            'resized_conv2d_weight_grad', 'resized_weight_grad_info'} <= set(nn.__all__)
    assert all(hasattr(nn, name) for name in nn.__all__)
    src = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'bilinear_train.hip')).read()
    dense = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'wgrad_dense.h')).read()  # the slab kernel, compiled inside the unit
    assert '#include "wgrad_dense.h"' in src and 'wgrad_dense.h' in build.HEADERS
    frag = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'mfma_frag.h')).read()  # the fragment idiom, included by the header
    assert '#include "mfma_frag.h"' in dense and 'mfma_frag.h' in build.HEADERS
    for text in (src, dense, frag):
        assert 'atomic' not in text.replace('No floating-point atomics', '') and 'fmaf' not in text and 'fma(' not in text
    assert 'ds_read_tr16_b64' in frag and 'mf_operand(' in dense and 'mfma_f32_32x32x16_bf16' in dense and 'ba_tap' in src and 'ba_first' in src
    adj = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'bilinear_adjoint.h')).read()
    assert 'fmaxf(scale * ((float) dst + 0.5f) - 0.5f, 0.f)' in adj and '*i0 + (*i0 < in_size - 1)' in adj
    assert 'fmaxf(fmaf(scale, (float) dst + 0.5f, -0.5f), 0.f)' in adj
    for name in ('conv_igemm.hip', 'misc_kernels.hip'):  # ... the rule the forward kernels state, token for token
        fwd = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', name)).read()
        assert re.search(r'fmaxf\(\w+(\.\w+)? \* \(\(float\) \w+ \+ 0\.5f\) - 0\.5f, 0\.f\)', fwd), name
    for doc in ('README.md',):
        assert 'resized_conv2d' in open(os.path.join(ROOT, doc)).read(), doc


def test_every_unsupported_argument_raises_naming_it():
    x = torch.zeros(2, 32, 3, 4)
    w = torch.zeros(32, 32, 3, 3)
    for args, name in (((x[0], w, None, (6, 8)), 'input of 3 dimensions'), ((x, w[0], None, (6, 8)), 'weight of 3 dimensions'),
                       ((x, torch.zeros(32, 32, 3, 5), None, (6, 8)), 'kernel_size'), ((x, torch.zeros(32, 32, 1, 1), None, (6, 8)), 'kernel_size 1'),
                       ((x, torch.zeros(32, 32, 9, 9), None, (6, 8)), 'kernel_size 9'),
                       ((torch.zeros(2, 48, 3, 4), torch.zeros(32, 48, 3, 3), None, (6, 8)), 'in_channels 48'),
                       ((x, torch.zeros(20, 32, 3, 3), None, (6, 8)), 'out_channels 20'), ((x, w.double(), None, (6, 8)), 'weight dtype'),
                       ((x.half(), w, None, (6, 8)), 'input dtype'), ((x, w, torch.zeros(32).double(), (6, 8)), 'bias'),
                       ((x, w, torch.zeros(16), (6, 8)), 'bias'), ((x, w, None, (2, 8)), 'upwards only'), ((x, w, None, (6, 3)), 'upwards only'),
                       ((x, w, None, 6), 'size 6'), ((torch.zeros(2, 32, 0, 4), w, None, (6, 8)), 'at least one pixel')):
        with pytest.raises(NotImplementedError, match=name):
            nn.resized_conv2d(*args)
    with pytest.raises(ValueError, match='channels'):
        nn.resized_conv2d(x, torch.zeros(32, 64, 3, 3), None, (6, 8))
    for call in (lambda: nn.resized_conv2d(x, w, None, (6, 8)), lambda: nn.resized_conv2d(x, w, None, (3, 4)), lambda: nn.resized_conv2d(x, w),
                 lambda: nn.ResizedConv2d(32, 32, 3)(x, (6, 8)), lambda: nn.ResizedConv2d(32, 32, 3)(x),
                 lambda: torch.nn.Sequential(nn.ResizedConv2d(32, 32, 7))(x), lambda: nn.bilinear_resize(x, (6, 8)),
                 lambda: nn.bilinear_resize(x, (3, 4)), lambda: nn.bilinear_resize(torch.zeros(2, 3, 3, 4), (6, 8)),
                 lambda: nn.bilinear_resize_backward(x, (2, 2)), lambda: nn.bilinear_resize_backward(torch.zeros(2, 3, 3, 4), (3, 4))):
        with pytest.raises(RuntimeError, match='MI355X'):  # supported arguments on the CPU: the usual device error, no fallback
            call()
    cl = torch.channels_last
    for t, size, name in ((torch.zeros(8, 5, 7), (10, 14), 'input of 3 dimensions'), (torch.zeros(2, 8, 5, 7).double(), (10, 14), 'input dtype'),
                          (torch.zeros(2, 8, 5, 7), (4, 14), 'upwards only'), (torch.zeros(2, 8, 5, 7), (10, 6), 'upwards only'),
                          (torch.zeros(2, 12, 5, 7).to(torch.bfloat16), (10, 14), '12 channels'),
                          (torch.zeros(2, 12, 5, 7).contiguous(memory_format=cl), (10, 14), '12 channels'),
                          (torch.zeros(2, 8, 0, 7), (10, 14), 'at least one pixel'), (torch.zeros(2, 8, 5, 7), 'big', 'size')):
        with pytest.raises(NotImplementedError, match=name):
            nn.bilinear_resize(t, size)
    for t, size, name in ((torch.zeros(8, 5, 7), (3, 4), 'input of 3 dimensions'), (torch.zeros(2, 8, 5, 7).double(), (3, 4), 'input dtype'),
                          (torch.zeros(2, 8, 5, 7), (6, 4), 'size'), (torch.zeros(2, 8, 5, 7), (3, 0), 'size'),
                          (torch.zeros(2, 12, 5, 7).to(torch.bfloat16), (3, 4), '12 channels')):
        with pytest.raises(NotImplementedError, match=name):
            nn.bilinear_resize_backward(t, size)
    for kwargs, name in ((dict(stride=2), 'stride'), (dict(groups=2), 'groups'), (dict(dilation=2), 'dilation'), (dict(padding=0), 'padding'),
                         (dict(padding_mode='reflect'), 'padding_mode'), (dict(kernel_size=9), 'kernel_size'), (dict(kernel_size=1), 'kernel_size'),
                         (dict(in_channels=48), 'in_channels'), (dict(out_channels=2), 'out_channels')):
        kw = dict(in_channels=64, out_channels=32, kernel_size=3)
        kw.update(kwargs)
        with pytest.raises(NotImplementedError, match=name):
            nn.ResizedConv2d(**kw)
    with pytest.raises(NotImplementedError, match='fork'):
        nn.ResizedConv2d(32, 32, 3)(x, (6, 8), fork=True)
    m = nn.ResizedConv2d(64, 32, 7, bias=False)
    stock = torch.nn.Conv2d(64, 32, 7, padding=3, bias=False)
    assert isinstance(m, torch.nn.Conv2d) and isinstance(m, nn.Conv2d) and list(m.state_dict()) == list(stock.state_dict())
    assert m.padding == (3, 3)
    m.load_state_dict(stock.state_dict())
    stock.load_state_dict(m.state_dict())


# ---- the core

def _core64(seed=0, **kw):
    torch.manual_seed(seed)
    return standin.randomise_(standin.Core(**kw), seed).double().eval()


@pytest.mark.parametrize('full_res', [True, False])
def test_the_stand_in_core_is_the_stock_expression(full_res):
    """float64, eval: the stand-in against the lines of the reference's forward written out with ``F.interpolate``."""
    core = _core64(uncertainty_head=True, refinement_full_res=full_res)
    g = torch.Generator().manual_seed(1)
    img = torch.randn(2, 3, 22, 26, generator=g, dtype=torch.float64)
    with torch.no_grad():
        scores, locations, refinement, fourier, uncertainty = core(img)
        feats = core.backbone(img)
        kw = dict(size=img.shape[2:], mode='bilinear', align_corners=False)
        assert tuple(feats['0'].shape) == tuple(feats['1'].shape) == (2, 32, 11, 13)
        _close(scores, core.score_head.block(feats['1']))
        _close(locations, core.location_head.block(feats['1']))
        _close(fourier, core.fourier_head.block(feats['1']))
        _close(uncertainty, torch.sigmoid(core.uncertainty_head.block(feats['1'])))
        if full_res:
            want = torch.tanh(core.refinement_head.block(F.interpolate(feats['0'], **kw))) * 3.
        else:
            want = F.interpolate(torch.tanh(core.refinement_head.block(feats['0'])) * 3., **kw)
        _close(refinement, want)
    assert refinement.shape == (2, 2, 22, 26) and scores.shape == (2, 2, 11, 13) and fourier.shape == (2, 12, 11, 13)


def _signature(net):
    return [(name, type(m), getattr(m, 'activation', None) if isinstance(m, torch.nn.BatchNorm2d) else None, getattr(m, 'p', None))
            for name, m in net.named_modules()]


class _Net(torch.nn.Module):
    def __init__(self, **kw):
        super().__init__()
        self.core = standin.Core(**kw)
        self.grouped = torch.nn.Conv2d(64, 64, 3, padding=1, groups=2)
        self.pool = torch.nn.MaxPool2d(3, 2, 1)


def test_convert_cpn_core_replaces_the_core_in_place():
    net = _Net()
    net.core.score_head.eval()
    hook = net.core.refinement_head.block[0].register_forward_hook(lambda *a: None)
    params, buffers, keys = dict(net.named_parameters()), dict(net.named_buffers()), list(net.state_dict().keys())
    heads = {name: getattr(net.core, name) for name in ('score_head', 'location_head', 'fourier_head', 'refinement_head', 'backbone')}
    block = net.core.refinement_head.block
    replaced, left = nn.convert_cpn_core_(net)
    assert (replaced, left) == (['core'], {})
    core = net.core
    assert type(core) is nn.CPNCore and all(getattr(core, k) is v for k, v in heads.items()) and core.refinement_head.block is block
    assert type(block[0]) is nn.ResizedConv2d and block[0]._forward_hooks and hook is not None
    assert [type(m) for m in block][1:] == [torch.nn.BatchNorm2d, torch.nn.ReLU, torch.nn.Dropout2d, torch.nn.Conv2d]
    assert type(core.score_head.block[0]) is torch.nn.Conv2d  # the other heads' convs are the other converts' business
    assert core.training and not core.score_head.training and core.refinement_head.training
    assert (core.order, core.refinement_full_res, core.refinement_interpolation, core.refinement_features) == (3, True, 'bilinear', '0')
    after_p, after_b = dict(net.named_parameters()), dict(net.named_buffers())
    assert after_p.keys() == params.keys() and all(after_p[k] is params[k] for k in params)  # the same Parameter objects
    assert after_b.keys() == buffers.keys() and all(after_b[k] is buffers[k] for k in buffers)
    assert list(net.state_dict().keys()) == keys
    fresh = _Net()
    fresh.load_state_dict(net.state_dict())  # state dicts interchange, both ways
    net.load_state_dict(fresh.state_dict())
    assert nn.convert_cpn_core_(net) == ([], {})  # a second call finds nothing to replace
    with pytest.raises(RuntimeError, match='MI355X'):  # the converted core runs this library's kernels: no CPU fallback
        core(torch.zeros(2, 3, 16, 16))
    # the root module is reported as left, never replaced; a class listed in core_types is a candidate
    assert nn.convert_cpn_core_(standin.Core()) == ([], {'': 'the root module cannot be replaced in place: convert its parent'})
    wrap = torch.nn.Sequential(standin.SameNames())
    assert nn.convert_cpn_core_(wrap) == ([], {}) and type(wrap[0]) is standin.SameNames
    assert nn.convert_cpn_core_(wrap, core_types=(standin.SameNames,)) == (['0'], {}) and type(wrap[0]) is nn.CPNCore
    twice = standin.Core()
    both = torch.nn.ModuleList([twice, twice])
    assert nn.convert_cpn_core_(both)[1] == {'0': 'the core sits in 2 slots', '1': 'the core sits in 2 slots'}
    # without refinement_full_res, or without a refinement head, nothing stands in front of a conv: the core is taken as it is
    for kw in (dict(refinement_full_res=False), dict(refinement_head=None)):
        wrap = torch.nn.Sequential(standin.Core(**kw))
        assert nn.convert_cpn_core_(wrap) == (['0'], {}) and type(wrap[0]) is nn.CPNCore
        assert wrap[0].refinement_head is None or type(wrap[0].refinement_head.block[0]) is torch.nn.Conv2d


def test_the_module_builds_from_converted_pieces_only():
    t = torch.nn
    head = standin.ReadOut(32, 2, 7, final_activation=standin.ScaledTanh(3.))
    head.block[0] = nn.ResizedConv2d(32, 32, 7)
    others = [standin.ReadOut(32, c, 7) for c in (1, 2, 12)]
    core = nn.CPNCore(standin.Backbone(), *others, refinement_head=head)
    assert core.refinement_full_res and core.uncertainty_head is None and core.refinement_interpolation == 'bilinear'
    assert list(core.state_dict())[0] == 'backbone.stem.0.weight' and 'refinement_head.block.0.weight' in core.state_dict()
    head.block[0] = t.Conv2d(32, 32, 7, padding=3)  # a stock conv would need the enlarged tensor
    with pytest.raises(NotImplementedError, match=r'refinement_head\.block\.0: Conv2d: not a ResizedConv2d'):
        nn.CPNCore(standin.Backbone(), *others, refinement_head=head)
    nn.CPNCore(standin.Backbone(), *others, refinement_head=head, refinement_full_res=False)


def test_every_ineligible_core_is_left_with_its_reason():
    t = torch.nn

    def left_of(core):
        keys = list(core.state_dict().keys())
        sig = _signature(core)
        replaced, left = nn.convert_cpn_core_(t.ModuleList([core]))
        assert replaced == [] and list(left) == ['0'] and _signature(core) == sig and list(core.state_dict().keys()) == keys
        return left['0']

    assert left_of(standin.Core(refinement_interpolation='bicubic')).startswith("refinement_interpolation: 'bicubic'")
    assert left_of(standin.Core(refinement_interpolation='nearest')).startswith('refinement_interpolation:')
    assert left_of(standin.Core(score_head=None)).startswith('score_head: None')
    core = standin.Core()
    del core.refinement_full_res
    assert left_of(core).startswith('refinement_full_res: the core has no such attribute')
    core = standin.Core()
    del core.contour_features
    assert left_of(core).startswith('contour_features: the core has no such attribute')
    core = standin.Core()
    core.refinement_head.block = t.ModuleList(list(core.refinement_head.block))
    assert left_of(core).startswith('refinement_head.block: ModuleList')
    core = standin.Core()
    core.refinement_head.attention = t.Identity()
    assert left_of(core).startswith('refinement_head.attention: Identity')
    core = standin.Core()
    core.refinement_head.block[0] = t.Conv2d(32, 32, 7, stride=2, padding=3)
    assert left_of(core).startswith('refinement_head.block.0: stride')
    core = standin.Core()
    core.refinement_head.block[0] = t.Conv2d(32, 32, 1)
    assert left_of(core).startswith('refinement_head.block.0: kernel_size (1, 1): square odd kernels (3, 5, 7) only')
    core = standin.Core()
    core.refinement_head.block[0] = t.Conv2d(32, 16, 7, padding=3)
    assert left_of(core).startswith('refinement_head.block.0: out_channels 16')
    core = standin.Core()
    core.refinement_head.block[0] = t.BatchNorm2d(32)
    assert left_of(core).startswith('refinement_head.block.0: BatchNorm2d')
    core = standin.Core()
    core.refinement_head.block[0] = nn.Conv2d(32, 32, 1)  # a converted conv outside the resized family
    assert left_of(core).startswith('refinement_head.block.0: kernel_size (1, 1): square odd kernels (3, 5, 7) only')


def test_any_order_with_the_other_converts_gives_the_same_modules():
    converts = [('conv', nn.convert_conv2d_), ('bn', nn.convert_batchnorm2d_), ('tail', nn.convert_readout_tail_),
                ('grouped', nn.convert_grouped_conv2d_), ('bottleneck', nn.convert_bottleneck_), ('decoder', nn.convert_unet_decoder_),
                ('stem', nn.convert_stem_conv2d_), ('pool', nn.convert_maxpool2d_)]
    orders = []
    for others in (converts, converts[::-1], converts[3:] + converts[:3]):
        for at in range(len(others) + 1):  # the core convert at every position among the others
            orders.append(others[:at] + [('core', nn.convert_cpn_core_)] + others[at:])
    want = None
    for order in orders:
        net = _Net()
        params, keys = dict(net.named_parameters()), list(net.state_dict().keys())
        for name, convert in order:
            out = convert(net)
            if name == 'core':
                assert out == (['core'], {}), [n for n, _ in order]
        sig = _signature(net)
        want = want or sig
        assert sig == want, [n for n, _ in order]
        after = dict(net.named_parameters())
        assert after.keys() == params.keys() and all(after[k] is params[k] for k in params) and list(net.state_dict().keys()) == keys
    core = net.core
    assert type(core) is nn.CPNCore
    assert [type(m) for m in core.refinement_head.block] == [nn.ResizedConv2d, nn.BatchNorm2d, torch.nn.Identity, torch.nn.Identity,
                                                             nn.DropoutConv1x1]
    assert [type(m) for m in core.score_head.block] == [nn.Conv2d, nn.BatchNorm2d, torch.nn.Identity, torch.nn.Identity, nn.DropoutConv1x1]
    assert type(core.backbone.stem[0]) is nn.StemConv2d and type(core.backbone.body[0]) is nn.Conv2d
    assert type(net.grouped) is nn.GroupedConv2d and type(net.pool) is nn.MaxPool2d
