"""GPU tests of the trainable bilinear resize (``cda.nn.bilinear_resize``, ``nn.resized_conv2d``, csrc/bilinear_train.hip) against the
fp64 statements and the judges of tests/bilinear_oracle.py.

Bounds (derived there, none measured).  The forward of the resize lies in the window of the fp64 blend with the fp32 lambdas:
gamma(6) B for the fp32 blend, and the bf16 values that window can round to.  The adjoint lies within gamma(F + 2) sum |c t| of its
fp64 statement, plus one rounding, F the footprint size from the header's own ranges.  The resized conv is judged on its virtual
operand X = bf16(blend), carried as the interval the blend window can round to: the forward by the rule of tests/conv_bounds.py
widened by sum |w| delta, dW by gamma(n) sum |dy| |X^| + sum |dy| delta with n from ``cpn_resized_conv_wgrad_info``, db as in the
dense conv, T by the conv rule, dx by the adjoint bound on the T the kernel wrote.  No allowance counts, no share of bad elements.
One-hot operands and small integers are exact.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bilinear_oracle as oracle
import celldetection_amd as cda
import conv_bounds as cb
import conv_train_oracle as dense
import cpn_core_standin as standin

pytestmark = pytest.mark.gpu
nn = cda.nn
N = 2


def bf16_exact(*shape, seed, scale=1.):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).float()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


# (H, W, h, w): exact x2; 7 -> 13 and 7 -> 14; 14 -> 46; 5 x 9 -> 15 x 27; 1 x 1 -> 6 x 10; one axis at identity; 17 x 35 -> 33 x 70
SHAPES = [(16, 16, 8, 8), (13, 14, 7, 7), (46, 6, 14, 3), (15, 27, 5, 9), (6, 10, 1, 1), (5, 14, 5, 7), (33, 70, 17, 35)]
# (H, W, h, w, C, Cout, k): k = 3 everywhere, 5 and 7 on two shapes; the last shapes give several 128-pixel chunks per slab
CASES = [(16, 16, 8, 8, 32, 32, 3), (13, 14, 7, 7, 64, 64, 3), (46, 6, 14, 3, 32, 32, 3), (15, 27, 5, 9, 96, 32, 3), (6, 10, 1, 1, 32, 64, 3),
         (5, 14, 5, 7, 32, 32, 3), (33, 70, 17, 35, 96, 64, 3), (13, 14, 7, 7, 32, 32, 5), (33, 70, 17, 35, 64, 32, 7), (13, 14, 7, 7, 32, 32, 7),
         (33, 70, 17, 35, 32, 32, 5)]
ids = lambda c: 'x'.join(map(str, c))  # noqa: E731


# ---- the resize alone

@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_bilinear_resize_forward_lies_in_the_blend_window(shape):
    H, W, h, w = shape
    for fused in (True, False):  # every output lies in two footprints per axis, in one at the clamp
        oracle.footprints(H, h, fused), oracle.footprints(W, w, fused)
    for c in (32, 96):
        x = bf16_exact(N, c, h, w, seed=H + W + c)
        for dtype in (torch.bfloat16, torch.float32):
            got = nn.bilinear_resize(x.to(dtype).cuda().contiguous(memory_format=torch.channels_last), (H, W))
            assert got.dtype == torch.bfloat16 and got.shape == (N, c, H, W) and got.is_contiguous(memory_format=torch.channels_last)
            r = oracle.check_blend(f'resize {shape} C {c} {dtype}', got.float(), x, (H, W))
        got16 = nn.bilinear_resize(x.to(torch.bfloat16).cuda(), (H, W))  # an NCHW-contiguous bf16 input: the same bits
        assert same_bits(got16, got)
    for c in (1, 2, 12):
        x = torch.randn(N, c, h, w, generator=torch.Generator().manual_seed(H + c))
        got = nn.bilinear_resize(x.cuda(), (H, W))
        assert got.dtype == torch.float32 and got.shape == (N, c, H, W) and got.is_contiguous()
        r = max(r, oracle.check_blend(f'resize {shape} planes {c}', got, x, (H, W), stored='fp32'))
    print(f'{shape}: largest error / window {r:.3f}')
    same = torch.zeros(N, 32, H, W, device='cuda')
    assert nn.bilinear_resize(same, (H, W)) is same


@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_adjoint_within_the_footprint_bound_and_adjoint_to_the_resize(shape):
    H, W, h, w = shape
    worst = 0.
    for c in (32, 64):
        t = bf16_exact(N, c, H, W, seed=3 * H + W + c)
        for dtype in (torch.bfloat16, torch.float32):
            got = nn.bilinear_resize_backward(t.to(dtype).cuda().contiguous(memory_format=torch.channels_last), (h, w))
            assert got.dtype == torch.bfloat16 and got.shape == (N, c, h, w) and got.is_contiguous(memory_format=torch.channels_last)
            worst = max(worst, oracle.check_adjoint(f'adjoint {shape} C {c} {dtype}', got.float(), t, (h, w)))
        assert same_bits(nn.bilinear_resize_backward(t.to(torch.bfloat16).cuda(), (h, w)), got)  # NCHW-contiguous bf16: the same bits
        # <resize(x), t> == <x, adjoint(t)> in fp64 on the operands read, to within what the adjoint's own bound leaves open
        x = bf16_exact(N, c, h, w, seed=H + c).double()
        b = oracle.adjoint_bounds(t, (h, w))
        slack = float((x.abs() * torch.maximum(b['hi'] - b['ref'], b['ref'] - b['lo'])).sum())
        lhs, rhs = float((oracle.resize(x, (H, W)) * t.double()).sum()), float((x * got.double().cpu()).sum())
        assert abs(lhs - rhs) <= slack + 1e-9 * abs(lhs), (shape, lhs, rhs, slack)
    for c in (1, 2, 12):
        t = torch.randn(N, c, H, W, generator=torch.Generator().manual_seed(H + c))
        got = nn.bilinear_resize_backward(t.cuda(), (h, w))
        assert got.dtype == torch.float32 and got.shape == (N, c, h, w) and got.is_contiguous()
        worst = max(worst, oracle.check_adjoint(f'adjoint {shape} planes {c}', got, t, (h, w), stored='fp32'))
        x = torch.randn(N, c, h, w, generator=torch.Generator().manual_seed(c)).double()
        b = oracle.adjoint_bounds(t, (h, w), stored='fp32')
        slack = float((x.abs() * torch.maximum(b['hi'] - b['ref'], b['ref'] - b['lo'])).sum())
        lhs, rhs = float((oracle.resize(x, (H, W), fused=False) * t.double()).sum()), float((x * got.double().cpu()).sum())
        assert abs(lhs - rhs) <= slack + 1e-9 * abs(lhs), (shape, lhs, rhs, slack)
    print(f'{shape}: largest error / bound {worst:.3f}')


def test_adjoint_is_bit_equal_on_small_integers_with_dyadic_lambdas():
    """The exact x2: lambdas 0, 1/4, 3/4, coefficients multiples of 1/16, integers in [-4, 4]: every fp32 product and sum is exact
    whatever its order, so the result is the statement rounded once; and two runs give the same bits."""
    H, W, h, w = 16, 16, 8, 8
    g = torch.Generator().manual_seed(1)
    t = torch.randint(-4, 5, (N, 40, H, W), generator=g).float()
    want, _, count = oracle.adjoint(t, (h, w))
    assert int(count.max()) == 25 and int(count.min()) == 9 and int(count[3, 3]) == 16  # 5 wide next to the border, 3 at it
    for dtype in (torch.float32, torch.bfloat16):
        got = nn.bilinear_resize_backward(t.to(dtype).cuda().contiguous(memory_format=torch.channels_last), (h, w))
        assert torch.equal(got.cpu(), want.float().to(torch.bfloat16))
        assert same_bits(got, nn.bilinear_resize_backward(t.to(dtype).cuda().contiguous(memory_format=torch.channels_last), (h, w)))
    planes = nn.bilinear_resize_backward(t[:, :3].contiguous().cuda(), (h, w))
    assert torch.equal(planes.cpu().double(), want[:, :3])  # (the exact x2: the split and the fused coordinate are the same numbers)
    x = torch.randint(-3, 4, (N, 40, h, w), generator=g).double()
    stock = F.interpolate(x, size=(H, W), mode='bilinear', align_corners=False)
    assert float((stock * t.double()).sum()) == float((x * want).sum())  # exact arithmetic: torch's own resize is the adjoint's


def test_bilinear_resize_autograd_saves_nothing_and_matches_stock():
    H, W, h, w = 13, 14, 7, 7
    for x, stored in ((bf16_exact(N, 32, h, w, seed=2).to(torch.bfloat16), 'bf16'), (torch.randn(N, 12, h, w), 'fp32')):
        x = x.cuda().requires_grad_(True)
        saved = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
            y = nn.bilinear_resize(x, (H, W))
        assert saved == []
        g = bf16_exact(*y.shape, seed=5).cuda()
        y.backward(g.to(y.dtype)[:, :, ::1].transpose(2, 3).contiguous().transpose(2, 3))  # a grad_output of other strides
        assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
        oracle.check_adjoint(f'autograd {stored}', x.grad.float(), g.cpu(), (h, w), stored=stored)


# ---- the resized conv

@functools.lru_cache(maxsize=None)
def operands(H, W, h, w, c, cout, k):
    """x, weight (fp32, not bf16-exact: the pack rounds it), bias, dY of one case and every fp64 reference of it, computed once."""
    seed = 7 * H + 13 * W + 3 * h + w + c + 5 * cout + k
    x, dy = bf16_exact(N, c, h, w, seed=seed + 1), bf16_exact(N, cout, H, W, seed=seed + 2)
    g = torch.Generator().manual_seed(seed + 3)
    wt = torch.randn(cout, c, k, k, generator=g) / math.sqrt(c * k * k)
    b = torch.randn(cout, generator=g)
    wq = wt.to(torch.bfloat16).double()
    top = cb.conv_with_noise(dy, dense.unpack(dense.pack_dgrad(wq), cout, k), None, 1, k // 2, n=cb.chain_length(k, k, cout))
    return dict(x=x, dy=dy, w=wt, b=b, wq=wq, fwd=oracle.forward_bounds(x, wq, b.double(), (H, W)), top=top, bgrad=oracle.bgrad(dy))


def check_sum(name, got, ref, S, chain):
    """|got - ref| <= gamma(chain) * S + one fp32 rounding of the result."""
    d = cb.gamma(chain) * S
    tol = d + cb.U * (ref.abs() + d)
    err = (got.double().cpu() - ref).abs()
    assert bool(torch.isfinite(got).all()) and bool((err <= tol).all()), (name, float((err / tol.clamp_min(1e-300)).max()))


def check_wgrad(case, slab_rows):
    H, W, h, w, c, cout, k = case
    o = operands(*case)
    info = nn.resized_weight_grad_info(N, H, W, c, (h, w), cout, k, slab_rows)
    chain = info['steps'] + 2 + info['reduce_chain']
    assert chain <= -(-N * H * W // 16) + 2 + info['slabs'], info  # the library cannot widen its own bound
    assert slab_rows == 0 or info['slab_rows'] == min(slab_rows, N * H)
    dw, db = nn.resized_conv2d_weight_grad(o['x'].cuda(), o['dy'].cuda(), k, slab_rows)
    assert dw.dtype == db.dtype == torch.float32 and dw.shape == (cout, c, k, k) and db.shape == (cout,)
    oracle.check_wgrad(f'dW {case} slab_rows {slab_rows} ({info["slabs"]} slabs)', dw, o['x'], o['dy'], k, chain)
    check_sum(f'db {case} slab_rows {slab_rows}', db, *o['bgrad'], info['bias_chain'])
    return info


@pytest.mark.parametrize('case', CASES, ids=ids)
def test_forward_and_gradients_within_the_bounds(case):
    H, W, h, w, c, cout, k = case
    o = operands(*case)
    x = o['x'].cuda().requires_grad_(True)
    wt, b = o['w'].cuda().requires_grad_(True), o['b'].cuda().requires_grad_(True)
    y = nn.resized_conv2d(x, wt, b, (H, W))
    assert y.dtype == torch.bfloat16 and y.shape == (N, cout, H, W) and y.is_contiguous(memory_format=torch.channels_last)
    ref, S, d = o['fwd']
    r = cb.check(f'forward {case}', y.detach().float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
    y.backward(o['dy'].cuda())
    # T, the gradient at size, as the backward computed it (the same deterministic call), by the conv rule; dx on that T
    t = nn._common._run_conv(nn._common._nhwc(o['dy'].cuda(), torch.bfloat16), nn.pack_weight(wt.detach(), 'dgrad'), None, cout, c, k)
    ref, S, d = o['top']
    r2 = cb.check(f'T {case}', t.float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    r3 = oracle.check_adjoint(f'dx {case}', x.grad.cpu(), t.float().cpu(), (h, w))
    assert same_bits(x.grad.to(torch.bfloat16), nn.bilinear_resize_backward(t, (h, w)))
    print(f'{case}: forward ratio {r:.3f}, T ratio {r2:.3f}, dx ratio {r3:.3f}')
    info = nn.resized_weight_grad_info(N, H, W, c, (h, w), cout, k)
    oracle.check_wgrad(f'dW {case} autograd', wt.grad, o['x'], o['dy'], k, info['steps'] + 2 + info['reduce_chain'])
    check_sum(f'db {case} autograd', b.grad, *o['bgrad'], info['bias_chain'])


@pytest.mark.parametrize('slab_rows', [1, 3, 0])
@pytest.mark.parametrize('case', [CASES[1], CASES[6], CASES[8]], ids=ids)
def test_weight_and_bias_gradient_within_the_chain_bound(case, slab_rows):
    info = check_wgrad(case, slab_rows)
    if slab_rows == 1:
        assert info['slabs'] == N * case[0]
    if slab_rows == 3 and case[0] in (13, 33):
        assert (N * case[0]) % info['slab_rows'] != 0 or case[0] == 33  # 26 rows: a partial last slab; 66 rows: 22 whole slabs


@pytest.mark.parametrize('case', [CASES[1], CASES[6], CASES[10]], ids=ids)
def test_slab_boundary_between_two_images(case):
    info = check_wgrad(case, case[0])
    assert info['slabs'] == N and info['slab_rows'] == case[0]
    if case[0] == 33:
        assert info['steps'] > 2 * 128 // 16  # 2310 pixels per slab: eighteen full chunks and a partial one


def test_weight_gradient_is_bit_identical_from_run_to_run_and_rounds_once():
    case = CASES[6]
    H, W, h, w, c, cout, k = case
    o = operands(*case)
    args = (o['x'].cuda(), o['dy'].cuda(), k)
    dw, db = nn.resized_conv2d_weight_grad(*args)
    for _ in range(2):
        dw2, db2 = nn.resized_conv2d_weight_grad(*args)
        assert same_bits(dw, dw2) and same_bits(db, db2)
    dw16, db16 = nn.resized_conv2d_weight_grad(*args, dtype=torch.bfloat16)
    assert dw16.dtype == db16.dtype == torch.bfloat16 and same_bits(dw16, dw.to(torch.bfloat16)) and same_bits(db16, db.to(torch.bfloat16))
    only_w = nn.resized_conv2d_weight_grad(*args, bias=False)
    only_b = nn.resized_conv2d_weight_grad(*args, weight=False)
    assert only_w[1] is None and only_b[0] is None and same_bits(only_w[0], dw) and same_bits(only_b[1], db)


# ---- the virtual operand, read out of each route

def forward_operand(x, size, c):
    """A one-hot weight (centre tap, co == ci): y IS the operand the loader handed to the MFMA (one product by 1, the rest zeros)."""
    wt = torch.zeros(c, c, 3, 3)
    wt[torch.arange(c), torch.arange(c), 1, 1] = 1.
    return nn.resized_conv2d(x.cuda(), wt.cuda(), None, size).float().cpu()


def wgrad_operand(x, size, c):
    """One-hot dY -- channel co at one pixel of its own per run --: dW[co, :, 1, 1] IS the operand the staging wrote at that pixel."""
    H, W = size
    pixels = N * H * W
    out = torch.zeros(pixels, c)
    for first in range(0, pixels, 32):
        dy = torch.zeros(pixels, 32)
        idx = torch.arange(first, min(first + 32, pixels))
        dy[idx, idx - first] = 1.
        dw, _ = nn.resized_conv2d_weight_grad(x.cuda(), dy.reshape(N, H, W, 32).permute(0, 3, 1, 2).cuda(), 3, bias=False)
        out[idx] = dw[:len(idx), :, 1, 1].cpu()
    return out.reshape(N, H, W, c).permute(0, 3, 1, 2)


@pytest.mark.parametrize('shape', [(13, 14, 7, 7), (6, 10, 1, 1), (5, 14, 5, 7)], ids=ids)
def test_one_hot_operands_read_the_virtual_operand_out_of_each_route(shape):
    H, W, h, w = shape
    c = 32
    x = bf16_exact(N, c, h, w, seed=H)
    ref, d = oracle.blend_window(x, (H, W))
    lo, hi = cb.bf16_bounds(ref, d)
    fwd, wg = forward_operand(x, (H, W), c), wgrad_operand(x, (H, W), c)
    cb.check(f'forward operand {shape}', fwd, lo, hi, ref)
    cb.check(f'weight-gradient operand {shape}', wg, lo, hi, ref)
    alone = nn.bilinear_resize(x.cuda(), (H, W)).float().cpu()
    print(f'{shape}: forward loader == staging: {torch.equal(fwd, wg)}; forward loader == bilinear_resize: {torch.equal(fwd, alone)}; '
          f'staging == bilinear_resize: {torch.equal(wg, alone)}')  # (recorded, not asserted: the loader is compiled with contraction)
    # a constant image is its own resize, exactly, and so is the identity (reached through the kernel itself)
    const = torch.arange(1, c + 1).float().reshape(1, c, 1, 1).expand(N, c, h, w).contiguous()
    assert torch.equal(forward_operand(const, (H, W), c), const[:, :, :1, :1].expand(N, c, H, W))
    assert torch.equal(wgrad_operand(const, (H, W), c), const[:, :, :1, :1].expand(N, c, H, W))
    assert torch.equal(wgrad_operand(x, (h, w), c), x)
    # the forward route at the identity: ``resized_conv2d`` falls through to ``conv2d`` there, and the bilinear descriptor itself,
    # handed to ``cpn_conv2d_sized`` with equal stored sizes, turns the loader's resize off (csrc/conv_args.hip): both give x itself
    assert torch.equal(forward_operand(x, (h, w), c), x)
    one_hot = torch.zeros(c, c, 3, 3)
    one_hot[torch.arange(c), torch.arange(c), 1, 1] = 1.
    xs = nn._common._nhwc(x.cuda(), torch.bfloat16)
    assert torch.equal(nn.resize._run_resized_conv(xs, nn.pack_weight(one_hot.cuda(), 'forward'), None, c, c, 3, (h, w)).float().cpu(), x)


def test_huge_values_outside_the_tensors_never_reach_a_result():
    """x and dY sit in buffers filled with 3.4e38 in front of and behind them (what a read one row above the first image, below the
    last, or behind the last real channel block would meet); Cin = 32 and 96 leave half of a 64-channel tile unreal."""
    for case in (CASES[1][:4] + (32, 32, 3), CASES[3]):
        H, W, h, w, c, cout, k = case
        x, dy = bf16_exact(N, c, h, w, seed=1), bf16_exact(N, cout, H, W, seed=2)
        wt = (torch.randn(cout, c, k, k, generator=torch.Generator().manual_seed(3)) / math.sqrt(c * k * k)).cuda()

        def inside(t):
            n, ch, hh, ww = t.shape
            view, buf = cb.guarded((n, hh, ww, ch), torch.bfloat16, 8 * ww * ch, 0x7f7f, 'cuda')
            view.copy_(t.permute(0, 2, 3, 1))
            return view.permute(0, 3, 1, 2), buf

        def run(xs, gs):
            xs = xs.detach().requires_grad_(True)
            w_ = wt.detach().requires_grad_(True)
            y = nn.resized_conv2d(xs, w_, None, (H, W))
            y.backward(gs)
            return y.detach(), xs.grad, w_.grad

        plain = run(x.cuda().to(torch.bfloat16), dy.cuda().to(torch.bfloat16))
        (xg, xbuf), (gg, gbuf) = inside(x), inside(dy)
        assert float(xbuf.float().abs().max()) > 1e38 and xg.is_contiguous(memory_format=torch.channels_last)
        guarded = run(xg, gg)
        assert all(bool(torch.isfinite(t.float()).all()) for t in guarded)
        assert all(same_bits(p, q) for p, q in zip(plain, guarded)), case
        assert same_bits(nn.bilinear_resize_backward(gg, (h, w)), nn.bilinear_resize_backward(dy.cuda().to(torch.bfloat16), (h, w)))


# ---- layout, dtypes and gradient plumbing

def run(x, wt, b, dy, size, need=(True, True, True)):
    x = x.detach().clone().requires_grad_(need[0])
    wt = wt.detach().clone().requires_grad_(need[1])
    b = None if b is None else b.detach().clone().requires_grad_(need[2])
    y = nn.resized_conv2d(x, wt, b, size)
    if any(need):
        y.backward(dy)
    return y.detach(), x.grad, wt.grad, None if b is None else b.grad


def test_layouts_dtypes_and_requested_gradients(monkeypatch):
    case = CASES[1]
    H, W, h, w, c, cout, k = case
    o = operands(*case)
    x32 = torch.randn(N, c, h, w, generator=torch.Generator().manual_seed(3)).cuda()  # not bf16-exact
    wt, b, dy = o['w'].cuda(), o['b'].cuda(), o['dy'].cuda().to(torch.bfloat16)
    cl = torch.channels_last
    base = run(x32.to(torch.bfloat16).contiguous(memory_format=cl), wt, b, dy, (H, W))
    assert base[1].dtype == torch.bfloat16 and base[2].dtype == base[3].dtype == torch.float32
    assert all(same_bits(p, q) for p, q in zip(base, run(x32.to(torch.bfloat16).contiguous(), wt, b, dy, (H, W)))), 'NCHW input differs'
    f32 = run(x32, wt, b, dy, (H, W))
    assert f32[1].dtype == torch.float32
    assert same_bits(base[0], f32[0]) and same_bits(base[1], f32[1].to(torch.bfloat16)) and same_bits(base[2], f32[2]) and \
        same_bits(base[3], f32[3]), 'an fp32 input differs from its bf16 rounding'
    p16 = run(x32, wt.to(torch.bfloat16), b.to(torch.bfloat16), dy, (H, W))  # bf16 parameters: bf16 gradients, rounded once
    w16 = run(x32, wt.to(torch.bfloat16).float(), b.to(torch.bfloat16).float(), dy, (H, W))
    assert p16[2].dtype == p16[3].dtype == torch.bfloat16
    assert same_bits(p16[0], w16[0]) and same_bits(p16[2], w16[2].to(torch.bfloat16)) and same_bits(p16[3], w16[3].to(torch.bfloat16))
    wide = torch.zeros(N, cout, H, 2 * W, device='cuda')  # a non-contiguous grad_output: every second column of a wider fp32 tensor
    wide[..., ::2] = dy.float()
    assert not wide[..., ::2].is_contiguous()
    assert all(same_bits(p, q) for p, q in zip(base, run(x32.to(torch.bfloat16), wt, b, wide[..., ::2], (H, W))))
    # only the requested gradients are returned, and a kernel whose gradient is not asked for is not run
    calls = []
    real_conv, real_sum, real_wgrad = nn.resize._run_conv, nn.resize.bilinear_resize_backward, nn.resize.resized_conv2d_weight_grad
    monkeypatch.setattr(nn.resize, '_run_conv', lambda *a, **kw: (calls.append(('conv', a[4])), real_conv(*a, **kw))[1])  # (a[4]: channels out)
    monkeypatch.setattr(nn.resize, 'bilinear_resize_backward', lambda *a, **kw: (calls.append(('sum',)), real_sum(*a, **kw))[1])
    monkeypatch.setattr(nn.resize, 'resized_conv2d_weight_grad', lambda *a, **kw: (calls.append(('wgrad', kw['weight'], kw['bias'])),
                                                                            real_wgrad(*a, **kw))[1])
    for need in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (True, False, False),
                 (False, True, False), (False, False, True)):
        del calls[:]
        got = run(x32.to(torch.bfloat16), wt, b, dy, (H, W), need)
        for j in range(3):
            assert (got[1 + j] is not None) == need[j], need
            assert got[1 + j] is None or same_bits(got[1 + j], base[1 + j]), need
        want = ([('conv', c), ('sum',)] if need[0] else []) + ([('wgrad', need[1], need[2])] if need[1] or need[2] else [])
        assert calls == want, (need, calls)
    monkeypatch.undo()
    nob = run(x32.to(torch.bfloat16), wt, None, dy, (H, W))
    assert nob[3] is None and same_bits(nob[1], base[1]) and same_bits(nob[2], base[2])
    with torch.no_grad():
        assert same_bits(nn.resized_conv2d(x32, wt, b, (H, W)), base[0])
    again = run(x32.to(torch.bfloat16).contiguous(memory_format=cl), wt, b, dy, (H, W))  # two runs: the same bits
    assert all(same_bits(p, q) for p, q in zip(base, again))
    assert same_bits(nn.resized_conv2d(x32, wt, b, (h, w)), nn.conv2d(x32, wt, b))  # equal sizes fall through to conv2d
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.resized_conv2d(x32.cpu(), wt.cpu(), b.cpu(), (H, W))


@pytest.mark.parametrize('case', [CASES[1], CASES[6]], ids=ids)
def test_nothing_of_the_sizes_extent_is_saved(case):
    H, W, h, w, c, cout, k = case
    o = operands(*case)
    saved = []
    x, wt = o['x'].cuda().requires_grad_(True), o['w'].cuda().requires_grad_(True)
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        y = nn.resized_conv2d(x, wt, o['b'].cuda().requires_grad_(True), (H, W))
    nbytes = sum(t.numel() * t.element_size() for t in saved)
    assert len(saved) == 2 and nbytes == 2 * N * c * h * w + wt.numel() * wt.element_size()  # N h w C 2 bytes and the weight
    assert all(t.shape[2:] != (H, W) for t in saved)
    stock = []  # the best before: stock F.interpolate feeding conv2d saves the enlarged tensor
    x2 = o['x'].cuda().requires_grad_(True)
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (stock.append(t), t)[1], lambda t: t):
        nn.conv2d(F.interpolate(x2.to(torch.bfloat16), size=(H, W), mode='bilinear', align_corners=False), wt, None)
    assert sum(t.numel() * t.element_size() for t in stock if t.dim() == 4 and t.shape[2:] == (H, W)) >= 2 * N * c * H * W
    y.backward(o['dy'].cuda())
    assert x.grad is not None and wt.grad is not None


def test_module_is_a_drop_in_and_takes_the_plain_tensor_too():
    case = CASES[1]
    H, W, h, w, c, cout, k = case
    o = operands(*case)
    torch.manual_seed(0)
    stock = torch.nn.Conv2d(c, cout, k, padding=k // 2).cuda()
    mine = nn.ResizedConv2d(c, cout, k).cuda()
    mine.load_state_dict(stock.state_dict())
    x = o['x'].cuda()
    y = mine(x, (H, W))
    ref, S, d = oracle.forward_bounds(o['x'], mine.weight.detach().to(torch.bfloat16).double().cpu(), mine.bias.detach().double().cpu(), (H, W))
    cb.check('module, resized', y.detach().float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
    assert same_bits(torch.nn.Sequential(mine)(x), nn.conv2d(x, mine.weight, mine.bias))  # the one-argument form is the plain conv
    y.float().sum().backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 and bool(p.grad.abs().sum() > 0) for p in mine.parameters())


# ---- a converted core: the new ops judged inside the chain on the operands they saw

def test_converted_core_chain_from_label_images():
    """The stand-in core converted by all converts, in training mode: label image -> ``CPNTargetGenerator`` -> core -> ``CPNObjective``
    -> ``backward()``.  (a) The refinement head's ``ResizedConv2d`` is judged on the operands it saw (captured by hooks): its output
    within the forward bound, its weight and bias gradients ``resized_conv2d_weight_grad`` of those operands bit for bit, the gradient
    that leaves it towards the features ``bilinear_resize_backward`` of the dgrad conv of what arrived, bit for bit and within the
    adjoint bound.  (b) With ``refinement_full_res=False`` the head map goes through ``bilinear_resize`` on fp32 planes: value and
    gradient are held against stock fp32 autograd of ``F.interpolate`` on the same planes, within the blend window and the adjoint
    bound."""
    H, W, order, S = 32, 40, 3, 8
    yy, xx = np.mgrid[:H, :W]
    gens = []
    for discs in (((8, 9, 6), (20, 28, 7), (24, 8, 5)), ((10, 12, 7), (21, 27, 8))):
        lab = np.zeros((H, W), np.int32)
        for i, (cy, cx, r) in enumerate(discs):
            lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = i + 1
        gen = cda.CPNTargetGenerator(samples=S, order=order)
        gen.feed(torch.as_tensor(lab[..., None]).cuda())
        gens.append(gen)
    targets = cda.collate_cpn_targets(gens)
    image = bf16_exact(N, 3, H, W, seed=9).cuda()
    for full_res in (True, False):
        torch.manual_seed(1)
        net = torch.nn.ModuleDict(dict(core=standin.randomise_(standin.Core(order=order, score_channels=1, refinement_full_res=full_res), 2)))
        net = net.cuda().train()
        assert nn.convert_cpn_core_(net) == (['core'], {})
        for convert in (nn.convert_stem_conv2d_, nn.convert_maxpool2d_, nn.convert_conv2d_, nn.convert_batchnorm2d_,
                        nn.convert_readout_tail_, nn.convert_grouped_conv2d_, nn.convert_bottleneck_, nn.convert_unet_decoder_):
            convert(net)  # all of them (the stand-in has no pool, grouped conv, bottleneck or decoder: those find nothing)
        core = net['core']
        block = core.refinement_head.block
        assert type(core) is nn.CPNCore and type(block[0]) is (nn.ResizedConv2d if full_res else nn.Conv2d)
        assert type(block[4]) is nn.DropoutConv1x1 and type(core.backbone.stem[0]) is nn.StemConv2d
        seen = {}

        def hook(module, args, output):
            seen['x'], seen['size'], seen['y'] = args[0].detach(), (args[1] if len(args) > 1 else None), output.detach()
            output.register_hook(lambda g: seen.__setitem__('dy', g.detach()))

        def alias(module, args):  # the features have a second consumer (the backbone's body): an alias takes this one's gradient alone
            x = args[0].view_as(args[0])
            x.register_hook(lambda g: seen.__setitem__('dx', g.detach()))
            return (x,) + tuple(args[1:])

        def plane_hook(module, args, output):
            seen['planes'] = output
            output.register_hook(lambda g: seen.__setitem__('dplanes', g.detach()))

        block[0].register_forward_pre_hook(alias)
        block[0].register_forward_hook(hook)
        core.refinement_head.register_forward_hook(plane_hook)
        torch.manual_seed(21)
        scores, locations, refinement, fourier, uncertainty = core(image)
        assert uncertainty is None and refinement.shape == (N, 2, H, W) and scores.shape == (N, 1, H // 2, W // 2)
        assert all(m.dtype == torch.float32 and m.is_contiguous() for m in (scores, locations, refinement, fourier))
        refinement.register_hook(lambda g: seen.__setitem__('dref', g.detach()))
        objective = cda.CPNObjective(order, S, refinement_iterations=2)
        loss, losses = objective(scores, locations, refinement, fourier, targets, size=(H, W))
        loss.backward()
        assert bool(torch.isfinite(loss))
        for name, p in net.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), name
        conv = block[0]
        if full_res:  # (a)
            assert tuple(seen['size']) == (H, W) and tuple(seen['x'].shape) == (N, 32, H // 2, W // 2) and 'planes' not in seen
            x, dy = seen['x'].float().cpu(), seen['dy']
            wq = conv.weight.detach().to(torch.bfloat16).double().cpu()
            ref, S_, d = oracle.forward_bounds(x, wq, conv.bias.detach().double().cpu(), (H, W))
            cb.check('chain: forward', seen['y'].float().cpu(), *cb.bf16_bounds(ref, d), ref, S_)
            dw, db = nn.resized_conv2d_weight_grad(seen['x'], dy, 7)
            assert same_bits(conv.weight.grad, dw) and same_bits(conv.bias.grad, db)
            info = nn.resized_weight_grad_info(N, H, W, 32, (H // 2, W // 2), 32, 7)
            oracle.check_wgrad('chain: dW', dw, x, dy.float().cpu(), 7, info['steps'] + 2 + info['reduce_chain'])
            t = nn._common._run_conv(nn._common._nhwc(dy, torch.bfloat16), nn.pack_weight(conv.weight.detach(), 'dgrad'), None, 32, 32, 7)
            assert same_bits(seen['dx'].to(torch.bfloat16), nn.bilinear_resize_backward(t, (H // 2, W // 2)))
            oracle.check_adjoint('chain: dx', seen['dx'].float().cpu(), t.float().cpu(), (H // 2, W // 2))
        else:  # (b)
            planes = seen['planes'].detach()
            assert planes.dtype == torch.float32 and tuple(planes.shape) == (N, 2, H // 2, W // 2)
            oracle.check_blend('chain: head map', refinement.detach(), planes.cpu(), (H, W), stored='fp32')
            oracle.check_adjoint('chain: head map gradient', seen['dplanes'], seen['dref'].cpu(), (H // 2, W // 2), stored='fp32')
            leaf = planes.clone().requires_grad_(True)
            stock = F.interpolate(leaf, size=(H, W), mode='bilinear', align_corners=False)
            stock.backward(seen['dref'])
            # stock's blend and stock's scatter (another order of the same terms) lie in the same windows: twice their half-width
            _, d = oracle.blend_window(planes.cpu(), (H, W), fused=False)
            assert bool(((stock.detach() - refinement.detach()).abs().cpu().double() <= 2 * d).all())
            b = oracle.adjoint_bounds(seen['dref'].cpu(), (H // 2, W // 2), stored='fp32')
            assert bool(((leaf.grad - seen['dplanes']).abs().cpu().double() <= 2 * (b['hi'] - b['ref'])).all())
