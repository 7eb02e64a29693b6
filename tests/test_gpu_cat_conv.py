"""GPU tests of the trainable concat convolution (``cda.nn.cat_conv2d``, csrc/cat_conv_train.hip) against the fp64 statements of
tests/cat_conv_oracle.py.

Bounds (derived, none measured).  Forward and the lateral's gradient are judged by the rule of tests/conv_bounds.py (imported,
unchanged): the fp64 conv of exactly the operands the kernel reads -- the virtual concat of the bf16 lateral and the resized bf16 top,
the bf16-rounded weights of the pack -- noise gamma(n) * S for the chain over the channels reduced, and the bf16 values that window can
round to.  The top's gradient: ``T``, the dgrad conv at the lateral's size, is a stored bf16 tensor whose every element lies in the
window ``cb.bf16_bounds`` gives it; ``d_top`` is the fp32 sum of F of them in a fixed order rounded once, so it lies in the interval
sum of the windows over the footprint widened by gamma(F) * sum |T| and one bf16 rounding.  A weight-gradient element lies within
gamma(n) * S of the fp64 sum plus one rounding of the result, n = MFMA steps per slab + 2 + reduce chain as
``cpn_cat_conv_wgrad_info`` reports them -- and the test holds n <= ceil(N H W / 16) + 2 + slabs, so the library cannot widen its own
bound.  The bias gradient likewise.  No allowance counts, no share of bad elements.  One-hot operands and small integers are exact.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import celldetection_amd as cda
import cat_conv_oracle as oracle
import conv_bounds as cb
import conv_train_oracle as dense
import unet_standin

pytestmark = pytest.mark.gpu
nn = cda.nn
N = 2


def bf16_exact(*shape, seed, scale=1.):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def operands(H, W, h, w, c0, c1, cout, k):
    """lateral (None: bridge), top, weight (fp32, not bf16-exact: the pack rounds it), bias, dY of one case and every fp64 reference of
    it, computed once."""
    seed = 7 * H + 13 * W + 3 * h + w + c0 + 3 * c1 + 5 * cout + k
    lateral = bf16_exact(N, c0, H, W, seed=seed) if c0 else None
    top, dy = bf16_exact(N, c1, h, w, seed=seed + 1), bf16_exact(N, cout, H, W, seed=seed + 2)
    g = torch.Generator().manual_seed(seed + 3)
    wt = torch.randn(cout, c0 + c1, k, k, generator=g) / math.sqrt((c0 + c1) * k * k)
    b = torch.randn(cout, generator=g)
    wq = wt.to(torch.bfloat16).double()
    xcat = oracle.concat(lateral, top)
    fwd = cb.conv_with_noise(xcat, wq, b.double(), 1, k // 2, n=cb.chain_length(k, k, c0 + c1))
    n_bwd = cb.chain_length(k, k, cout)
    bwd_l = None
    if c0:
        bwd_l = cb.conv_with_noise(dy, dense.unpack(dense.pack_dgrad(wq[:, :c0]), cout, k), None, 1, k // 2, n=n_bwd)
    return dict(lateral=lateral, top=top, dy=dy, w=wt, b=b, fwd=fwd, bwd_l=bwd_l, dtop=dtop_bounds(dy, wq[:, c0:], (h, w)),
                wgrad=oracle.wgrad(lateral, top, dy, k), bgrad=oracle.bgrad(dy))


def dtop_bounds(dy, wq_top, size):
    """The accepted interval of every element of ``d_top`` for the gradient ``dy`` and the top's half ``wq_top`` [Cout, C1, k, k] of
    the bf16-rounded weights (module docstring) -> dict(lo, hi, ref, S)."""
    cout, k = wq_top.shape[0], wq_top.shape[2]
    t_ref, t_S, t_d = cb.conv_with_noise(dy, dense.unpack(dense.pack_dgrad(wq_top), cout, k), None, 1, k // 2,
                                         n=cb.chain_length(k, k, cout))
    t_lo, t_hi = cb.bf16_bounds(t_ref, t_d)  # the stored T lies in [t_lo, t_hi], element by element
    sum_lo, _, count = oracle.d_top(t_lo, size)
    sum_hi = oracle.d_top(t_hi, size)[0]
    sum_abs = oracle.d_top(torch.maximum(t_lo.abs(), t_hi.abs()), size)[0]
    noise = cb.gamma(count.double().clamp_min(1.)) * sum_abs  # F adds in fp32, in a fixed order
    return dict(lo=cb.bf16_down(sum_lo - noise), hi=cb.bf16_up(sum_hi + noise), ref=oracle.d_top(t_ref, size)[0], S=sum_abs)


def check_sum(name, got, ref, S, chain):
    """|got - ref| <= gamma(chain) * S + one fp32 rounding of the result."""
    d = cb.gamma(chain) * S
    tol = d + cb.U * (ref.abs() + d)
    err = (got.double().cpu() - ref).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f'{name}: chain {chain}, largest error / bound {worst:.3f}')
    assert bool(torch.isfinite(got).all()) and bool((err <= tol).all()), (name, worst)
    return worst


def check_wgrad(case, slab_rows):
    H, W, h, w, c0, c1, cout, k = case
    o = operands(*case)
    info = nn.cat_weight_grad_info(N, H, W, c0, c1, (h, w), cout, k, slab_rows)
    chain = info['steps'] + 2 + info['reduce_chain']
    assert chain <= -(-N * H * W // 16) + 2 + info['slabs'], info
    assert slab_rows == 0 or info['slab_rows'] == min(slab_rows, N * H)
    lateral = None if o['lateral'] is None else o['lateral'].cuda()
    dw, db = nn.cat_conv2d_weight_grad(lateral, o['top'].cuda(), o['dy'].cuda(), k, slab_rows)
    assert dw.dtype == db.dtype == torch.float32 and dw.shape == (cout, c0 + c1, k, k) and db.shape == (cout,)
    check_sum(f'dW {case} slab_rows {slab_rows} ({info["slabs"]} slabs)', dw, *o['wgrad'], chain)
    check_sum(f'db {case} slab_rows {slab_rows}', db, *o['bgrad'], info['bias_chain'])
    return info


# (H, W, h, w, C0, C1, Cout, k): exact x2, ceil half, floor half, ratio 3, identity resize, one footprint is the image, more than one
# 128-pixel chunk per slab with a 64-channel tile that straddles the sources (3x3 and 1x1); C0 = 0: the bridge level (H = 2 h)
CASES = [(6, 8, 3, 4, 32, 32, 32, 3), (5, 7, 3, 4, 32, 64, 64, 3), (5, 7, 2, 3, 64, 32, 32, 3), (9, 10, 3, 3, 64, 32, 32, 1),
         (5, 7, 5, 7, 32, 32, 32, 3), (3, 40, 1, 1, 32, 32, 64, 3), (17, 33, 9, 17, 96, 32, 160, 3), (17, 33, 9, 17, 32, 96, 64, 1),
         (2, 2, 1, 1, 0, 32, 32, 3), (6, 10, 3, 5, 0, 64, 32, 3), (34, 40, 17, 20, 0, 32, 64, 3),
         # the two larger kernels of the family: the two-source forward and the one-fragment instantiations of the weight gradient
         (5, 7, 3, 4, 32, 32, 32, 5), (5, 7, 3, 4, 32, 32, 32, 7)]
SLAB_CASES = [CASES[1], CASES[6], CASES[7], CASES[9]]
LARGE_K_CASES = [(17, 33, 9, 17, 32, 32, 32, 5), (17, 33, 9, 17, 32, 32, 32, 7)]
ids = lambda c: 'x'.join(map(str, c))  # noqa: E731


@pytest.mark.parametrize('case', CASES, ids=ids)
def test_forward_and_gradients_within_the_bounds(case):
    H, W, h, w, c0, c1, cout, k = case
    o = operands(*case)
    lateral = None if c0 == 0 else o['lateral'].cuda().requires_grad_(True)
    top = o['top'].cuda().requires_grad_(True)
    wt, b = o['w'].cuda().requires_grad_(True), o['b'].cuda().requires_grad_(True)
    y = nn.cat_conv2d(lateral, top, wt, b)
    assert y.dtype == torch.bfloat16 and y.shape == (N, cout, H, W) and y.is_contiguous(memory_format=torch.channels_last)
    ref, S, d = o['fwd']
    r = cb.check(f'forward {case}', y.detach().float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
    y.backward(o['dy'].cuda())
    r2 = 0.
    if c0:
        ref, S, d = o['bwd_l']
        assert lateral.grad.dtype == torch.float32 and lateral.grad.shape == lateral.shape
        r2 = cb.check(f'd_lateral {case}', lateral.grad.cpu(), *cb.bf16_bounds(ref, d), ref, S)
    t = o['dtop']
    assert top.grad.dtype == torch.float32 and top.grad.shape == top.shape
    r3 = cb.check(f'd_top {case}', top.grad.cpu(), t['lo'], t['hi'], t['ref'], t['S'])
    print(f'{case}: forward ratio {r:.3f}, d_lateral ratio {r2:.3f}, d_top ratio {r3:.3f}')
    info = nn.cat_weight_grad_info(N, H, W, c0, c1, (h, w), cout, k)
    check_sum(f'dW {case} autograd', wt.grad, *o['wgrad'], info['steps'] + 2 + info['reduce_chain'])
    check_sum(f'db {case} autograd', b.grad, *o['bgrad'], info['bias_chain'])


@pytest.mark.parametrize('slab_rows', [1, 3, 0])
@pytest.mark.parametrize('case', SLAB_CASES, ids=ids)
def test_weight_and_bias_gradient_within_the_chain_bound(case, slab_rows):
    info = check_wgrad(case, slab_rows)
    if slab_rows == 1:
        assert info['slabs'] == N * case[0]
    if slab_rows == 3 and case[0] in (5, 17):
        assert (N * case[0]) % info['slab_rows'] != 0  # a partial last slab


@pytest.mark.parametrize('case', [CASES[1], CASES[6]], ids=ids)
def test_slab_boundary_between_two_images(case):
    info = check_wgrad(case, case[0])
    assert info['slabs'] == N and info['slab_rows'] == case[0]


@pytest.mark.parametrize('case', LARGE_K_CASES, ids=ids)
def test_large_kernels_with_several_chunks_per_slab(case):
    """k = 5 and 7 run one fragment per wave and stage 132 / 134 rows per chunk, all of them through the source-pixel table: a slab
    of one image (561 pixels: four full chunks and a partial one), the auto partition, and the forward with every gradient."""
    info = check_wgrad(case, case[0])
    assert info['slabs'] == N and info['steps'] > 2 * 128 // 16
    check_wgrad(case, 0)
    test_forward_and_gradients_within_the_bounds(case)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_weight_gradient_is_bit_identical_from_run_to_run_and_rounds_once():
    case = CASES[6]
    H, W, h, w, c0, c1, cout, k = case
    o = operands(*case)
    args = (o['lateral'].cuda(), o['top'].cuda(), o['dy'].cuda(), k)
    dw, db = nn.cat_conv2d_weight_grad(*args)
    for _ in range(2):
        dw2, db2 = nn.cat_conv2d_weight_grad(*args)
        assert same_bits(dw, dw2) and same_bits(db, db2)
    dw16, db16 = nn.cat_conv2d_weight_grad(*args, dtype=torch.bfloat16)
    assert dw16.dtype == db16.dtype == torch.bfloat16 and same_bits(dw16, dw.to(torch.bfloat16)) and same_bits(db16, db.to(torch.bfloat16))
    only_w = nn.cat_conv2d_weight_grad(*args, bias=False)
    only_b = nn.cat_conv2d_weight_grad(*args, weight=False)
    assert only_w[1] is None and only_b[0] is None and same_bits(only_w[0], dw) and same_bits(only_b[1], db)


# ---- one slab kernel, three sources (csrc/wgrad_dense.h): at an identity map the gathered and the blended rows ARE the rows of the
# materialised tensor, and the partitions coincide, so the routes agree with the dense one bit for bit

IDENTITY_HW = (5, 7)


def same_partition(a, b):
    assert a == b, (a, b)
    return a


@pytest.mark.parametrize('slab_rows', [1, 0])
@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('c1', [32, 64])
def test_concat_route_at_an_identity_map_is_the_dense_route_bit_for_bit(c1, k, slab_rows):
    H, W = IDENTITY_HW
    c0 = cout = 32
    lateral, top = bf16_exact(N, c0, H, W, seed=300 + c1 + k).cuda(), bf16_exact(N, c1, H, W, seed=400 + c1 + k).cuda()
    dy = bf16_exact(N, cout, H, W, seed=500 + c1 + k).cuda()
    info = same_partition(nn.cat_weight_grad_info(N, H, W, c0, c1, (H, W), cout, k, slab_rows),
                          nn.weight_grad_info(N, H, W, c0 + c1, cout, k, slab_rows))
    assert slab_rows == 0 or info['slabs'] == N * H
    assert bool(torch.isfinite(lateral).all() and torch.isfinite(top).all() and torch.isfinite(dy).all())
    dw, db = nn.cat_conv2d_weight_grad(lateral, top, dy, k, slab_rows)
    dw_dense, db_dense = nn.conv2d_weight_grad(torch.cat((lateral, top), 1), dy, k, slab_rows)
    assert same_bits(dw, dw_dense) and same_bits(db, db_dense), (c1, k, slab_rows, info)
    if slab_rows == 0:  # ... and as autograd calls them: nn.cat_conv2d against nn.conv2d on the materialised concat
        wt, b = bf16_exact(cout, c0 + c1, k, k, seed=600 + c1 + k, scale=.1).cuda(), bf16_exact(cout, seed=700 + c1 + k).cuda()
        grads = []
        for conv in (lambda w_, b_: nn.cat_conv2d(lateral, top, w_, b_), lambda w_, b_: nn.conv2d(torch.cat((lateral, top), 1), w_, b_)):
            w_, b_ = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
            conv(w_, b_).backward(dy)
            grads.append((w_.grad, b_.grad))
        assert same_bits(grads[0][0], grads[1][0]) and same_bits(grads[0][1], grads[1][1]) and same_bits(grads[0][0], dw)


@pytest.mark.parametrize('slab_rows', [1, 0])
@pytest.mark.parametrize('k', [3, 7])
@pytest.mark.parametrize('c', [32, 96])
def test_resized_route_at_an_identity_map_is_the_dense_route_bit_for_bit(c, k, slab_rows):
    """both lambdas are 0 at equal sizes: the blend is 1 * (1 * a + 0 * b) + 0 * (...) = a on finite values"""
    H, W = IDENTITY_HW
    cout = 32
    x, dy = bf16_exact(N, c, H, W, seed=100 + c + k).cuda(), bf16_exact(N, cout, H, W, seed=200 + c + k).cuda()
    info = same_partition(nn.resized_weight_grad_info(N, H, W, c, (H, W), cout, k, slab_rows),
                          nn.weight_grad_info(N, H, W, c, cout, k, slab_rows))
    assert slab_rows == 0 or info['slabs'] == N * H
    assert bool(torch.isfinite(x).all() and torch.isfinite(dy).all())
    dw, db = nn.resized_conv2d_weight_grad(x, dy, k, slab_rows)
    dw_dense, db_dense = nn.conv2d_weight_grad(x, dy, k, slab_rows)
    assert same_bits(dw, dw_dense) and same_bits(db, db_dense), (c, k, slab_rows, info)


# ---- the adjoint of the resize alone, exact

@pytest.mark.parametrize('shape', [(6, 8, 3, 4), (5, 7, 3, 4), (5, 7, 2, 3), (9, 10, 3, 3), (5, 7, 5, 7), (3, 40, 1, 1), (46, 3, 14, 2),
                                   (17, 33, 9, 17)], ids=ids)
def test_nearest_resize_backward_is_bit_equal_on_small_integers(shape):
    """integers in [-4, 4]: every fp32 sum is exact whatever its order, so the result is the statement rounded once"""
    H, W, h, w = shape
    g = torch.Generator().manual_seed(H + W)
    t = torch.randint(-4, 5, (N, 40, H, W), generator=g).float()
    want, _, count = oracle.d_top(t, (h, w))
    assert int(count.sum()) == H * W
    for dtype in (torch.float32, torch.bfloat16):
        got = nn.nearest_resize_backward(t.to(dtype).cuda(), (h, w))
        assert got.dtype == torch.bfloat16 and got.shape == (N, 40, h, w) and got.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got.cpu(), want.float().to(torch.bfloat16)), shape
    # ... and it is the adjoint of torch's own resize: <resize(x), t> == <x, adjoint(t)> in exact integer arithmetic
    x = torch.randint(-3, 4, (N, 40, h, w), generator=g).double()
    assert float((F.interpolate(x, size=(H, W), mode='nearest') * t.double()).sum()) == float((x * want).sum())
    nchw = nn.nearest_resize_backward(t.cuda().contiguous(), (h, w))  # an NCHW-contiguous input: the same bits
    assert torch.equal(nchw.cpu(), want.float().to(torch.bfloat16))


# ---- the index map, exact

@pytest.mark.parametrize('shape', [(5, 7, 3, 4), (46, 3, 14, 2), (9, 10, 3, 3)], ids=ids)
def test_one_hot_operands_are_exact_everywhere(shape):
    """k = 1, the top one-hot at one pixel and channel: the output is the weight column on exactly the pixel's footprint; dY one-hot:
    d_top is the weight row at exactly the source pixel; with small-integer dY the weight gradient counts the footprint exactly.
    46 <- 14 is a size at which the float rule and integer arithmetic place a pixel differently."""
    H, W, h, w = shape
    c0 = c1 = cout = 32
    g = torch.Generator().manual_seed(H)
    wt = torch.randn(cout, c0 + c1, 1, 1, generator=g).to(torch.bfloat16).float()
    lateral = torch.zeros(N, c0, H, W)
    dy_int = torch.randint(-3, 4, (N, cout, H, W), generator=g).float()
    sy, sx = oracle.src_index(H, h).tolist(), oracle.src_index(W, w).tolist()
    moved = [d for d in range(H) if sy[d] != oracle.src_index(H, h, 'integer_footprint')[d]]  # rows the integer rule would misplace
    assert bool(moved) == (shape == (46, 3, 14, 2))
    for n0, i, j, c in ((0, 0, 0, 5), (1, h - 1, w - 1, 31), (1, h // 2, w // 2, 0), (0, sy[moved[0]] if moved else 1, 0, 17)):
        top = torch.zeros(N, c1, h, w)
        top[n0, c, i, j] = 1.
        want = torch.zeros(N, cout, H, W)
        for y in range(H):
            for x in range(W):
                if sy[y] == i and sx[x] == j:
                    want[n0, :, y, x] = wt[:, c0 + c, 0, 0]
        assert bool((want != 0).any())
        lt, tp, wg = lateral.cuda().requires_grad_(True), top.cuda().requires_grad_(True), wt.cuda().requires_grad_(True)
        y_ = nn.cat_conv2d(lt, tp, wg)
        assert torch.equal(y_.detach().float().cpu(), want), (shape, n0, i, j, c)
        y_.backward(dy_int.cuda())
        dw_want = oracle.wgrad(lateral, top, dy_int, 1)[0]
        assert torch.equal(wg.grad.double().cpu(), dw_want), (shape, n0, i, j, c)
    for n0, y, x, co in ((0, 0, 0, 3), (1, H - 1, W - 1, 31), (1, H // 2, W // 2, 16), (0, moved[0] if moved else 1, W - 1, 0)):
        dy = torch.zeros(N, cout, H, W)
        dy[n0, co, y, x] = 1.
        lt, tp, wg = lateral.cuda().requires_grad_(True), torch.zeros(N, c1, h, w).cuda().requires_grad_(True), wt.cuda()
        nn.cat_conv2d(lt, tp, wg).backward(dy.cuda())
        want_t = torch.zeros(N, c1, h, w)
        want_t[n0, :, sy[y], sx[x]] = wt[co, c0:, 0, 0]
        want_l = torch.zeros(N, c0, H, W)
        want_l[n0, :, y, x] = wt[co, :c0, 0, 0]
        assert torch.equal(tp.grad.cpu(), want_t) and torch.equal(lt.grad.cpu(), want_l), (shape, n0, y, x, co)


# ---- layout, dtypes and gradient plumbing

def run(lateral, top, wt, b, dy, need=(True, True, True, True)):
    lateral = None if lateral is None else lateral.detach().clone().requires_grad_(need[0])
    top = top.detach().clone().requires_grad_(need[1])
    wt = wt.detach().clone().requires_grad_(need[2])
    b = None if b is None else b.detach().clone().requires_grad_(need[3])
    y = nn.cat_conv2d(lateral, top, wt, b)
    if any(need):
        y.backward(dy)
    return y.detach(), None if lateral is None else lateral.grad, top.grad, wt.grad, None if b is None else b.grad


def test_layouts_dtypes_and_requested_gradients(monkeypatch):
    case = CASES[1]
    H, W, h, w, c0, c1, cout, k = case
    o = operands(*case)
    g = torch.Generator().manual_seed(3)
    lat32, top32 = torch.randn(N, c0, H, W, generator=g).cuda(), torch.randn(N, c1, h, w, generator=g).cuda()  # not bf16-exact
    wt, b, dy = o['w'].cuda(), o['b'].cuda(), o['dy'].cuda().to(torch.bfloat16)
    cl = torch.channels_last
    base = run(lat32.to(torch.bfloat16).contiguous(memory_format=cl), top32.to(torch.bfloat16).contiguous(memory_format=cl), wt, b, dy)
    assert base[1].dtype == base[2].dtype == torch.bfloat16 and base[3].dtype == base[4].dtype == torch.float32
    nchw = run(lat32.to(torch.bfloat16).contiguous(), top32.to(torch.bfloat16).contiguous(), wt, b, dy)
    assert all(same_bits(p, q) for p, q in zip(base, nchw)), 'NCHW-contiguous inputs differ'
    f32 = run(lat32, top32, wt, b, dy)
    assert f32[1].dtype == f32[2].dtype == torch.float32
    assert same_bits(base[0], f32[0]) and same_bits(base[1], f32[1].to(torch.bfloat16)) and same_bits(base[2], f32[2].to(torch.bfloat16)) \
        and same_bits(base[3], f32[3]) and same_bits(base[4], f32[4]), 'fp32 inputs differ from their bf16 rounding'
    mixed = run(lat32, top32.to(torch.bfloat16), wt, b, dy)  # every input's gradient in its own dtype
    assert mixed[1].dtype == torch.float32 and mixed[2].dtype == torch.bfloat16 and same_bits(mixed[2], base[2])
    p16 = run(lat32, top32, wt.to(torch.bfloat16), b.to(torch.bfloat16), dy)  # bf16 parameters: bf16 gradients, rounded once
    w16 = run(lat32, top32, wt.to(torch.bfloat16).float(), b.to(torch.bfloat16).float(), dy)
    assert p16[3].dtype == p16[4].dtype == torch.bfloat16
    assert same_bits(p16[0], w16[0]) and same_bits(p16[3], w16[3].to(torch.bfloat16)) and same_bits(p16[4], w16[4].to(torch.bfloat16))
    perm = dy.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).float()  # grad_output fp32 with channels-last strides
    assert all(same_bits(p, q) for p, q in zip(base, run(lat32.to(torch.bfloat16), top32.to(torch.bfloat16), wt, b, perm)))
    # only the requested gradients are returned, and a conv whose gradient is not asked for is not run
    calls = []
    real_conv, real_sum, real_wgrad = nn.cat_conv._run_conv, nn.cat_conv.nearest_resize_backward, nn.cat_conv.cat_conv2d_weight_grad
    monkeypatch.setattr(nn.cat_conv, '_run_conv', lambda *a, **kw: (calls.append(('conv', a[4])), real_conv(*a, **kw))[1])  # (a[4]: channels out)
    monkeypatch.setattr(nn.cat_conv, 'nearest_resize_backward', lambda *a, **kw: (calls.append(('sum',)), real_sum(*a, **kw))[1])
    monkeypatch.setattr(nn.cat_conv, 'cat_conv2d_weight_grad', lambda *a, **kw: (calls.append(('wgrad', kw['weight'], kw['bias'])),
                                                                        real_wgrad(*a, **kw))[1])
    for need in ((False, True, True, True), (True, False, True, True), (True, True, False, True), (True, True, True, False),
                 (False, False, True, False), (True, False, False, False), (False, True, False, False), (False, False, False, True)):
        del calls[:]
        got = run(lat32.to(torch.bfloat16), top32.to(torch.bfloat16), wt, b, dy, need)
        for j in range(4):
            assert (got[1 + j] is not None) == need[j], need
            assert got[1 + j] is None or same_bits(got[1 + j], base[1 + j]), need
        want = ([('conv', c0)] if need[0] else []) + ([('conv', c1), ('sum',)] if need[1] else []) + \
            ([('wgrad', need[2], need[3])] if need[2] or need[3] else [])
        assert calls == want, (need, calls)
    monkeypatch.undo()
    nob = run(lat32.to(torch.bfloat16), top32.to(torch.bfloat16), wt, None, dy)
    assert nob[4] is None and same_bits(nob[1], base[1]) and same_bits(nob[2], base[2]) and same_bits(nob[3], base[3])
    with torch.no_grad():
        assert same_bits(nn.cat_conv2d(lat32, top32, wt, b), base[0])
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.cat_conv2d(lat32.cpu(), top32.cpu(), wt.cpu(), b.cpu())


@pytest.mark.parametrize('case', [CASES[1], CASES[9]], ids=ids)
def test_nothing_of_the_concats_size_is_saved(case):
    H, W, h, w, c0, c1, cout, k = case
    o = operands(*case)
    saved = []
    lateral = None if c0 == 0 else o['lateral'].cuda().requires_grad_(True)
    top, wt = o['top'].cuda().requires_grad_(True), o['w'].cuda().requires_grad_(True)
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        y = nn.cat_conv2d(lateral, top, wt, o['b'].cuda().requires_grad_(True))
    nbytes = sum(t.numel() * t.element_size() for t in saved)
    budget = 2 * N * c0 * H * W + 2 * N * c1 * h * w + wt.numel() * wt.element_size()
    print(f'{case}: saved {nbytes} bytes in {len(saved)} tensors, budget {budget}; the concat alone: {2 * N * (c0 + c1) * H * W}')
    assert nbytes <= budget and all(t.shape[2:] != (H, W) or t.shape[1] == c0 for t in saved if t.dim() == 4 and t is not wt)
    y.backward(o['dy'].cuda())
    assert top.grad is not None and wt.grad is not None


def test_module_is_a_drop_in_and_takes_the_concatenated_tensor_too():
    case = CASES[1]
    H, W, h, w, c0, c1, cout, k = case
    o = operands(*case)
    torch.manual_seed(0)
    stock = torch.nn.Conv2d(c0 + c1, cout, k, padding=k // 2).cuda()
    mine = nn.CatConv2d(c0 + c1, cout, k).cuda()
    mine.load_state_dict(stock.state_dict())
    lateral, top = o['lateral'].cuda(), o['top'].cuda()
    y = mine(lateral, top)
    cat = torch.cat((lateral, F.interpolate(top, size=(H, W), mode='nearest')), 1)
    one = torch.nn.Sequential(mine)(cat)  # the one-tensor form is conv2d on the materialised concat
    assert same_bits(one, nn.conv2d(cat, mine.weight, mine.bias))

    def within(name, got, x, m):
        r, S, d = cb.conv_with_noise(x.cpu(), m.weight.detach().to(torch.bfloat16).double().cpu(), m.bias.detach().double().cpu(), 1,
                                     k // 2, n=cb.chain_length(k, k, x.shape[1]))
        cb.check(name, got.detach().float().cpu(), *cb.bf16_bounds(r, d), r, S)

    within('module, two inputs', y, cat, mine)
    within('module, one input', one, cat, mine)
    y.float().sum().backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 and bool(p.grad.abs().sum() > 0) for p in mine.parameters())
    bridge = nn.CatConv2d(c1, cout, k).cuda()
    yb = bridge(None, top)
    up = F.interpolate(top, scale_factor=2, mode='nearest')
    assert yb.shape == (N, cout, 2 * h, 2 * w)
    within('module, bridge', yb, up, bridge)
    within('module, bridge, one input', bridge(up), up, bridge)


# ---- a converted decoder: every new op judged inside the chain on the operands it saw, at the bounds above

def test_converted_decoder_chain_against_stock_autograd():
    """The stand-in decoder (levels = the reference's kind of ``nn.Sequential`` subclass) converted by all converts, in training mode,
    forward and backward.
    (a) Every level's ``CatConv2d`` is judged inside the chain on the operands it saw (captured by hooks): its output within the
    forward bound, its weight gradient ``cat_conv2d_weight_grad`` of those operands bit for bit, the gradient that leaves it towards
    the top within the ``d_top`` interval, and -- where the lateral is an input of the decoder -- the lateral's gradient within the
    dgrad bound.
    (b) The inner 1x1 convs, which ``UNetDecoder`` runs BEFORE the resize: the gradient that arrives at their output is the ``d_top``
    of (a) at the low resolution; their weight and bias gradients lie within the chain bound of ``oracle.inner_gradients`` on the
    operands seen, and for the deepest one, whose input is an input of the decoder, ``d_last`` lies within the dgrad bound.
    (c) The whole decoder against the stock stand-in in fp32 on the same parameters: every stored activation is rounded to bf16
    (relative 2^-9), a level stores four of them and its inner conv one, three levels: at most 16 roundings reach the output, each
    of at most 2^-8 of the largest magnitude once the batch norms have rescaled it -- 16 * 2^-8 of the largest output magnitude, a
    coarse bound that any change of rule (a misplaced pixel, a swapped concat) exceeds by an order.  The gradients of the whole
    chain have no bound of that kind (a batch norm's backward divides by a standard deviation that itself moved): they are covered
    op by op in (a) and (b), and here only as finite and of stock's shapes."""
    torch.manual_seed(2)
    stock = unet_standin.randomise_(unet_standin.Decoder(), 2).cuda().train()
    net = torch.nn.ModuleDict(dict(unet=unet_standin.Decoder())).cuda().train()
    net['unet'].load_state_dict(stock.state_dict())
    assert all(type(b) is unet_standin.TwoConvNormRelu for b in net['unet'].layer_blocks)
    assert nn.convert_unet_decoder_(net) == (['unet'], {})
    nn.convert_conv2d_(net)
    nn.convert_batchnorm2d_(net)
    dec = net['unet']
    assert type(dec) is nn.UNetDecoder and all(type(b[0]) is nn.CatConv2d and type(b[3]) is nn.Conv2d for b in dec.layer_blocks)
    assert [type(m) for m in dec.inner_blocks] == [nn.Conv2d, torch.nn.Identity, nn.Conv2d]
    feats = {k: v.requires_grad_(True) for k, v in unet_standin.features(N, 36, 52, seed=4, device='cuda').items()}
    feats_ref = {k: v.detach().clone().requires_grad_(True) for k, v in feats.items()}
    seen = {i: {} for i in range(3)}
    inner_in = {}

    def cat_hook(i):
        def hook(module, args, output):
            s = seen[i]
            s['lateral'], s['top'], s['y'] = None if args[0] is None else args[0].detach(), args[1].detach(), output.detach()
            output.register_hook(lambda g: s.__setitem__('dy', g.detach()))
            args[1].register_hook(lambda g: s.__setitem__('dtop', g.detach()))
        return hook

    for i in range(3):
        dec.layer_blocks[i][0].register_forward_hook(cat_hook(i))
    for i in (0, 2):
        dec.inner_blocks[i].register_forward_hook(lambda module, args, output, i=i: inner_in.__setitem__(i, args[0].detach()))
    out = dec(feats, (36, 52))
    ref = stock(feats_ref, (36, 52))
    assert list(out) == list(ref) and out['out'].shape == ref['out'].shape == (N, 32, 36, 52)
    gout = bf16_exact(N, 32, 36, 52, seed=6).cuda()
    (out['out'].float() * gout).sum().backward()
    (ref['out'] * gout).sum().backward()
    # (a) every level's CatConv2d on the operands it saw: level -> (lateral size, top size, C0, C1, the decoder input that is its lateral)
    levels = {2: ((9, 13), (5, 7), 64, 64, '1'), 1: ((18, 26), (9, 13), 64, 64, '0'), 0: ((36, 52), (18, 26), 0, 32, None)}
    for i, (size, tsize, c0, c1, lat_key) in levels.items():
        s, cat = seen[i], dec.layer_blocks[i][0]
        lateral = None if s['lateral'] is None else s['lateral'].float().cpu()
        top, dy = s['top'].float().cpu(), s['dy'].float().cpu()
        assert tuple(top.shape[1:]) == (c1,) + tsize and tuple(dy.shape[2:]) == size and s['top'].dtype == s['dy'].dtype == torch.bfloat16
        assert (lateral is None) == (c0 == 0) and (lateral is None or tuple(lateral.shape[1:]) == (c0,) + size)
        cout = cat.out_channels
        wq = cat.weight.detach().to(torch.bfloat16).double().cpu()
        r, S, d = cb.conv_with_noise(oracle.concat(lateral, top), wq, None, 1, 1, n=cb.chain_length(3, 3, c0 + c1))
        cb.check(f'chain, level {i}: forward', s['y'].float().cpu(), *cb.bf16_bounds(r, d), r, S)
        dw, _ = nn.cat_conv2d_weight_grad(s['lateral'], s['top'], s['dy'], 3, bias=False)
        assert same_bits(cat.weight.grad, dw), i
        t = dtop_bounds(dy, wq[:, c0:], tsize)
        assert s['dtop'].dtype == torch.bfloat16 and tuple(s['dtop'].shape) == tuple(s['top'].shape)
        cb.check(f'chain, level {i}: d_top', s['dtop'].float().cpu(), t['lo'], t['hi'], t['ref'], t['S'])
        if lat_key is not None:
            r, S, d = cb.conv_with_noise(dy, dense.unpack(dense.pack_dgrad(wq[:, :c0]), cout, 3), None, 1, 1, n=cb.chain_length(3, 3, cout))
            cb.check(f'chain, level {i}: d_lateral', feats[lat_key].grad.cpu(), *cb.bf16_bounds(r, d), r, S)
    # (b) the inner convs at the low resolution: the gradient at their output is the d_top of (a)
    for i, cin, c1 in ((2, 128, 64), (0, 64, 32)):
        conv = dec.inner_blocks[i]
        last, g = inner_in[i].float().cpu(), seen[i]['dtop'].float().cpu()
        assert tuple(last.shape) == (N, cin) + tuple(g.shape[2:]) and g.shape[1] == c1
        wq = conv.weight.detach().to(torch.bfloat16).double().cpu()
        d_last, dw_ref, db_ref = oracle.inner_gradients(last, wq, g)  # (g is at the low resolution already: footprints of one pixel)
        info = nn.weight_grad_info(N, last.shape[2], last.shape[3], cin, c1, 1)
        dw_dense, S = dense.wgrad(last, g, 1)
        torch.testing.assert_close(dw_dense, dw_ref, rtol=1e-12, atol=1e-12)
        check_sum(f'chain, inner {i}: dW', conv.weight.grad, dw_ref, S, info['steps'] + 2 + info['reduce_chain'])
        check_sum(f'chain, inner {i}: db', conv.bias.grad, db_ref, dense.bgrad(g)[1], info['bias_chain'])
        if i == 2:  # its input is feats['2'], an input of the decoder that nothing else differentiates
            r, S, d = cb.conv_with_noise(g, dense.unpack(dense.pack_dgrad(wq), c1, 1), None, 1, 0, n=cb.chain_length(1, 1, c1))
            torch.testing.assert_close(r, d_last, rtol=1e-12, atol=1e-12)
            cb.check('chain, inner 2: d_last', feats['2'].grad.cpu(), *cb.bf16_bounds(r, d), r, S)
    # (c) the whole decoder against stock
    tol = 16 * 2. ** -8
    for key in ('out', '0', '1', '2'):
        err = float((out[key].detach().float() - ref[key].detach()).abs().max()) / float(ref[key].detach().abs().max())
        print(f'decoder output {key}: largest error {err:.4f} of the largest magnitude (bound {tol:.4f})')
        assert err <= tol, key
    assert all(out[f'encoder.{k}'] is feats[k] for k in feats)
    params, params_ref = dict(dec.named_parameters()), dict(stock.named_parameters())
    assert params.keys() == params_ref.keys()
    for name, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and p.grad.shape == params_ref[name].grad.shape, name
    for k in feats:
        assert feats[k].grad is not None and bool(torch.isfinite(feats[k].grad).all()) and bool((feats[k].grad != 0).any()), k


