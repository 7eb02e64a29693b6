"""GPU tests of the trainable grouped 3x3 convolution (the grouped part of ``cda.nn``, csrc/grouped_conv_train.hip) against the fp64
statements of tests/grouped_conv_oracle.py.

Bounds.  The packs and the dilation are equal bit for bit.  Forward and input gradient are judged by the rule of
tests/conv_bounds.py (imported, unchanged): the fp64 conv of exactly the operands the kernel reads, noise gamma(n) * S for the chain
over the bw channels of a bundle, and the bf16 values that noise window can round to.  A weight-gradient element lies within
gamma(n) * S of the fp64 sum plus one fp32 rounding of the result (``check_sum`` of tests/test_gpu_conv_train.py, imported), S = sum
|dZ| |X|, n = MFMA steps per slab + 2 + reduce chain as ``cpn_grouped_conv_wgrad_info`` reports them -- and the test holds
n <= ceil(N H W / 16) + 2 + slabs, so the library cannot widen its own bound.  The bias gradient likewise with the chain of its own
sum.  No allowance counts, no fraction of bad elements.  One-hot operands are exact.
"""
import functools
import math

import pytest
import torch

import celldetection_amd as cda
import conv_bounds as cb
import grouped_conv_oracle as oracle
from test_gpu_cat_conv import same_partition
from test_gpu_conv_train import bf16_exact, check_sum, same_bits
from test_grouped_conv import GPU_SHAPES, Bottleneck

pytestmark = pytest.mark.gpu
nn = cda.nn
SHAPES = GPU_SHAPES  # (N, H, W, C, channels per group)


def _id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def weights(c, cig):
    """weight (fp32, not bf16-exact: the pack rounds it), bias, and the dense weights the dgrad conv reads, computed once."""
    g = torch.Generator().manual_seed(5 * c + cig)
    wt = torch.randn(c, cig, 3, 3, generator=g) / math.sqrt(cig * 9)
    b = torch.randn(c, generator=g)
    wq = wt.to(torch.bfloat16).double()
    bw, bundles = oracle.geometry(c, cig)[:2]
    wd = oracle.unpack(oracle.pack_dgrad(wq)).reshape(c, bw, 3, 3)  # [bundle * bw input channels of the conv, bw, 3, 3]
    return wt, b, wq, wd


@functools.lru_cache(maxsize=None)
def operands(shape, stride):
    """x, dY of one case and every fp64 reference of it, computed once."""
    n, h, w, c, cig = shape
    seed = 7 * h + 13 * w + c + 3 * cig + stride
    ho, wo = oracle.out_size(h, stride), oracle.out_size(w, stride)
    x, dy = bf16_exact(n, c, h, w, seed=seed), bf16_exact(n, c, ho, wo, seed=seed + 1)
    wt, b, wq, wd = weights(c, cig)
    bw, bundles = oracle.geometry(c, cig)[:2]
    chain = cb.chain_length(3, 3, bw)
    fwd = cb.conv_with_noise(x, wq, b.double(), stride, 1, c // cig, n=chain)
    dz = dy.double() if stride == 1 else oracle.dilate(dy.double(), (h, w))
    bwd = cb.conv_with_noise(dz, wd, None, 1, 1, bundles, n=chain)
    return dict(x=x, dy=dy, w=wt, b=b, fwd=fwd, bwd=bwd, wgrad=oracle.wgrad(x, dy, cig, stride), bgrad=oracle.bgrad(dy))


def wgrad_info(shape, stride, slab_rows):
    n, h, w, c, cig = shape
    info = nn.grouped_weight_grad_info(n, h, w, c, c // cig, stride, slab_rows)
    chain = info['steps'] + 2 + info['reduce_chain']
    assert chain <= -(-n * h * w // 16) + 2 + info['slabs'], info
    assert slab_rows == 0 or info['slab_rows'] == min(slab_rows, n * h)
    ho, wo = oracle.out_size(h, stride), oracle.out_size(w, stride)
    assert info['bias_chain'] <= -(-n * ho * wo // 8) + 8 + n * ho, info
    return info, chain


# ---- packs and dilation, bit for bit

@pytest.mark.parametrize('c,cig', [(32, 4), (64, 8), (64, 16), (96, 32), (128, 64), (32, 32), (64, 64)])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_packs_are_bit_equal_to_the_statement(c, cig, dtype):
    """one, two and three bundles; the padding item of EVERY 32-wide bundle; groups = 1 as the one-bundle edge"""
    g = torch.Generator().manual_seed(c + cig)
    w = torch.randn(c, cig, 3, 3, generator=g)
    w.view(-1)[:4] = torch.tensor([1. + 2. ** -8, 1. + 3 * 2. ** -8, -(1. + 2. ** -8), 2. ** -140])  # ties to even, a subnormal
    w = w.to(dtype)
    wq = w.to(torch.bfloat16)
    for mode, statement in (('forward', oracle.pack_forward), ('dgrad', oracle.pack_dgrad)):
        got = nn.grouped_pack_weight(w.cuda(), c // cig, mode).cpu()
        want = statement(wq.double()).to(torch.bfloat16)
        assert got.dtype == torch.bfloat16 and got.shape == want.shape, (mode, got.shape, want.shape)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), mode
        assert int((got.float() != 0).sum()) <= c * cig * 9  # off-group entries and padding items: exact zeros


@pytest.mark.parametrize('size', [(1, 1), (1, 2), (2, 1), (5, 7), (6, 9), (8, 8), (33, 2)], ids=_id)
def test_dilation_is_dy_on_the_even_grid_and_zero_elsewhere(size):
    h, w = size
    for n, c in ((2, 32), (3, 96)):
        dy = bf16_exact(n, c, oracle.out_size(h, 2), oracle.out_size(w, 2), seed=h + w + c)
        dy[dy == 0] = 1.
        dz = nn.grouped_dilate(dy.cuda(), size)
        assert dz.dtype == torch.bfloat16 and dz.shape == (n, c, h, w) and dz.is_contiguous(memory_format=torch.channels_last)
        dz = dz.float().cpu()
        assert torch.equal(dz[:, :, ::2, ::2], dy)
        assert int((dz != 0).sum()) == dy.numel() and torch.equal(dz.double(), oracle.dilate(dy.double(), size))
    with pytest.raises(ValueError, match='stride-2 output'):
        nn.grouped_dilate(torch.zeros(1, 32, 3, 3).cuda(), (4, 5))


# ---- forward, input gradient, weight and bias gradient against fp64

@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_forward_and_gradients_within_the_bounds(shape, stride):
    n, h, w, c, cig = shape
    o = operands(shape, stride)
    x = o['x'].cuda().requires_grad_(True)
    wt, b = o['w'].cuda().requires_grad_(True), o['b'].cuda().requires_grad_(True)
    y = nn.grouped_conv2d(x, wt, b, stride, c // cig)
    ref, S, d = o['fwd']
    assert y.dtype == torch.bfloat16 and y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
    r = cb.check(f'forward {shape} stride {stride}', y.detach().float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
    y.backward(o['dy'].cuda())
    ref, S, d = o['bwd']
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    r2 = cb.check(f'dgrad {shape} stride {stride}', x.grad.cpu(), *cb.bf16_bounds(ref, d), ref, S)
    print(f'{shape} stride {stride}: forward ratio {r:.3f}, dgrad ratio {r2:.3f}')
    info, chain = wgrad_info(shape, stride, 0)  # the parameter gradients of the same call: slab_rows 0
    assert wt.grad.dtype == b.grad.dtype == torch.float32 and wt.grad.shape == (c, cig, 3, 3) and b.grad.shape == (c,)
    check_sum(f'dW {shape} stride {stride} autograd', wt.grad, *o['wgrad'], chain)
    check_sum(f'db {shape} stride {stride} autograd', b.grad, *o['bgrad'], info['bias_chain'])


@pytest.mark.parametrize('slab_rows', [0, 1, 3])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_weight_and_bias_gradient_within_the_chain_bound(shape, stride, slab_rows):
    n, h, w, c, cig = shape
    o = operands(shape, stride)
    info, chain = wgrad_info(shape, stride, slab_rows)
    if slab_rows == 1:
        assert info['slabs'] == n * h
    if slab_rows == 3 and (h, w) in ((5, 7), (17, 33)):
        assert h % 3 and info['slabs'] == -(-n * h // 3)  # a slab crosses from one image into the next; the last one is partial
    dw, db = nn.grouped_conv2d_weight_grad(o['x'].cuda(), o['dy'].cuda(), c // cig, stride, slab_rows)
    assert dw.dtype == db.dtype == torch.float32 and dw.shape == (c, cig, 3, 3) and db.shape == (c,)
    check_sum(f'dW {shape} stride {stride} slab_rows {slab_rows} ({info["slabs"]} slabs)', dw, *o['wgrad'], chain)
    check_sum(f'db {shape} stride {stride} slab_rows {slab_rows}', db, *o['bgrad'], info['bias_chain'])


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('c,cig', [(64, 8), (96, 16), (32, 4)])
def test_off_group_products_never_reach_dw(c, cig, stride):
    """dY lives in one group; X is huge in every OTHER group's channels: the off-group entries of that bundle's fragment hold sums
    of the order of 1e30 in the workspace, and dW stays within the bound of its own small terms (exact zeros outside the group)."""
    n, h, w, g0 = 2, 5, 7, 1
    ho, wo = oracle.out_size(h, stride), oracle.out_size(w, stride)
    mine = slice(g0 * cig, (g0 + 1) * cig)
    x = torch.full((n, c, h, w), 2. ** 100)
    x[:, mine] = bf16_exact(n, cig, h, w, seed=c)
    dy = torch.zeros(n, c, ho, wo)
    dy[:, mine] = bf16_exact(n, cig, ho, wo, seed=c + 1)
    ref, S = oracle.wgrad(x, dy, cig, stride)
    assert float(ref.abs().max()) < 1e3 and bool((ref[(g0 + 1) * cig:] == 0).all()) and bool((ref[:g0 * cig] == 0).all())
    for slab_rows in (0, 3):
        info = nn.grouped_weight_grad_info(n, h, w, c, c // cig, stride, slab_rows)
        dw = nn.grouped_conv2d_weight_grad(x.cuda(), dy.cuda(), c // cig, stride, slab_rows, bias=False)[0]
        check_sum(f'dW {c} / {cig} stride {stride}', dw, ref, S, info['steps'] + 2 + info['reduce_chain'])
        outside = torch.cat((dw[:g0 * cig], dw[(g0 + 1) * cig:])).cpu()
        assert bool((outside == 0).all())


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('c,cig', [(64, 16), (128, 64), (32, 8)])
def test_one_hot_operands_hit_exactly_the_predicted_element(c, cig, stride):
    """X one-hot at one pixel and channel ci0 of group g; dY one-hot per output channel, the channels of a group spread evenly over the
    output pixels: dW[co] has at most one non-zero, and only for co in group g: a 1 at (cl0, y0 - s i + 1, x0 - s j + 1) where that is a tap."""
    n, h, w = 2, 5, 6
    ho, wo = oracle.out_size(h, stride), oracle.out_size(w, stride)
    g, cl0 = c // cig - 1, cig - 3
    ci0 = g * cig + cl0
    hits = 0
    for n0, y0, x0 in ((0, 0, 0), (1, 0, w - 1), (0, h - 1, 0), (1, h - 1, w - 1), (1, 2, 3)):
        x = torch.zeros(n, c, h, w)
        x[n0, ci0, y0, x0] = 1.
        dy = torch.zeros(n, c, ho, wo)
        want = torch.zeros(c, cig, 3, 3, dtype=torch.float64)
        for co in range(c):
            i, j = divmod(co % cig * (ho * wo) // cig, wo)
            dy[:, co, i, j] = 1.  # (the other image holds no X: contributes nothing)
            ky, kx = y0 - stride * i + 1, x0 - stride * j + 1
            if co // cig == g and 0 <= ky < 3 and 0 <= kx < 3:
                want[co, cl0, ky, kx] = 1.
        assert torch.equal(oracle.wgrad(x, dy, cig, stride)[0], want)
        hits += int(want.sum())
        for slab_rows in (0, 1):
            dw, db = nn.grouped_conv2d_weight_grad(x.cuda(), dy.cuda(), c // cig, stride, slab_rows)
            assert torch.equal(dw.double().cpu(), want), (n0, y0, x0, slab_rows, dw.nonzero().tolist()[:8])
            assert torch.equal(db.cpu(), dy.sum((0, 2, 3)))
    assert hits >= 3, hits


@pytest.mark.parametrize('slab_rows', [8, 1])
@pytest.mark.parametrize('c', [32, 64])
def test_grouped_route_at_one_group_is_the_dense_route_bit_for_bit(c, slab_rows):
    """One group of 32 channels is one 32-wide bundle, one of 64 the four fragments of a 64-wide group: the diagonal fragments are then
    the whole (co, ci) matrix, and both routes run the same slab kernel (csrc/wgrad_dense.h) under two tilings.  With the same slabs
    both add the same 16-pixel steps in the same ascending order into one accumulator per element, and the reduce adds the same slabs
    in the same order.  N = 3, 5 x 33: at slab_rows 8 a slab has 264 pixels, which the dense grid cuts into chunks of 128, 128, 8 and the
    grouped one into 64, 64, 64, 64, 8 -- the same partial last step, the second image starting inside a chunk in both; at 1 every slab
    is one partial chunk of 33 pixels.  slab_rows 0 is left out: the two auto partitions ask for different numbers of slabs."""
    n, h, w = 3, 5, 33
    x, dy = bf16_exact(n, c, h, w, seed=800 + c).cuda(), bf16_exact(n, c, h, w, seed=900 + c).cuda()
    info = same_partition(nn.grouped_weight_grad_info(n, h, w, c, 1, 1, slab_rows), nn.weight_grad_info(n, h, w, c, c, 3, slab_rows))
    assert (info['slabs'], info['slab_rows'], info['steps']) == (-(-n * h // slab_rows), slab_rows, -(-slab_rows * w // 16)), info
    assert bool(torch.isfinite(x).all() and torch.isfinite(dy).all())
    dw, db = nn.grouped_conv2d_weight_grad(x, dy, 1, 1, slab_rows)
    dw_dense, db_dense = nn.conv2d_weight_grad(x, dy, 3, slab_rows)
    assert dw.shape == dw_dense.shape == (c, c, 3, 3) and bool((dw != 0).any())
    assert same_bits(dw, dw_dense) and same_bits(db, db_dense), (c, slab_rows, info, (dw != dw_dense).nonzero()[:4].tolist())


# ---- layout and gradient plumbing

def run_grouped(x, wt, b, dy, stride, groups, need=(True, True, True)):
    x = x.detach().clone().requires_grad_(need[0])
    wt = wt.detach().clone().requires_grad_(need[1])
    b = None if b is None else b.detach().clone().requires_grad_(need[2])
    y = nn.grouped_conv2d(x, wt, b, stride, groups)
    if any(need):
        y.backward(dy)
    return y.detach(), x.grad, wt.grad, None if b is None else b.grad


@pytest.mark.parametrize('stride', [1, 2])
def test_layouts_dtypes_and_requested_gradients(stride):
    shape = (2, 17, 33, 160, 32)
    n, h, w, c, cig = shape
    groups = c // cig
    o = operands(shape, stride)
    g = torch.Generator().manual_seed(3)
    x32 = torch.randn(n, c, h, w, generator=g).cuda()  # not bf16-exact
    xb = x32.to(torch.bfloat16)
    wt, b, dy = o['w'].cuda(), o['b'].cuda(), o['dy'].cuda().to(torch.bfloat16)
    ho, wo = dy.shape[2:]
    base = run_grouped(xb.contiguous(memory_format=torch.channels_last), wt, b, dy, stride, groups)
    again = run_grouped(xb.contiguous(memory_format=torch.channels_last), wt, b, dy, stride, groups)
    assert all(same_bits(p, q) for p, q in zip(base, again)), 'two runs differ'
    nchw = run_grouped(xb.contiguous(), wt, b, dy, stride, groups)
    assert all(same_bits(p, q) for p, q in zip(base, nchw)), 'an NCHW-contiguous input differs'
    f32 = run_grouped(x32, wt, b, dy, stride, groups)
    assert f32[1].dtype == torch.float32 and base[1].dtype == torch.bfloat16
    assert same_bits(base[0], f32[0]) and same_bits(base[1], f32[1].to(torch.bfloat16)) and same_bits(base[2], f32[2]) and \
        same_bits(base[3], f32[3]), 'an fp32 input differs from its bf16 rounding'
    # grad_output non-contiguous (every second column of a wider tensor; a permuted fp32 view; a view at an odd offset)
    wide = torch.zeros(n, c, ho, 2 * wo, dtype=torch.bfloat16, device='cuda')
    wide[..., ::2] = dy
    assert not wide[..., ::2].is_contiguous()
    assert all(same_bits(p, q) for p, q in zip(base, run_grouped(xb, wt, b, wide[..., ::2], stride, groups)))
    perm = dy.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).float()
    assert all(same_bits(p, q) for p, q in zip(base, run_grouped(xb, wt, b, perm, stride, groups)))
    flat = torch.zeros(dy.numel() + 1, dtype=torch.bfloat16, device='cuda')
    odd = flat[1:].view(n, ho, wo, c).permute(0, 3, 1, 2)  # channels-last memory that starts 2 bytes off a 16-byte boundary
    odd.copy_(dy)
    assert odd.data_ptr() % 16 and all(same_bits(p, q) for p, q in zip(base, run_grouped(xb, wt, b, odd, stride, groups)))
    # grad_output halved: every gradient halves exactly (a power of two), the output does not move
    half = run_grouped(xb, wt, b, dy * .5, stride, groups)
    assert same_bits(half[0], base[0]) and all(torch.equal(p.float() * 2, q.float()) for p, q in zip(half[1:], base[1:]))
    # only the requested gradients are returned
    for need in ((False, True, True), (True, False, True), (True, True, False), (False, False, True), (True, False, False),
                 (False, True, False)):
        got = run_grouped(xb, wt, b, dy, stride, groups, need)
        for j in range(3):
            assert (got[1 + j] is not None) == need[j], need
            assert got[1 + j] is None or same_bits(got[1 + j], base[1 + j]), need
    nob = run_grouped(xb, wt, None, dy, stride, groups)
    assert nob[3] is None and same_bits(nob[1], base[1]) and same_bits(nob[2], base[2])
    with torch.no_grad():
        assert same_bits(nn.grouped_conv2d(x32, wt, b, stride, groups), base[0])
    # bf16 parameters get bf16 gradients: the fp32 sums rounded once
    p16 = run_grouped(xb, wt.to(torch.bfloat16), b.to(torch.bfloat16), dy, stride, groups)
    q32 = run_grouped(xb, wt.to(torch.bfloat16).float(), b.to(torch.bfloat16).float(), dy, stride, groups)
    assert p16[2].dtype == p16[3].dtype == torch.bfloat16
    assert same_bits(p16[0], q32[0]) and same_bits(p16[1], q32[1]) and same_bits(p16[2], q32[2].to(torch.bfloat16)) and \
        same_bits(p16[3], q32[3].to(torch.bfloat16))
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.grouped_conv2d(x32.cpu(), wt.cpu(), b.cpu(), stride, groups)


@pytest.mark.parametrize('stride', [1, 2])
def test_module_is_a_drop_in_for_torch_conv2d_with_32_groups(stride):
    torch.manual_seed(0)
    stock = torch.nn.Conv2d(128, 128, 3, stride, 1, groups=32).cuda()
    mine = nn.GroupedConv2d(128, 128, stride=stride, groups=32).cuda()
    assert list(mine.state_dict()) == list(stock.state_dict())
    mine.load_state_dict(stock.state_dict())
    x = bf16_exact(2, 128, 9, 11, seed=4)
    y = mine(x.cuda())
    ref, S, d = cb.conv_with_noise(x, stock.weight.detach().cpu().to(torch.bfloat16).double(), stock.bias.detach().cpu().double(), stride, 1,
                                   32, n=cb.chain_length(3, 3, 32))
    cb.check(f'module stride {stride}', y.detach().float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
    y.float().sum().backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 and bool(p.grad.abs().sum() > 0) for p in mine.parameters())
    stock.load_state_dict(mine.state_dict())  # ... and back
    converted = torch.nn.Sequential(stock)
    assert nn.convert_grouped_conv2d_(converted) == (['0'], {}) and converted[0].weight is stock.weight
    assert same_bits(converted(x.cuda()), y.detach())


def test_a_converted_bottleneck_trains_end_to_end():
    torch.manual_seed(1)
    net = torch.nn.Sequential(Bottleneck(64, 128, 32, 2, 256), Bottleneck(256, 128, 32, 1, 256)).cuda()
    assert nn.convert_conv2d_(net)[0] and nn.convert_batchnorm2d_(net)[0]
    assert nn.convert_readout_tail_(net) == ([], {'0.downsample.0': 'stride (2, 2): stride 1 only'})  # the strided shortcut stays stock
    assert nn.convert_grouped_conv2d_(net) == (['0.conv2', '1.conv2'], {})
    seen = {}

    def hook(name):
        def fn(module, args, output):
            seen[name + '.x'] = args[0].detach()
            output.register_hook(lambda g: seen.__setitem__(name + '.dy', g.detach()))
        return fn

    for i in (0, 1):
        net[i].conv2.register_forward_hook(hook(str(i)))
    x = bf16_exact(2, 64, 18, 22, seed=9).cuda().requires_grad_(True)
    y = net(x)
    assert y.shape == (2, 256, 9, 11)
    y.float().square().mean().backward()
    assert bool(torch.isfinite(x.grad).all()) and bool((x.grad != 0).any())
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), name
    for i, stride in ((0, 2), (1, 1)):
        dw, _ = nn.grouped_conv2d_weight_grad(seen[f'{i}.x'], seen[f'{i}.dy'], 32, stride, bias=False)
        assert same_bits(net[i].conv2.weight.grad, dw), i
