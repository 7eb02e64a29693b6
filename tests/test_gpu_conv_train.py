"""GPU tests of the trainable convolution (``cda.nn``, csrc/conv_train.hip) against the fp64 statements of
tests/conv_train_oracle.py.

Bounds.  The packs are equal bit for bit.  Forward and input gradient are judged by the rule of tests/conv_bounds.py (imported,
unchanged): the fp64 conv of exactly the operands the kernel reads, noise gamma(n) * S for the chain over the channels actually
reduced, and the bf16 values that noise window can round to.  A weight-gradient element lies within gamma(n) * S of the fp64 sum
plus one fp32 rounding of the result, S = sum |dY| |X|, n = MFMA steps per slab + 2 + reduce chain as ``cpn_conv_wgrad_info``
reports them -- and the test holds n <= ceil(N H W / 16) + 2 + slabs, so the library cannot widen its own bound.  The bias gradient
likewise with the chain of its own sum.  No allowance counts, no fraction of bad elements.  One-hot operands are exact.
"""
import functools
import math

import numpy as np
import pytest
import torch

import celldetection_amd as cda
import conv_bounds as cb
import conv_train_oracle as oracle

pytestmark = pytest.mark.gpu
nn = cda.nn
N = 2


def bf16_exact(*shape, seed, scale=1.):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def operands(h, w, cin, cout, k):
    """x, weight (fp32, not bf16-exact: the pack rounds it), bias, dY of one case and every fp64 reference of it, computed once."""
    seed = 7 * h + 13 * w + cin + 3 * cout + k
    x, dy = bf16_exact(N, cin, h, w, seed=seed), bf16_exact(N, cout, h, w, seed=seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    wt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g)
    wq = wt.to(torch.bfloat16).double()
    fwd = cb.conv_with_noise(x, wq, b.double(), 1, k // 2, n=cb.chain_length(k, k, cin))
    wd = oracle.unpack(oracle.pack_dgrad(wq), cout, k)  # the weights the dgrad conv reads
    bwd = cb.conv_with_noise(dy, wd, None, 1, k // 2, n=cb.chain_length(k, k, cout))
    return dict(x=x, dy=dy, w=wt, b=b, fwd=fwd, bwd=bwd, wgrad=oracle.wgrad(x, dy, k), bgrad=oracle.bgrad(dy))


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
    h, w, cin, cout, k = case
    o = operands(*case)
    info = nn.weight_grad_info(N, h, w, cin, cout, k, slab_rows)
    chain = info['steps'] + 2 + info['reduce_chain']
    assert chain <= -(-N * h * w // 16) + 2 + info['slabs'], info
    assert slab_rows == 0 or info['slab_rows'] == min(slab_rows, N * h)
    dw, db = nn.conv2d_weight_grad(o['x'].cuda(), o['dy'].cuda(), k, slab_rows)
    assert dw.dtype == db.dtype == torch.float32 and dw.shape == (cout, cin, k, k) and db.shape == (cout,)
    check_sum(f'dW {case} slab_rows {slab_rows} ({info["slabs"]} slabs)', dw, *o['wgrad'], chain)
    check_sum(f'db {case} slab_rows {slab_rows}', db, *o['bgrad'], info['bias_chain'])
    return info


# ---- pack

@pytest.mark.parametrize('cin,cout,k', [(32, 32, 1), (96, 64, 3), (32, 160, 7)])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_pack_is_bit_equal_to_the_statement(cin, cout, k, dtype):
    """odd item counts (1, 27, 49) and, with the roles swapped, even ones (2 x 9, 5 x 49 is odd again): both ends of the zero item"""
    g = torch.Generator().manual_seed(cin + cout + k)
    w = torch.randn(cout, cin, k, k, generator=g)
    w.view(-1)[:4] = torch.tensor([1. + 2. ** -8, 1. + 3 * 2. ** -8, -(1. + 2. ** -8), 2. ** -140])  # ties to even, a subnormal
    w = w.to(dtype)
    wq = w.to(torch.bfloat16)
    for mode, statement in (('forward', oracle.pack_forward), ('dgrad', oracle.pack_dgrad)):
        got = nn.pack_weight(w.cuda(), mode).cpu()
        want = statement(wq.double()).to(torch.bfloat16)
        assert got.dtype == torch.bfloat16 and got.shape == want.shape, (mode, got.shape, want.shape)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), mode


# ---- forward, input gradient, weight and bias gradient against fp64

# (H, W, Cin, Cout, k): 1 x 1, narrower than a 7 x 7 window (every tap meets padding), odd sizes, more than one chunk of 128 pixels
# per slab and more than one 64-channel tile; k = 5 on one shape
CASES = [(1, 1, 32, 32, 1), (1, 1, 96, 64, 3), (1, 1, 64, 160, 7),
         (5, 7, 32, 32, 3), (5, 7, 96, 64, 7), (5, 7, 64, 160, 1), (5, 7, 32, 32, 5),
         (3, 40, 32, 32, 7), (3, 40, 96, 64, 3), (3, 40, 64, 160, 1),
         (17, 33, 32, 32, 1), (17, 33, 96, 64, 3), (17, 33, 64, 160, 7),
         (33, 70, 32, 32, 7), (33, 70, 96, 64, 1), (33, 70, 64, 160, 3)]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_forward_and_input_gradient_within_the_conv_bounds(case):
    h, w, cin, cout, k = case
    o = operands(*case)
    x = o['x'].cuda().requires_grad_(True)
    wt, b = o['w'].cuda().requires_grad_(True), o['b'].cuda().requires_grad_(True)
    y = nn.conv2d(x, wt, b, padding=k // 2)
    assert y.dtype == torch.bfloat16 and y.shape == (N, cout, h, w) and y.is_contiguous(memory_format=torch.channels_last)
    ref, S, d = o['fwd']
    r = cb.check(f'forward {case}', y.detach().float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
    y.backward(o['dy'].cuda())
    ref, S, d = o['bwd']
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    r2 = cb.check(f'dgrad {case}', x.grad.cpu(), *cb.bf16_bounds(ref, d), ref, S)
    print(f'{case}: forward ratio {r:.3f}, dgrad ratio {r2:.3f}')
    # the parameter gradients of the same call: slab_rows 0
    info = nn.weight_grad_info(N, h, w, cin, cout, k)
    check_sum(f'dW {case} autograd', wt.grad, *o['wgrad'], info['steps'] + 2 + info['reduce_chain'])
    check_sum(f'db {case} autograd', b.grad, *o['bgrad'], info['bias_chain'])


@pytest.mark.parametrize('slab_rows', [1, 3, 0])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_weight_and_bias_gradient_within_the_chain_bound(case, slab_rows):
    info = check_wgrad(case, slab_rows)
    h = case[0]
    if slab_rows == 1:
        assert info['slabs'] == N * h
    if slab_rows == 3 and h in (5, 17, 1):
        assert (N * h) % info['slab_rows'] != 0 or N * h < 3  # a partial last slab


@pytest.mark.parametrize('case', [(5, 7, 96, 64, 7), (17, 33, 96, 64, 3)], ids=lambda c: 'x'.join(map(str, c)))
def test_slab_boundary_between_two_images(case):
    info = check_wgrad(case, case[0])
    assert info['slabs'] == N and info['slab_rows'] == case[0]


def test_bf16_parameters_get_bf16_gradients_rounded_once():
    case = (5, 7, 32, 32, 3)
    o = operands(*case)
    x, dy = o['x'].cuda(), o['dy'].cuda()
    dw32, db32 = nn.conv2d_weight_grad(x, dy, 3)
    dw16, db16 = nn.conv2d_weight_grad(x, dy, 3, dtype=torch.bfloat16)
    assert dw16.dtype == db16.dtype == torch.bfloat16
    assert torch.equal(dw16, dw32.to(torch.bfloat16)) and torch.equal(db16, db32.to(torch.bfloat16))


# ---- tap localisation, exact

@pytest.mark.parametrize('k', [3, 7])
def test_one_hot_operands_hit_exactly_the_predicted_tap(k):
    """X one-hot at one pixel and channel; dY one-hot per output channel, channel co at pixel co of the 5 x 6 image: dW[co] has at
    most one non-zero, a 1 at tap (y0 - y1 + p, x0 - x1 + p) where that is a tap -- for the four corners and a centre pixel."""
    h, w, p, ci0 = 5, 6, k // 2, 17
    for n0, y0, x0 in ((0, 0, 0), (1, 0, w - 1), (0, h - 1, 0), (1, h - 1, w - 1), (1, 2, 3)):
        x = torch.zeros(N, 32, h, w)
        x[n0, ci0, y0, x0] = 1.
        dy = torch.zeros(N, 32, h, w)
        for co in range(h * w):
            dy[n0, co, co // w, co % w] = 1.
            dy[1 - n0, co, co // w, co % w] = 1.  # the other image holds no X: contributes nothing
        want = torch.zeros(32, 32, k, k, dtype=torch.float64)
        for co in range(h * w):
            ky, kx = y0 - co // w + p, x0 - co % w + p
            if 0 <= ky < k and 0 <= kx < k:
                want[co, ci0, ky, kx] = 1.
        assert torch.equal(oracle.wgrad(x, dy, k)[0], want)
        for slab_rows in (0, 1):
            dw, db = nn.conv2d_weight_grad(x.cuda(), dy.cuda(), k, slab_rows)
            assert torch.equal(dw.double().cpu(), want), (k, n0, y0, x0, slab_rows, dw.nonzero().tolist()[:8])
            assert torch.equal(db.cpu(), dy.sum((0, 2, 3)))


@pytest.mark.parametrize('k', [3, 7])
def test_constant_x_gives_the_count_pattern_of_the_padding(k):
    h, w, p = 4, 9, k // 2
    x = torch.ones(N, 64, h, w)
    for y1, x1 in ((0, 0), (h - 1, w - 1), (0, w - 1)):
        dy = torch.zeros(N, 32, h, w)
        dy[1, 5, y1, x1] = 1.
        dw = nn.conv2d_weight_grad(x.cuda(), dy.cuda(), k)[0].cpu()
        ky, kx = np.mgrid[:k, :k]
        inside = (0 <= y1 + ky - p) & (y1 + ky - p < h) & (0 <= x1 + kx - p) & (x1 + kx - p < w)
        want = torch.zeros(32, 64, k, k)
        want[5] = torch.as_tensor(inside, dtype=torch.float32)
        assert torch.equal(dw, want), (k, y1, x1)
    dy = torch.ones(N, 32, h, w)  # ... and with dY constant too: the number of pixels whose tap lies inside the image
    dw = nn.conv2d_weight_grad(x.cuda(), dy.cuda(), k)[0].cpu()
    count = torch.tensor([[N * (h - abs(a - p)) * max(w - abs(c - p), 0) if h > abs(a - p) else 0 for c in range(k)] for a in range(k)])
    assert torch.equal(dw, count.float().expand(32, 64, k, k))


# ---- layout and gradient plumbing

def run_conv2d(x, wt, b, dy, need=(True, True, True)):
    x = x.detach().clone().requires_grad_(need[0])
    wt = wt.detach().clone().requires_grad_(need[1])
    b = None if b is None else b.detach().clone().requires_grad_(need[2])
    y = nn.conv2d(x, wt, b)
    if any(need):
        y.backward(dy)
    return y.detach(), x.grad, wt.grad, None if b is None else b.grad


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_layouts_dtypes_and_requested_gradients():
    case = (17, 33, 96, 64, 3)
    o = operands(*case)
    g = torch.Generator().manual_seed(3)
    x32 = torch.randn(N, 96, 17, 33, generator=g).cuda()  # not bf16-exact
    wt, b, dy = o['w'].cuda(), o['b'].cuda(), o['dy'].cuda().to(torch.bfloat16)
    base = run_conv2d(x32.to(torch.bfloat16).contiguous(memory_format=torch.channels_last), wt, b, dy)
    again = run_conv2d(x32.to(torch.bfloat16).contiguous(memory_format=torch.channels_last), wt, b, dy)
    assert all(same_bits(p, q) for p, q in zip(base, again)), 'two runs differ'
    nchw = run_conv2d(x32.to(torch.bfloat16).contiguous(), wt, b, dy)
    assert all(same_bits(p, q) for p, q in zip(base, nchw)), 'an NCHW-contiguous input differs'
    f32 = run_conv2d(x32, wt, b, dy)
    assert f32[1].dtype == torch.float32 and base[1].dtype == torch.bfloat16
    assert same_bits(base[0], f32[0]) and same_bits(base[1], f32[1].to(torch.bfloat16)) and same_bits(base[2], f32[2]) and \
        same_bits(base[3], f32[3]), 'an fp32 input differs from its bf16 rounding'
    # grad_output non-contiguous (every second column of a wider tensor; a permuted view)
    wide = torch.zeros(N, 64, 17, 66, dtype=torch.bfloat16, device='cuda')
    wide[..., ::2] = dy
    assert not wide[..., ::2].is_contiguous()
    assert all(same_bits(p, q) for p, q in zip(base, run_conv2d(x32.to(torch.bfloat16), wt, b, wide[..., ::2])))
    perm = dy.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).float()  # fp32, channels-last strides
    assert all(same_bits(p, q) for p, q in zip(base, run_conv2d(x32.to(torch.bfloat16), wt, b, perm)))
    # only the requested gradients are returned
    for need in ((False, True, True), (True, False, True), (True, True, False), (False, False, True), (True, False, False),
                 (False, True, False)):
        got = run_conv2d(x32.to(torch.bfloat16), wt, b, dy, need)
        for j in range(3):
            assert (got[1 + j] is not None) == need[j], need
            assert got[1 + j] is None or same_bits(got[1 + j], base[1 + j]), need
    nob = run_conv2d(x32.to(torch.bfloat16), wt, None, dy)
    assert nob[3] is None and same_bits(nob[1], base[1]) and same_bits(nob[2], base[2])
    with torch.no_grad():
        assert same_bits(nn.conv2d(x32, wt, b), base[0])
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.conv2d(x32.cpu(), wt.cpu(), b.cpu())


def test_a_view_that_starts_off_a_16_byte_address_gives_the_bits_of_its_clone():
    """A channels-last bf16 view one element into a buffer: the kernels' 16-byte loads only ever see the aligned clone ``_nhwc``
    makes of it, so output and all three gradients are those of ``view.clone()`` bit for bit."""
    n, c, h, w, k = 1, 32, 4, 5, 3
    g = torch.Generator().manual_seed(5)
    buf = torch.randn(n * h * w * c + 1, generator=g).to(torch.bfloat16).cuda()
    view = buf[1:].view(n, h, w, c).permute(0, 3, 1, 2)
    assert view.is_contiguous(memory_format=torch.channels_last) and view.data_ptr() % 16 == 2
    wt, b = torch.randn(c, c, k, k, generator=g).cuda(), torch.randn(c, generator=g).cuda()
    dy = torch.randn(n, c, h, w, generator=g).to(torch.bfloat16).cuda()

    def run(x):  # (run_conv2d clones x, which would align it)
        x, wp, bp = x.detach().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = nn.conv2d(x, wp, bp)
        y.backward(dy)
        return y.detach(), x.grad, wp.grad, bp.grad

    aligned = view.clone()
    assert aligned.data_ptr() % 16 == 0 and torch.equal(aligned, view)
    got, ref = run(view), run(aligned)
    for name, p, q in zip(('y', 'dx', 'dw', 'db'), got, ref):
        assert same_bits(p, q) and torch.equal(p, q), name


def test_module_is_a_drop_in_for_torch_conv2d():
    torch.manual_seed(0)
    stock = torch.nn.Conv2d(32, 64, 5, padding=2).cuda()
    mine = nn.Conv2d(32, 64, 5).cuda()
    mine.load_state_dict(stock.state_dict())
    x = bf16_exact(N, 32, 9, 11, seed=4).cuda()
    y = mine(x)
    ref = torch.nn.functional.conv2d(x.double(), stock.weight.detach().double(), stock.bias.detach().double(), padding=2)
    assert y.dtype == torch.bfloat16 and float((y.detach().double() - ref).abs().max()) < 2e-2 * float(ref.abs().max())
    y.float().sum().backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 and bool(p.grad.abs().sum() > 0) for p in mine.parameters())


# ---- the chain: label image -> targets -> converted model -> objective -> backward

class _Net(torch.nn.Module):
    def __init__(self, order):
        super().__init__()
        self.trunk = torch.nn.Sequential(torch.nn.Conv2d(32, 32, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(32, 32, 7, padding=3))
        self.heads = torch.nn.ModuleDict(dict(scores=torch.nn.Conv2d(32, 1, 1), locations=torch.nn.Conv2d(32, 2, 1),
                                              refinement=torch.nn.Conv2d(32, 2, 1), fourier=torch.nn.Conv2d(32, 4 * order, 1)))

    def forward(self, x):
        f = self.trunk(x).float()
        return {k: head(f) for k, head in self.heads.items()}


def test_training_chain_from_label_images():
    H, W, order, S = 32, 40, 3, 8
    yy, xx = np.mgrid[:H, :W]
    gens = []
    np.random.seed(5)
    for discs in (((8, 9, 6), (20, 28, 7), (24, 8, 5)), ((10, 12, 7), (21, 27, 8))):
        lab = np.zeros((H, W), np.int32)
        for i, (cy, cx, r) in enumerate(discs):
            lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = i + 1
        gen = cda.CPNTargetGenerator(samples=S, order=order)
        gen.feed(torch.as_tensor(lab[..., None]).cuda())
        gens.append(gen)
    targets = cda.collate_cpn_targets(gens)
    torch.manual_seed(1)
    net = _Net(order).cuda()
    replaced, left = nn.convert_conv2d_(net)
    assert replaced == ['trunk.0', 'trunk.2'] and set(left) == {f'heads.{k}' for k in net.heads}
    assert all('out_channels' in why for why in left.values())
    seen = {}
    conv7 = net.trunk[2]

    def hook(module, args, output):
        seen['x'] = args[0].detach()
        output.register_hook(lambda g: seen.__setitem__('dy', g.detach()))

    conv7.register_forward_hook(hook)
    image = bf16_exact(N, 32, H, W, seed=9).cuda()
    maps = net(image)
    objective = cda.CPNObjective(order, S, refinement_iterations=2)
    loss, losses = objective(maps['scores'], maps['locations'], maps['refinement'], maps['fourier'], targets, size=(H, W))
    loss.backward()
    assert bool(torch.isfinite(loss))
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), name
    assert seen['x'].dtype == seen['dy'].dtype == torch.bfloat16
    dw, db = nn.conv2d_weight_grad(seen['x'], seen['dy'], 7)
    assert same_bits(conv7.weight.grad, dw) and same_bits(conv7.bias.grad, db)
