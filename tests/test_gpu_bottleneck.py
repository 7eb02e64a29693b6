"""GPU tests of the trainable bottleneck block (``cda.nn.batch_norm(..., residual=)``, ``strided_conv1x1``, ``subsample2d``,
``conv2d_fork``, ``Bottleneck``; csrc/batch_norm.hip, csrc/grouped_conv_train.hip) against the fp64 statements and the judges of
tests/bottleneck_oracle.py (its docstring states the tail's bound; tests/test_bottleneck.py shows on the CPU that the judge accepts the
stated arithmetic and rejects a tail that rounds t to bf16 before the add).  The convs are judged by the rule of tests/conv_bounds.py,
the weight gradient by the chain bound of tests/test_gpu_conv_train.py, the norm's gradients by the bounds of
tests/batch_norm_oracle.py.  No allowance counts, no fraction of bad elements.
"""
import functools
import itertools
import math

import pytest
import torch

import celldetection_amd as cda
import bottleneck_oracle as oracle
import conv_bounds as cb
import conv_train_oracle
from bottleneck_oracle import same_bits
from test_bottleneck import Block
from test_gpu_conv_train import bf16_exact, check_sum

pytestmark = pytest.mark.gpu
nn = cda.nn
CL = torch.channels_last
EPS = 1e-5


def _id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def dev(t):
    if t is None:
        return None
    return t.cuda().contiguous(memory_format=CL) if t.dim() == 4 else t.cuda()


# ---- the norm's residual tail

# (N, C, H, W): M = 2; one vector; V = 3 (a partial row of lanes); V = 33 (7 pixels per step, M no multiple of it); two channel blocks
# (C = 2056); many steps and slabs
TAIL_SHAPES = [(2, 8, 1, 1), (1, 8, 1, 2), (2, 24, 5, 7), (2, 264, 3, 5), (1, 2056, 1, 3), (2, 8, 33, 70)]


@functools.lru_cache(maxsize=None)
def tail_operands(shape, dtype):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(7 * h + 13 * w + c)
    spread = 1 + torch.arange(c, dtype=torch.float32).reshape(1, c, 1, 1) % 7 / 4
    x = (torch.randn(n, c, h, w, generator=g) * spread + torch.randn(1, c, 1, 1, generator=g)).to(dtype)
    r = (torch.randn(n, c, h, w, generator=g) * 1.5).to(dtype)
    dy = torch.randn(n, c, h, w, generator=g).to(dtype)
    wt, b = torch.randn(c, generator=g), torch.randn(c, generator=g)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + .5
    return x, r, dy, wt, b, rm, rv


def chain_of(m, c, slab_pixels):
    info = nn.batch_norm_info(m, c, slab_pixels)
    assert info['chain'] <= m + info['slabs'] + 8, info
    return info['chain']


def run_tail(name, x, r, dy, wt, b, rm, rv, training, relu, slab_pixels=0):
    """forward primitive + autograd function on the same operands, everything judged -> dict of what the GPU returned (on the CPU)."""
    c = x.shape[1]
    m = x.numel() // c
    chain = chain_of(m, c, slab_pixels)
    act = 'relu' if relu else None
    y, mean, invstd, scale, shift = nn.batch_norm_forward(dev(x), dev(rm), dev(rv), dev(wt), dev(b), training, 0.1, EPS, act,
                                                          slab_pixels, residual=dev(r))
    assert y.dtype == x.dtype and y.shape == x.shape and y.is_contiguous(memory_format=CL)
    plain = nn.batch_norm_forward(dev(x), dev(rm), dev(rv), dev(wt), dev(b), training, 0.1, EPS, act, slab_pixels)
    assert all(same_bits(p, q) for p, q in zip(plain[1:], (mean, invstd, scale, shift)))  # the statistics pass is unchanged
    got = dict(y=y.cpu(), save_mean=mean.cpu(), save_invstd=invstd.cpu(), scale=scale.cpu(), shift=shift.cpu())
    oracle.judge_tail_y(name, x, r, got['y'], got['scale'], got['shift'], relu)
    xg, rg, wg, bg = (dev(t).requires_grad_(True) for t in (x, r, wt, b))
    y2 = nn.batch_norm(xg, dev(rm), dev(rv), wg, bg, training, 0.1, EPS, act, slab_pixels, residual=rg)
    assert same_bits(y2.detach().cpu(), got['y'])
    y2.backward(dev(dy))
    assert xg.grad.dtype == rg.grad.dtype == x.dtype and xg.grad.shape == rg.grad.shape == x.shape
    got.update(dx=xg.grad.cpu(), dr=rg.grad.cpu(), dgamma=wg.grad.cpu(), dbeta=bg.grad.cpu())
    oracle.judge_tail_grads(name, x, dy, got['y'], got, chain, wt, got['save_mean'], got['save_invstd'], relu, training)
    return got


@pytest.mark.parametrize('slab_pixels', [0, 1, 3])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('shape', TAIL_SHAPES, ids=_id)
def test_tail_forward_and_gradients_within_the_bounds(shape, dtype, slab_pixels):
    x, r, dy, wt, b, rm, rv = tail_operands(shape, dtype)
    for training, relu in ((True, True), (False, True), (True, False), (False, False)):
        if training and x.numel() // x.shape[1] < 2:
            continue
        run_tail(f'{shape} slab_pixels {slab_pixels} training {training} relu {relu}', x, r, dy, wt, b, rm, rv, training, relu, slab_pixels)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_sum_exactly_zero_gives_output_and_gradients_exactly_zero(dtype):
    """Eval mode with the coefficients of the batch norm's own designed case: t1 = 2 x - 2 is 0 and +- 2^-6 at x = 1 and 1 +- 2^-7;
    r takes 0 and +- 2^-6 against each of them, so t1 + r is exactly 0, +- 2^-6 and +- 2^-5.  Output and both gradients are exactly
    0 at and below zero; dy passes (times 2 into dx, as it is into dr) right next to it."""
    n, c, eps = 2, 16, 2.0 ** -4
    idx = torch.arange(n * c * 3 * 6)
    x = torch.tensor([1., 1. + 2. ** -7, 1. - 2. ** -7])[idx % 3].reshape(n, c, 3, 6).to(dtype)
    r = torch.tensor([0., 2. ** -6, -2. ** -6])[idx // 3 % 3].reshape(n, c, 3, 6).to(dtype)
    dy = (idx.float().reshape(n, c, 3, 6) % 5 + 1).to(dtype)
    s = 2 * x.float() - 2 + r.float()
    assert sorted(set(s.reshape(-1).tolist())) == [-2. ** -5, -2. ** -6, 0., 2. ** -6, 2. ** -5]
    rm, rv, wt, b = torch.zeros(c), torch.full((c,), .25 - eps), torch.ones(c), torch.full((c,), -2.)
    xg, rg = dev(x).requires_grad_(True), dev(r).requires_grad_(True)
    y = nn.batch_norm(xg, dev(rm), dev(rv), dev(wt), dev(b), False, 0.1, eps, 'relu', residual=rg)
    y.backward(dev(dy))
    zero = torch.zeros_like(s)
    assert torch.equal(y.detach().cpu().float(), torch.where(s > 0, s, zero))
    assert torch.equal(rg.grad.cpu().float(), torch.where(s > 0, dy.float(), zero))
    assert torch.equal(xg.grad.cpu().float(), torch.where(s > 0, 2 * dy.float(), zero))
    assert int((s == 0).sum()) >= 32 and bool((xg.grad.cpu().float()[s == 0] == 0).all())


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_tail_operand_forms(dtype):
    """residual is x itself; an fp32 / NCHW residual beside a bf16 channels-last x; views off a 16-byte boundary; grad_output
    halved or NCHW; two runs; residual=None."""
    shape = (2, 24, 5, 7)
    x, r, dy, wt, b, rm, rv = tail_operands(shape, dtype)

    def step(xt, rt, dyt, needs=(True, True, True, True), training=True):
        xg, rg = xt.detach().clone(memory_format=torch.preserve_format).requires_grad_(needs[0]), None
        if rt is not None:
            rg = rt.detach().clone(memory_format=torch.preserve_format).requires_grad_(needs[1])
        wg, bg = dev(wt).requires_grad_(needs[2]), dev(b).requires_grad_(needs[3])
        bufs = dev(rm), dev(rv)
        kw = {} if rt is None else dict(residual=rg)
        y = nn.batch_norm(xg, *bufs, wg, bg, training, 0.1, EPS, 'relu', **kw)
        if y.requires_grad:
            y.backward(dyt)
        return (y.detach(), xg.grad, None if rg is None else rg.grad, wg.grad, bg.grad) + bufs

    full = step(dev(x), dev(r), dev(dy))
    again = step(dev(x), dev(r), dev(dy))  # two runs: bit-identical, the updated running buffers included
    assert not torch.equal(full[5].cpu(), rm) and all(same_bits(p, q) for p, q in zip(again, full))
    # every needs_input_grad subset of (x, residual, weight, bias), training and eval
    for training in (True, False):
        base = step(dev(x), dev(r), dev(dy), training=training)
        for needs in itertools.product((True, False), repeat=4):
            got = step(dev(x), dev(r), dev(dy), needs, training)
            assert same_bits(got[0], base[0]) and same_bits(got[5], base[5]) and same_bits(got[6], base[6])
            for need, g, f in zip(needs, got[1:5], base[1:5]):
                assert (g is None) == (not need) and (g is None or same_bits(g, f)), (needs, training)
    # the residual in fp32 and / or NCHW beside x: brought to x's dtype and channels-last; its gradient comes in ITS dtype
    other = torch.float32 if dtype == torch.bfloat16 else torch.bfloat16
    r_other = r.to(other)  # (bf16 -> fp32 is exact; fp32 -> bf16 rounds: compare with the rounded residual then)
    want = step(dev(x), dev(r_other.to(dtype)), dev(dy))
    got = step(dev(x), r_other.cuda().contiguous(), dev(dy))
    assert got[2].dtype == other and same_bits(got[2].to(dtype), want[2].to(other).to(dtype))
    assert all(same_bits(p, q) for p, q in zip(got[:2] + got[3:], want[:2] + want[3:]))
    # views that start off a 16-byte boundary

    def off(t):
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
        view = flat[1:].view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2)
        view.copy_(t.cuda())
        assert view.data_ptr() % 16 != 0 and view.is_contiguous(memory_format=CL)
        return view

    xg, rg = off(x).requires_grad_(True), off(r).requires_grad_(True)
    wg, bg = dev(wt).requires_grad_(True), dev(b).requires_grad_(True)
    y = nn.batch_norm(xg, dev(rm), dev(rv), wg, bg, True, 0.1, EPS, 'relu', residual=rg)
    y.backward(off(dy))
    assert all(same_bits(p, q) for p, q in zip((y.detach(), xg.grad, rg.grad, wg.grad, bg.grad), full))
    # grad_output NCHW-contiguous, and halved: every sum, coefficient and fma halves exactly
    nchw = dy.cuda().contiguous()
    assert not nchw.is_contiguous(memory_format=CL)
    assert all(same_bits(p, q) for p, q in zip(step(dev(x), dev(r), nchw), full))
    half = step(dev(x), dev(r), dev((dy.float() * .5).to(dtype)))
    assert all(same_bits(p, (q.float() * .5).to(q.dtype)) for p, q in zip(half[1:5], full[1:5])) and same_bits(half[0], full[0])
    # residual is the same tensor as x: autograd adds the two gradients of it
    xg = dev(x).requires_grad_(True)
    y = nn.batch_norm(xg, dev(rm), dev(rv), dev(wt), dev(b), True, 0.1, EPS, 'relu', residual=xg)
    y.backward(dev(dy))
    apart = step(dev(x), dev(x), dev(dy))
    assert same_bits(y.detach(), apart[0]) and same_bits(xg.grad, apart[1] + apart[2])
    _, _, _, scale, shift = nn.batch_norm_forward(dev(x), dev(rm), dev(rv), dev(wt), dev(b), True, 0.1, EPS, 'relu', residual=dev(x))
    oracle.judge_tail_y('residual is x', x, x, y.detach().cpu(), scale.cpu(), shift.cpu(), True)
    # residual=None: the call without the argument, bit for bit
    none = step(dev(x), None, dev(dy))
    xg, wg, bg = dev(x).requires_grad_(True), dev(wt).requires_grad_(True), dev(b).requires_grad_(True)
    bufs = dev(rm), dev(rv)
    y = nn.batch_norm(xg, *bufs, wg, bg, True, 0.1, EPS, 'relu', 0, None)
    y.backward(dev(dy))
    assert all(same_bits(p, q) for p, q in zip((y.detach(), xg.grad, wg.grad, bg.grad) + bufs, none[:2] + none[3:]))
    mod = nn.BatchNorm2d(shape[1]).cuda()
    with torch.no_grad():
        assert same_bits(mod(dev(x), None), mod(dev(x))) and same_bits(mod(dev(x), None, None), mod(dev(x)))
        mod.eval()
        assert same_bits(mod(dev(x), dev(r), 'relu'), nn.batch_norm(dev(x), mod.running_mean, mod.running_var, mod.weight, mod.bias,
                                                                     False, 0.1, mod.eps, 'relu', residual=dev(r)))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_tail_saves_x_its_output_and_per_channel_vectors_not_the_residual(dtype):
    x, r, dy, wt, b, rm, rv = tail_operands((2, 24, 5, 7), dtype)
    saved = []
    xg, rg, wg, bg = (dev(t).requires_grad_(True) for t in (x, r, wt, b))
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = nn.batch_norm(xg, dev(rm), dev(rv), wg, bg, True, 0.1, EPS, 'relu', residual=rg)
    big = [t for t in saved if t.numel() == x.numel()]
    small = [t for t in saved if t.numel() != x.numel()]
    assert len(big) == 2 and big[0].data_ptr() == xg.data_ptr() and big[1].data_ptr() == y.data_ptr()  # y's storage is the output's
    assert all(t.data_ptr() != rg.data_ptr() for t in saved)
    c = x.shape[1]
    assert len(small) == 5 and all(tuple(t.shape) == (c,) for t in small)  # gamma and four fp32 vectors
    assert sum(t.dtype == torch.float32 and not t.requires_grad for t in small) == 4
    y.backward(dev(dy))
    y = nn.batch_norm(xg, dev(rm), dev(rv), wg, bg, True, 0.1, EPS, 'relu', residual=rg)  # (without hooks: autograd's own saving)
    y.relu_()  # an in-place operation on the saved output: autograd refuses the backward
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        y.backward(dev(dy))


# ---- the subsample

@pytest.mark.parametrize('size', [(1, 1), (1, 2), (2, 1), (5, 7), (6, 9), (8, 8), (33, 2)], ids=_id)
def test_subsample_is_x_on_the_even_grid_bit_for_bit(size):
    h, w = size
    ho, wo = oracle.out_size(h), oracle.out_size(w)
    lib = cda._lib.load()
    for n, c in ((2, 8), (3, 32), (2, 264)):
        x = bf16_exact(n, c, h, w, seed=h + w + c)
        got = nn.subsample2d(x.cuda())
        assert got.dtype == torch.bfloat16 and got.shape == (n, c, ho, wo) and got.is_contiguous(memory_format=CL)
        assert torch.equal(got.float().cpu(), oracle.sub(x))
        # straight into a guarded buffer: one whole row of pixels of sentinels before and after the output stays untouched
        out, buf, guard = cb.guarded_nhwc_bf16(n, ho, wo, c, 'cuda')
        assert out.data_ptr() % 16 == 0
        xs = x.cuda().to(torch.bfloat16).contiguous(memory_format=CL)
        cda._lib.check(lib.cpn_subsample2d(cda._lib.ptr(xs), n, h, w, c, 2, cda._lib.ptr(out), cda._lib.stream_ptr()), 'subsample2d')
        torch.cuda.synchronize()
        cb.assert_guards(f'subsample {size} {c}', buf, guard, cb.BF16_GUARD)
        assert torch.equal(out.float().cpu().permute(0, 3, 1, 2), oracle.sub(x))


# ---- the strided 1x1 conv

STRIDED = [(cin, cout, h, w) for cin, cout in ((32, 64), (96, 32), (64, 288)) for h, w in ((9, 11), (6, 8), (1, 1), (1, 2))]
N = 2


@functools.lru_cache(maxsize=None)
def strided_operands(cin, cout, h, w):
    seed = 7 * h + 13 * w + cin + 3 * cout
    ho, wo = oracle.out_size(h), oracle.out_size(w)
    x, dy = bf16_exact(N, cin, h, w, seed=seed), bf16_exact(N, cout, ho, wo, seed=seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    wt = torch.randn(cout, cin, 1, 1, generator=g) / math.sqrt(cin)
    b = torch.randn(cout, generator=g)
    wq = wt.to(torch.bfloat16).double()
    fwd = cb.conv_with_noise(x, wq, b.double(), 2, 0, n=cb.chain_length(1, 1, cin))
    wd = conv_train_oracle.unpack(conv_train_oracle.pack_dgrad(wq), cout, 1)  # the weights the dgrad conv reads
    bwd = cb.conv_with_noise(dy, wd, None, 1, 0, n=cb.chain_length(1, 1, cout))  # at the small size
    return dict(x=x, dy=dy, w=wt, b=b, fwd=fwd, bwd=bwd, wgrad=conv_train_oracle.wgrad(oracle.sub(x), dy, 1), bgrad=conv_train_oracle.bgrad(dy))


def strided_chain(cin, cout, h, w, slab_rows):
    ho, wo = oracle.out_size(h), oracle.out_size(w)
    info = nn.weight_grad_info(N, ho, wo, cin, cout, 1, slab_rows)
    chain = info['steps'] + 2 + info['reduce_chain']
    assert chain <= -(-N * ho * wo // 16) + 2 + info['slabs'], info
    return info, chain


@pytest.mark.parametrize('case', STRIDED, ids=_id)
def test_strided_conv_forward_and_gradients_within_the_bounds(case):
    cin, cout, h, w = case
    o = strided_operands(*case)
    x = o['x'].cuda().requires_grad_(True)
    wt, b = o['w'].cuda().requires_grad_(True), o['b'].cuda().requires_grad_(True)
    y = nn.strided_conv1x1(x, wt, b)
    ref, S, d = o['fwd']
    assert y.dtype == torch.bfloat16 and y.shape == ref.shape and y.is_contiguous(memory_format=CL)
    assert same_bits(y.detach(), nn.strided_conv1x1(x.detach().contiguous(memory_format=CL), wt.detach(), b.detach()))
    cb.check(f'forward {case}', y.detach().float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
    y.backward(o['dy'].cuda())
    dx = x.grad.cpu()
    assert dx.dtype == torch.float32 and dx.shape == x.shape
    ref, S, d = o['bwd']
    cb.check(f'dgrad {case}', dx[..., ::2, ::2], *cb.bf16_bounds(ref, d), ref, S)
    off_grid = dx.clone()
    off_grid[..., ::2, ::2] = 0
    assert bool((off_grid == 0).all())  # exact zeros off the even grid
    info, chain = strided_chain(*case, 0)
    assert wt.grad.dtype == b.grad.dtype == torch.float32 and wt.grad.shape == (cout, cin, 1, 1)
    check_sum(f'dW {case} autograd', wt.grad, *o['wgrad'], chain)
    check_sum(f'db {case} autograd', b.grad, *o['bgrad'], info['bias_chain'])
    for slab_rows in (1, 3):  # the same two steps the backward takes, with the reduction's partition forced
        info, chain = strided_chain(*case, slab_rows)
        dw, db = nn.conv2d_weight_grad(nn.subsample2d(o['x'].cuda()), o['dy'].cuda(), 1, slab_rows)
        check_sum(f'dW {case} slab_rows {slab_rows}', dw, *o['wgrad'], chain)
        check_sum(f'db {case} slab_rows {slab_rows}', db, *o['bgrad'], info['bias_chain'])


def test_strided_conv_gradient_subsets_and_one_hot_operands():
    cin, cout, h, w = 64, 96, 5, 6
    o_x, o_dy = bf16_exact(N, cin, h, w, seed=1), bf16_exact(N, cout, 3, 3, seed=2)
    wt = bf16_exact(cout, cin, 1, 1, seed=3, scale=.1)
    b = bf16_exact(cout, seed=4)

    def run(need):
        x, wg, bg = (t.cuda().requires_grad_(n) for t, n in zip((o_x, wt, b), need))
        y = nn.strided_conv1x1(x, wg, bg)
        if any(need):
            y.backward(o_dy.cuda())
        return y.detach(), x.grad, wg.grad, bg.grad

    base = run((True, True, True))
    for need in itertools.product((True, False), repeat=3):
        got = run(need)
        assert same_bits(got[0], base[0])
        for n_, g, f in zip(need, got[1:], base[1:]):
            assert (g is None) == (not n_) and (g is None or same_bits(g, f)), need
    # one-hot: x at one pixel and channel, dy at one output pixel and channel, w one-hot
    for (y0, x0), hit in (((2, 4), True), ((4, 0), True), ((1, 2), False), ((2, 3), False)):  # on and off the even grid
        x = torch.zeros(N, cin, h, w)
        x[1, 5, y0, x0] = 1.
        dy = torch.zeros(N, cout, 3, 3)
        dy[1, 7, y0 // 2, x0 // 2] = 1.
        w1 = torch.zeros(cout, cin, 1, 1)
        w1[7, 5] = 1.
        xg, wg = x.cuda().requires_grad_(True), w1.cuda().requires_grad_(True)
        y = nn.strided_conv1x1(xg, wg)
        want = torch.zeros(N, cout, 3, 3)
        if hit:
            want[1, 7, y0 // 2, x0 // 2] = 1.
        assert torch.equal(y.detach().float().cpu(), want)
        y.backward(dy.cuda())
        want_dw = torch.zeros(cout, cin, 1, 1)
        want_dw[7, 5] = 1. if hit else 0.
        assert torch.equal(wg.grad.cpu(), want_dw)
        want_dx = torch.zeros(N, cin, h, w)
        want_dx[1, 5, y0 // 2 * 2, x0 // 2 * 2] = 1.
        assert torch.equal(xg.grad.cpu(), want_dx)


def test_strided_module_is_a_drop_in_for_torch_conv2d():
    torch.manual_seed(0)
    stock = torch.nn.Conv2d(64, 128, 1, 2, bias=False).cuda()
    mine = nn.StridedConv1x1(64, 128, bias=False).cuda()
    assert list(mine.state_dict()) == list(stock.state_dict())
    mine.load_state_dict(stock.state_dict())
    x = bf16_exact(2, 64, 9, 11, seed=4)
    y = mine(x.cuda())
    ref, S, d = cb.conv_with_noise(x, stock.weight.detach().cpu().to(torch.bfloat16).double(), None, 2, 0, n=cb.chain_length(1, 1, 64))
    cb.check('module', y.detach().float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
    y.float().sum().backward()
    assert mine.weight.grad is not None and mine.weight.grad.dtype == torch.float32 and bool(mine.weight.grad.abs().sum() > 0)
    stock.load_state_dict(mine.state_dict())  # ... and back


# ---- the fork

@pytest.mark.parametrize('case', [(5, 7, 32, 64, 1), (9, 11, 96, 32, 1), (5, 7, 64, 64, 3)], ids=_id)
def test_fork_adds_the_skip_gradient_in_the_dgrad_epilogue(case):
    h, w, cin, cout, k = case
    x, dy, dskip = bf16_exact(N, cin, h, w, seed=1), bf16_exact(N, cout, h, w, seed=2), bf16_exact(N, cin, h, w, seed=3)
    g = torch.Generator().manual_seed(5)
    wt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g)

    def plain(xt):
        xg, wg, bg = xt.clone().requires_grad_(True), wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        y = nn.conv2d(xg, wg, bg)
        y.backward(dy.cuda())
        return y.detach(), xg.grad, wg.grad, bg.grad

    def fork(xt, with_skip):
        xg, wg, bg = xt.clone().requires_grad_(True), wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        y, skip = nn.conv2d_fork(xg, wg, bg)
        assert skip.data_ptr() == xg.data_ptr() and skip.grad_fn is not None and type(skip.grad_fn) is type(y.grad_fn) and skip.shape == xg.shape
        if with_skip:
            torch.autograd.backward([y, skip], [dy.cuda(), dskip.cuda().to(skip.dtype)])
        else:
            y.backward(dy.cuda())
        return y.detach(), xg.grad, wg.grad, bg.grad

    for xt in (x.cuda().to(torch.bfloat16).contiguous(memory_format=CL), x.cuda()):  # bf16 channels-last, and an fp32 NCHW x
        base = plain(xt)
        assert all(same_bits(p, q) for p, q in zip(fork(xt, False), base))  # no skip gradient: conv2d's backward, bit for bit
        got = fork(xt, True)
        assert same_bits(got[0], base[0]) and same_bits(got[2], base[2]) and same_bits(got[3], base[3]) and got[1].dtype == xt.dtype
        wq = wt.to(torch.bfloat16).double()
        wd = conv_train_oracle.unpack(conv_train_oracle.pack_dgrad(wq), cout, k)
        ref, S, d = cb.conv_with_noise(dy, wd, None, 1, k // 2, n=cb.chain_length(k, k, cout), res=dskip)
        cb.check(f'fork dx {case}', got[1].float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
    # only the skip is used: its gradient passes through
    xg = x.cuda().requires_grad_(True)
    _, skip = nn.conv2d_fork(xg, wt.cuda(), None)
    skip.backward(dskip.cuda())
    assert torch.equal(xg.grad.cpu(), dskip)
    mod = nn.Conv2d(cin, cout, k).cuda()
    with torch.no_grad():
        xc = x.cuda()
        y, skip = mod(xc, fork=True)
        assert same_bits(y, mod(xc)) and skip.data_ptr() == xc.data_ptr()


# ---- two converted blocks end to end

def _rel(got, ref):
    return float((got.double().cpu() - ref).norm() / ref.norm())


def test_two_converted_blocks_train_end_to_end():
    def make():
        torch.manual_seed(1)
        net = torch.nn.Sequential(Block(64, 128, 32, 2, 256), Block(256, 128, 32, 1, 256, None))
        g = torch.Generator().manual_seed(2)
        with torch.no_grad():
            for name, p in net.named_parameters():
                if p.dim() == 1:
                    p.copy_(torch.randn(p.shape, generator=g) * .3 + (1. if name.endswith('weight') else 0.))
                p.copy_(p.to(torch.bfloat16).float())  # bf16-exact parameters: every path reads the same numbers
        return net

    x = bf16_exact(2, 64, 18, 22, seed=9)
    dy = bf16_exact(2, 256, 9, 11, seed=10)
    # fp64 CPU autograd of the stock modules
    stock = make().double()
    x64 = x.double().requires_grad_(True)
    y64 = stock(x64)
    y64.backward(dy.double())
    ref = dict(y=y64.detach(), x=x64.grad, **{name: p.grad for name, p in stock.named_parameters()})

    def run(net):
        net = net.cuda()
        xg = x.cuda().requires_grad_(True)
        y = net(xg)
        y.backward(dy.cuda())
        return net, dict(y=y.detach(), x=xg.grad, **{name: p.grad for name, p in net.named_parameters()})

    parent = make()  # the four other converts only: the path before this block existed
    nn.convert_conv2d_(parent), nn.convert_batchnorm2d_(parent), nn.convert_readout_tail_(parent), nn.convert_grouped_conv2d_(parent)
    assert type(parent[0]) is Block
    _, got_parent = run(parent)

    net = make()
    assert nn.convert_bottleneck_(net) == (['0', '1'], {})
    seen = {}

    def keep(key, t):
        seen[key] = t.detach()
        if t.requires_grad:
            t.register_hook(lambda g: seen.__setitem__('d' + key, g.detach()))

    def tail_hook(i):
        def fn(module, args, kwargs, output):
            keep(f'{i}.tail.x', args[0]), keep(f'{i}.tail.r', kwargs['residual']), keep(f'{i}.tail.y', output)
        return fn

    def fork_hook(i):
        def fn(module, args, kwargs, output):
            assert kwargs == dict(fork=True)
            keep(f'{i}.fork.x', args[0]), keep(f'{i}.fork.y', output[0]), keep(f'{i}.fork.skip', output[1])
        return fn

    def strided_hook(module, args, output):
        keep('0.down.x', args[0]), keep('0.down.y', output)

    for i in (0, 1):
        net[i].bn3.register_forward_hook(tail_hook(i), with_kwargs=True)
        net[i].conv1.register_forward_hook(fork_hook(i), with_kwargs=True)
    net[0].downsample[0].register_forward_hook(strided_hook)
    net, got = run(net)
    assert got['y'].shape == (2, 256, 9, 11) and bool(torch.isfinite(got['x']).all()) and bool((got['x'] != 0).any())
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), name

    cpu = {k: v.cpu() for k, v in seen.items()}
    for i in (0, 1):
        # the tail, judged on the operands it saw
        bn = net[i].bn3
        tx, tr, ty = cpu[f'{i}.tail.x'], cpu[f'{i}.tail.r'], cpu[f'{i}.tail.y']
        _, mean, invstd, scale, shift = nn.batch_norm_forward(seen[f'{i}.tail.x'], None, None, bn.weight, bn.bias, True, 0., bn.eps)
        oracle.judge_tail_y(f'block {i} tail', tx, tr, ty, scale.cpu(), shift.cpu(), True)
        m = tx.numel() // tx.shape[1]
        grads = dict(dr=cpu[f'd{i}.tail.r'].to(ty.dtype), dx=cpu[f'd{i}.tail.x'], dgamma=bn.weight.grad.cpu(), dbeta=bn.bias.grad.cpu())
        oracle.judge_tail_grads(f'block {i} tail', tx, cpu[f'd{i}.tail.y'], ty, grads, chain_of(m, tx.shape[1], 0), bn.weight.detach().cpu(),
                                mean.cpu(), invstd.cpu(), True, True)
        # the fork: y is conv2d's, skip is x, dx = dgrad(dy) + dskip within the conv's bounds
        conv = net[i].conv1
        assert same_bits(seen[f'{i}.fork.y'], nn.conv2d(seen[f'{i}.fork.x'], conv.weight.detach()))
        assert seen[f'{i}.fork.skip'].data_ptr() == seen[f'{i}.fork.x'].data_ptr()
        wq = conv.weight.detach().cpu().to(torch.bfloat16).double()
        wd = conv_train_oracle.unpack(conv_train_oracle.pack_dgrad(wq), wq.shape[0], 1)
        dskip = cpu[f'd{i}.fork.skip'].to(torch.bfloat16)
        ref_dx, S, d = cb.conv_with_noise(cpu[f'd{i}.fork.y'].float(), wd, None, 1, 0, n=cb.chain_length(1, 1, wq.shape[0]), res=dskip.float())
        dx = got['x'] if i == 0 else seen['d0.tail.y']
        cb.check(f'block {i} fork dx', dx.float().cpu(), *cb.bf16_bounds(ref_dx, d), ref_dx, S)
    # the strided shortcut of block 0
    conv = net[0].downsample[0]
    wq = conv.weight.detach().cpu().to(torch.bfloat16).double()
    ref_y, S, d = cb.conv_with_noise(cpu['0.down.x'].float(), wq, None, 2, 0, n=cb.chain_length(1, 1, 64))
    cb.check('shortcut forward', cpu['0.down.y'].float(), *cb.bf16_bounds(ref_y, d), ref_y, S)
    dw, _ = nn.conv2d_weight_grad(nn.subsample2d(seen['0.down.x']), seen['d0.down.y'], 1, bias=False)
    assert same_bits(conv.weight.grad, dw)
    check_sum('shortcut dW', conv.weight.grad, *conv_train_oracle.wgrad(oracle.sub(cpu['0.down.x'].double()), cpu['d0.down.y'].double(), 1),
              strided_chain(64, 256, 18, 22, 0)[1])
    dskip0 = cpu['d0.fork.skip'].float()
    off_grid = dskip0.clone()
    off_grid[..., ::2, ::2] = 0
    assert bool((off_grid == 0).all()) and bool((dskip0[..., ::2, ::2] != 0).any())

    # eval mode runs
    net.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(net(x.cuda())).all())

    # the whole net against fp64: no more than twice the error of the parent's path on any result.  Both are bf16 chains with the
    # same operand roundings, and the new one rounds once less at the add; a wrong mask or a missing skip term is an error of order 1.
    worst = 0.
    for key in ref:
        e_new, e_parent = _rel(got[key], ref[key]), _rel(got_parent[key], ref[key])
        print(f'{key}: relative L2 error {e_new:.3e} (convert_bottleneck_), {e_parent:.3e} (the four other converts)')
        worst = max(worst, e_new / e_parent)
    print(f'largest ratio {worst:.3f}')
    for key in ref:
        assert _rel(got[key], ref[key]) <= 2 * _rel(got_parent[key], ref[key]), key
