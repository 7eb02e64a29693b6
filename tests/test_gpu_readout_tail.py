"""GPU tests of the trainable ReadOut tail (``cda.nn.dropout_conv1x1``, csrc/readout_tail.hip) against the fp64 statements of
tests/readout_tail_oracle.py.

Bounds, derived from the roundings (tests/conv_bounds.py imported unchanged).  The references are the fp64 statements on exactly
the operands the kernels read: x (bf16-exact), the bf16 rounding of the weights and of grad_output, the keep mask, and s as the
fp32 value nearest to 1 / (1 - p).  With u = 2^-24 and gamma(n) = n u / (1 - n u):

* y lies within d = gamma(n) * s * S of the reference, plus the one rounding of fmaf(acc, s, bias) (u * (|ref| + d)); a bf16 output
  is one of the bf16 values that window rounds to.  n = the forward chain of ``cpn_tail_info``, which the test holds <= Cin / 16 + 3.
* dx is one of the bf16 values the window gamma(dx steps + 2) * s * S + u * (|ref| + d) (the multiplication by s) rounds to.
* dW lies within gamma(chain) * s * S + one rounding, chain = MFMA steps per slab + 2 + reduce chain as ``cpn_tail_info`` reports
  them, which the test holds <= ceil(N HW / 16) + 2 + slabs + 1; db likewise with its own chain (<= ceil(N HW / 8) + 8 + slabs).

No allowance counts, no fraction of bad elements.  Exact operands give exact results.
"""
import functools
import math

import numpy as np
import pytest
import torch

import celldetection_amd as cda
import conv_bounds as cb
import readout_tail_oracle as oracle

pytestmark = pytest.mark.gpu
nn = cda.nn
N = 3


def bf16_exact(*shape, seed, scale=1., shift=0.):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(torch.bfloat16).float()


def s32(p):
    """s as the kernels get it: the fp32 value nearest to 1 / (1 - p); 0 for p = 1"""
    return 0. if p >= 1. else float(np.float32(1. / (1. - p)))


@functools.lru_cache(maxsize=None)
def operands(h, w, cin, cout):
    """x (bf16-exact), weight and bias (fp32, not bf16-exact: the kernels round the weight), grad_output (fp32, not bf16-exact)"""
    seed = 7 * h + 13 * w + cin + 3 * cout
    x = bf16_exact(N, cin, h, w, seed=seed, shift=.25)
    g = torch.Generator().manual_seed(seed + 1)
    dy = torch.randn(N, cout, h, w, generator=g) + .125
    wt = torch.randn(cout, cin, 1, 1, generator=g) / math.sqrt(cin)
    b = torch.randn(cout, generator=g)
    return dict(x=x, dy=dy, w=wt, b=b, wq=wt.to(torch.bfloat16).double().reshape(cout, cin), gq=dy.to(torch.bfloat16).double())


MASKS = ('all_kept', 'p0.1', 'p0.5', 'image0_kept_image1_dropped', 'one_channel_kept', 'p1')


@functools.lru_cache(maxsize=None)
def mask(kind, cin):
    """-> (keep bool [N, cin], p)"""
    g = torch.Generator().manual_seed(cin + len(kind))
    if kind == 'all_kept':
        return torch.ones(N, cin, dtype=torch.bool), .25
    if kind in ('p0.1', 'p0.5'):
        p = float(kind[1:])
        return torch.rand(N, cin, generator=g) >= p, p
    if kind == 'image0_kept_image1_dropped':
        keep = torch.rand(N, cin, generator=g) >= .5
        keep[0], keep[1] = True, False
        return keep, .5
    if kind == 'one_channel_kept':
        keep = torch.zeros(N, cin, dtype=torch.bool)
        keep[:, 5] = True
        return keep, .5
    assert kind == 'p1'
    return torch.zeros(N, cin, dtype=torch.bool), 1.


@functools.lru_cache(maxsize=None)
def references(case, kind):
    o = operands(*case)
    keep, p = mask(kind, case[2])
    s, m = s32(p), keep.double()
    return dict(y=oracle.forward(o['x'], o['wq'], o['b'], m, s), dx=oracle.input_grad(o['gq'], o['wq'], m, s),
                dw=oracle.weight_grad(o['x'], o['gq'], m, s), db=oracle.bias_grad(o['gq']))


def check_sum(name, got, ref, S, chain, s=1.):
    """|got - ref| <= gamma(chain) * s * S + one fp32 rounding of the result."""
    d = cb.gamma(chain) * s * S
    tol = d + cb.U * (ref.abs() + d)
    err = (got.double().cpu().reshape(ref.shape) - ref).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f'{name}: chain {chain}, largest error / bound {worst:.3f}')
    assert bool(torch.isfinite(got).all()) and bool((err <= tol).all()), (name, worst)


def check_forward(name, y, case, kind, out_dtype=torch.float32):
    h, w, cin, cout = case
    ref, S = references(case, kind)['y']
    s = s32(mask(kind, cin)[1])
    n = nn.readout_tail_info(N, h * w, cin, cout)['forward_chain']
    assert n <= cin // 16 + 3
    assert y.dtype == out_dtype and tuple(y.shape) == (N, cout, h, w) and y.is_contiguous()
    d = cb.gamma(n) * s * S
    d = d + cb.U * (ref.abs() + d)  # the rounding of the fma
    if out_dtype == torch.float32:
        r = cb.check(name, y.cpu(), ref - d, ref + d, ref, S)
    else:
        r = cb.check(name, y.float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
    print(f'{name}: chain {n}, ratio {r:.3f}')


def check_dx(name, dx, case, kind):
    h, w, cin, cout = case
    ref, S = references(case, kind)['dx']
    keep, p = mask(kind, cin)
    s = s32(p)
    steps = nn.readout_tail_info(N, h * w, cin, cout)['dx_steps']
    assert steps == (2 if cout > 16 else 1)
    assert tuple(dx.shape) == (N, cin, h, w) and dx.is_contiguous(memory_format=torch.channels_last)
    d = cb.gamma(steps + 2) * s * S
    d = d + cb.U * (ref.abs() + d)  # the multiplication by s
    r = cb.check(name, dx.float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
    dropped = (~keep)[:, :, None, None].expand(N, cin, h, w)
    assert bool((dx.float().cpu()[dropped] == 0).all()), f'{name}: dx is not exactly 0 on a dropped channel'
    print(f'{name}: ratio {r:.3f}')


def check_param_grads(name, dw, db, case, kind, slab_pixels=0):
    h, w, cin, cout = case
    refs = references(case, kind)
    keep, p = mask(kind, cin)
    info = nn.readout_tail_info(N, h * w, cin, cout, slab_pixels)
    chain = info['steps'] + 2 + info['reduce_chain']
    assert chain <= -(-N * h * w // 16) + 2 + info['slabs'] + 1, info
    assert info['bias_chain'] <= -(-N * h * w // 8) + 8 + info['slabs'], info
    assert slab_pixels == 0 or info['slab_pixels'] == min(slab_pixels, h * w)
    assert tuple(dw.shape) == (cout, cin, 1, 1) and tuple(db.shape) == (cout,)
    check_sum(f'dW {name} ({info["slabs"]} slabs)', dw, *refs['dw'], chain, s32(p))
    check_sum(f'db {name}', db, *refs['db'], info['bias_chain'])
    gone = ~keep.any(0)
    assert bool((dw.float().cpu().reshape(cout, cin)[:, gone] == 0).all()), f'{name}: dW of a channel dropped in every image is not 0'
    return info


def run(case, kind, out_dtype=torch.float32, x=None, dy=None, need=(True, True, True), bias=True, p=None, keep=None, training=True,
        params=torch.float32):
    """One forward + backward through autograd -> (y, dx, dW, db)"""
    o = operands(*case)
    k, pp = mask(kind, case[2])
    x = o['x'].cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last) if x is None else x
    x = x.detach().requires_grad_(need[0])  # (a new leaf on the same memory: the address under test stays)
    wt = o['w'].cuda().to(params).requires_grad_(need[1])
    b = o['b'].cuda().to(params).requires_grad_(need[2]) if bias else None
    y = nn.dropout_conv1x1(x, wt, b, pp if p is None else p, training, k.cuda() if keep is None else keep, out_dtype)
    if any(need):
        y.backward(o['dy'].cuda() if dy is None else dy)
    return y.detach(), x.grad, wt.grad, None if b is None else b.grad


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def all_same(p, q):
    return all((a is None and b is None) or same_bits(a, b) for a, b in zip(p, q))


# (H, W, Cin, Cout): 1 x 1, 35 and 561 pixels per image (an image boundary inside a 32-pixel span of the flat range), 120, 2310
# (more than one chunk, tile and workgroup); every Cout at every MFMA padding (1, 2, 16 | 17, 20, 32); Cin 32 / 96 (one channel
# tile per wave, idle waves), 256 (two); 512 and 1024: the other two instantiations, whose LDS image exceeds 64 KB
CASES = [(1, 1, 32, 1), (1, 1, 96, 17), (1, 1, 256, 32),
         (5, 7, 32, 2), (5, 7, 96, 20), (5, 7, 256, 16),
         (3, 40, 32, 17), (3, 40, 96, 1), (3, 40, 256, 20),
         (17, 33, 32, 32), (17, 33, 96, 2), (17, 33, 256, 17),
         (33, 70, 32, 20), (33, 70, 96, 16), (33, 70, 256, 1), (33, 70, 256, 32),
         (5, 7, 512, 20), (3, 40, 1024, 17)]


def ids(case):
    return 'x'.join(map(str, case))


@pytest.mark.parametrize('case', CASES, ids=ids)
def test_all_four_results_within_the_derived_bounds(case):
    """every case with a random mask (p = 0.1 and 0.5 in turn) and one of the other four masks in turn"""
    i = CASES.index(case)
    for kind in (MASKS[1 + i % 2], ('all_kept', 'image0_kept_image1_dropped', 'one_channel_kept', 'p1')[i % 4]):
        y, dx, dw, db = run(case, kind)
        check_forward(f'y {case} {kind}', y, case, kind)
        check_dx(f'dx {case} {kind}', dx, case, kind)
        assert dx.dtype == torch.bfloat16 and dw.dtype == db.dtype == torch.float32
        check_param_grads(f'{case} {kind}', dw, db, case, kind)


@pytest.mark.parametrize('kind', MASKS)
@pytest.mark.parametrize('case', [(5, 7, 96, 20), (17, 33, 256, 17)], ids=ids)
def test_every_mask(case, kind):
    y, dx, dw, db = run(case, kind, out_dtype=torch.bfloat16)
    check_forward(f'y bf16 {case} {kind}', y, case, kind, torch.bfloat16)
    check_dx(f'dx {case} {kind}', dx, case, kind)
    check_param_grads(f'{case} {kind}', dw, db, case, kind)
    if kind == 'p1':  # everything dropped: the output is the bias
        assert torch.equal(y.float().cpu(), operands(*case)['b'].to(torch.bfloat16).float().reshape(1, -1, 1, 1).expand(y.shape))
        assert not bool(dx.any()) and not bool(dw.any())


@pytest.mark.parametrize('slab_pixels', [1, 3, 0, 'more than HW'])
@pytest.mark.parametrize('case', CASES[:16], ids=ids)
def test_weight_and_bias_gradient_for_every_slab_size(case, slab_pixels):
    h, w, cin, cout = case
    sp = h * w + 5 if slab_pixels == 'more than HW' else slab_pixels
    o = operands(*case)
    kind = 'p0.5'
    keep, p = mask(kind, cin)
    dx, dw, db = nn.dropout_conv1x1_backward(o['x'].cuda(), o['dy'].cuda(), o['w'].cuda(), keep.cuda(), p, sp, input_grad=False)
    assert dx is None
    info = check_param_grads(f'{case} slab_pixels {sp}', dw, db, case, kind, sp)
    if slab_pixels == 1:
        assert info['slabs'] == N * h * w
    if slab_pixels == 'more than HW':
        assert info['slabs'] == N and info['slab_pixels'] == h * w  # one slab per image: the slabs end where the images end
    if slab_pixels == 3 and (h * w) % 3:
        assert info['slabs_per_image'] * 3 > h * w  # a partial last slab in every image


# ---- exactness

def test_one_hot_operands_give_exact_results():
    """x one-hot per image, grad_output one-hot, weights k / 8, integer bias, s = 2: every product and sum is exact, so the results
    equal the fp64 statements bit for bit -- at the first and last pixel of an image and across the 32-pixel tile edge."""
    h, w, cin, cout = 5, 7, 96, 20
    g = torch.Generator().manual_seed(1)
    wt = (torch.randint(-16, 17, (cout, cin, 1, 1), generator=g) / 8.)
    b = torch.randint(-4, 5, (cout,), generator=g).float()
    keep = torch.rand(N, cin, generator=g) >= .5
    for (n0, c0, q0), (n1, o1, q1) in (((0, 0, 0), (0, 0, 0)), ((1, 95, 34), (1, 19, 34)), ((2, 37, 31), (2, 7, 32)), ((1, 64, 32), (2, 3, 32))):
        keep[n0, c0] = True
        x = torch.zeros(N, cin, h * w)
        x[n0, c0, q0] = 1.
        x[(n0 + 1) % N, (c0 + 1) % cin, q0] = 3.
        dy = torch.zeros(N, cout, h * w)
        dy[n1, o1, q1] = 1.
        dy[n0, (o1 + 1) % cout, q0] = -2.
        x, dy = x.reshape(N, cin, h, w), dy.reshape(N, cout, h, w)
        want = oracle.statements(x, dy, wt.reshape(cout, cin), b, keep.double(), 2.)
        xg = x.cuda().requires_grad_(True)
        wg, bg = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        for sp in (0, 1):
            xg.grad = wg.grad = bg.grad = None
            y = nn.dropout_conv1x1(xg, wg, bg, .5, True, keep.cuda(), slab_pixels=sp)
            y.backward(dy.cuda())
            assert torch.equal(y.detach().double().cpu(), want['y']), (n0, c0, q0)
            assert torch.equal(xg.grad.double().cpu(), want['dx']) and xg.grad.dtype == torch.float32, (n1, o1, q1)
            assert torch.equal(wg.grad.double().cpu().reshape(cout, cin), want['dw']), ((n0, c0, q0), (n1, o1, q1), sp)
            assert torch.equal(bg.grad.double().cpu(), want['db'])


def test_eval_p0_and_all_ones_keep_are_bit_equal():
    case = (17, 33, 96, 2)
    ones = torch.ones(N, 96, dtype=torch.bool, device='cuda')
    base = run(case, 'p0.5', training=False)                      # eval: the mask and p are not looked at
    assert all_same(base, run(case, 'p0.5', p=0., training=True))  # p = 0
    assert all_same(base, run(case, 'p0.5', p=0., keep=ones))
    o = operands(*case)
    direct = nn.dropout_conv1x1_backward(o['x'].cuda(), o['dy'].cuda(), o['w'].cuda(), ones, 0.)
    assert all_same(base[1:], direct) and all_same(direct, nn.dropout_conv1x1_backward(o['x'].cuda(), o['dy'].cuda(), o['w'].cuda()))
    ref, S = oracle.forward(o['x'], o['wq'], o['b'], torch.ones(N, 96).double(), 1.)
    d = cb.gamma(96 // 16 + 2) * S
    cb.check('eval y', base[0].cpu(), ref - d - cb.U * (ref.abs() + d), ref + d + cb.U * (ref.abs() + d), ref, S)


def test_padding_rows_of_cout_17_read_zeros():
    """weight and bias are the first 17 rows of larger buffers whose other rows hold 3e38: a padded MFMA row that read them would
    put inf - inf = NaN or 3e38 into the results; they equal those of the stand-alone parameters bit for bit"""
    case = (17, 33, 256, 17)
    o = operands(*case)
    keep, p = mask('p0.5', 256)
    big_w = torch.full((32, 256, 1, 1), 3e38, device='cuda')
    big_b = torch.full((32,), 3e38, device='cuda')
    big_w[:17], big_b[:17] = o['w'].cuda(), o['b'].cuda()
    x, dy = o['x'].cuda().to(torch.bfloat16), o['dy'].cuda()
    out = []
    for wt, b in ((big_w[:17], big_b[:17]), (o['w'].cuda(), o['b'].cuda())):
        xg = x.clone().requires_grad_(True)
        wt, b = wt.detach().requires_grad_(True), b.detach().requires_grad_(True)
        y = nn.dropout_conv1x1(xg, wt, b, p, True, keep.cuda())
        y.backward(dy)
        out.append((y.detach(), xg.grad, wt.grad, b.grad))
        assert all(bool(torch.isfinite(t).all()) for t in out[-1])
    assert all_same(*out)
    assert bool((big_w[17:] == 3e38).all()) and bool((big_b[17:] == 3e38).all())


# ---- layout and gradient plumbing

def test_layouts_dtypes_and_requested_gradients():
    case = (17, 33, 96, 20)
    o = operands(*case)
    kind = 'p0.5'
    g = torch.Generator().manual_seed(3)
    x32 = (torch.randn(N, 96, 17, 33, generator=g) + .25).cuda()  # not bf16-exact
    x16 = x32.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dy = o['dy'].cuda()
    base = run(case, kind, x=x16)
    assert base[1].dtype == torch.bfloat16 and base[1].is_contiguous(memory_format=torch.channels_last)
    assert all_same(base, run(case, kind, x=x16)), 'two runs differ'
    assert all_same(base, run(case, kind, x=x32.to(torch.bfloat16).contiguous())), 'an NCHW-contiguous input differs'
    f32 = run(case, kind, x=x32)
    assert f32[1].dtype == torch.float32 and same_bits(base[0], f32[0]) and same_bits(base[1], f32[1].to(torch.bfloat16)) and \
        same_bits(base[1].float(), f32[1]) and all_same(base[2:], f32[2:]), 'an fp32 input differs from its bf16 rounding'
    # a view that starts 8 bytes off a 16-byte boundary (channels-last strides inside a flat buffer)
    flat = torch.zeros(x16.numel() + 8, dtype=torch.bfloat16, device='cuda')
    off = flat[4:4 + x16.numel()].view(N, 17, 33, 96).permute(0, 3, 1, 2)
    off.copy_(x16)
    assert off.data_ptr() % 16 == 8 and off.is_contiguous(memory_format=torch.channels_last)
    assert all_same(base, run(case, kind, x=off)), 'a view off a 16-byte boundary differs'
    # grad_output: bf16 (the same rounding the kernel applies), non-contiguous (every second column of a wider tensor), halved
    assert all_same(base, run(case, kind, x=x16, dy=dy.to(torch.bfloat16)))
    wide = torch.zeros(N, 20, 17, 66, device='cuda')
    wide[..., ::2] = dy
    assert not wide[..., ::2].is_contiguous() and all_same(base, run(case, kind, x=x16, dy=wide[..., ::2]))
    assert all_same(base, run(case, kind, x=x16, dy=dy.contiguous(memory_format=torch.channels_last)))
    half = run(case, kind, x=x16, dy=dy * .5)
    assert same_bits(half[1].float() * 2, base[1].float()) and same_bits(half[2] * 2, base[2]) and same_bits(half[3] * 2, base[3])
    # only the requested gradients are computed and returned
    for need in ((False, True, True), (True, False, True), (True, True, False), (False, False, True), (True, False, False),
                 (False, True, False)):
        got = run(case, kind, x=x16, need=need)
        for j in range(3):
            assert (got[1 + j] is not None) == need[j], need
            assert got[1 + j] is None or same_bits(got[1 + j], base[1 + j]), need
    nob = run(case, kind, x=x16, bias=False)
    assert nob[3] is None and same_bits(nob[1], base[1]) and same_bits(nob[2], base[2])
    ref, S = oracle.forward(x16.float().cpu(), o['wq'], None, mask(kind, 96)[0].double(), 2.)
    d = cb.gamma(96 // 16 + 2) * 2. * S
    cb.check('y without bias', nob[0].cpu(), ref - d - cb.U * (ref.abs() + d), ref + d + cb.U * (ref.abs() + d), ref, S)
    with torch.no_grad():
        k, p = mask(kind, 96)
        assert same_bits(nn.dropout_conv1x1(x32, o['w'].cuda(), o['b'].cuda(), p, True, k.cuda()), base[0])
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.dropout_conv1x1(x32.cpu(), o['w'], o['b'])


def test_bf16_parameters_get_bf16_gradients_rounded_once():
    case = (5, 7, 96, 20)
    o = operands(*case)
    keep, p = mask('p0.5', 96)
    x, dy = o['x'].cuda(), o['dy'].cuda()
    w16, b16 = o['w'].cuda().to(torch.bfloat16), o['b'].cuda().to(torch.bfloat16)
    out = []
    for wt, b in ((w16, b16), (w16.float(), b16.float())):
        wt, b = wt.requires_grad_(True), b.requires_grad_(True)
        y = nn.dropout_conv1x1(x, wt, b, p, True, keep.cuda())
        y.backward(dy)
        out.append((y.detach(), wt.grad, b.grad))
    assert out[0][1].dtype == out[0][2].dtype == torch.bfloat16 and out[1][1].dtype == torch.float32
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1].to(torch.bfloat16)) and \
        same_bits(out[0][2], out[1][2].to(torch.bfloat16))


def test_drawn_mask_is_reproducible_and_the_same_in_forward_and_backward():
    """the mask is the stated draw from torch's default generator: the same seed gives the same bits, and they are the bits of a
    call with that draw as explicit ``keep`` -- whose forward and backward are judged against the fp64 statements above.  A mask
    that varied inside an (n, c) plane, or differed between forward and backward, would differ from it."""
    case = (17, 33, 96, 20)
    o = operands(*case)
    x = o['x'].cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    p = .5

    def drawn(seed):
        torch.manual_seed(seed)
        xg = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        wt, b = o['w'].cuda().requires_grad_(True), o['b'].cuda().requires_grad_(True)
        y = nn.dropout_conv1x1(xg, wt, b, p, True)
        y.backward(o['dy'].cuda())
        return y.detach(), xg.grad, wt.grad, b.grad

    first = drawn(11)
    assert all_same(first, drawn(11)) and not same_bits(first[0], drawn(12)[0])
    torch.manual_seed(11)
    keep = torch.empty((N, 96, 1, 1), dtype=x.dtype, device=x.device).bernoulli_(1 - p).reshape(N, 96) != 0
    assert 0 < int(keep.sum()) < keep.numel()
    assert all_same(first, run(case, 'p0.5', x=x, keep=keep, p=p))
    dropped = (~keep)[:, :, None, None].expand_as(first[1])
    assert bool((first[1][dropped] == 0).all()) and bool((first[1][~dropped] != 0).any())
    state = torch.cuda.get_rng_state()
    nn.dropout_conv1x1(x, o['w'].cuda(), o['b'].cuda(), p, False)  # eval, p = 0 and p = 1 draw nothing
    nn.dropout_conv1x1(x, o['w'].cuda(), o['b'].cuda(), 0., True)
    nn.dropout_conv1x1(x, o['w'].cuda(), o['b'].cuda(), 1., True)
    assert torch.equal(state, torch.cuda.get_rng_state())


def test_module_is_a_drop_in_for_dropout2d_and_conv2d():
    torch.manual_seed(0)
    stock = torch.nn.Conv2d(64, 20, 1).cuda()
    mine = nn.DropoutConv1x1(64, 20, p=.25).cuda()
    mine.load_state_dict(stock.state_dict())
    x = bf16_exact(N, 64, 9, 11, seed=4).cuda()
    mine.eval()
    y = mine(x)
    ref = torch.nn.functional.conv2d(x.double(), stock.weight.detach().double(), stock.bias.detach().double())
    assert y.dtype == torch.float32 and float((y.detach().double() - ref).abs().max()) < 2e-2 * float(ref.abs().max())
    mine.train()
    y = mine(x)
    y.sum().backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 and bool(p.grad.abs().sum() > 0) for p in mine.parameters())


# ---- the chain: label image -> targets -> converted model -> objective -> backward

class _Net(torch.nn.Module):
    """ReadOut.block-shaped heads (Conv 7x7 -> BatchNorm2d -> ReLU -> Dropout2d(0.1) -> Conv 1x1) on a small trunk"""

    def __init__(self, order):
        super().__init__()
        t = torch.nn
        self.trunk = t.Sequential(t.Conv2d(32, 32, 3, padding=1), t.BatchNorm2d(32), t.ReLU())

        def head(cout):
            return t.Sequential(t.Conv2d(32, 32, 7, padding=3), t.BatchNorm2d(32), t.ReLU(), t.Dropout2d(.1), t.Conv2d(32, cout, 1))

        self.heads = t.ModuleDict(dict(scores=head(1), locations=head(2), refinement=head(2), fourier=head(4 * order)))

    def forward(self, x):
        f = self.trunk(x)
        return {k: head(f) for k, head in self.heads.items()}


def test_training_chain_from_label_images():
    H, W, order, S = 32, 40, 3, 8
    yy, xx = np.mgrid[:H, :W]
    gens = []
    np.random.seed(5)
    for discs in (((8, 9, 6), (20, 28, 7), (24, 8, 5)), ((10, 12, 7), (21, 27, 8)), ((16, 20, 9),)):
        lab = np.zeros((H, W), np.int32)
        for i, (cy, cx, r) in enumerate(discs):
            lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = i + 1
        gen = cda.CPNTargetGenerator(samples=S, order=order)
        gen.feed(torch.as_tensor(lab[..., None]).cuda())
        gens.append(gen)
    targets = cda.collate_cpn_targets(gens)
    torch.manual_seed(1)
    net = _Net(order).cuda()
    assert len(nn.convert_conv2d_(net)[0]) == 5 and len(nn.convert_batchnorm2d_(net)[1]) == 5
    replaced, left = nn.convert_readout_tail_(net)
    assert replaced == [f'heads.{k}.4' for k in net.heads] and left == {}
    assert all(type(h[3]) is torch.nn.Identity and type(h[4]) is nn.DropoutConv1x1 and h[4].p == .1 for h in net.heads.values())
    seen = {}

    def hook(name):
        def fn(module, args, output):
            seen[name] = [args[0].detach(), None]
            output.register_hook(lambda g: seen[name].__setitem__(1, g.detach()))
        return fn

    for k, h in net.heads.items():
        h[4].register_forward_hook(hook(k))
    image = bf16_exact(N, 32, H, W, seed=9).cuda()
    torch.manual_seed(21)
    maps = net(image)
    assert all(m.dtype == torch.float32 and m.is_contiguous() for m in maps.values())
    objective = cda.CPNObjective(order, S, refinement_iterations=2)
    loss, losses = objective(maps['scores'], maps['locations'], maps['refinement'], maps['fourier'], targets, size=(H, W))
    loss.backward()
    assert bool(torch.isfinite(loss))
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), name
    torch.manual_seed(21)  # the heads drew their masks in this order, and nothing else draws
    for k, h in net.heads.items():
        x, dy = seen[k]
        assert x.dtype == torch.bfloat16 and dy.dtype == torch.float32
        keep = torch.empty((N, 32, 1, 1), dtype=x.dtype, device=x.device).bernoulli_(1 - .1).reshape(N, 32) != 0
        dx, dw, db = nn.dropout_conv1x1_backward(x, dy, h[4].weight, keep, .1, input_grad=False, bias_dtype=torch.float32)
        assert same_bits(h[4].weight.grad, dw) and same_bits(h[4].bias.grad, db), k
