"""GPU tests of the trainable batch normalisation with fused ReLU (``cda.nn.batch_norm``, csrc/batch_norm.hip) against the fp64
statements and the judge of tests/batch_norm_oracle.py (its docstring lists every bound; tests/test_batch_norm.py shows on the CPU
that the judge accepts the stated arithmetic and rejects an fp32 sum of squares, one bf16 step and a mask from unrounded
coefficients).  The chain of the fp64 sums comes from ``batch_norm_info`` and is held <= M + slabs + 8 here, so the library cannot
widen its own bound.  No allowance counts, no fraction of bad elements.
"""
import functools
import itertools

import pytest
import torch

import celldetection_amd as cda
import batch_norm_oracle as oracle

pytestmark = pytest.mark.gpu
nn = cda.nn
N = 2
CL = torch.channels_last
EPS = 1e-5

# (H, W, C): M = 2; two pixels; V = 3 (idle lanes); odd sizes; more than one step, slab and workgroup; C = 2048: one pixel per
# step; C = 2056: two channel blocks
SHAPES = [(1, 1, 8), (1, 2, 8), (5, 7, 24), (5, 7, 32), (3, 40, 96), (17, 33, 160), (33, 70, 64), (1, 3, 2048), (1, 3, 2056)]


@functools.lru_cache(maxsize=None)
def operands(h, w, c, dtype, offset=0.):
    """x and dy in the kernels' dtype (so that every reference sees exactly what the kernel reads), fp32 parameters and buffers."""
    g = torch.Generator().manual_seed(7 * h + 13 * w + c)
    spread = 1 + torch.arange(c, dtype=torch.float32).reshape(1, c, 1, 1) % 7 / 4
    x = (torch.randn(N, c, h, w, generator=g) * spread + offset + torch.randn(1, c, 1, 1, generator=g)).to(dtype)
    dy = torch.randn(N, c, h, w, generator=g).to(dtype)
    wt, b = torch.randn(c, generator=g), torch.randn(c, generator=g)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + .5
    return x, dy, wt, b, rm, rv


def dev(t):
    if t is None:
        return None
    return t.cuda().contiguous(memory_format=CL) if t.dim() == 4 else t.cuda()


def chain_of(m, c, slab_pixels):
    info = nn.batch_norm_info(m, c, slab_pixels)
    assert info['chain'] <= m + info['slabs'] + 8, info
    assert slab_pixels == 0 or info['slab_pixels'] == min(slab_pixels, m)
    return info['chain']


def run_and_judge(name, x, dy, wt, b, rm, rv, training, relu, slab_pixels=0, param_dtype=torch.float32):
    """forward primitive + autograd function on the same operands, everything judged -> dict of what the GPU returned (on the CPU)."""
    c = x.shape[1]
    m = x.numel() // c
    chain = chain_of(m, c, slab_pixels)
    act = 'relu' if relu else None
    use_batch = training or rm is None
    bufs = [None if t is None else dev(t) for t in (rm, rv)]
    y, mean, invstd, scale, shift = nn.batch_norm_forward(dev(x), bufs[0], bufs[1], dev(wt), dev(b), training, 0.1, EPS, act, slab_pixels)
    assert y.dtype == x.dtype and y.shape == x.shape and y.is_contiguous(memory_format=CL)
    got = dict(y=y.cpu(), save_mean=mean.cpu(), save_invstd=invstd.cpu(), scale=scale.cpu(), shift=shift.cpu(),
               running_mean=None if rm is None else bufs[0].cpu(), running_var=None if rv is None else bufs[1].cpu())
    assert all(got[k].dtype == torch.float32 and got[k].shape == (c,) for k in ('save_mean', 'save_invstd', 'scale', 'shift'))
    oracle.judge_stats(name, x, got, chain, wt, b, rm, rv, training, 0.1, EPS, torch.float32 if rm is None else rm.dtype)
    if not training and rm is not None:
        assert torch.equal(got['running_mean'], rm) and torch.equal(got['running_var'], rv)
    oracle.judge_y(name, x, got['y'], got['scale'], got['shift'], relu)
    # the autograd function: the same forward bit for bit, then the gradients
    xg = dev(x).requires_grad_(True)
    wg, bg = [None if t is None else dev(t).requires_grad_(True) for t in (wt, b)]
    bufs2 = [None if t is None else dev(t) for t in (rm, rv)]
    y2 = nn.batch_norm(xg, bufs2[0], bufs2[1], wg, bg, training, 0.1, EPS, act, slab_pixels)
    assert torch.equal(y2.detach().cpu().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                       got['y'].view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32))
    if rm is not None:
        assert torch.equal(bufs2[0].cpu(), got['running_mean']) and torch.equal(bufs2[1].cpu(), got['running_var'])
    y2.backward(dev(dy))
    assert xg.grad.dtype == x.dtype and xg.grad.shape == x.shape
    got.update(dx=xg.grad.cpu(), dgamma=None if wt is None else wg.grad.cpu(), dbeta=None if b is None else bg.grad.cpu())
    assert wt is None or (got['dgamma'].dtype == wt.dtype and got['dbeta'].dtype == b.dtype)
    oracle.judge_grads(name, x, dy, got, chain, wt, got['save_mean'], got['save_invstd'], got['scale'], got['shift'], relu,
                       use_batch, param_dtype)
    return got


@pytest.mark.parametrize('slab_pixels', [0, 1, 3])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_forward_and_gradients_within_the_bounds(shape, dtype, slab_pixels):
    x, dy, wt, b, rm, rv = operands(*shape, dtype)
    for training, relu in ((True, True), (False, True), (True, False), (False, False)):
        run_and_judge(f'{shape} slab_pixels {slab_pixels} training {training} relu {relu}', x, dy, wt, b, rm, rv, training, relu,
                      slab_pixels)


# ---- designed cases

@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_t_exactly_zero_gives_output_and_gradient_exactly_zero(dtype):
    """Eval mode, running_var + eps = 0.25 (invstd 2), gamma 1, beta -2, running_mean 0: t = 2 x - 2 is exactly 0 at x = 1 and
    +- 2^-6 at x = 1 +- 2^-7.  Output and gradient are exactly 0 at t <= 0; dy passes (times 2) right next to it."""
    c, eps = 16, 2.0 ** -4
    vals = torch.tensor([1., 1. + 2. ** -7, 1. - 2. ** -7])
    x = vals[torch.arange(N * c * 3 * 5) % 3].reshape(N, c, 3, 5).to(dtype)
    dy = (torch.arange(N * c * 3 * 5, dtype=torch.float32).reshape(N, c, 3, 5) % 5 + 1).to(dtype)
    rm, rv = torch.zeros(c), torch.full((c,), .25 - eps)
    wt, b = torch.ones(c), torch.full((c,), -2.)
    xg = dev(x).requires_grad_(True)
    y = nn.batch_norm(xg, dev(rm), dev(rv), dev(wt), dev(b), False, 0.1, eps, 'relu')
    y.backward(dev(dy))
    up = x.float() > 1
    assert torch.equal(y.detach().cpu().float(), torch.where(up, torch.full_like(x.float(), 2. ** -6), torch.zeros_like(x.float())))
    assert torch.equal(xg.grad.cpu().float(), torch.where(up, 2 * dy.float(), torch.zeros_like(dy.float())))
    assert bool((y.detach().cpu().float()[x.float() == 1] == 0).all()) and bool((xg.grad.cpu().float()[x.float() == 1] == 0).all())
    _, mean, invstd, scale, shift = nn.batch_norm_forward(dev(x), dev(rm), dev(rv), dev(wt), dev(b), False, 0.1, eps, 'relu')
    assert bool((invstd.cpu() == 2).all()) and bool((scale.cpu() == 2).all()) and bool((shift.cpu() == -2).all()) and \
        bool((mean.cpu() == 0).all())


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_constant_channel(dtype):
    """A channel of the constant 1.5 with eps = 2^-10, gamma 1, beta 0.75: sum x and sum x^2 are exact, var is exactly 0, invstd
    exactly 32, t = 1.5 * 32 - 47.25 = beta exactly.  With a constant dy on that channel sum g x = mean sum g exactly: dgamma is
    exactly 0 and dx = fma(a, g, -a g) = 0.  The other channels are judged as usual."""
    h, w, c, eps = 5, 7, 16, 2.0 ** -10
    x, dy, wt, b, rm, rv = [t.clone() for t in operands(h, w, c, dtype)]
    x[:, 3], dy[:, 3], wt[3], b[3] = 1.5, 0.5, 1., .75
    xg, wg, bg = dev(x).requires_grad_(True), dev(wt).requires_grad_(True), dev(b).requires_grad_(True)
    bufs = dev(rm), dev(rv)
    y = nn.batch_norm(xg, *bufs, wg, bg, True, 0.1, eps, 'relu')
    y.backward(dev(dy))
    assert bool((y.detach().cpu().float()[:, 3] == .75).all()) and bool((xg.grad.cpu().float()[:, 3] == 0).all())
    assert float(wg.grad[3]) == 0 and float(bg.grad[3]) == .5 * N * h * w
    _, mean, invstd, scale, shift = nn.batch_norm_forward(dev(x), dev(rm), dev(rv), dev(wt), dev(b), True, 0.1, eps, 'relu')
    assert float(mean[3]) == 1.5 and float(invstd[3]) == 32 and float(scale[3]) == 32 and float(shift[3]) == .75 - 48
    assert float(bufs[1][3]) == float((torch.tensor(.9, dtype=torch.float64) * rv[3].double()).float())  # 0.9 rv + 0.1 * 0
    chain = chain_of(N * h * w, c, 0)
    got = dict(save_mean=mean.cpu(), save_invstd=invstd.cpu(), scale=scale.cpu(), shift=shift.cpu(), running_mean=bufs[0].cpu(),
               running_var=bufs[1].cpu(), dx=xg.grad.cpu(), dgamma=wg.grad.cpu(), dbeta=bg.grad.cpu())
    oracle.judge_stats('constant channel', x, got, chain, wt, b, rm, rv, True, 0.1, eps)
    oracle.judge_y('constant channel', x, y.detach().cpu(), got['scale'], got['shift'], True)
    oracle.judge_grads('constant channel', x, dy, got, chain, wt, got['save_mean'], got['save_invstd'], got['scale'], got['shift'], True)


@pytest.mark.parametrize('slab_pixels', [0, 3])
def test_large_mean_in_bf16(slab_pixels):
    """x = 300 + randn in bf16 (steps of 2 at that magnitude): the one-pass variance cancels 1e5 against 1e5 and still meets the
    fp64 bound."""
    x, dy, wt, b, rm, rv = operands(17, 33, 160, torch.bfloat16, 300.)
    assert 299 < float(x.float().mean()) < 301
    for training in (True, False):
        run_and_judge(f'x = 300 + randn, training {training}', x, dy, wt, b, rm, rv, training, True, slab_pixels)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('affine,buffers', [(False, True), (True, False), (False, False)], ids=['no-affine', 'no-buffers', 'neither'])
def test_affine_or_running_buffers_absent(dtype, affine, buffers):
    x, dy, wt, b, rm, rv = operands(5, 7, 24, dtype)
    wt, b = (wt, b) if affine else (None, None)
    rm, rv = (rm, rv) if buffers else (None, None)
    for training, relu in ((True, True), (False, True), (True, False)):
        run_and_judge(f'affine {affine} buffers {buffers} training {training}', x, dy, wt, b, rm, rv, training, relu)


# ---- module behaviour

@pytest.mark.parametrize('momentum', [0.1, 1.0, None], ids=str)
def test_module_running_statistics_over_three_steps(momentum):
    h, w, c = 5, 7, 24
    mod = nn.BatchNorm2d(c, momentum=momentum, activation='relu').cuda()
    ref = torch.nn.BatchNorm2d(c, momentum=momentum)
    ref.load_state_dict(mod.state_dict())
    chain = chain_of(N * h * w, c, 0)
    for step in range(1, 4):
        x = operands(h + step, w, c, torch.float32)[0][:, :, :h]
        before = mod.running_mean.cpu().clone(), mod.running_var.cpu().clone()
        mod(dev(x))
        ref(x)
        assert int(mod.num_batches_tracked) == step == int(ref.num_batches_tracked)
        factor = 1. / step if momentum is None else momentum
        got = dict(zip(('save_mean', 'save_invstd', 'scale', 'shift'),
                       (t.cpu() for t in nn.batch_norm_forward(dev(x), None, None, mod.weight, mod.bias, True, 0., mod.eps)[1:])))
        got.update(running_mean=mod.running_mean.cpu(), running_var=mod.running_var.cpu())
        oracle.judge_stats(f'momentum {momentum} step {step}', x, got, chain, mod.weight.detach().cpu(), mod.bias.detach().cpu(),
                           *before, True, factor, mod.eps)
        torch.testing.assert_close(got['running_mean'], ref.running_mean, rtol=1e-5, atol=1e-6)  # (torch's own fp32 module)
        torch.testing.assert_close(got['running_var'], ref.running_var, rtol=1e-5, atol=1e-6)
    mod.eval()
    before = mod.running_mean.clone(), mod.running_var.clone()
    mod(dev(x))
    assert int(mod.num_batches_tracked) == 3 and torch.equal(mod.running_mean, before[0]) and torch.equal(mod.running_var, before[1])


def test_training_on_one_value_per_channel_raises():
    mod = nn.BatchNorm2d(8).cuda()
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        mod(torch.zeros(1, 8, 1, 1, device='cuda'))
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        nn.batch_norm(torch.zeros(1, 8, 1, 1, device='cuda'), None, None, training=True)
    mod.eval()
    assert mod(torch.zeros(1, 8, 1, 1, device='cuda')).shape == (1, 8, 1, 1)  # eval mode runs on a single value


def test_bf16_parameters_and_gradients():
    h, w, c = 5, 7, 32
    x, dy, wt, b, rm, rv = operands(h, w, c, torch.bfloat16)
    wt, b, rm, rv = (t.to(torch.bfloat16) for t in (wt, b, rm, rv))
    got = run_and_judge('bf16 parameters', x, dy, wt, b, rm, rv, True, True, 0, torch.bfloat16)
    assert got['dgamma'].dtype == got['dbeta'].dtype == got['running_mean'].dtype == got['running_var'].dtype == torch.bfloat16
    mod = nn.BatchNorm2d(c, activation='relu').cuda().to(torch.bfloat16)
    y = mod(dev(x))
    y.backward(dev(dy))
    assert y.dtype == mod.weight.grad.dtype == mod.bias.grad.dtype == mod.running_var.dtype == torch.bfloat16
    assert mod.num_batches_tracked.dtype == torch.int64 and int(mod.num_batches_tracked) == 1


# ---- autograd behaviour

def _step(x, dy, wt, b, rm, rv, needs=(True, True, True), training=True):
    """-> (y, dx, dgamma, dbeta, running_mean, running_var) of one step: the two buffers as the step left them"""
    xg, wg, bg = (dev(t).requires_grad_(n) for t, n in zip((x, wt, b), needs))
    bufs = dev(rm), dev(rv)
    y = nn.batch_norm(xg, *bufs, wg, bg, training, 0.1, EPS, 'relu')
    if y.requires_grad:
        y.backward(dy if dy.is_cuda else dev(dy))
    return (y.detach(), xg.grad, wg.grad, bg.grad) + bufs


def _bits(t):
    return t.cpu().view({2: torch.int16, 4: torch.int32}[t.element_size()])


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_every_needs_input_grad_subset(dtype):
    for training in (True, False):
        ops = operands(5, 7, 32, dtype)
        full = _step(*ops, training=training)
        for needs in itertools.product((True, False), repeat=3):
            got = _step(*ops, needs=needs, training=training)
            assert all(torch.equal(_bits(got[i]), _bits(full[i])) for i in (0, 4, 5))
            for need, g, f in zip(needs, got[1:4], full[1:4]):
                assert (g is None) == (not need)
                assert g is None or torch.equal(_bits(g), _bits(f)), (needs, training)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_grad_output_layout_scale_and_determinism(dtype):
    x, dy, wt, b, rm, rv = operands(17, 33, 160, dtype)
    full = _step(x, dy, wt, b, rm, rv)
    again = _step(x, dy, wt, b, rm, rv)  # two runs: bit-identical in every output, the updated running buffers included
    assert len(full) == 6 and not torch.equal(full[4].cpu(), rm) and not torch.equal(full[5].cpu(), rv)
    assert all(torch.equal(_bits(a), _bits(f)) for a, f in zip(again, full))
    nchw = dy.cuda().contiguous()  # an NCHW-contiguous grad_output
    assert not nchw.is_contiguous(memory_format=CL)
    assert all(torch.equal(_bits(a), _bits(f)) for a, f in zip(_step(x, nchw, wt, b, rm, rv), full))
    half = _step(x, (dy.float() * .5).to(dtype), wt, b, rm, rv)  # grad_output * 0.5: every sum, coefficient and fma halves exactly
    assert all(torch.equal(_bits(a), _bits((f.float() * .5).to(f.dtype))) for a, f in zip(half[1:4], full[1:4]))
    assert all(torch.equal(_bits(half[i]), _bits(full[i])) for i in (0, 4, 5))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_views_that_start_off_a_16_byte_boundary(dtype):
    """x and grad_output as channels-last-contiguous views one element (2 or 4 bytes) into a flat buffer: the
    kernels load 16 bytes at a time, so such a view is copied to an aligned tensor first -- same bits as from an aligned one."""
    x, dy, wt, b, rm, rv = operands(5, 7, 24, dtype)
    full = _step(x, dy, wt, b, rm, rv)

    def off(t):
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
        view = flat[1:].view(N, 5, 7, 24).permute(0, 3, 1, 2)
        view.copy_(t.cuda())
        assert view.data_ptr() % 16 != 0 and view.is_contiguous(memory_format=CL)
        return view

    xg = off(x).requires_grad_(True)
    wg, bg = dev(wt).requires_grad_(True), dev(b).requires_grad_(True)
    bufs = dev(rm), dev(rv)
    y = nn.batch_norm(xg, *bufs, wg, bg, True, 0.1, EPS, 'relu')
    y.backward(off(dy))
    got = (y.detach(), xg.grad, wg.grad, bg.grad) + bufs
    assert all(torch.equal(_bits(a), _bits(f)) for a, f in zip(got, full))
    fwd = nn.batch_norm_forward(off(x), dev(rm), dev(rv), dev(wt), dev(b), True, 0.1, EPS, 'relu')
    assert torch.equal(_bits(fwd[0]), _bits(full[0]))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_saves_x_and_per_channel_vectors_only(dtype):
    x, dy, wt, b, rm, rv = operands(17, 33, 160, dtype)
    saved = []

    def pack(t):
        saved.append(t.numel() * t.element_size())
        return t

    xg, wg, bg = (dev(t).requires_grad_(True) for t in (x, wt, b))
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y = nn.batch_norm(xg, dev(rm), dev(rv), wg, bg, True, 0.1, EPS, 'relu')
    c = x.shape[1]
    assert sum(saved) <= x.numel() * x.element_size() + 64 * c, saved
    y.backward(dev(dy))
    assert xg.grad is not None


# ---- composition with the trainable conv

def test_conv_norm_relu_after_both_converts():
    h, w, c = 5, 7, 32
    g = torch.Generator().manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(c, c, 3, padding=1), torch.nn.BatchNorm2d(c), torch.nn.ReLU())
    with torch.no_grad():
        net[1].weight.copy_(torch.randn(c, generator=g))
        net[1].bias.copy_(torch.randn(c, generator=g))
    assert nn.convert_conv2d_(net)[0] == ['0'] and nn.convert_batchnorm2d_(net)[:2] == (['1'], ['1'])
    assert type(net[0]) is nn.Conv2d and type(net[1]) is nn.BatchNorm2d and type(net[2]) is torch.nn.Identity
    net.cuda()
    seen = {}
    net[0].register_forward_hook(lambda mod, args, out: seen.update(conv=out))
    x, dy = operands(h, w, c, torch.bfloat16)[:2]
    before = net[1].running_mean.cpu().clone(), net[1].running_var.cpu().clone()
    xg = dev(x).requires_grad_(True)
    y = net(xg)
    conv = seen['conv'].detach()
    assert conv.dtype == torch.bfloat16 and conv.is_contiguous(memory_format=CL) and y.dtype == torch.bfloat16
    y.backward(dev(dy))
    wt, b = net[1].weight.detach().cpu(), net[1].bias.detach().cpu()
    # the norm against the oracle on the conv's own bf16 output
    _, mean, invstd, scale, shift = nn.batch_norm_forward(conv, None, None, net[1].weight, net[1].bias, True, 0.1, net[1].eps, 'relu')
    got = dict(save_mean=mean.cpu(), save_invstd=invstd.cpu(), scale=scale.cpu(), shift=shift.cpu(),
               running_mean=net[1].running_mean.cpu(), running_var=net[1].running_var.cpu(), dgamma=net[1].weight.grad.cpu(),
               dbeta=net[1].bias.grad.cpu())
    chain = chain_of(N * h * w, c, 0)
    oracle.judge_stats('conv -> norm', conv.cpu(), got, chain, wt, b, *before, True, 0.1, net[1].eps)
    oracle.judge_y('conv -> norm', conv.cpu(), y.detach().cpu(), got['scale'], got['shift'], True)
    oracle.judge_grads('conv -> norm', conv.cpu(), dy, got, chain, wt, got['save_mean'], got['save_invstd'], got['scale'], got['shift'],
                       True)
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all()) and bool(torch.isfinite(net[0].weight.grad).all())
    assert float(net[0].weight.grad.abs().max()) > 0
