"""GPU tests of the trainable stem and max-pool (``cda.nn.stem_conv2d``, ``stem_weight_grad``, ``max_pool2d`` and the entry points
behind them; csrc/stem_train.hip, csrc/pool_train.hip) against the fp64 statements of tests/stem_oracle.py.  The forward is judged by the rule of
tests/conv_bounds.py with the 14 MFMA steps the kernel runs, the weight and bias gradients by the chain ``stem_weight_grad_info``
reports (which the test itself caps), the pool's forward bit for bit, its gradient by a chain of three adds.  No allowance counts,
no fraction of bad elements.  Outputs and workspaces of the direct launches lie in guarded buffers."""
import functools

import pytest
import torch

import celldetection_amd as cda
import conv_bounds as cb
import stem_oracle as oracle
from celldetection_amd import _lib
from test_gpu_conv_train import bf16_exact, check_sum
from test_stem import ORDERS, _Encoder, converted

pytestmark = pytest.mark.gpu
nn = cda.nn
N = 2
CL = torch.channels_last
DT = {torch.float32: 0, torch.bfloat16: 1}
SHAPES = [(1, 1), (2, 2), (5, 7), (3, 65), (3, 66), (4, 259), (33, 70)]
GEOMETRIES = [(3, 2, 1), (2, 2, 0)]
FWD_CHAIN = cb.chain_length(7, 8, 4)  # the 14 MFMA steps of a filter window of 7 rows x (8 taps x 4 channels), + the epilogue


def _id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def same_bits(a, b):
    ity = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(ity), b.contiguous().view(ity))


@functools.lru_cache(maxsize=None)
def operands(h, w, c, cout):
    """x, weight (fp32, not bf16-exact: the pack rounds it), bias, dY of one case and every fp64 reference of it, computed once."""
    seed = 7 * h + 13 * w + c + 3 * cout
    ho, wo = oracle.out_size(h, w)
    x, dy = bf16_exact(N, c, h, w, seed=seed), bf16_exact(N, cout, ho, wo, seed=seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    wt = torch.randn(cout, c, 7, 7, generator=g) / (7 * c ** .5)
    b = torch.randn(cout, generator=g)
    wq = wt.to(torch.bfloat16).double()
    return dict(x=x, dy=dy, w=wt, b=b, fwd=cb.conv_with_noise(x, wq, b.double(), 2, 3, n=FWD_CHAIN), wgrad=oracle.wgrad(x, dy),
                bgrad=oracle.bgrad(dy))


def guarded(shape, dtype, device='cuda'):
    guard, bits = {torch.bfloat16: (64, cb.BF16_GUARD), torch.float32: (64, cb.F32_GUARD), torch.uint8: (64, 0xa5)}[dtype]
    t, buf = cb.guarded(shape, dtype, guard, bits, device)
    assert t.data_ptr() % 16 == 0
    return t, (buf, guard, bits)


def assert_guards(name, g):
    cb.assert_guards(name, *g)


def run_forward(x, wt, b):
    """The three launches behind stem_conv2d, outputs in guarded buffers -> y [N, Cout, Hout, Wout] fp32 on the CPU."""
    lib = _lib.load()
    n, c, h, w = x.shape
    cout = wt.shape[0]
    ho, wo = oracle.out_size(h, w)
    xp, gx = guarded((n, h + 6, w + 8, 4), torch.bfloat16)
    packed, gp = guarded((7, cout, 32), torch.bfloat16)
    y, gy = guarded((n, ho, wo, cout), torch.bfloat16)
    xd, wd = x.cuda().float().contiguous(), wt.cuda().contiguous()
    bd = None if b is None else b.cuda().float()
    _lib.check(lib.cpn_convert_input_stem(_lib.ptr(xd), 0, _lib.ptr(xp), n, c, h, w, None, _lib.stream_ptr()), 'convert_input_stem')
    _lib.check(lib.cpn_stem_train_pack(_lib.ptr(wd), DT[wd.dtype], cout, c, _lib.ptr(packed), _lib.stream_ptr()), 'pack')
    _lib.check(lib.cpn_stem_train_forward(_lib.ptr(xp), _lib.ptr(packed), _lib.ptr(bd), n, h, w, cout, _lib.ptr(y), _lib.stream_ptr()), 'forward')
    torch.cuda.synchronize()
    for name, g in (('xp', gx), ('packed', gp), ('y', gy)):
        assert_guards(name, g)
    return y.cpu().permute(0, 3, 1, 2).float(), xp, packed.cpu()


def run_wgrad(xp, size, c, dy, slab_rows, dtype=torch.float32):
    """cpn_stem_wgrad with dW, db and the workspace in guarded buffers -> (dW, db) on the CPU."""
    lib = _lib.load()
    n, h, w = size
    cout = dy.shape[1]
    gs = dy.cuda().to(torch.bfloat16).contiguous(memory_format=CL)
    nbytes = int(lib.cpn_stem_wgrad_workspace_bytes(n, h, w, cout, slab_rows))
    assert nbytes > 0 and nbytes % 16 == 0
    ws, gw = guarded((nbytes,), torch.uint8)
    dw, gd = guarded((cout, c, 7, 7), dtype)
    db, gb = guarded((cout,), dtype)
    _lib.check(lib.cpn_stem_wgrad(_lib.ptr(xp), _lib.ptr(gs), n, h, w, c, cout, slab_rows, _lib.ptr(dw), DT[dtype], _lib.ptr(db), DT[dtype],
                                  _lib.ptr(ws), nbytes, _lib.stream_ptr()), 'stem_wgrad')
    torch.cuda.synchronize()
    for name, g in (('workspace', gw), ('dW', gd), ('db', gb)):
        assert_guards(name, g)
    assert bool(torch.isfinite(ws.view(torch.float32)).all())  # every element of the workspace is written, the kx = 7 columns too
    return dw.cpu(), db.cpu()


def chain_of(h, w, cout, slab_rows):
    info = nn.stem_weight_grad_info(N, h, w, cout, slab_rows)
    ho, wo = oracle.out_size(h, w)
    chain = info['steps'] + 2 + info['reduce_chain']  # (no cross-wave sum: the header states one accumulator per element)
    assert chain <= -(-N * ho * wo // 16) + 2 + info['slabs'] + 3, info  # the library cannot widen its own bound
    assert slab_rows == 0 or info['slab_rows'] == min(slab_rows, N * ho)
    return info, chain


# ---- the pack

@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_pack_is_the_statement_bit_for_bit(dtype):
    for c in (1, 3, 4):
        for cout in (32, 64):
            g = torch.Generator().manual_seed(c + cout)
            wt = torch.randn(cout, c, 7, 7, generator=g)
            flat = wt.view(-1)
            flat[:5] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 2.0 ** -133, -(2.0 ** -140)])  # ties; subnormals
            wt = wt.to(dtype)
            got = nn.stem_pack_weight(wt.cuda())
            assert same_bits(got.cpu(), oracle.pack(wt)), (c, cout)
            assert got.cpu().reshape(7, cout, 8, 4)[0, 0, :2, 0].tolist() == [1.0, 1 + 2.0 ** -6]  # ties to even: down, up


# ---- forward and gradients against fp64

@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_forward_and_gradients_within_the_bounds(shape):
    h, w = shape
    for c in (1, 3, 4):
        for cout in (32, 64):
            o = operands(h, w, c, cout)
            y, xp, packed = run_forward(o['x'], o['w'], o['b'])
            assert same_bits(packed, oracle.pack(o['w']))
            ref, S, d = o['fwd']
            cb.check(f'forward {shape} C {c} Cout {cout}', y, *cb.bf16_bounds(ref, d), ref, S)
            for slab_rows in (0, 1, 3):
                info, chain = chain_of(h, w, cout, slab_rows)
                dw, db = run_wgrad(xp, (N, h, w), c, o['dy'], slab_rows)
                check_sum(f'dW {shape} C {c} Cout {cout} slab_rows {slab_rows} ({info["slabs"]} slabs)', dw, *o['wgrad'], chain)
                check_sum(f'db {shape} Cout {cout} slab_rows {slab_rows}', db, *o['bgrad'], info['bias_chain'])


def test_one_hot_operands_are_exact():
    """A single 1 in x and a single 1 in dY: dW holds a single 1 where a tap joins them and exact zeros everywhere else."""
    h, w, c, cout = 4, 259, 3, 64
    ho, wo = oracle.out_size(h, w)
    assert wo == 130
    cases = [((0, 0), (0, 0)), ((0, w - 1), (0, wo - 1)), ((h - 1, 0), (ho - 1, 0)), ((h - 1, w - 1), (ho - 1, wo - 1)),
             ((1, 2 * 127 + 1), (0, 127)),  # the last pixel of the first 128-pixel chunk
             ((0, 0), (ho - 1, wo - 1))]    # no tap joins them
    for n_x, n_dy in ((0, 0), (1, 1), (0, 1)):
        for (iy, ix), (oy, ox) in cases:
            x, dy = torch.zeros(N, c, h, w), torch.zeros(N, cout, ho, wo)
            x[n_x, 2, iy, ix] = 1.
            dy[n_dy, 37, oy, ox] = 1.
            want = oracle.wgrad(x, dy)[0]
            ky, kx = iy + 3 - 2 * oy, ix + 3 - 2 * ox
            joined = n_x == n_dy and 0 <= ky < 7 and 0 <= kx < 7
            assert int((want != 0).sum()) == int(joined) and (not joined or want[37, 2, ky, kx] == 1)
            for slab_rows in (0, 1):
                dw, db = nn.stem_weight_grad(x.cuda(), dy.cuda(), slab_rows)
                assert torch.equal(dw.cpu().double(), want), ((iy, ix), (oy, ox), n_x, n_dy, slab_rows)
                assert torch.equal(db.cpu(), dy.sum((0, 2, 3)))


def test_nothing_from_outside_the_image_reaches_a_sum():
    """x at the bf16 maximum in the image's border pixels, dY small enough for every sum to stay finite: dW within its bound."""
    h, w, c, cout = 5, 7, 3, 32
    big = float(torch.finfo(torch.bfloat16).max)
    x = bf16_exact(N, c, h, w, seed=1)
    x[:, :, 0], x[:, :, -1], x[:, :, :, 0], x[:, :, :, -1] = big, -big, big, -big
    dy = bf16_exact(N, cout, *oracle.out_size(h, w), seed=2, scale=2.0 ** -12)
    info, chain = chain_of(h, w, cout, 0)
    dw, db = nn.stem_weight_grad(x.cuda(), dy.cuda())
    ref, S = oracle.wgrad(x, dy)
    assert bool(torch.isfinite(ref.float()).all())
    check_sum('dW with the bf16 maximum in the border pixels', dw, ref, S, chain)


# ---- behaviour

def test_behaviour_of_the_function_and_the_module():
    h, w, c, cout = 9, 13, 3, 64
    o = operands(h, w, c, cout)
    x, dy = o['x'].cuda(), o['dy'].cuda()
    info, chain = chain_of(h, w, cout, 0)
    ref, S, d = o['fwd']
    results = {}
    for dtype in (torch.float32, torch.bfloat16):
        wt = o['w'].to(dtype).cuda().requires_grad_(True)
        b = o['b'].to(dtype).cuda().requires_grad_(True)
        xin = x.to(dtype)
        y = nn.stem_conv2d(xin, wt, b)
        assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=CL) and y.shape == (N, cout, *oracle.out_size(h, w))
        y.backward(dy)
        assert wt.grad.dtype == b.grad.dtype == dtype and wt.grad.shape == wt.shape
        results[dtype] = (y.detach(), wt.grad, b.grad)
        if dtype == torch.float32:
            cb.check('stem_conv2d forward', y.detach().float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
            check_sum('stem_conv2d dW', wt.grad, *o['wgrad'], chain)
            check_sum('stem_conv2d db', b.grad, *o['bgrad'], info['bias_chain'])
    # bf16 parameters: the fp32 sums rounded once (the bf16 weight is the rounded fp32 one, so dW's operands are the same)
    assert same_bits(results[torch.bfloat16][1], results[torch.float32][1].to(torch.bfloat16))
    assert same_bits(results[torch.bfloat16][2], results[torch.float32][2].to(torch.bfloat16))
    y32, dw32, db32 = results[torch.float32]
    # two runs: bit-identical
    wt = o['w'].cuda().requires_grad_(True)
    b = o['b'].cuda().requires_grad_(True)
    y = nn.stem_conv2d(x, wt, b)
    y.backward(dy)
    assert same_bits(y.detach(), y32) and same_bits(wt.grad, dw32) and same_bits(b.grad, db32)
    # every needs_input_grad subset
    for need_w in (False, True):
        for need_b in (False, True, None):
            wt = o['w'].cuda().requires_grad_(need_w)
            b = None if need_b is None else o['b'].cuda().requires_grad_(need_b)
            y = nn.stem_conv2d(x, wt, b)
            if not (need_w or need_b):
                assert not y.requires_grad
                continue
            y.backward(dy)
            assert (wt.grad is not None) == need_w and (not need_w or same_bits(wt.grad, dw32))
            assert b is None or (b.grad is not None) == need_b and (not need_b or same_bits(b.grad, db32))
    # an NCHW grad_output, grad_output x 0.5 (exact), a view that starts off a 16-byte boundary
    wt = o['w'].cuda().requires_grad_(True)
    nn.stem_conv2d(x, wt).backward(dy.contiguous())
    assert not dy.contiguous().is_contiguous(memory_format=CL) and same_bits(wt.grad, dw32)
    wt = o['w'].cuda().requires_grad_(True)
    nn.stem_conv2d(x, wt).backward(dy * .5)
    assert same_bits(wt.grad, dw32 * .5)
    buf = torch.zeros(dy.numel() + 8, dtype=torch.bfloat16, device='cuda')
    off = buf[1:1 + dy.numel()].view(N, *dy.shape[2:], cout).permute(0, 3, 1, 2)
    off.copy_(dy)
    xbuf = torch.zeros(x.numel() + 8, device='cuda')
    xoff = xbuf[1:1 + x.numel()].view(x.shape)
    xoff.copy_(x)
    assert off.data_ptr() % 16 and xoff.data_ptr() % 16 and off.is_contiguous(memory_format=CL)
    wt = o['w'].cuda().requires_grad_(True)
    y = nn.stem_conv2d(xoff, wt)
    y.backward(off)
    assert same_bits(wt.grad, dw32)
    with pytest.raises(NotImplementedError, match='x requires a gradient'):
        nn.stem_conv2d(x.clone().requires_grad_(True), wt)
    # the module is a drop-in; the saved tensor is the padded input alone
    mod = nn.StemConv2d(c, cout).cuda()
    with torch.no_grad():
        mod.weight.copy_(o['w']), mod.bias.copy_(o['b'])
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        ym = mod(x)
    assert same_bits(ym.detach(), y32)
    assert [tuple(t.shape) for t in saved] == [(N, h + 6, w + 8, 4)] and saved[0].dtype == torch.bfloat16
    dw_alone, db_alone = nn.stem_weight_grad(x, dy)
    assert same_bits(dw_alone, dw32) and same_bits(db_alone, db32)
    assert nn.stem_weight_grad(x, dy, weight=False)[0] is None and nn.stem_weight_grad(x, dy, bias=False)[1] is None


# ---- the pool

POOL_SIZES = [(1, 1), (1, 2), (2, 2), (3, 3), (5, 7), (33, 70)]


@functools.lru_cache(maxsize=None)
def pool_case(h, w, c, geometry, kind='relu'):
    k, s, pad = geometry
    g = torch.Generator().manual_seed(5 * h + w + c + k)
    if kind == 'relu':  # post-ReLU: more than half exact zeros, ties everywhere
        x = (torch.randn(N, c, h, w, generator=g) - .4).clamp_min(0.).to(torch.bfloat16).float()
    elif kind == 'constant':
        x = torch.full((N, c, h, w), 1.5)
    else:  # strictly increasing in raster order per channel plane (bf16-exact: small integers)
        assert h * w <= 256
        x = torch.arange(h * w, dtype=torch.float32).reshape(1, 1, h, w).expand(N, c, h, w).contiguous()
    y, index = oracle.pool_forward(x, k, s, pad)
    dy = bf16_exact(*y.shape, seed=h + w)
    return x, y, index, dy, oracle.pool_backward(dy, index, (h, w), k, s, pad)


def run_pool(x, geometry, dtype):
    """cpn_maxpool2d_indexed with y and the index in guarded buffers -> (y NCHW, index NCHW) on the CPU."""
    k, s, pad = geometry
    n, c, h, w = x.shape
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    xs = x.to(dtype).cuda().contiguous(memory_format=CL)
    y, gy = guarded((n, ho, wo, c), dtype)
    index, gi = guarded((n, ho, wo, c), torch.uint8)
    _lib.check(_lib.load().cpn_maxpool2d_indexed(_lib.ptr(xs), DT[dtype], n, h, w, c, k, s, pad, _lib.ptr(y), _lib.ptr(index),
                                                 _lib.stream_ptr()), 'maxpool2d_indexed')
    torch.cuda.synchronize()
    assert_guards('pool y', gy), assert_guards('pool index', gi)
    return xs, y, index


def run_pool_backward(dy, index, size, geometry, dtype):
    k, s, pad = geometry
    n, c, ho, wo = dy.shape
    h, w = size
    gs = dy.to(dtype).cuda().contiguous(memory_format=CL)
    dx, gd = guarded((n, h, w, c), dtype)
    _lib.check(_lib.load().cpn_maxpool2d_backward(_lib.ptr(gs), _lib.ptr(index), DT[dtype], n, h, w, c, k, s, pad, _lib.ptr(dx),
                                                  _lib.stream_ptr()), 'maxpool2d_backward')
    torch.cuda.synchronize()
    assert_guards('pool dx', gd)
    return dx.cpu().permute(0, 3, 1, 2)


def judge_pool_gradient(name, got, ref, S, count, dtype):
    """Exactly 0 where no window names the pixel; elsewhere three fp32 adds at most, then one rounding to the tensor's dtype."""
    got = got.double()
    assert bool((got[count == 0] == 0).all()), name
    d = cb.gamma(3) * S
    if dtype == torch.bfloat16:
        cb.check(name, got, *cb.bf16_bounds(ref, d), ref, S)
    else:
        tol = d + cb.U * (ref.abs() + d)
        assert bool(((got - ref).abs() <= tol).all()), (name, float(((got - ref).abs() / tol.clamp_min(1e-300)).max()))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('geometry', GEOMETRIES, ids=_id)
def test_pool_forward_and_gradient(geometry, dtype):
    k, s, pad = geometry
    lib = _lib.load()
    for h, w in POOL_SIZES:
        if h + 2 * pad < k or w + 2 * pad < k:  # no window fits: refused as torch refuses it (tests/test_stem.py)
            with pytest.raises(ValueError, match='empty'):
                nn.max_pool2d(torch.zeros(N, 8, h, w, device='cuda'), k, s, pad)
            continue
        for c in (8, 24, 72):
            x, y, index, dy, (ref, S, count) = pool_case(h, w, c, geometry)
            xs, got_y, got_i = run_pool(x, geometry, dtype)
            assert same_bits(got_y.cpu().permute(0, 3, 1, 2), y.to(dtype)), (h, w, c)
            assert torch.equal(got_i.cpu().permute(0, 3, 1, 2), index), (h, w, c)
            if dtype == torch.bfloat16:  # the inference pool gives the same bits
                stock = torch.empty_like(got_y)
                _lib.check(lib.cpn_maxpool2d(_lib.ptr(xs), _lib.ptr(stock), N, h, w, c, k, s, pad, _lib.stream_ptr()), 'maxpool2d')
                assert same_bits(stock, got_y.contiguous())
            dx = run_pool_backward(dy, got_i, (h, w), geometry, dtype)
            judge_pool_gradient(f'pool dx {geometry} {h}x{w} C {c}', dx, ref, S, count, dtype)
            if k == 2:
                assert bool((dx[:, :, 2 * y.shape[2]:] == 0).all()) and bool((dx[:, :, :, 2 * y.shape[3]:] == 0).all())


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('geometry', GEOMETRIES, ids=_id)
def test_pool_gradient_cases(geometry, dtype):
    k, s, pad = geometry
    h, w, c = 5, 7, 8
    for kind in ('relu', 'constant', 'increasing'):
        x, y, index, dy, (ref, S, count) = pool_case(h, w, c, geometry, kind)
        if kind == 'relu':
            assert float((x == 0).float().mean()) > .5
        xd = x.to(dtype).cuda().contiguous(memory_format=CL).requires_grad_(True)
        saved = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
            out = nn.max_pool2d(xd, k, s, pad)
        assert out.dtype == dtype and out.is_contiguous(memory_format=CL) and same_bits(out.detach().cpu(), y.to(dtype))
        # saved: the uint8 index alone, one byte per output element
        assert len(saved) == 1 and saved[0].dtype == torch.uint8 and saved[0].numel() * saved[0].element_size() == y.numel()
        g1, = torch.autograd.grad(out, xd, dy.to(dtype).cuda(), retain_graph=True)
        g2, = torch.autograd.grad(out, xd, dy.to(dtype).cuda())
        assert g1.dtype == dtype and g1.is_contiguous(memory_format=CL) and same_bits(g1, g2)  # two runs: bit-identical
        judge_pool_gradient(f'max_pool2d dx {geometry} {kind}', g1.cpu(), ref, S, count, dtype)
        want = torch.zeros(N, c, h, w, dtype=torch.float64)
        for oy in range(y.shape[2]):
            for ox in range(y.shape[3]):
                if kind == 'constant':  # the whole gradient of a window lands on its first in-image pixel
                    want[:, :, max(oy * s - pad, 0), max(ox * s - pad, 0)] += dy[:, :, oy, ox].double()
                if kind == 'increasing':  # every window's maximum is its last pixel
                    want[:, :, min(oy * s - pad + k, h) - 1, min(ox * s - pad + k, w) - 1] += dy[:, :, oy, ox].double()
        if kind != 'relu':
            assert torch.equal(ref, want) and bool(((g1.cpu().double() != 0) <= (want != 0)).all())
    # gradients of magnitudes 2^-20 and 2^20 meeting in one pixel: (1, 1) is the maximum of all its windows
    x = torch.zeros(N, c, h, w)
    x[:, :, 1, 1] = 3.
    y, index = oracle.pool_forward(x, k, s, pad)
    dy = torch.full(y.shape, 2.0 ** -20)
    dy[:, :, 0, 0] = 2.0 ** 20
    if k == 3:
        dy[:, :, 1, 0] = -(2.0 ** 20)
    ref, S, count = oracle.pool_backward(dy, index, (h, w), k, s, pad)
    assert int(count[0, 0, 1, 1]) == (4 if k == 3 else 1)
    xs, got_y, got_i = run_pool(x, geometry, dtype)
    judge_pool_gradient(f'pool dx {geometry} magnitudes', run_pool_backward(dy, got_i, (h, w), geometry, dtype), ref, S, count, dtype)
    # the module
    assert same_bits(nn.MaxPool2d(k, s, pad)(xs).cpu(), got_y.cpu().permute(0, 3, 1, 2))


# ---- the chain

def _rel(got, ref):
    return float((got.double().cpu() - ref).norm() / ref.norm())


def _make(seed=1):
    torch.manual_seed(seed)
    net = _Encoder(3, fused_initial=False)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * .3 + (1. if name.endswith('weight') else 0.))
            p.copy_(p.to(torch.bfloat16).float())  # bf16-exact parameters: every path reads the same numbers
    return net


class _RoundedStock(torch.nn.Module):
    """The stock module with its output rounded to bf16, as autocast would run it: the path before the stem and the pool ran here."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x.float()).to(torch.bfloat16)


def test_the_converted_encoder_trains_end_to_end():
    """Sequential(conv, bn, relu) -> Sequential(pool, layer1) after all six converts, in two orders: the new pieces judged on the
    operands they saw, the whole against torch's float64 autograd of the stock modules."""
    h, w = 36, 44
    x = bf16_exact(N, 3, h, w, seed=9)
    dy = bf16_exact(N, 256, 9, 11, seed=10)
    stock = _make().double()
    y64 = stock(x.double())
    y64.backward(dy.double())
    ref = dict(y=y64.detach(), **{name: p.grad for name, p in stock.named_parameters()})

    def run(net, hooks=None):
        net = net.cuda()
        if hooks:
            hooks(net)
        y = net(x.cuda())
        y.backward(dy.cuda())
        return net, dict(y=y.detach(), **{name.replace('.inner', ''): p.grad for name, p in net.named_parameters()})

    parent = _make()  # the four other converts only: the path before this pull request, stem and pool in stock torch
    converted(parent, ('conv', 'bn', 'grouped', 'bottleneck'))
    parent[0][0], parent[1][0] = _RoundedStock(parent[0][0]), _RoundedStock(parent[1][0])
    _, got_parent = run(parent)

    seen = {}

    def keep(key, t):
        seen[key] = t.detach()
        if t.requires_grad:
            t.register_hook(lambda g: seen.__setitem__('d' + key, g.detach()))

    def watch(key):
        def fn(module, args, output):  # (returns None: the output stays the module's own)
            keep(key + '.x', args[0]), keep(key + '.y', output)
        return fn

    def hooks(net):
        net[0][0].register_forward_hook(watch('stem'))
        net[1][0].register_forward_hook(watch('pool'))

    first = None
    for order in ORDERS[:2]:
        net = converted(_make(), order)
        before = {k_: v.clone() for k_, v in net.named_buffers()}
        net, got = run(net, hooks)
        assert type(net[0][0]) is nn.StemConv2d and type(net[1][0]) is nn.MaxPool2d and type(net[0][2]) is torch.nn.Identity
        if first is not None:  # the order of the converts does not matter: the same modules, the same bits
            assert all(same_bits(got[key], first[key]) for key in got)
        first = first or got
    for name, b in net.named_buffers():  # the running buffers are updated
        assert not torch.equal(b.cpu(), before[name]), name
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), name
    cpu = {k_: v.cpu() for k_, v in seen.items()}
    # the stem on the operands it saw
    conv = net[0][0]
    wq = conv.weight.detach().cpu().to(torch.bfloat16).double()
    ref_y, S, d = cb.conv_with_noise(cpu['stem.x'].float(), wq, None, 2, 3, n=FWD_CHAIN)
    cb.check('stem forward in the chain', cpu['stem.y'].float(), *cb.bf16_bounds(ref_y, d), ref_y, S)
    info, chain = chain_of(h, w, 64, 0)
    check_sum('stem dW in the chain', conv.weight.grad, *oracle.wgrad(cpu['stem.x'].double(), cpu['dstem.y'].double()), chain)
    # the pool on the operands it saw: the forward bit for bit, the gradient within three adds
    py, pidx = oracle.pool_forward(cpu['pool.x'].float(), 3, 2, 1)
    assert same_bits(cpu['pool.y'], py.to(torch.bfloat16)) and float((cpu['pool.x'] == 0).float().mean()) > .3  # (post-ReLU: ties)
    pref, pS, pcount = oracle.pool_backward(cpu['dpool.y'].float(), pidx, cpu['pool.x'].shape[2:], 3, 2, 1)
    judge_pool_gradient('pool dx in the chain', cpu['dpool.x'].float(), pref, pS, pcount, torch.bfloat16)
    # the whole against fp64: no more than twice the error of the parent's path on any result.  Both are bf16 chains with the same
    # rounding points (the stem's and the pool's outputs are bf16 in both); a wrong tap, tie rule or a lost slab is an error of order 1.
    for key in ref:
        e_new, e_parent = _rel(got[key], ref[key]), _rel(got_parent[key], ref[key])
        print(f'{key}: relative L2 error {e_new:.3e} (all six converts), {e_parent:.3e} (stem and pool stock)')
    for key in ref:
        assert _rel(got[key], ref[key]) <= 2 * _rel(got_parent[key], ref[key]), key


def test_the_stems_output_feeds_the_pool_and_a_lateral():
    """As in the U-Net: the norm's output goes to the pool and to a second consumer; autograd's sum of the two gradients reaches the
    norm, and through it the stem."""
    h, w = 18, 22
    x = bf16_exact(N, 3, h, w, seed=3).cuda()
    stem, bn = nn.StemConv2d(3, 64, bias=False).cuda(), nn.BatchNorm2d(64, activation='relu').cuda()
    lateral = nn.Conv2d(64, 32, 3).cuda()
    seen = {}
    hmap = bn(stem(x))
    hmap.register_hook(lambda g: seen.__setitem__('dh', g.detach()))
    a, b = nn.max_pool2d(hmap, 3, 2, 1), lateral(hmap)
    da, db = bf16_exact(*a.shape, seed=4).cuda(), bf16_exact(*b.shape, seed=5).cuda()
    torch.autograd.backward([a, b], [da, db])
    # each branch alone, on a detached copy of the same tensor
    h1 = hmap.detach().clone().requires_grad_(True)
    g_pool, = torch.autograd.grad(nn.max_pool2d(h1, 3, 2, 1), h1, da)
    h2 = hmap.detach().clone().requires_grad_(True)
    g_lat, = torch.autograd.grad(lateral(h2), h2, db)
    assert bool((g_pool != 0).any()) and bool((g_lat != 0).any())
    assert same_bits(seen['dh'].contiguous(memory_format=CL), (g_pool + g_lat).contiguous(memory_format=CL))  # autograd's add, in bf16
    assert bool(torch.isfinite(stem.weight.grad).all()) and bool((stem.weight.grad != 0).any()) and bool((bn.weight.grad != 0).any())
