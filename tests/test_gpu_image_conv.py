"""GPU tests of the trainable image conv (``cda.nn.image_conv2d``, ``image_weight_grad`` and the entry points behind them;
csrc/image_conv_train.hip) against the fp64 statements of tests/image_conv_oracle.py.  The forward is judged by the rule of
tests/conv_bounds.py with the accumulation steps the header states for an output, the weight and bias gradients by the chain
``image_weight_grad_info`` reports (which the test itself caps), with the judges of tests/test_gpu_stem.py.  No allowance counts, no
fraction of bad elements, no tolerance of its own.  Outputs and workspaces of the direct launches lie in guarded buffers; the
operands of one test lie between bands of NaNs, zeros and plausible numbers (tests/read_guards.py), which no result may depend on.

The images: the 32-pixel fragment of the forward and the 128-pixel chunk of the weight gradient from both sides, rows shorter than a
fragment, a single pixel, and an image of more rows than a slab."""
import functools

import pytest
import torch

import celldetection_amd as cda
import conv_bounds as cb
import image_conv_oracle as oracle
import read_guards as rg
from celldetection_amd import _lib
from test_gpu_conv_train import bf16_exact, check_sum
from test_gpu_stem import assert_guards, guarded, same_bits

pytestmark = pytest.mark.gpu
nn = cda.nn
N = 2
CL = torch.channels_last
DT = {torch.float32: 0, torch.bfloat16: 1}
SHAPES = [(1, 1), (1, 2), (2, 2), (5, 7), (3, 31), (3, 32), (3, 33), (2, 65), (4, 129), (33, 70)]
COUTS = (32, 64, 128)
# the header: 3 MFMA steps per output in one fp32 accumulator, + 2 for the MFMA-internal sum, + the bias add.  (chain_length(3, 4, 4)
# counts a zero slab and a three-step epilogue on top, which this loop does not run: the true count is the smaller one.)
FWD_CHAIN = 3 + 2 + 1
assert FWD_CHAIN <= cb.chain_length(3, 4, 4)


def _id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def operands(h, w, c, cout):
    """x, weight (fp32, not bf16-exact: the pack rounds it), bias, dY of one case and every fp64 reference of it, computed once."""
    seed = 7 * h + 13 * w + c + 3 * cout
    x, dy = bf16_exact(N, c, h, w, seed=seed), bf16_exact(N, cout, h, w, seed=seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    wt = torch.randn(cout, c, 3, 3, generator=g) / (3 * c ** .5)
    b = torch.randn(cout, generator=g)
    wq = wt.to(torch.bfloat16).double()
    return dict(x=x, dy=dy, w=wt, b=b, fwd=cb.conv_with_noise(x, wq, b.double(), 1, 1, n=FWD_CHAIN), wgrad=oracle.wgrad(x, dy),
                bgrad=oracle.bgrad(dy))


def run_forward(x, wt, b, embed=None):
    """The three launches behind image_conv2d, outputs in guarded buffers -> (y [N, Cout, H, W] fp32 on the CPU, Xq, packed)."""
    lib = _lib.load()
    n, c, h, w = x.shape
    cout = wt.shape[0]
    xq, gx = guarded((n, h + 2, w + 3, 4), torch.bfloat16)
    packed, gp = guarded((3, cout, 16), torch.bfloat16)
    y, gy = guarded((n, h, w, cout), torch.bfloat16)
    xd, wd = x.cuda().float().contiguous(), wt.cuda().contiguous()
    bd = None if b is None else b.cuda().float()
    _lib.check(lib.cpn_image_conv_pad(_lib.ptr(xd), n, c, h, w, _lib.ptr(xq), _lib.stream_ptr()), 'pad')
    _lib.check(lib.cpn_image_conv_pack(_lib.ptr(wd), DT[wd.dtype], cout, c, _lib.ptr(packed), _lib.stream_ptr()), 'pack')
    e = rg.Embedding(embed)
    xq_in, packed_in, bd_in = e('xq', xq), e('packed', packed), e('bias', bd)
    with e.watch(lib, 'cpn_image_conv_forward'):
        _lib.check(lib.cpn_image_conv_forward(_lib.ptr(xq_in), _lib.ptr(packed_in), _lib.ptr(bd_in), n, h, w, cout, _lib.ptr(y),
                                              _lib.stream_ptr()), 'forward')
    torch.cuda.synchronize()
    e.check()
    for name, g in (('xq', gx), ('packed', gp), ('y', gy)):
        assert_guards(name, g)
    return y.cpu().permute(0, 3, 1, 2).float(), xq, packed.cpu()


def run_wgrad(xq, size, c, dy, slab_rows, dtype=torch.float32, embed=None):
    """cpn_image_conv_wgrad with dW, db and the workspace in guarded buffers -> (dW, db) on the CPU."""
    lib = _lib.load()
    n, h, w = size
    cout = dy.shape[1]
    gs = dy.cuda().to(torch.bfloat16).contiguous(memory_format=CL)
    nbytes = int(lib.cpn_image_conv_wgrad_workspace_bytes(n, h, w, cout, slab_rows))
    assert nbytes > 0 and nbytes % 16 == 0
    ws, gw = guarded((nbytes,), torch.uint8)
    dw, gd = guarded((cout, c, 3, 3), dtype)
    db, gb = guarded((cout,), dtype)
    e = rg.Embedding(embed)
    xq_in, gs_in = e('xq', xq), e('dy', gs)
    with e.watch(lib, 'cpn_image_conv_wgrad'):
        _lib.check(lib.cpn_image_conv_wgrad(_lib.ptr(xq_in), _lib.ptr(gs_in), n, h, w, c, cout, slab_rows, _lib.ptr(dw), DT[dtype], _lib.ptr(db),
                                            DT[dtype], _lib.ptr(ws), nbytes, _lib.stream_ptr()), 'image_conv_wgrad')
    torch.cuda.synchronize()
    e.check()
    for name, g in (('workspace', gw), ('dW', gd), ('db', gb)):
        assert_guards(name, g)
    assert bool(torch.isfinite(ws.view(torch.float32)).all())  # every element of the workspace is written, the kx = 3 columns too
    return dw.cpu(), db.cpu()


def chain_of(h, w, cout, slab_rows):
    info = nn.image_weight_grad_info(N, h, w, cout, slab_rows)
    chain = info['steps'] + 2 + info['reduce_chain']  # (no cross-wave sum: the header states one accumulator per element)
    assert chain <= -(-N * h * w // 16) + 2 + info['slabs'] + 3, info  # the library cannot widen its own bound
    assert slab_rows == 0 or info['slab_rows'] == min(slab_rows, N * h)
    return info, chain


# ---- the pad and the pack

def _ties(t):
    flat = t.view(-1)
    k = min(5, flat.numel())
    flat[:k] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 2.0 ** -133, -(2.0 ** -140)])[:k]  # ties; subnormals
    return t


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_pack_is_the_statement_bit_for_bit(dtype):
    for c in (1, 3, 4):
        for cout in COUTS:
            g = torch.Generator().manual_seed(c + cout)
            wt = _ties(torch.randn(cout, c, 3, 3, generator=g)).to(dtype)
            got = nn.image_pack_weight(wt.cuda())
            assert same_bits(got.cpu(), oracle.pack(wt)), (c, cout)
            assert got.cpu().reshape(3, cout, 4, 4)[0, 0, :2, 0].tolist() == [1.0, 1 + 2.0 ** -6]  # ties to even: down, up


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_pad_is_the_statement_bit_for_bit(dtype):
    from celldetection_amd.nn.image_conv import _image_pad
    lib = _lib.load()
    for i, (h, w) in enumerate(SHAPES):
        c = (1, 3, 4)[i % 3]
        g = torch.Generator().manual_seed(h + w)
        x = _ties(torch.randn(N, c, h, w, generator=g)).to(dtype)
        got = _image_pad(x.cuda())
        assert got.shape == (N, h + 2, w + 3, 4) and same_bits(got.cpu(), oracle.pad(x)), (h, w, c)
        if dtype == torch.float32:  # the launch itself, into a guarded buffer
            xq, gx = guarded((N, h + 2, w + 3, 4), torch.bfloat16)
            xd = x.cuda()
            _lib.check(lib.cpn_image_conv_pad(_lib.ptr(xd), N, c, h, w, _lib.ptr(xq), _lib.stream_ptr()), 'pad')
            torch.cuda.synchronize()
            assert_guards('xq', gx)
            assert same_bits(xq.cpu(), oracle.pad(x))
    # channels_last and a view off a 16-byte boundary give the same bits
    x = bf16_exact(N, 3, 5, 7, seed=1)
    buf = torch.zeros(x.numel() + 8, device='cuda')
    off = buf[1:1 + x.numel()].view(x.shape)
    off.copy_(x)
    assert off.data_ptr() % 16
    want = oracle.pad(x)
    assert same_bits(_image_pad(off).cpu(), want) and same_bits(_image_pad(x.cuda().contiguous(memory_format=CL)).cpu(), want)


# ---- forward and gradients against fp64

@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_forward_and_gradients_within_the_bounds(shape):
    h, w = shape
    for cout in COUTS:
        for c in (1, 3, 4):
            o = operands(h, w, c, cout)
            y, xq, packed = run_forward(o['x'], o['w'], o['b'])
            assert same_bits(packed, oracle.pack(o['w'])) and same_bits(xq.cpu(), oracle.pad(o['x']))
            ref, S, d = o['fwd']
            cb.check(f'forward {shape} C {c} Cout {cout}', y, *cb.bf16_bounds(ref, d), ref, S)
            for slab_rows in (0, 1, 3):
                info, chain = chain_of(h, w, cout, slab_rows)
                dw, db = run_wgrad(xq, (N, h, w), c, o['dy'], slab_rows)
                check_sum(f'dW {shape} C {c} Cout {cout} slab_rows {slab_rows} ({info["slabs"]} slabs)', dw, *o['wgrad'], chain)
                check_sum(f'db {shape} Cout {cout} slab_rows {slab_rows}', db, *o['bgrad'], info['bias_chain'])
    # without a bias, and bf16 gradients: the fp32 sums rounded once
    o = operands(h, w, 3, 64)
    y, xq, _ = run_forward(o['x'], o['w'], None)
    ref, S, d = cb.conv_with_noise(o['x'], o['w'].to(torch.bfloat16).double(), None, 1, 1, n=FWD_CHAIN)
    cb.check(f'forward {shape} without a bias', y, *cb.bf16_bounds(ref, d), ref, S)
    dw32, db32 = run_wgrad(xq, (N, h, w), 3, o['dy'], 0)
    dw16, db16 = run_wgrad(xq, (N, h, w), 3, o['dy'], 0, torch.bfloat16)
    assert same_bits(dw16, dw32.to(torch.bfloat16)) and same_bits(db16, db32.to(torch.bfloat16))


@pytest.mark.parametrize('shape', [(3, 33), (4, 129), (1, 1)], ids=_id)
def test_no_result_depends_on_bytes_around_the_operands(shape):
    """Xq, the packed weights, the bias and dY each lie between two bands of one byte pattern: a read one pixel past Xq's last row, or
    past the last pixel of dY, would take the pattern in, and the results of the three patterns would differ."""
    h, w = shape
    for cout in COUTS:
        o = operands(h, w, 3, cout)
        results = {}
        for pattern in rg.PATTERNS:
            y, xq, _ = run_forward(o['x'], o['w'], o['b'], embed=pattern)
            dw, db = run_wgrad(xq, (N, h, w), 3, o['dy'], 0, embed=pattern)
            dw1, _ = run_wgrad(xq, (N, h, w), 3, o['dy'], 1, embed=pattern)
            results[pattern] = dict(y=y, dw=dw, db=db, dw1=dw1)
        rg.same_bits_across(results)


def test_one_hot_operands_are_exact():
    """A single 1 in x and a single 1 in dY: dW holds a single 1 where a tap joins them and exact zeros everywhere else -- also where
    the pixel is the one the zero column kx = 3 meets."""
    h, w, c = 4, 129, 3
    cases = [((0, 0), (0, 0)), ((0, w - 1), (0, w - 1)), ((h - 1, 0), (h - 1, 0)), ((h - 1, w - 1), (h - 1, w - 1)),
             ((1, 127), (0, 127)),      # the last pixel of the first 128-pixel chunk
             ((1, 128), (1, 127)),      # a tap across the chunk's edge
             ((2, 5), (2, 3)),          # kx = 3: the pixel meets the zero column, no tap joins them
             ((0, 0), (0, w - 1)),      # the row's last pixel reads the padding in front of the next row, not its first pixel
             ((0, 0), (h - 1, w - 1))]  # no tap joins them
    for cout in COUTS:
        for n_x, n_dy in ((0, 0), (1, 1), (0, 1)):
            for (iy, ix), (oy, ox) in cases:
                x, dy = torch.zeros(N, c, h, w), torch.zeros(N, cout, h, w)
                x[n_x, 2, iy, ix] = 1.
                dy[n_dy, cout - 27, oy, ox] = 1.
                want = oracle.wgrad(x, dy)[0]
                ky, kx = iy + 1 - oy, ix + 1 - ox
                joined = n_x == n_dy and 0 <= ky < 3 and 0 <= kx < 3
                assert int((want != 0).sum()) == int(joined) and (not joined or want[cout - 27, 2, ky, kx] == 1)
                for slab_rows in (0, 1):
                    dw, db = nn.image_weight_grad(x.cuda(), dy.cuda(), slab_rows)
                    assert torch.equal(dw.cpu().double(), want), ((iy, ix), (oy, ox), n_x, n_dy, slab_rows, cout)
                    assert torch.equal(db.cpu(), dy.sum((0, 2, 3)))
                if cout == 64 and n_x == n_dy:  # the forward: a one-hot weight copies the image, shifted by the tap
                    wt = torch.zeros(cout, c, 3, 3)
                    wt[5, 2, min(max(ky, 0), 2), min(max(kx, 0), 2)] = 1.
                    y = nn.image_conv2d(x.cuda(), wt.cuda()).float().cpu()
                    assert torch.equal(y.double(), oracle.forward(x, wt))


def test_nothing_from_outside_the_image_reaches_a_sum():
    """An image that is nothing but its border pixels, at the bf16 maximum, and an image whose last column is at the bf16 maximum:
    the column kx = 3 multiplies it by a zero weight, which must leave every sum finite and within its bound.  The weights and dY
    are small enough for every true sum to stay finite."""
    big = float(torch.finfo(torch.bfloat16).max)
    for (h, w), cout in (((5, 7), 32), ((3, 33), 64), ((4, 129), 128)):
        c = 3
        border = torch.zeros(N, c, h, w)
        border[:, :, 0], border[:, :, -1], border[:, :, :, 0], border[:, :, :, -1] = big, -big, big, -big
        column = bf16_exact(N, c, h, w, seed=1)
        column[:, :, :, -1] = big
        g = torch.Generator().manual_seed(cout)
        wt = (torch.randn(cout, c, 3, 3, generator=g) * 2.0 ** -12).to(torch.bfloat16).float()
        b = torch.randn(cout, generator=g)
        dy = bf16_exact(N, cout, h, w, seed=2, scale=2.0 ** -12)
        info, chain = chain_of(h, w, cout, 0)
        for name, x in (('border-only image', border), ('huge last column', column)):
            ref, S, d = cb.conv_with_noise(x, wt.double(), b.double(), 1, 1, n=FWD_CHAIN)
            assert bool(torch.isfinite(ref.float()).all()) and bool(torch.isfinite(S.float()).all())
            y = nn.image_conv2d(x.cuda(), wt.cuda(), b.cuda()).float().cpu()
            cb.check(f'forward of the {name} {h}x{w}', y, *cb.bf16_bounds(ref, d), ref, S)
            dw, db = nn.image_weight_grad(x.cuda(), dy.cuda())
            ref, S = oracle.wgrad(x, dy)
            assert bool(torch.isfinite(ref.float()).all())
            check_sum(f'dW of the {name} {h}x{w}', dw, ref, S, chain)


def test_channels_the_image_does_not_have_never_reach_dw():
    """cpn_image_conv_wgrad on an Xq whose channels >= cin hold numbers: dW is, bit for bit, what the clean Xq gives, and so is what
    the columns kx < 3 of the real channels give when column kx = 3 alone changes (the zero columns behind the image filled)."""
    h, w = 5, 37
    for c, cout in ((1, 32), (3, 64), (3, 128)):
        o = operands(h, w, c, cout)
        clean = oracle.pad(o['x']).cuda()
        dirty = clean.clone()
        dirty[..., c:] = torch.randn(N, h + 2, w + 3, 4 - c, generator=torch.Generator().manual_seed(c)).to(torch.bfloat16).cuda()
        for slab_rows in (0, 3):
            want = run_wgrad(clean, (N, h, w), c, o['dy'], slab_rows)
            got = run_wgrad(dirty, (N, h, w), c, o['dy'], slab_rows)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (c, cout, slab_rows)
        # the last padding column (x = W + 2 of Xq) is met by kx = 3 alone
        last = clean.clone()
        last[:, :, w + 2, :] = 3.
        assert same_bits(run_wgrad(last, (N, h, w), c, o['dy'], 0)[0], run_wgrad(clean, (N, h, w), c, o['dy'], 0)[0])


# ---- behaviour

def test_behaviour_of_the_function_and_the_module():
    h, w, c, cout = 9, 35, 3, 64
    o = operands(h, w, c, cout)
    x, dy = o['x'].cuda(), o['dy'].cuda()
    info, chain = chain_of(h, w, cout, 0)
    ref, S, d = o['fwd']
    results = {}
    for dtype in (torch.float32, torch.bfloat16):
        wt = o['w'].to(dtype).cuda().requires_grad_(True)
        b = o['b'].to(dtype).cuda().requires_grad_(True)
        xin = x.to(dtype)
        y = nn.image_conv2d(xin, wt, b)
        assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=CL) and y.shape == (N, cout, h, w)
        y.backward(dy)
        assert wt.grad.dtype == b.grad.dtype == dtype and wt.grad.shape == wt.shape
        results[dtype] = (y.detach(), wt.grad, b.grad)
        if dtype == torch.float32:
            cb.check('image_conv2d forward', y.detach().float().cpu(), *cb.bf16_bounds(ref, d), ref, S)
            check_sum('image_conv2d dW', wt.grad, *o['wgrad'], chain)
            check_sum('image_conv2d db', b.grad, *o['bgrad'], info['bias_chain'])
    # bf16 parameters: the fp32 sums rounded once (the bf16 weight is the rounded fp32 one, so dW's operands are the same; the bf16
    # bias is another number than the fp32 one, so the outputs are compared to their own reference)
    assert same_bits(results[torch.bfloat16][1], results[torch.float32][1].to(torch.bfloat16))
    assert same_bits(results[torch.bfloat16][2], results[torch.float32][2].to(torch.bfloat16))
    ref16, S16, d16 = cb.conv_with_noise(o['x'], o['w'].to(torch.bfloat16).double(), o['b'].to(torch.bfloat16).double(), 1, 1, n=FWD_CHAIN)
    cb.check('image_conv2d forward, bf16 parameters', results[torch.bfloat16][0].float().cpu(), *cb.bf16_bounds(ref16, d16), ref16, S16)
    y32, dw32, db32 = results[torch.float32]
    # a channels_last image gives the same bits
    wt = o['w'].cuda().requires_grad_(True)
    assert same_bits(nn.image_conv2d(x.contiguous(memory_format=CL), wt, o['b'].cuda()).detach(), y32)
    # two runs: bit-identical
    wt = o['w'].cuda().requires_grad_(True)
    b = o['b'].cuda().requires_grad_(True)
    y = nn.image_conv2d(x, wt, b)
    y.backward(dy)
    assert same_bits(y.detach(), y32) and same_bits(wt.grad, dw32) and same_bits(b.grad, db32)
    # every needs_input_grad subset
    for need_w in (False, True):
        for need_b in (False, True, None):
            wt = o['w'].cuda().requires_grad_(need_w)
            b = None if need_b is None else o['b'].cuda().requires_grad_(need_b)
            y = nn.image_conv2d(x, wt, b)
            if not (need_w or need_b):
                assert not y.requires_grad
                continue
            y.backward(dy)
            assert (wt.grad is not None) == need_w and (not need_w or same_bits(wt.grad, dw32))
            assert b is None or (b.grad is not None) == need_b and (not need_b or same_bits(b.grad, db32))
    # an NCHW grad_output, grad_output x 0.5 (exact), a view that starts off a 16-byte boundary
    wt = o['w'].cuda().requires_grad_(True)
    nn.image_conv2d(x, wt).backward(dy.contiguous())
    assert not dy.contiguous().is_contiguous(memory_format=CL) and same_bits(wt.grad, dw32)
    wt = o['w'].cuda().requires_grad_(True)
    nn.image_conv2d(x, wt).backward(dy * .5)
    assert same_bits(wt.grad, dw32 * .5)
    buf = torch.zeros(dy.numel() + 8, dtype=torch.bfloat16, device='cuda')
    off = buf[1:1 + dy.numel()].view(N, *dy.shape[2:], cout).permute(0, 3, 1, 2)
    off.copy_(dy)
    xbuf = torch.zeros(x.numel() + 8, device='cuda')
    xoff = xbuf[1:1 + x.numel()].view(x.shape)
    xoff.copy_(x)
    assert off.data_ptr() % 16 and xoff.data_ptr() % 16 and off.is_contiguous(memory_format=CL)
    wt = o['w'].cuda().requires_grad_(True)
    y = nn.image_conv2d(xoff, wt)
    y.backward(off)
    assert same_bits(wt.grad, dw32)
    with pytest.raises(NotImplementedError, match='x requires a gradient'):
        nn.image_conv2d(x.clone().requires_grad_(True), wt)
    # the module is a drop-in; the saved tensor is the padded input alone; state_dicts interchange with a stock Conv2d
    stock = torch.nn.Conv2d(c, cout, 3, 1, 1)
    with torch.no_grad():
        stock.weight.copy_(o['w']), stock.bias.copy_(o['b'])
    mod = nn.ImageConv2d(c, cout).cuda()
    mod.load_state_dict(stock.state_dict())
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        ym = mod(x)
    assert same_bits(ym.detach(), y32)
    assert [tuple(t.shape) for t in saved] == [(N, h + 2, w + 3, 4)] and saved[0].dtype == torch.bfloat16
    ym.backward(dy)
    assert same_bits(mod.weight.grad, dw32) and same_bits(mod.bias.grad, db32)
    back = torch.nn.Conv2d(c, cout, 3, 1, 1)
    back.load_state_dict(mod.state_dict())
    assert torch.equal(back.weight, stock.weight) and torch.equal(back.bias, stock.bias)
    dw_alone, db_alone = nn.image_weight_grad(x, dy)
    assert same_bits(dw_alone, dw32) and same_bits(db_alone, db32)
    assert nn.image_weight_grad(x, dy, weight=False)[0] is None and nn.image_weight_grad(x, dy, bias=False)[1] is None
    # a converted stock conv shares its parameters and gives the same bits
    holder = torch.nn.ModuleDict(dict(conv=stock)).cuda()
    assert nn.convert_image_conv2d_(holder) == (['conv'], {}) and holder['conv'].weight is stock.weight
    assert same_bits(holder['conv'](x).detach(), y32)
