"""CPU proof that tests/conv_bounds.py is tight and not flaky: emulations of the conv kernels' arithmetic (bf16 or e4m3
operands, fp32 partial sums of 16 / 64 products accumulated sequentially in a K order different from the reference's,
fp32 epilogue, RNE output rounding) are accepted in every accumulation order; every mutant a subtly wrong kernel would
produce is rejected on every seed; and the acceptance rule the conv tests used before lets at least the truncating
epilogue through (which is why it was replaced)."""
import pytest
import torch
import torch.nn.functional as F

import conv_bounds as cb

SEEDS = [0, 1, 2, 3, 4]
ORDERS = ['forward', 'reversed', 'pairwise', 'shuffled']


def _bf16(t):
    return t.to(torch.bfloat16).float()


def _rtz_bf16(t):
    """fp32 -> bf16 by truncation (round toward zero)."""
    return (t.float().view(torch.int32) & -65536).view(torch.float32)


def _chunk_sums(prod, chunk, block_bits=None):
    """prod [..., K] fp32 exact products -> [..., K / chunk] fp32 partial sums, each summed sequentially; block_bits:
    each block sum truncated to that many significant bits (a block sum less accurate than fp32, like the e4m3 MFMA's)."""
    k = prod.shape[-1]
    prod = F.pad(prod, (0, (-k) % chunk)).reshape(*prod.shape[:-1], -1, chunk)
    if block_bits:
        exact = prod.double().sum(-1)
        e = torch.floor(torch.log2(exact.abs().clamp_min(1e-300))) - (block_bits - 1)
        return (torch.trunc(exact / torch.exp2(e)) * torch.exp2(e)).float()
    acc = prod[..., 0]
    for i in range(1, chunk):
        acc = acc + prod[..., i]
    return acc


def _accumulate(parts, order, seed):
    """fp32 accumulation of the partial sums [..., m] in the given order."""
    m = parts.shape[-1]
    if order == 'pairwise':
        while parts.shape[-1] > 1:
            if parts.shape[-1] % 2:
                parts = F.pad(parts, (0, 1))
            parts = parts[..., 0::2] + parts[..., 1::2]
        return parts[..., 0]
    idx = {'forward': list(range(m)), 'reversed': list(range(m - 1, -1, -1)),
           'shuffled': torch.randperm(m, generator=torch.Generator().manual_seed(seed)).tolist()}[order]
    acc = torch.zeros_like(parts[..., 0])
    for i in idx:
        acc = acc + parts[..., i]
    return acc


def _products(x, w, stride=1, pad=0):
    """x [1, cin, H, W] fp32, w [cout, cin, k, k] fp32 -> exact fp32 products [cout, Ho, Wo, K] in tap-major K order."""
    cout, cin, k, _ = w.shape
    cols = F.unfold(x, k, padding=pad, stride=stride)[0]  # [cin * k * k, L] (channel-major)
    ho = (x.shape[2] + 2 * pad - k) // stride + 1
    wo = (x.shape[3] + 2 * pad - k) // stride + 1
    cols = cols.reshape(cin, k * k, -1).permute(1, 0, 2).reshape(k * k * cin, -1)  # tap-major like the kernel
    wk = w.reshape(cout, cin, k * k).permute(0, 2, 1).reshape(cout, -1)
    prod = wk[:, :, None] * cols[None]  # exact: bf16 x bf16 fits fp32
    return prod.permute(0, 2, 1).reshape(cout, ho, wo, -1)


def _emulate(x, w, b, order='forward', seed=0, res=None, chunk=16, mult=None, pad=None, prod=None, block_bits=None):
    """The kernel's fp32 arithmetic -> pre-activation values [1, cout, Ho, Wo]."""
    k = w.shape[-1]
    prod = _products(x, w, pad=k // 2 if pad is None else pad) if prod is None else prod
    acc = _accumulate(_chunk_sums(prod, chunk, block_bits), order, seed)
    if mult is not None:
        acc = acc * mult[:, None, None]
    v = acc + b[:, None, None]
    if res is not None:
        v = v + res[0]
    return v[None]


def _case(seed, cin=64, cout=32, h=16, w=40, k=3, res=False):
    g = torch.Generator().manual_seed(seed)
    x = _bf16(torch.randn(1, cin, h, w, generator=g))
    wt = _bf16(torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** .5)
    b = torch.randn(cout, generator=g) * .5
    r = _bf16(torch.randn(1, cout, h, w, generator=g)) if res else None
    return x, wt, b, r


def _check_bf16(name, got, x, wt, b, r=None, act='relu', xin=None):
    k = wt.shape[-1]
    n = cb.chain_length(k, k, wt.shape[1])
    ref, S, d = cb.conv_with_noise(x if xin is None else xin, wt, b, pad=k // 2, n=n, res=r)
    lo, hi = cb.bf16_bounds(ref, d, act)
    return cb.check(name, got, lo, hi, cb.apply_act(ref, act), S), cb.old_rule_accepts(got, cb.apply_act(ref, act))


# ---- faithful emulations are accepted ------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('seed', SEEDS)
def test_bf16_emulation_accepted(seed, order):
    x, wt, b, r = _case(seed, res=seed % 2 == 1)
    got = _bf16(F.relu(_emulate(x, wt, b, order, seed, res=r)))
    ratio, _ = _check_bf16('emulation', got, x, wt, b, r)
    assert ratio <= 1


@pytest.mark.parametrize('block_bits', [None, 14])
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('seed', SEEDS)
def test_e4m3_emulation_accepted(seed, order, block_bits):
    """block_bits = 14: 64-product block sums truncated to 14 significant bits (error < 2^-13 of the block's sum of
    absolute terms): what conv_bounds assumes of the scaled e4m3 MFMA (E4M3_BLOCK_U, measured: see its docstring).  This
    shows the checker is consistent with that model; the GPU tests show the model covers the hardware."""
    got, lo, hi, ref = _e4m3_case(seed, order, block_bits=block_bits)
    assert cb.check('e4m3 emulation', got, lo, hi, ref) <= 1


@pytest.mark.parametrize('fuse_act', ['none', 'tanh_scaled', 'sigmoid'])
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('seed', SEEDS)
def test_fused_tail_emulation_accepted(seed, order, fuse_act):
    got, _, (ref2, S2, d2) = _fused_case(seed, order, fuse_act)
    lo, hi = cb.f32_bounds(ref2, d2, fuse_act, 3.)
    assert cb.check('fused tail emulation', got, lo, hi, cb.apply_act(ref2, fuse_act, 3.), S2) <= 1


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('seed', SEEDS)
def test_bilinear_emulation_accepted(seed, order, size=(16, 40)):
    x0, wt, b, xb, got = _bilinear_case(seed, order, size=size)
    mid, half = cb.bilinear_bf16_operand(x0, xb.shape[-2:])
    ref, S, d = cb.conv_with_noise(mid, wt, b, pad=1, n=cb.chain_length(3, 3, wt.shape[1]), x_half=half)
    lo, hi = cb.bf16_bounds(ref, d, 'relu')
    assert cb.check('bilinear emulation', got, lo, hi, F.relu(ref), S) <= 1


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('seed', SEEDS)
def test_bilinear_emulation_accepted_at_odd_sizes(seed, order):
    """17 x 41 from 8 x 20: the scales 8 / 17 and 20 / 41 are no fp32 numbers, the emulation computes its source coordinates in fp32."""
    test_bilinear_emulation_accepted(seed, order, size=(17, 41))


@pytest.mark.parametrize('seed', SEEDS)
def test_f32_sigmoid_tanh_outputs_accepted(seed):
    x, wt, b, _ = _case(seed, cout=3)
    v = _emulate(x, wt, b, 'reversed', seed)
    n = cb.chain_length(3, 3, 64)
    ref, S, d = cb.conv_with_noise(x, wt, b, pad=1, n=n)
    for act, got in (('sigmoid', 1. / (1. + torch.exp(-v))), ('tanh_scaled', torch.tanh(v) * 3.), ('none', v)):
        lo, hi = cb.f32_bounds(ref, d, act, 3.)
        assert cb.check(act, got, lo, hi, cb.apply_act(ref, act, 3.)) <= 1


# ---- helpers of the e4m3 / fused / bilinear cases --------------------------------------------------------------------
def _e4m3_case(seed, order, rtz=False, block_bits=None):
    g = torch.Generator().manual_seed(seed)
    cin, cout, k = 128, 32, 3
    sx = .02
    xc = (torch.randn(1, cin, 12, 40, generator=g) / sx).clamp(-448, 448).to(torch.float8_e4m3fn).float()
    wf = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / (cin * k * k) ** .5
    wscale = (wf.abs().amax((1, 2, 3)) * sx / 448.)
    wc = (wf * sx / wscale[:, None, None, None]).float().to(torch.float8_e4m3fn).float()
    mult = wscale.float()
    b = torch.randn(cout, generator=g) * .5
    v = F.relu(_emulate(xc, wc, b, order, seed, chunk=64, mult=mult, block_bits=block_bits))
    inv = torch.tensor(1. / 0.01, dtype=torch.float32)
    t = v * inv
    got = t.clamp(-448, 448).to(torch.float8_e4m3fn).float()
    if rtz:  # one code toward zero wherever RNE rounded away from zero
        away = got.abs() > t.abs()
        codes = got.to(torch.float8_e4m3fn).view(torch.uint8).to(torch.int32)
        got = torch.where(away, (codes - 1).to(torch.uint8).view(torch.float8_e4m3fn).float(), got)
    # reference: codes x effective weights in fp64 (the kernel's acc * mult)
    weff = wc.double() * wscale[:, None, None, None]
    ref, S, d = cb.conv_with_noise(xc.double(), weff, b, pad=1, n=cb.chain_length(k, k, cin, 64), block_u=cb.E4M3_BLOCK_U)
    lo, hi = cb.e4m3_bounds(ref, d, inv, 'relu')
    ref_v = F.relu(ref) * float(inv)
    return got, lo, hi, ref_v


def _fused_case(seed, order, fuse_act, flip=False):
    g = torch.Generator().manual_seed(seed)
    x, wt, b, _ = _case(seed, cin=32, cout=64, h=8, w=24)
    w2 = _bf16(torch.randn(20, 64, generator=g) / 8.)
    b2 = torch.randn(20, generator=g) * .5
    hid = _bf16(F.relu(_emulate(x, wt, b, order, seed)))  # [1, 64, H, W], rounded to bf16 inside the kernel
    n = cb.chain_length(3, 3, 32)
    ref1, S1, d1 = cb.conv_with_noise(x, wt, b, pad=1, n=n)
    tail = cb.fused_tail(ref1, d1, w2, b2, act='relu')
    if flip:  # one hidden unit rounded to the far neighbour although it sits nowhere near a rounding midpoint
        mid, half = cb.hidden_bf16(ref1, d1, 'relu')
        gain = torch.where((half == 0) & (hid > 0), w2.abs().amax(0)[None, :, None, None] * hid.abs(), torch.zeros_like(hid.double()))
        i = int(torch.argmax(gain))
        h = hid.reshape(-1)
        bits = h[i:i + 1].to(torch.bfloat16).view(torch.int16)
        up = float(ref1.reshape(-1)[i]) > float(h[i])  # RNE went down -> the wrong way is up
        h[i] = (bits + (1 if up else -1)).view(torch.bfloat16).float()[0]
    prod = (w2[:, :, None, None] * hid[0][None]).permute(0, 2, 3, 1)  # [20, H, W, 64] exact products
    acc2 = _accumulate(_chunk_sums(prod, 16), order, seed) + b2[:, None, None]
    got = cb.apply_act(acc2[None].double(), fuse_act, 3.).float()
    return got, hid, tail


def _bilinear_case(seed, order, wrong_index=False, size=(16, 40)):
    g = torch.Generator().manual_seed(seed)
    x0 = _bf16(torch.randn(1, 32, 8, 20, generator=g))
    wt = _bf16(torch.randn(32, 32, 3, 3, generator=g) / 17.)
    b = torch.randn(32, generator=g) * .5
    H, W = size
    # the kernel's blend: fy = max(fl(Hs / Hin) * (y + 0.5) - 0.5, 0), weights hy = 1 - ly ... fp32 (exact at x2: 0.5 (y + 0.5) - 0.5)
    sy, sx = torch.tensor(8., dtype=torch.float32) / H, torch.tensor(20., dtype=torch.float32) / W
    fy = ((torch.arange(H, dtype=torch.float32) + .5) * sy - .5).clamp_min(0.)
    fx = ((torch.arange(W, dtype=torch.float32) + .5) * sx - .5).clamp_min(0.)
    y0, x0i = fy.long(), fx.long()
    y1, x1i = (y0 + 1).clamp_max(7), (x0i + 1).clamp_max(19)
    ly, lx = fy - y0, fx - x0i
    hy, hx = 1 - ly, 1 - lx
    a = lambda yy, xx: x0[0][:, yy][:, :, xx]
    blend = hy[:, None] * (hx * a(y0, x0i) + lx * a(y0, x1i)) + ly[:, None] * (hx * a(y1, x0i) + lx * a(y1, x1i))
    xb = _bf16(blend)[None]
    got = _bf16(F.relu(_emulate(xb, wt, b, order, seed)))
    return x0, wt, b, xb, got


def test_bilinear_operand_carries_fp32_source_coordinates():
    """At an exact x2 the kernel's fp32 source coordinates are exact and the operand's interval is the blend's own noise;
    at 17 x 41 from 8 x 20 (scales 8 / 17, 20 / 41) they are not: over 64 maps some fp32 blends round to a bf16 value the
    exact-coordinate window does not hold, and every one of them lies in the window that carries (3 f + 1.5) u."""
    x = _bf16(torch.randn(64, 32, 8, 20, generator=torch.Generator().manual_seed(0)))
    assert bool((cb._bilinear_coordinate_noise(x, (16, 40)) == 0).all())
    sy, sx = torch.tensor(8., dtype=torch.float32) / 17, torch.tensor(20., dtype=torch.float32) / 41
    fy = ((torch.arange(17, dtype=torch.float32) + .5) * sy - .5).clamp_min(0.)
    fx = ((torch.arange(41, dtype=torch.float32) + .5) * sx - .5).clamp_min(0.)
    y0, x0 = fy.long(), fx.long()
    y1, x1 = (y0 + 1).clamp_max(7), (x0 + 1).clamp_max(19)
    ly, lx = (fy - y0)[:, None], fx - x0
    a = lambda yy, xx: x[:, :, yy][:, :, :, xx]
    kernel = _bf16((1 - ly) * ((1 - lx) * a(y0, x0) + lx * a(y0, x1)) + ly * ((1 - lx) * a(y1, x0) + lx * a(y1, x1))).double()
    exact = F.interpolate(x.double(), size=(17, 41), mode='bilinear', align_corners=False)
    s = F.interpolate(x.double().abs(), size=(17, 41), mode='bilinear', align_corners=False)
    mid, half = cb.hidden_bf16(exact, cb.gamma(8) * s)
    assert int(((kernel < mid - half) | (kernel > mid + half)).sum()) > 0
    mid, half = cb.bilinear_bf16_operand(x, (17, 41))
    assert int(((kernel < mid - half) | (kernel > mid + half)).sum()) == 0
    # (3 f + 1.5) u < 2^-18 at f < 20, adjacent pixels differ by at most 2 max|x|, two axes: far below a bf16 ulp (2^-8)
    assert float(cb._bilinear_coordinate_noise(x, (17, 41)).max()) <= 2. ** -16 * float(x.abs().max())


# ---- mutants are rejected, on every seed ---------------------------------------------------------------------------
def _mutant(kind, seed):
    """-> (got, args of _check_bf16) for a kernel subtly wrong in one way."""
    x, wt, b, r = _case(seed, res=kind == 'res_after_act')
    v = _emulate(x, wt, b, 'forward', seed)
    if kind == 'rtz_output':
        return _rtz_bf16(F.relu(v)), (x, wt, b)
    if kind == 'dropped_term':
        prod = _products(x, wt, pad=1)
        prod[..., 100] = 0.
        return _bf16(F.relu(_emulate(x, wt, b, prod=prod))), (x, wt, b)
    if kind == 'missing_chunk_tile_row':  # 32-channel chunk 1 of tap 4 missing on row 7 (last row of the first 8-row tile)
        prod = _products(x, wt, pad=1)
        prod[:, 7, :, 4 * 64 + 32:4 * 64 + 64] = 0.
        return _bf16(F.relu(_emulate(x, wt, b, prod=prod))), (x, wt, b)
    if kind == 'halo_shift_tile_edge':  # the output column 31 (right edge of a 32-wide tile) reads its halo one pixel right
        xs = torch.cat((x[..., 1:], torch.zeros_like(x[..., :1])), -1)
        vs = _emulate(xs, wt, b, 'forward', seed)
        v = v.clone()
        v[..., 31] = vs[..., 31]
        return _bf16(F.relu(v)), (x, wt, b)
    if kind == 'bias_missing_one_channel':
        v = v.clone()
        v[:, 5] -= b[5]
        return _bf16(F.relu(v)), (x, wt, b)
    if kind == 'res_after_act':
        v = _emulate(x, wt, b, 'forward', seed)
        return _bf16(F.relu(v) + r), (x, wt, b, r)
    if kind == 'nearest_half_index_odd':  # dst >> 1 instead of floor(dst * Hs / Hin) at Hin = 13, Hs = 6
        xs = x[:, :, :6, :6]
        right = F.interpolate(xs, size=(13, 13), mode='nearest')
        idx = (torch.arange(13) >> 1).clamp_max(5)
        wrong = xs[:, :, idx][:, :, :, idx]
        return _bf16(F.relu(_emulate(wrong, wt, b))), (right, wt, b)
    raise KeyError(kind)


BF16_MUTANTS = ['rtz_output', 'dropped_term', 'missing_chunk_tile_row', 'halo_shift_tile_edge', 'bias_missing_one_channel',
                'res_after_act', 'nearest_half_index_odd']


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('kind', BF16_MUTANTS)
def test_bf16_mutant_rejected(kind, seed):
    got, args = _mutant(kind, seed)
    with pytest.raises(cb.BoundError):
        _check_bf16(kind, got, *args)


@pytest.mark.parametrize('seed', SEEDS)
def test_e4m3_rtz_rejected(seed):
    got, lo, hi, ref = _e4m3_case(seed, 'forward', rtz=True)
    with pytest.raises(cb.BoundError):
        cb.check('e4m3 rtz', got, lo, hi, ref)


@pytest.mark.parametrize('seed', SEEDS)
def test_fused_tail_hidden_flip_rejected(seed):
    got, _, (ref2, S2, d2) = _fused_case(seed, 'forward', 'none', flip=True)
    lo, hi = cb.f32_bounds(ref2, d2)
    with pytest.raises(cb.BoundError):
        cb.check('hidden flip', got, lo, hi, ref2, S2)


def test_old_rule_accepts_the_truncating_epilogue():
    """Why the rule changed: err <= 1e-2 max(max|ref|, 1) + 8e-3 |ref| lets an epilogue that truncates through on every
    seed (truncation loses < 2^-7 |x|).  Which other mutants it accepts is printed for the record."""
    for seed in SEEDS:
        got, (x, wt, b) = _mutant('rtz_output', seed)
        ref = F.relu(F.conv2d(x.double(), wt.double(), b.double(), padding=1))
        assert cb.old_rule_accepts(got, ref)
    for kind in BF16_MUTANTS:
        got, args = _mutant(kind, 0)
        xin, wt, b = args[:3]
        ref = F.conv2d(xin.double(), wt.double(), b.double(), padding=1)
        if len(args) > 3:
            ref = ref + args[3]
        print(f'old rule accepts {kind}: {cb.old_rule_accepts(got, F.relu(ref))}')


def test_bounds_are_half_an_ulp_scale():
    """The accepted set is one bf16 value for most outputs (two neighbours only where the noise window holds a rounding
    midpoint): the accumulation noise is a small fraction of a bf16 ulp."""
    x, wt, b, _ = _case(0)
    ref, S, d = cb.conv_with_noise(x, wt, b, pad=1, n=cb.chain_length(3, 3, 64))
    lo, hi = cb.bf16_bounds(ref, d, 'none')
    two = (hi > lo).double().mean().item()
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs())) - 7)
    print(f'two accepted values: {two:.3f} of the outputs; median noise {float((d / ulp).median()):.3g} bf16 ulp')
    assert two < .2 and float((d / ulp).median()) < 1 / 16
