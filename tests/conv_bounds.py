"""Bound-based acceptance of the conv kernels' outputs (test helper, not a conftest).

The reference is an fp64 conv on exactly the operands the kernel reads (bf16- or e4m3-rounded activations, folded weights
rounded as graph.pack rounds them), together with S = conv(|x|, |w|) + |bias| + |res|, the sum of the absolute terms of
every output.  An output is accepted iff the kernel's output rounding can produce it from some value within the fp32
accumulation noise of the exact result:

    d = gamma(n) * S,   gamma(n) = n u / (1 - n u)

n is the length of the kernel's sequential fp32 chain for that op: one step per MFMA (K_padded / 16 for the bf16 MFMA,
K_padded / 64 for the scaled e4m3 MFMA), +2 for the MFMA-internal sum, plus the epilogue's multiplier / bias / residual
steps; u = 2^-24.  No allowance counts, no fraction of bad elements, no max(scale, 1).

The one exception found on the MI355X: the block-scaled e4m3 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4) does not return its
64-product block sum to fp32 accuracy.  fp32 outputs of single-MFMA reductions (a 1x1 conv over 3 channels, no activation)
sit up to 2^-13.55 of S from the exact sum (worst of 89 fp32-output cases), far beyond an fp32 chain; the instruction's
internal precision is not documented.  It is modelled as one more rounding per block, with E4M3_BLOCK_U = 2^-13 relative to
the block's sum of absolute terms (block_u of conv_with_noise): the smallest power of two above that measurement
(profiles/e4m3_block_sum_error.txt; test_conv_fp8_vs_dequantised_reference and fuzz_conv print it).

Output rounding, applied to the interval [ref - d, ref + d] pushed through the (monotone) activation:

* bf16: got must be one of the bf16 values between RNE(lo) and RNE(hi) -- one value, or two neighbours when the
  interval holds a rounding midpoint.
* e4m3: the same at the tensor's code scale (RNE to e4m3fn after the fp32 product v * inv_scale, saturated at 448,
  subnormal step included).
* fp32: the interval, argument widened by 4 u |x| for expf / tanhf, plus 4 ulp of the result.

Rounding points the kernel performs internally without storing them are modelled as intervals, not slack:

* the fused ReadOut tail's hidden activation relu(conv + bias) -> bf16 (OUT_FUSED_HEAD);
* the bilinear blend of MODE_BL, rounded to bf16 before it enters the MFMA.  Its source coordinates are fp32: exact for
  the x2 resize of the models, within (3 f + 1.5) u of the exact coordinate f otherwise (_bilinear_coordinate_noise).

Each such value is carried as the bf16 interval [RNE(lo), RNE(hi)] of its own noise window (hidden_bf16): where the window
holds no midpoint both ends coincide and kernel and reference round the same way; where it does, the next stage adds
|w_j| * (hi_j - lo_j) / 2 to its noise.  Stored intermediates (sub-pixel partial sums, the two-launch pair / bridge paths) are
not modelled here: each launch is checked against the fp64 conv of what it actually read.
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24            # fp32 unit roundoff (round to nearest)
E4M3_BLOCK_U = 2.0 ** -13  # the scaled e4m3 MFMA's block sum (module docstring)


def gamma(n, u=U):
    return n * u / (1 - n * u)


def chain_length(kh, kw, cin_read, mfma_k=16, epilogue=3):
    """n for one output: MFMA steps over the (padded) reduction (+1 for the zero slab of an odd item count), +2 for the
    MFMA-internal sum, the epilogue's adds.  cin_read = input channels the kernel reduces over per tap, padding included."""
    return -(-kh * kw * cin_read // mfma_k) + 1 + 2 + epilogue


def cin_read(cin, cout, groups, kc=32):
    """Channels one output's reduction runs over in the packed layout (graph.pack): a bundle's cin_b for grouped convs
    packed as bundles, the padded total for dense or densified ones."""
    from celldetection_amd import graph
    geo = graph._bundle_geometry(cin, cout, groups, kc)
    return geo[1] if geo is not None else -(-cin // kc) * kc


def conv64(x, w, bias=None, stride=1, pad=0, groups=1, xabs=None):
    """fp64 conv and S = conv(|x|, |w|) + |bias|.  xabs: an upper bound of |x| to use for S (interval operands)."""
    x, w = x.double(), w.double()
    ref = F.conv2d(x, w, None, stride, pad, 1, groups)
    S = F.conv2d(x.abs() if xabs is None else xabs.double(), w.abs(), None, stride, pad, 1, groups)
    if bias is not None:
        b = bias.double().reshape(1, -1, 1, 1)
        ref, S = ref + b, S + b.abs()
    return ref, S


# ---- rounding of fp64 interval ends, outward: the exact end may lie between two fp32 values ------------------------
def _f32_down(x):
    f = x.float()
    return torch.where(f.double() > x, torch.nextafter(f, torch.full_like(f, -math.inf)), f)


def _f32_up(x):
    f = x.float()
    return torch.where(f.double() < x, torch.nextafter(f, torch.full_like(f, math.inf)), f)


def bf16_down(x):
    """RNE to bf16 of some fp32 value <= x: a lower end of the set {RNE_bf16(v) : v >= x}."""
    return _f32_down(x).to(torch.bfloat16).double()


def bf16_up(x):
    return _f32_up(x).to(torch.bfloat16).double()


def e4m3_down(x):
    return _f32_down(x.clamp(-448., 448.)).to(torch.float8_e4m3fn).double()


def e4m3_up(x):
    return _f32_up(x.clamp(-448., 448.)).to(torch.float8_e4m3fn).double()


def apply_act(x, act, act_scale=1.):
    if act == 'relu':
        return x.clamp_min(0.)
    if act == 'sigmoid':
        return torch.sigmoid(x)
    if act == 'tanh_scaled':
        return torch.tanh(x) * act_scale
    assert act in ('none', None), act
    return x


def _act_interval(ref, d, act, act_scale):
    lo, hi = apply_act(ref - d, act, act_scale), apply_act(ref + d, act, act_scale)
    if act == 'tanh_scaled' and act_scale < 0:
        lo, hi = hi, lo
    return lo, hi


def hidden_bf16(ref, d, act='none', act_scale=1.):
    """A value the kernel rounds to bf16 internally (never stored): -> (mid, half) with the kernel's bf16 value in
    [mid - half, mid + half]; half = 0 wherever the noise window holds no rounding midpoint."""
    lo, hi = _act_interval(ref.double(), d.double(), act, act_scale)
    lo, hi = bf16_down(lo), bf16_up(hi)
    return (lo + hi) / 2, (hi - lo) / 2


def bf16_bounds(ref, d, act='none', act_scale=1.):
    lo, hi = _act_interval(ref.double(), d.double(), act, act_scale)
    return bf16_down(lo), bf16_up(hi)


def e4m3_bounds(ref, d, inv_scale, act='none'):
    """Accepted e4m3 code VALUES (decoded codes, not multiplied by the scale) for an output stored as
    RNE_e4m3(sat(fl32(v * inv_scale))); inv_scale = the fp32 value the kernel receives."""
    lo, hi = _act_interval(ref.double(), d.double(), act, 1.)
    inv = float(inv_scale)
    tl, th = lo * inv, hi * inv
    return e4m3_down(tl - tl.abs() * U), e4m3_up(th + th.abs() * U)


def _ulp32(x):
    m = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(m)) - 23)


def f32_bounds(ref, d, act='none', act_scale=1., ulps=4):
    ref, d = ref.double(), d.double()
    if act in ('sigmoid', 'tanh_scaled'):  # expf / tanhf: the argument's own rounding inside the library routine
        d = d + 4 * U * (ref.abs() + d)
    lo, hi = _act_interval(ref, d, act, act_scale)
    return lo - ulps * _ulp32(lo), hi + ulps * _ulp32(hi)


def conv_with_noise(x, w, bias=None, stride=1, pad=0, groups=1, *, n, x_half=None, res=None, block_u=0.):
    """-> (ref, S, d) of an fp64 conv whose operand x is known to within +-x_half (an interval operand: hidden bf16
    values), with an optional residual added before the activation.  block_u: relative error of the MFMA's own block
    sums (E4M3_BLOCK_U for the e4m3 kernel, 0 for bf16)."""
    xabs = None if x_half is None else x.double().abs() + x_half.double()
    ref, S = conv64(x, w, bias, stride, pad, groups, xabs)
    if res is not None:
        ref, S = ref + res.double(), S + res.double().abs()
    d = (gamma(n) + block_u) * S
    if x_half is not None:
        d = d + F.conv2d(x_half.double(), w.double().abs(), None, stride, pad, 1, groups)
    return ref, S, d


def _bilinear_coordinate_noise(x, size):
    """What the fp32 source coordinates of the kernel's blend can move a blended value by.

    The kernel (like the fp32 bilinear kernel of PyTorch it follows) computes f = max(fl(fl(s^ * (i + 0.5)) - 0.5), 0) with
    s^ = fl(Hs / Hin); i + 0.5 is exact.  With p = s (i + 0.5) = f + 0.5:  |f^ - f| <= p (2u + u^2) + u |p^ - 0.5|
    <= (3 f + 1.5) u.  Where Hs / Hin is a power of two (the exact x2 of the models) every step is exact: 0.  The blend is
    continuous and piecewise linear in f, with slope at most the largest difference of adjacent source pixels in that direction
    among the cells f^ can fall into (a floor that flips reaches one row / column further): taken over the 5 x 5 pixels around
    the exact floor."""
    x = x.double()
    hs, ws = x.shape[-2:]

    def axis(n_src, n_dst):
        f = ((torch.arange(n_dst, dtype=torch.float64) + .5) * n_src / n_dst - .5).clamp_min(0.)
        exact = math.frexp(n_src / n_dst)[0] == .5 and n_src * (1 << 30) % n_dst == 0
        return f.floor().long().clamp_max(n_src - 1), torch.zeros_like(f) if exact else (3. * f + 1.5) * U

    y0, dy = axis(hs, size[0])
    x0, dx = axis(ws, size[1])
    gy = F.pad((x[..., 1:, :] - x[..., :-1, :]).abs(), (0, 0, 0, 1))
    gx = F.pad((x[..., :, 1:] - x[..., :, :-1]).abs(), (0, 1, 0, 0))
    gy, gx = F.max_pool2d(gy, 5, 1, 2), F.max_pool2d(gx, 5, 1, 2)
    return dy[:, None] * gy[..., y0, :][..., x0] + dx[None, :] * gx[..., y0, :][..., x0]


def bilinear_bf16_operand(x, size):
    """MODE_BL's operand: F.interpolate(x, size, 'bilinear', align_corners=False) blended in fp32 (four products, three
    adds, two more products) from fp32 source coordinates and rounded to bf16 inside the kernel -> (mid, half) as for
    hidden_bf16."""
    x = x.double()
    mid = F.interpolate(x, size=size, mode='bilinear', align_corners=False)
    s = F.interpolate(x.abs(), size=size, mode='bilinear', align_corners=False)
    return hidden_bf16(mid, gamma(8) * s + _bilinear_coordinate_noise(x, size))


def fused_tail(ref1, d1, w2, b2, *, act, act_scale=1.):
    """The fused ReadOut tail: hidden = bf16(act(conv + bias)) (never stored), then a 1x1 conv with bf16 weights w2
    [fuse_cout, cout] accumulated by the bf16 MFMA over the hidden channels, + b2 -> (ref2, S2, d2) before fuse_act."""
    mid, half = hidden_bf16(ref1, d1, act, act_scale)
    n2 = chain_length(1, 1, -(-w2.shape[1] // 32) * 32)
    return conv_with_noise(mid, w2.double().reshape(w2.shape[0], -1, 1, 1), b2, n=n2, x_half=half)


def guarded(shape, dtype, guard_elems, sentinel_bits, device):
    """A tensor of `shape` inside a flat buffer with `guard_elems` sentinel elements before and after it (and the tensor
    itself filled with the sentinel): -> (tensor view, buffer)."""
    numel = int(math.prod(shape))
    ity = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[dtype]
    buf = torch.full((numel + 2 * guard_elems,), sentinel_bits, dtype=ity, device=device).view(dtype)
    return buf[guard_elems:guard_elems + numel].view(shape), buf


def assert_guards(name, buf, guard_elems, sentinel_bits):
    ity = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[buf.dtype]
    bits = buf.cpu().view(ity)
    for side, g_ in (('before', bits[:guard_elems]), ('after', bits[bits.numel() - guard_elems:])):
        touched = (g_ != sentinel_bits).nonzero()
        assert touched.numel() == 0, f'{name}: the kernel wrote {touched.numel()} guard elements {side} its output ' \
                                     f'(first at offset {int(touched[0])})'


BF16_GUARD = 0x7fc1   # sentinel bits (a bf16 NaN) of the guard bands around bf16 outputs
F32_GUARD = 0x7fa5a5a5  # ... and around fp32 outputs


def guarded_nhwc_bf16(n, h, w, c, device):
    """A bf16 NHWC output with one whole row of pixels as guard band before and after it: -> (tensor, buffer, guard)."""
    t, buf = guarded((n, h, w, c), torch.bfloat16, w * c, BF16_GUARD, device)
    return t, buf, w * c


def assert_nhwc_bf16(name, buf, guard, t, c_real):
    """Guards untouched, padded channels c_real.. zero; -> the real channels as fp32 NCHW on the CPU."""
    assert_guards(name, buf, guard, BF16_GUARD)
    t = t.cpu()
    pad = t[..., c_real:].float()
    assert bool((pad == 0).all()), f'{name}: padded output channels {c_real}..{t.shape[-1]} are not zero ' \
                                   f'({int((pad != 0).sum())} elements, e.g. {pad[pad != 0][:4].tolist()})'
    return t[..., :c_real].permute(0, 3, 1, 2).float()


class BoundError(AssertionError):
    pass


def check(name, got, lo, hi, ref=None, S=None):
    """Asserts lo <= got <= hi elementwise (got as stored values, fp64-comparable).  Returns the largest
    |got - ref| / (distance from ref to the accepted end on got's side) -- <= 1 iff accepted."""
    got = got.double()
    assert got.shape == lo.shape == hi.shape, (name, tuple(got.shape), tuple(lo.shape))
    ref = (lo + hi) / 2 if ref is None else ref.double().expand_as(got)
    nonfinite = ~torch.isfinite(got)
    side = torch.where(got >= ref, hi - ref, ref - lo).clamp_min(0.)
    dev = (got - ref).abs()
    ratio = torch.where(dev == 0, torch.zeros_like(dev), dev / side)
    ratio = torch.where(nonfinite, torch.full_like(ratio, math.inf), ratio)
    bad = (got < lo) | (got > hi) | nonfinite
    worst = int(torch.argmax(torch.nan_to_num(ratio, nan=math.inf)).item())
    r = float(ratio.reshape(-1)[worst])
    if bool(bad.any()):
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), got.shape))
        s = f', S {float(S.expand_as(got)[idx]):.4e}' if S is not None else ''
        raise BoundError(f'{name}: {int(bad.sum())} / {got.numel()} outside the rounding bound; worst at {idx}: got '
                         f'{float(got[idx]):.8e}, ref {float(ref[idx]):.8e}, accepted [{float(lo[idx]):.8e}, '
                         f'{float(hi[idx]):.8e}]{s} (ratio {r:.3g})')
    return r


def old_rule_accepts(got, ref, f32=False):
    """The acceptance rule the conv tests used before this module (kept to document what it let through)."""
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    scale = ref.abs().max().item() + 1e-6
    tol = (2e-3 if f32 else 1e-2) * max(scale, 1.)
    return int((err > tol + (0 if f32 else 8e-3) * ref.abs()).sum()) == 0


class Bounds:
    """The accepted set [lo, hi] of every output element with its fp64 reference (after the activation) and S."""

    def __init__(self, ref, S, lo, hi):
        self.ref, self.S, self.lo, self.hi = ref, S, lo, hi

    def __call__(self, name, got):
        return check(name, got, self.lo, self.hi, self.ref, self.S)
