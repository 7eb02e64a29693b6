"""float64 references, error bounds, cases and judges for the kernels that sit between the convs of every plan: input conversion,
max-pool, bilinear / bicubic resize, the elementwise activation op and the calibration abs-max, in all three precisions
(csrc/misc_kernels.hip, csrc/misc_fp8.hip, the helpers of csrc/conv_f32.hip, input_stem_kernel of csrc/stem.hip).

Plain numpy / torch-CPU; nothing here touches the GPU.  ``tests/test_graph_ops.py`` runs every judge with torch-CPU fp32 arithmetic
followed by the precision's rounding standing in for the kernels (so each bound is shown to be satisfiable) and measures the constants
the bounds leave open; ``tests/test_gpu_graph_ops.py`` runs the same cases and judges on the kernels.

Stored formats.  bf16: RNE of the fp32 value.  fp32: the value.  fp8: OCP e4m3 codes of RNE(sat_448(fl32(value * fl32(1 / scale)))).
A case holds VALUES; ``encode`` gives what a tensor stores, in fp8 in code units (value / scale) -- the fp8 pool and resize kernels
decode, compute and encode with one scale, so they work on code values and the scale drops out.

Exact family (byte for byte).
  max-pool     a maximum rounds nothing; windows never mix +0 and -0 (fmaxf may return either).
  input        bf16 RNE(v) | v | e4m3 RNE(sat(fl32(v * fl32(1 / scale)))), v = the f32 source or IEEE fp32 u8 / 255; padded channels 0.
  abs-max      max |x| of a bf16 tensor is one of its values.
  bilinear at dyadic ratios (same size, x2, x4) on grid values k / 16, |k| <= 15 (4 significant bits: bf16, e4m3 and fp32 hold
               them): source coordinates and weights are multiples of 1/8, every product and sum of the fp32 blend is a multiple of
               2^-10 below 2^14, hence exact, fused or not; the result is the float64 value rounded once, ties included.

Interval family: got must lie in [down(ref - e), up(ref + e)], down / up = the output format's rounding of the interval ends
(conv_bounds: bf16_down / e4m3_down / fp32 outward).  u = 2^-24.

  bilinear, non-dyadic ratio.  The kernel computes f^ = max(fl(fl(s^ (o + .5)) - .5), 0), s^ = fl(in / out): |f^ - f| <= (3 f + 1.5) u
  <= 6 u max(f, 1) (conv_bounds._bilinear_coordinate_noise).  The blend is continuous and piecewise linear in f with slope at most the
  largest difference of vertically / horizontally adjacent source pixels in the cells f^ can fall into: the 3 x 3 pixels around the
  exact floor.  l = f^ - floor(f^) is exact; h = fl(1 - l), two products, an add, a product and an add lie on the path of every
  tap: 6 roundings, e_arith = 6 u sum_taps w |v|.  e = e_coord + e_arith per pixel.  Inputs are positive in [0.5, 2]: no
  cancellation, so the intervals stay narrow -- at most TWO_VALUED_CAP of a case's bf16 / e4m3 outputs may have an interval that
  holds two values of the format and none more than two (an fp32 interval always holds several fp32 values: no cap there).

  bicubic.  The rule of the fp32 bicubic head-map kernel (head_maps_oracle): e = BICUBIC_MARGIN x the error of torch-CPU fp32
  bicubic against float64 on the same case (committed measurement, units of 2^-23 max|x|); FMA contraction and the order of the
  weight polynomials differ between implementations, no more.

  activations (cpn_kernels.h act_apply = the torch.nn fp32 formulas).  r(y) = u |y| is one rounding; a library function f is allowed
  L_f ulps = 2 L_f u |f|, L_f = 2 x (worst error in ulps of the torch-CPU fp32 function against float64 on the cases' own arguments)
  + 1 -- the device's libm is another one (head_maps_oracle.exp_allowance has the same rule and reason).  q = sigmoid(-x) = t / (1 + t),
  t = exp(-x).  Before the output rounding:
    relu          exact
    leaky_relu    u |y|                      (x > 0: exact; the slope is the fp32 constant 0.01f)
    sigmoid       (2 L_exp q + 2) u y        (exp, the sum, the division; d y / y = -q d t / t)
    silu          (2 L_exp q + 2) u |y|
    gelu          y = 0.5 x s, s = 1 + erf(a), a = fl(x c): a carries 2 u relative (c's own rounding, the product), erf moves by
                  |a| erf'(a) 2 u; erff adds 2 L_erf u |erf|; the sum and the product one rounding each:
                  e = 0.5 |x| (2 L_erf u |erf| + 2 u |a| erf'(a) + 2 u (1 + |erf|)) -- relative to 0.5 |x| (1 + |erf|), not to y:
                  in the negative tail s cancels to 0 and y is lost entirely, which the formula (torch's too) does
    elu           x > 0: exact; else 2 L_expm1 u |y|
    selu          x > 0: u |y|; else (2 L_expm1 + 2) u |y|   (the constants are the fp32 ones)
    tanh          2 L_tanh u |y|
    hardswish     y = x c / 6, c = clamp(fl(x + 3), 0, 6): the sum's rounding u |x + 3| reaches y only inside the clamp; the product
                  and the (correctly rounded) division: e = |x| u |x + 3| / 6 [0 < x + 3 < 6] + 2 u |y|.  Where |x c| exceeds the fp32
                  range the formula overflows (torch's too): the expected result is +-inf, exactly.
    softplus      x > 20: x (the formula's switch; the tail exp(-x) it drops is e_sp there); else sp = log1p(t'), t' = exp(x):
                  e_sp = 2 L_exp u p + 2 L_log1p u sp, p = sigmoid(x) = t' / (1 + t') (d sp = p d t' / t')
    mish          y = x tanh(sp): e = |x| ((1 - tanh^2 sp) e_sp + 2 L_tanh u tanh sp) + u |y|   (three library calls in a chain)
  plus, for the formulas with a library call, an absolute floor of 2^-120: 1 + exp(-x) overflows for x < -88.73, where the kernel
  returns 0 for a y with |y| = |x| e^x < 2^-121, and results below the normal range may be flushed.
  fp8: the argument is the fp32 product code * in_scale (the reference forms the same IEEE product); the result is multiplied by
  fl32(1 / out_scale) (one more rounding, conv_bounds.e4m3_bounds) and encoded.

How the fp32 / fp8 kernels are reached: hand-written conv-free plans (``Plan``), the tensor under test read back from the workspace.
A plan's resize goes to the input size, so its ratios come from max-pool chains; sizes no chain can produce (5x3 -> 33x47 and
1x7 -> 5x13: a pool maps the larger extent to the larger extent) and the downscale run on the bf16 entry point only.
"""
import functools
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import conv_bounds as cb
from celldetection_amd import _lib

U = 2.0 ** -24
ACT_FLOOR = 2.0 ** -120
F32_MAX = float(np.finfo(np.float32).max)
TWO_VALUED_CAP = 0.02
BICUBIC_MARGIN = 4.
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = os.path.join(ROOT, 'tests', 'golden', 'graph_ops_measured.json')
PRECISIONS = ('bf16', 'fp32', 'fp8')
PRECISION_CODE = {'bf16': _lib.PRECISION_BF16, 'fp32': _lib.PRECISION_F32, 'fp8': _lib.PRECISION_FP8}
STORE = {'bf16': torch.bfloat16, 'fp32': torch.float32, 'fp8': torch.float8_e4m3fn}
BITS = {'bf16': torch.int16, 'fp32': torch.int32, 'fp8': torch.uint8}
ELEM = {'bf16': 2, 'fp32': 4, 'fp8': 1}
C = 64  # channels of every plan tensor: a multiple of 32 and of the 64 an fp8 tensor needs


def measured():
    with open(MEASURED) as f:
        return json.load(f)


# ---- formats ---------------------------------------------------------------------------------------------------------------------
def encode(prec, v):
    """What a tensor of ``prec`` stores for fp32-representable values v (fp8: v in code units) -- one RNE."""
    v = torch.as_tensor(v).float()
    return v.clamp(-448., 448.).to(STORE[prec]) if prec == 'fp8' else v.to(STORE[prec])


def bits(prec, t):
    return t.contiguous().view(BITS[prec])


def inv_scale(scale):
    """fl32(1 / scale) as the executor computes it."""
    return float(np.float32(1.) / np.float32(scale))


def bf16_patterns():
    """Every finite bf16 bit pattern (65 280) as fp32 values."""
    b = torch.arange(65536, dtype=torch.int32)
    return b[(b & 0x7f80) != 0x7f80].to(torch.int16).view(torch.bfloat16).float()


def e4m3_patterns():
    """Every finite e4m3 code (254) as fp32 code values."""
    b = torch.arange(256, dtype=torch.int32)
    return b[(b & 0x7f) != 0x7f].to(torch.uint8).view(torch.float8_e4m3fn).float()


def widened_patterns():
    """The bf16 patterns with random low mantissa bits: fp32 values over the whole finite range."""
    hi = bf16_patterns().view(torch.int32)
    low = torch.randint(0, 1 << 16, hi.shape, generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    return (hi | low).view(torch.float32)


def nhwc(x, cpad=None):
    """NCHW -> NHWC with zero-padded channels."""
    x = x.permute(0, 2, 3, 1)
    return x.contiguous() if cpad in (None, x.shape[-1]) else F.pad(x, (0, cpad - x.shape[-1])).contiguous()


def random_values(prec, shape, seed, lo=None, hi=None):
    """Values the precision holds exactly (fp8: code values): random signs and magnitudes, never zero; or uniform in [lo, hi]."""
    g = torch.Generator().manual_seed(seed)
    if lo is not None:
        return encode(prec, lo + (hi - lo) * torch.rand(shape, generator=g)).float()
    if prec == 'fp8':
        codes = e4m3_patterns()
        codes = codes[codes != 0]
        return codes[torch.randint(0, codes.numel(), shape, generator=g)]
    x = torch.randn(shape, generator=g)
    x = torch.where(x == 0, torch.ones_like(x), x)
    return encode(prec, x).float()


def grid_values(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-15, 16, shape, generator=g).float() / 16


# ---- judges ----------------------------------------------------------------------------------------------------------------------
def judge_exact(name, prec, got, exp):
    """Byte for byte: got and exp are tensors of the stored dtype."""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (name, tuple(got.shape), tuple(exp.shape), got.dtype, exp.dtype)
    g, e = bits(prec, got).reshape(-1), bits(prec, exp).reshape(-1)
    bad = (g != e).nonzero().reshape(-1)
    if bad.numel():
        i = int(bad[0])
        raise AssertionError(f'{name}: {bad.numel()} / {g.numel()} stored values differ; first at flat index {i} of '
                             f'{tuple(got.shape)}: got bits {int(g[i]) & 0xffffffff:#x} ({float(got.reshape(-1)[i].float())!r}), '
                             f'expected {int(e[i]) & 0xffffffff:#x} ({float(exp.reshape(-1)[i].float())!r})')
    return 0.


def interval(prec, ref, e, out_inv_scale=None):
    """[lo, hi] in the stored format (fp64 tensors of stored values) for an exact value within e of ref."""
    ref, e = ref.double(), torch.as_tensor(e).double()
    if prec == 'bf16':
        return cb.bf16_down(ref - e), cb.bf16_up(ref + e)
    if prec == 'fp32':
        return cb._f32_down(ref - e).double(), cb._f32_up(ref + e).double()
    if out_inv_scale is not None:
        return cb.e4m3_bounds(ref, e, out_inv_scale)
    return cb.e4m3_down(ref - e), cb.e4m3_up(ref + e)


def needed_error(prec, got, ref):
    """Smallest |v - ref| over the values v that the format's rounding maps to got: 0 where got is the rounding of ref itself, the
    distance to the midpoint between got and that rounding otherwise (they are neighbours once the interval judge has passed)."""
    got, ref = got.double(), ref.double()
    if prec == 'fp32':  # what the stored value is off by beyond the rounding of ref itself (subnormal results: e is below an ulp)
        return ((got - ref).abs() - (ref.float().double() - ref).abs()).clamp_min(0.)
    near = encode(prec, ref).float().double()
    return torch.where(got == near, torch.zeros_like(ref), ((got + near) / 2 - ref).abs())


def judge_interval(name, got, lo, hi, ref, prec=None, e=None):
    """lo <= got <= hi elementwise (infinite ends accept exactly that infinity, NaN is never accepted).  Returns the worst error /
    bound: with the format and e given, the error the kernel needed to arrive at its stored value (``needed_error``) over e;
    without them |got - ref| over the distance from ref to the accepted end on got's side."""
    got, ref = got.double(), ref.double().expand_as(lo)
    assert got.shape == lo.shape == hi.shape, (name, tuple(got.shape), tuple(lo.shape))
    bad = ~((got >= lo) & (got <= hi))
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        f = lambda t: float(t.reshape(-1)[i])
        raise cb.BoundError(f'{name}: {int(bad.sum())} / {got.numel()} outside the bound; first at flat index {i} of '
                            f'{tuple(got.shape)}: got {f(got):.9e}, ref {f(ref):.9e}, accepted [{f(lo):.9e}, {f(hi):.9e}]')
    fin = torch.isfinite(got) & torch.isfinite(ref) & torch.isfinite(lo) & torch.isfinite(hi)
    if e is not None:
        dev, side = needed_error(prec, got, ref), torch.as_tensor(e).double().expand_as(got)
    else:
        dev, side = (got - ref).abs(), torch.where(got >= ref, hi - ref, ref - lo)
    dev = torch.where(fin, dev, torch.zeros_like(got))
    ratio = torch.where(dev == 0, torch.zeros_like(dev), dev / side.clamp_min(1e-300))
    return float(ratio.max())


def _ordinal(prec, v):
    """Position of stored values in the format's order (+0 and -0 share one)."""
    b = bits(prec, v.float().to(STORE[prec])).to(torch.int64)
    mag_mask = 0x7fff if prec == 'bf16' else 0x7f
    mag, neg = b & mag_mask, (b & (mag_mask + 1)) != 0
    return torch.where(neg, -mag, mag)


def interval_widths(prec, lo, hi):
    """-> (share of intervals that hold two values of the format, number that hold more than two)."""
    n = _ordinal(prec, hi) - _ordinal(prec, lo) + 1
    assert bool((n >= 1).all())
    return float((n == 2).double().mean()), int((n > 2).sum())


# ---- max-pool --------------------------------------------------------------------------------------------------------------------
POOLS = ((3, 2, 1), (2, 2, 0))


def pool_ref(x, k, s, p):
    return F.max_pool2d(x.double(), k, s, p).float()


@functools.lru_cache(maxsize=None)
def pool_cases(prec):
    """[(name, x [N, C, H, W] values, ((k, s, p), ...))]"""
    out = []
    for name, shape, seed in (('odd', (2, C, 15, 21), 1), ('even', (1, C, 16, 22), 2)):
        out.append((name, random_values(prec, shape, seed), POOLS))
    out.append(('smaller_than_window', random_values(prec, (1, C, 2, 1), 3), ((3, 2, 1),)))
    out.append(('one_pixel', random_values(prec, (2, C, 1, 1), 4), ((3, 2, 1),)))
    out.append(('window_2x3', random_values(prec, (1, C, 2, 3), 5), POOLS))
    out.append(('all_negative', -random_values(prec, (1, C, 9, 11), 6).abs(), POOLS))
    x = -random_values(prec, (1, C, 9, 11), 7).abs()  # the maximum on the last row / column, which 2/2/0 drops at odd sizes
    top = 448. if prec == 'fp8' else 1000.
    x[:, ::2, -1, 3], x[:, 1::2, 4, -1] = top, top
    out.append(('max_on_last_row_and_column', x, POOLS))
    return out


def identity_values(prec):
    """[1, C, H, W] holding every finite pattern of the precision (fp8: code values, repeated to fill 64 x 2 x 2)."""
    if prec == 'fp8':
        v = e4m3_patterns()
        return torch.cat((v, v[:2])).view(1, C, 2, 2)
    v = bf16_patterns() if prec == 'bf16' else widened_patterns()
    return v.view(1, C, 30, 34)


# ---- input conversion ------------------------------------------------------------------------------------------------------------
FP8_INPUT_SCALES = (2.0 ** -9, 1. / 448.)  # a power of two, and the calibrated scale of a [0, 1] input (not one)


def input_ref(prec, src, scale=None):
    """-> the stored real channels [N, C, H, W] of the converted source (f32 or u8 NCHW)."""
    v = src.float() / 255. if src.dtype == torch.uint8 else src.float()
    if prec == 'fp8':
        v = v * torch.tensor(inv_scale(scale), dtype=torch.float32)
    return encode(prec, v)


@functools.lru_cache(maxsize=None)
def input_sources(channels, scale=None):
    """(f32 source, u8 source), [2, channels, 5, 7] in [0, 1], with exact rounding ties in front: bf16 midpoints (even and odd
    neighbours), e4m3 midpoints times the scale, 0, -0 and 1."""
    g = torch.Generator().manual_seed(20 + channels)
    x = torch.rand(2, channels, 5, 7, generator=g)
    j = torch.arange(12, dtype=torch.float32)
    special = torch.cat([torch.tensor([0., -0., 1.]), .5 + (j + .5) * 2.0 ** -8, .25 + (j + .5) * 2.0 ** -9])
    for c in range(channels):
        x[0, c].view(-1)[:special.numel()] = special
    if scale is not None:
        cv = e4m3_patterns()
        cv = cv[cv > 0].sort().values  # (the midpoint between 0 and the smallest code is half that code)
        cv = torch.cat((cv[:1] * 0, cv))
        mid = ((cv[1:] + cv[:-1]) / 2 * torch.tensor(scale, dtype=torch.float32))
        mid = mid[mid <= 1][::4][:35]
        for c in range(channels):
            x[1, c].view(-1)[:mid.numel()] = mid
    u8 = torch.randint(0, 256, (2, channels, 5, 7), generator=g, dtype=torch.uint8)
    u8[0, 0].view(-1)[:] = torch.arange(35, dtype=torch.uint8) * 7 + 10
    u8.view(-1)[-1], u8.view(-1)[0] = 255, 0
    return x, u8


def range_flag_sources():
    """[(name, source [2, 3, 4, 5], expected flag)]: the offending value is the very last element of the last image."""
    base = torch.zeros(2, 3, 4, 5)
    base.view(-1)[::3], base.view(-1)[1::3] = 1., -0.
    out = [('in_range_f32', base, 0), ('in_range_u8', torch.full((2, 3, 4, 5), 255, dtype=torch.uint8), 0)]
    for name, v in (('one_plus_ulp', float(np.nextafter(np.float32(1), np.float32(2)))), ('minus_ulp', -2.0 ** -23),
                    ('minus_min_normal', -2.0 ** -126), ('nan', math.nan)):
        x = base.clone()
        x.view(-1)[-1] = v
        out.append((name, x, 1))
    return out


def stem_ref(src):
    """The padded record of the stem fast path: bf16 [N][H + 6][W + 8][4], 3 zero rows / columns in front."""
    n, c, h, w = src.shape
    out = torch.zeros(n, h + 6, w + 8, 4, dtype=torch.bfloat16)
    out[:, 3:3 + h, 3:3 + w, :c] = nhwc(input_ref('bf16', src))
    return out


# ---- bilinear --------------------------------------------------------------------------------------------------------------------
def _axis(n_in, n_out):
    """Exact source coordinates of one axis: floor index, its neighbour, the weight of the neighbour and the coordinate -- rational
    arithmetic on integers, one float64 rounding of the final fraction."""
    o = torch.arange(n_out, dtype=torch.int64)
    num, den = ((2 * o + 1) * n_in - n_out).clamp_min(0), 2 * n_out  # f = num / den
    i0 = (num // den).clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, (num - i0 * den).double() / den, num.double() / den


def bilinear_ref(x, size):
    """float64 bilinear resize (align_corners=False) of x [N, C, H, W] from exact coordinates, with the per-pixel error allowance of
    the interval judge -> (ref, e)."""
    x = x.double()
    y0, y1, ly, fy = _axis(x.shape[2], size[0])
    x0, x1, lx, fx = _axis(x.shape[3], size[1])
    ly, lx = ly[:, None], lx[None, :]
    hy, hx = 1 - ly, 1 - lx

    def blend(v):
        r0, r1 = v[:, :, y0], v[:, :, y1]
        return hy * (hx * r0[..., x0] + lx * r0[..., x1]) + ly * (hx * r1[..., x0] + lx * r1[..., x1])

    ref = blend(x)
    gy = F.pad((x[:, :, 1:] - x[:, :, :-1]).abs(), (0, 0, 0, 1))
    gx = F.pad((x[..., 1:] - x[..., :-1]).abs(), (0, 1, 0, 0))
    gy, gx = F.max_pool2d(gy, 3, 1, 1), F.max_pool2d(gx, 3, 1, 1)
    dy, dx = 6 * U * fy.clamp_min(1.)[:, None], 6 * U * fx.clamp_min(1.)[None, :]
    e = dy * gy[:, :, y0][..., x0] + dx * gx[:, :, y0][..., x0] + 6 * U * blend(x.abs())
    return ref, e


def is_dyadic(n_in, n_out):
    return n_out % n_in == 0 and (n_out // n_in) & (n_out // n_in - 1) == 0


# (source size, output size, the max-pool chain that produces the source from the output size in a plan | None: bf16 entry only)
RESIZE_CASES = (((19, 25), (75, 101), ((3, 2, 1), (2, 2, 0))),
                ((10, 13), (75, 101), ((3, 2, 1), (3, 2, 1), (3, 2, 1))),
                ((38, 51), (75, 101), ((3, 2, 1),)),
                ((3, 1), (12, 4), ((4, 4, 0),)),
                ((5, 3), (33, 47), None),
                ((1, 7), (5, 13), None),
                ((76, 102), (75, 101), None))
DYADIC_CASES = (((6, 10), (6, 10), None),  # same size: a plan aliases it, no kernel runs
                ((6, 10), (12, 20), ((2, 2, 0),)),
                ((5, 7), (20, 28), ((2, 2, 0), (2, 2, 0))))


def chain_size(size, chain):
    for k, s, p in chain:
        size = tuple((v + 2 * p - k) // s + 1 for v in size)
    return size


def chain_ref(x, chain):
    for k, s, p in chain:
        x = pool_ref(x, k, s, p)
    return x


def resize_name(case):
    return '{}x{}->{}x{}'.format(*case[0], *case[1])


def expand(src, chain, size):
    """A plan input of ``size`` whose max-pool chain is exactly ``src``: every source value sits at the first tap that only its own
    window holds (stride * i), everything else is the smallest source value."""
    sizes = [tuple(size)]
    for c in chain:
        sizes.append(chain_size(sizes[-1], (c,)))
    assert sizes[-1] == tuple(src.shape[2:]), (sizes, src.shape)
    x = src
    for (k, s, p), sz in zip(reversed(chain), reversed(sizes[:-1])):
        y = torch.full(tuple(src.shape[:2]) + sz, float(src.min()))
        y[:, :, ::s, ::s][:, :, :x.shape[2], :x.shape[3]] = x
        x = y
    return x


def _two_valued(prec, src, size):
    ref, e = bilinear_ref(src, size)
    lo, hi = interval(prec, ref, e)
    return _ordinal(prec, hi) != _ordinal(prec, lo)


@functools.lru_cache(maxsize=None)
def resize_source(prec, case, direct, kind):
    """-> (plan input or None, source of the resize): values of the precision (fp8: code values).  kind 'interval': positive in
    [0.5, 2]; 'grid': k / 16; 'bicubic': both signs.  direct: the bf16 entry point reads the source itself; else the source is
    the max-pool chain of the plan's input (``expand``).

    Where an axis of an interval case has a dyadic ratio (3x1 -> 12x4: x4 in y) the blend is exact there and a tenth of random
    sources land on a rounding tie of the output format, whose interval holds both neighbours whatever e is.  Ties are the exact
    family's job: the maps (n, c) with such an output are drawn again until none is left."""
    src, size, chain = case
    shape = (2, C) + src
    seed = 100 + 7 * RESIZE_CASES.index(case) if case in RESIZE_CASES else 200 + DYADIC_CASES.index(case)
    if kind == 'grid':
        x = grid_values(shape, seed)
    elif kind == 'interval':
        x = random_values(prec, shape, seed, .5, 2.)
        if prec != 'fp32' and (is_dyadic(src[0], size[0]) or is_dyadic(src[1], size[1])):
            for attempt in range(1, 200):
                again = _two_valued(prec, x, size).flatten(2).any(2)
                if not bool(again.any()):
                    break
                x = torch.where(again[:, :, None, None], random_values(prec, shape, seed + 1000 * attempt, .5, 2.), x)
    else:
        x = random_values(prec, shape, seed)
    return (None if direct else expand(x, chain, size)), x


def bicubic_ref(x, size):
    return F.interpolate(x.double(), size, mode='bicubic', align_corners=False)


def bicubic_error(x, size, got):
    """Largest |got - float64 reference| in units of 2^-23 max|x|."""
    return float((got.double() - bicubic_ref(x, size)).abs().max() / (2 * U * x.abs().max().double()))


def bicubic_bound(prec, case):
    return BICUBIC_MARGIN * measured()['bicubic_cases'][f'{prec}_{resize_name(case)}']


def bicubic_interval(prec, case, x):
    ref = bicubic_ref(x, case[1])
    return ref, interval(prec, ref, bicubic_bound(prec, case) * 2 * U * float(x.abs().max()))


# ---- activations -----------------------------------------------------------------------------------------------------------------
ACTS = {'relu': _lib.ACT_RELU, 'sigmoid': _lib.ACT_SIGMOID, 'leaky_relu': _lib.ACT_LEAKY_RELU, 'silu': _lib.ACT_SILU,
        'gelu': _lib.ACT_GELU, 'elu': _lib.ACT_ELU, 'tanh': _lib.ACT_TANH, 'hardswish': _lib.ACT_HARDSWISH, 'mish': _lib.ACT_MISH,
        'selu': _lib.ACT_SELU, 'softplus': _lib.ACT_SOFTPLUS}
LIB_FUNCTIONS = ('exp', 'erf', 'tanh', 'log1p', 'expm1')
SELU_L, SELU_A = float(np.float32(1.0507009873554804934193349852946)), float(np.float32(1.6732632423543772848170429916717))
LEAKY, RSQRT2 = float(np.float32(0.01)), float(np.float32(0.70710678118654752440))
FP8_ACT_SCALES = ((2.0 ** -4, 2.0 ** -5), (0.0371, 0.0119), (0.21, 0.6))  # (in_scale, out scale), in != out


def act_f32(kind, x):
    """The formula in torch-CPU fp32, operation by operation as act_apply writes it (the stand-in for the kernels)."""
    x = x.float()
    one = torch.ones((), dtype=torch.float32)
    sp = lambda: torch.where(x > 20, x, torch.log1p(torch.exp(torch.where(x > 20, torch.zeros_like(x), x))))
    if kind == 'relu':
        return torch.maximum(x, torch.zeros_like(x))
    if kind == 'sigmoid':
        return one / (one + torch.exp(-x))
    if kind == 'leaky_relu':
        return torch.where(x > 0, x, torch.tensor(LEAKY, dtype=torch.float32) * x)
    if kind == 'silu':
        return x / (one + torch.exp(-x))
    if kind == 'gelu':
        return .5 * x * (one + torch.erf(x * torch.tensor(RSQRT2, dtype=torch.float32)))
    if kind == 'elu':
        return torch.where(x > 0, x, torch.expm1(x))
    if kind == 'tanh':
        return torch.tanh(x)
    if kind == 'hardswish':
        return x * torch.clamp(x + 3., 0., 6.) / 6.
    if kind == 'mish':
        return x * torch.tanh(sp())
    if kind == 'selu':
        return torch.tensor(SELU_L, dtype=torch.float32) * torch.where(x > 0, x, torch.tensor(SELU_A, dtype=torch.float32) * torch.expm1(x))
    assert kind == 'softplus', kind
    return sp()


def lib_arguments(x):
    """The fp32 arguments the formulas hand to each library function for the inputs x."""
    x = x.float().reshape(-1)
    small = x[x <= 20]
    sp = torch.log1p(torch.exp(small))
    return {'exp': torch.cat((-x, small)), 'erf': x * torch.tensor(RSQRT2, dtype=torch.float32), 'tanh': torch.cat((x, sp, x[x > 20])),
            'log1p': torch.exp(small), 'expm1': x[x <= 0]}


def lib_error_ulps(fn, args):
    """Worst |torch-CPU fp32 fn - float64 fn| in fp32 ulps of the true value, over the arguments whose true result is a normal fp32."""
    a = args.float()
    true = getattr(torch, fn)(a.double())
    ok = (true.abs() >= 2.0 ** -126) & (true.abs() <= F32_MAX)
    ulp = torch.exp2(torch.floor(torch.log2(true[ok].abs())) - 23)
    return float(((getattr(torch, fn)(a)[ok].double() - true[ok]).abs() / ulp).max())


def lib_allowance(ulps=None):
    """{function: L} from the (committed) measurement: L = 2 x worst ulps + 1."""
    ulps = measured()['lib_ulps'] if ulps is None else ulps
    return {f: 2. * ulps[f] + 1. for f in LIB_FUNCTIONS}


def act_ref(kind, x, L=None):
    """float64 reference of the fp32 formula at the fp32 arguments x and its error allowance before the output rounding -> (ref, e)."""
    L = lib_allowance() if L is None else L
    x = x.double()
    ax, zero = x.abs(), torch.zeros_like(x)
    q, p = torch.sigmoid(-x), torch.sigmoid(x)
    xs = torch.where(x > 20, zero, x)
    sp = torch.where(x > 20, x, torch.log1p(torch.exp(xs)))
    e_sp = torch.where(x > 20, torch.exp(-x), 2 * L['exp'] * U * p + 2 * L['log1p'] * U * sp)
    floor = ACT_FLOOR
    if kind == 'relu':
        ref, e, floor = x.clamp_min(0.), zero, 0.
    elif kind == 'leaky_relu':
        ref = torch.where(x > 0, x, LEAKY * x)
        e, floor = torch.where(x > 0, zero, U * ref.abs()), 0.
    elif kind == 'sigmoid':
        ref = p
        e = (2 * L['exp'] * q + 2) * U * ref
    elif kind == 'silu':
        ref = x * p
        e = (2 * L['exp'] * q + 2) * U * ref.abs()
    elif kind == 'gelu':
        a = x * math.sqrt(.5)
        erf = torch.erf(a)
        ref = .5 * x * (1 + erf)
        d_erf = 2 * L['erf'] * U * erf.abs() + 2 * U * a.abs() * (2 / math.sqrt(math.pi)) * torch.exp(-a * a)
        e = .5 * ax * (d_erf + 2 * U * (1 + erf.abs()))
    elif kind == 'elu':
        ref = torch.where(x > 0, x, torch.expm1(x))
        e = torch.where(x > 0, zero, 2 * L['expm1'] * U * ref.abs())
    elif kind == 'selu':
        ref = SELU_L * torch.where(x > 0, x, SELU_A * torch.expm1(x))
        e = torch.where(x > 0, U * ref.abs(), (2 * L['expm1'] + 2) * U * ref.abs())
    elif kind == 'tanh':
        ref = torch.tanh(x)
        e = 2 * L['tanh'] * U * ref.abs()
    elif kind == 'hardswish':
        c = (x + 3).clamp(0., 6.)
        prod = x * c
        inside = (x + 3 > 0) & (x + 3 < 6)
        ref = torch.where(prod.abs() > F32_MAX * (1 + U / 2), torch.sign(prod) * math.inf, prod / 6)
        e = torch.where(torch.isinf(ref), zero, torch.where(inside, ax * U * (x + 3).abs() / 6, zero) + 2 * U * (prod / 6).abs())
        floor = 0.
    elif kind == 'mish':
        th = torch.tanh(sp)
        ref = x * th
        e = ax * ((1 - th * th) * e_sp + 2 * L['tanh'] * U * th) + U * ref.abs()
    else:
        assert kind == 'softplus', kind
        ref, e = sp, e_sp
    return ref, e + floor


def act_inputs(prec, pair=None):
    """fp32 arguments of the activation cases [1 | 2, C, H, W] -> (plan input, arguments): bf16 every finite pattern, fp32 those widened
    with random low bits, fp8 every finite code times in_scale (the IEEE fp32 product the kernel forms)."""
    if prec == 'fp8':
        cv = identity_values('fp8')
        x = cv * torch.tensor(pair[0], dtype=torch.float32)
        return x, x
    x = identity_values('bf16')
    if prec == 'fp32':  # (the unwidened patterns too: the knees 0, +-3 and 20 themselves)
        x = torch.cat((x, identity_values('fp32')))
    return x, x


def act_interval(prec, kind, x, pair=None, L=None):
    """-> (ref, lo, hi, e) in the units the destination stores (fp8: code units of the destination's scale, the product's rounding
    included in e)."""
    ref, e = act_ref(kind, x, L)
    if prec == 'fp8':
        inv = inv_scale(pair[1])
        lo, hi = interval(prec, ref, e, inv)
        return (ref * inv).clamp(-448., 448.), lo, hi, e * inv + (ref * inv).abs() * U
    return (ref,) + interval(prec, ref, e) + (e,)


def act_standin(prec, kind, x, pair=None):
    y = act_f32(kind, x)
    if prec == 'fp8':
        y = y * torch.tensor(inv_scale(pair[1]), dtype=torch.float32)
    return encode(prec, y)


# ---- grid-stride laps ------------------------------------------------------------------------------------------------------------
LAP_ITEMS = 256 * 16 * 256  # thread items of one lap of the capped grids (8 bf16 / e4m3 values per item)
LAP_SHAPE = (2, C, 260, 260)  # 1 081 600 items of 8 values: a second, ragged lap; 8 652 800 elements


@functools.lru_cache(maxsize=None)
def lap_values(prec):
    """Values of the lap cases: a short random sequence of the precision's values tiled over the tensor with a prime period, so a
    shifted or dropped item shows; in [0, 1] so the fp8 / bf16 input conversions hold them too (fp8: scale 2^-9, code values)."""
    g = torch.Generator().manual_seed(31)
    if prec == 'fp8':
        cv = e4m3_patterns()
        cv = cv[cv > 0]
        seq = cv[torch.randint(0, cv.numel(), (8191,), generator=g)]
    else:
        seq = encode('bf16', torch.rand(8191, generator=g) * .9 + .05).float()
    n = math.prod(LAP_SHAPE)
    return seq.repeat(-(-n // 8191))[:n].view(LAP_SHAPE)


# ---- plans -----------------------------------------------------------------------------------------------------------------------
class Plan:
    """Descriptor arrays of a conv-free plan: tensor 0 is the input op's destination, op i + 1 writes tensor i + 1.

    ops: ('pool', k, s, p) | ('resize', mode) | ('act', kind); each reads ``src`` (default: the tensor before it).  scales: the
    fp8 scale of every tensor."""

    def __init__(self, prec, in_channels, ops, scales=None, channels=None):
        self.prec, self.in_channels = prec, in_channels
        channels = (C if prec == 'fp8' else 32 * -(-in_channels // 32)) if channels is None else channels
        nt = len(ops) + 1
        scales = [1.] * nt if scales is None else list(scales)
        self.tensors = (_lib.TensorDesc * nt)()
        for i in range(nt):
            self.tensors[i].channels, self.tensors[i].down, self.tensors[i].scale = channels, 1, scales[i]
        self.ops = (_lib.OpDesc * nt)()
        for o in self.ops:
            o.src0 = o.src1 = o.res = o.dst = -1
            o.weight_offset = o.bias_offset = o.fuse_weight_offset = o.fuse_bias_offset = -1
            o.mult_offset = -1
        self.ops[0].op, self.ops[0].dst, self.ops[0].in_channels = _lib.OP_INPUT, 0, in_channels
        for i, spec in enumerate(ops, 1):
            o = self.ops[i]
            o.src0, o.dst = i - 1, i
            if spec[0] == 'pool':
                o.op, o.kh, o.kw, o.stride, o.pad = _lib.OP_MAXPOOL, spec[1], spec[1], spec[2], spec[3]
            elif spec[0] == 'resize':
                o.op, o.act = _lib.OP_BILINEAR, spec[1]
            else:
                o.op, o.act = _lib.OP_ACT, ACTS[spec[1]]
        self.channels = channels


def pool_ops(chain):
    return [('pool',) + tuple(c) for c in chain]
