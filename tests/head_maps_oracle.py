"""float64 references, error bounds, cases and judges for the fp32 head-map kernels of csrc/decode_nms.hip: class_scores_kernel,
certainty_kernel, gather_channels_kernel, the bicubic branch of resize_f32_kernel and the fused decode at its loop edges.

Plain numpy / torch-CPU; nothing here touches the GPU.  ``tests/test_head_maps.py`` runs every judge with torch-CPU fp32 standing
in for the kernels (so each bound is shown to be satisfiable) and measures the two quantities the bounds leave open;
``tests/test_gpu_head_maps.py`` runs the same judges on the kernels' results.

Softmax bound.  With d_c = fl(x_c - max x) the kernel computes p_c = fl(e_c / S), e_c = expf(d_c), S = fl(sum_c e_c).  Relative to
the exact softmax, in units of u = 2^-23:
  |d_c| / 2   the rounded subtraction: d_c (1 + delta), |delta| <= u / 2, gives exp(d_c) a factor exp(d_c delta)
  E           expf itself, numerator and (as the weighted mean over the terms) denominator
  C - 1       the additions of S and the part of the terms' own subtraction error that reaches S (e^d |d| <= 1 / e per term)
  + 3         the division and slack
  => (|d_c| / 2 + E + C + 2) u, plus an absolute floor of 2^-126 (results below the normal range).
E = 2 E_measured + 1 where E_measured is the worst error in ulps of torch-CPU fp32 exp on the cases' own arguments (the device's expf
is another libm than the CPU's: twice its error and one ulp more are allowed).
"""
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -23
FLOOR = 2.0 ** -126
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = os.path.join(ROOT, 'tests', 'golden', 'head_maps_measured.json')
BICUBIC_MARGIN = 4.  # GPU bound = 4 x the error of torch-CPU fp32 bicubic (FMA contraction, order of the weight polynomials)
N, H, W = 3, 17, 23  # 391 pixels per image = two 256-thread blocks with a ragged tail; 1173 pixels: block borders inside images


def measured():
    with open(MEASURED) as f:
        return json.load(f)


def exp_allowance(e_measured=None):
    """E of the softmax bound from the (committed) measurement."""
    return 2. * (measured()['exp_ulps'] if e_measured is None else e_measured) + 1.


def bits(t):
    """int32 view of an fp32 tensor (byte-for-byte comparisons: -0.0 != 0.0, and no NaN surprises)."""
    return torch.as_tensor(t).detach().cpu().contiguous().view(torch.int32)


# ---- 1. class scores ---------------------------------------------------------------------------------------------------------
def exp_arguments(logits):
    """The fp32 arguments x_c - max_c x that the softmax of ``logits`` hands to exp."""
    x = logits.float()
    return x - x.amax(1, keepdim=True)


def exp_error_ulps(args):
    """Worst |torch-CPU fp32 exp - float64 exp| in fp32 ulps of the true value, over the arguments whose result is a normal number."""
    a = args.reshape(-1).float()
    true = torch.exp(a.double())
    ok = true >= FLOOR
    ulp = torch.exp2(torch.floor(torch.log2(true[ok])) - 23)
    return float(((torch.exp(a)[ok].double() - true[ok]).abs() / ulp).max())


def _bounds_maps(g, kind, which, shape):
    """lower / upper maps [N,1,h,w] (or None): 0/1 masks (the slide loop's) or fractional values in [0.2, 0.8]."""
    def one():
        r = torch.rand(shape, generator=g)
        return (r > .3).float() if kind == 'mask' else (.2 + .6 * r).float()
    lo = one() if which in ('lower', 'both') else None
    up = one() if which in ('upper', 'both') else None
    if kind == 'mask' and lo is not None:
        lo = 1 - lo  # mostly 0: a lower bound of 1 forces class 0
    return lo, up


BOUND_KINDS = (('none', None),) + tuple((w, k) for k in ('mask', 'frac') for w in ('lower', 'upper', 'both'))


@functools.lru_cache(maxsize=None)
def class_cases(C, scale, shape=(N, H, W)):
    """[(name, logits, lower, upper)] for one channel count and logit scale: no bounds, one of them, both; masks and fractions."""
    n, h, w = shape
    g = torch.Generator().manual_seed(0)
    out = []
    for which, kind in BOUND_KINDS:
        logits = torch.randn(n, C, h, w, generator=g) * scale
        lo, up = _bounds_maps(g, kind, which, (n, 1, h, w)) if kind else (None, None)
        out.append((f'C{C}_s{scale}_{which}_{kind}', logits, lo, up))
    return out


CLASS_C = (2, 3, 4, 7, 33)
CLASS_SCALES = (.5, 3, 30)


@functools.lru_cache(maxsize=None)
def tie_case():
    """Designed ties, C = 4 on 3 x 17 x 23.  Returns (logits, lower, upper, {name: (mask [N,h,w], expected class)})."""
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(N, 4, H, W, generator=g) * 3
    lower, upper = torch.zeros(N, 1, H, W), torch.ones(N, 1, H, W)
    region = torch.zeros(N, H, W, dtype=torch.long)
    region[0, :, :6] = 1   # channels 1 and 2 share the largest logit: class 1
    region[0, :, 6:12] = 2  # channels 0, 2, 3 share it: class 0
    region[0, :, 12:18] = 3  # channels 2 and 3: class 2
    region[1, :8] = 4  # upper = 0: every channel clamps to 0, class 0
    region[1, 8:] = 5  # lower = 1: every channel is 1, class 0
    region[2, :9] = 6  # fractional upper below the top two probabilities (channels 2 > 1 > rest): first clamped index, class 1
    top = logits.amax(1) + 1
    for r, chans in ((1, (1, 2)), (2, (0, 2, 3)), (3, (2, 3))):
        for c in chans:
            logits[:, c] = torch.where(region == r, top, logits[:, c])
    upper[:, 0][region == 4] = 0.
    lower[:, 0][region == 5] = 1.
    m = region == 6
    for c, v in ((0, -4.), (1, 1.), (2, 1.5), (3, -4.)):  # p = (.0016, .377, .621, .0016)
        logits[:, c] = torch.where(m, torch.full_like(top, v), logits[:, c])
    upper[:, 0][m] = .3
    expected = {'tie_1_2': (region == 1, 1), 'tie_0_2_3': (region == 2, 0), 'tie_2_3': (region == 3, 2),
                'upper_0': (region == 4, 0), 'lower_1': (region == 5, 0), 'upper_frac_tie': (region == 6, 1)}
    return logits, lower, upper, expected


def class_reference(logits, lower=None, upper=None, E=None):
    """float64 softmax + bounds + first argmax with the per-probability tolerance and the pixels whose class it decides.

    A probability's tolerance is ``tol = bound * p + 2^-126``.  Each channel gets the interval [p - 2 tol, p + 2 tol] (twice the
    bound), clipped to [0, 1] (exp(0) = 1 is exact and S >= 1, so no implementation leaves it) and pushed through min(., ub),
    max(., lb).  The class c* of the float64 argmax is decided when every earlier channel's interval lies strictly below c*'s and
    every later one's not above it.  A channel whose logit equals an earlier channel's exactly computes the same bits and loses the
    tie by index: it takes no part.  ``pinned``: interval collapsed onto a bound, the value must equal that bound exactly."""
    E = exp_allowance() if E is None else E
    x = logits.double()
    n, C, h, w = x.shape
    d = (x - x.amax(1, keepdim=True)).abs()
    p = torch.softmax(x, 1)
    tol = (d / 2 + E + C + 2) * U * p + FLOOR
    ub = torch.full((n, 1, h, w), np.inf, dtype=torch.float64) if upper is None else upper.double()
    lb = torch.full((n, 1, h, w), -np.inf, dtype=torch.float64) if lower is None else lower.double()
    clamp = lambda v: torch.maximum(torch.minimum(v, ub), lb)
    q = clamp(p)
    lo, hi = clamp((p - 2 * tol).clamp(0, 1)), clamp((p + 2 * tol).clamp(0, 1))
    dup = torch.zeros_like(x, dtype=torch.bool)
    for c in range(1, C):
        dup[:, c] = (x[:, :c] == x[:, c:c + 1]).any(1)
    cls = torch.argmax(torch.where(dup, torch.full_like(q, -np.inf), q), 1)  # first maximum
    idx = torch.arange(C).view(1, C, 1, 1)
    star = cls[:, None]
    lo_star = lo.gather(1, star)
    beaten = torch.where(idx < star, hi < lo_star, hi <= lo_star) | (idx == star) | dup
    return dict(p=p, q=q, tol=tol, cls=cls, decided=beaten.all(1), pinned=lo == hi, pinned_value=lo, C=C)


def class_f32_standin(logits, lower=None, upper=None):
    """What the reference model does in fp32 on the CPU (softmax, bounds, argmax): stands in for the kernel in the CPU test."""
    p = torch.softmax(logits.float(), 1)
    if upper is not None:
        p = torch.minimum(p, upper.float())
    if lower is not None:
        p = torch.maximum(p, lower.float())
    cls = torch.argmax(p, 1)
    return p.gather(1, cls[:, None]), cls.to(torch.int32), (cls > 0).float()[:, None], p


def judge_class_scores(sel, cls, fg, probs, ref, what, cap=.01):
    """Asserts one class_scores result (with probabilities) against ``class_reference``; returns (worst error / bound, undecided
    fraction)."""
    sel, cls, fg, probs = (torch.as_tensor(t).detach().cpu() for t in (sel, cls, fg, probs))
    err = (probs.double() - ref['q']).abs()
    ratio = float((err / ref['tol']).max())
    undecided = 1. - float(ref['decided'].double().mean())
    print(f'{what}: worst error / bound = {ratio:.3f}, undecided = {100 * undecided:.3f} %')
    assert ratio <= 1., f'{what}: probability off by {ratio:.3f} x its bound'
    pin = ref['pinned']
    assert torch.equal(probs[pin].double(), ref['pinned_value'][pin]), f'{what}: a clamped probability is not the bound itself'
    assert undecided <= cap, f'{what}: {100 * undecided:.2f} % of the pixels are undecided'
    dec = ref['decided']
    assert torch.equal(cls.long()[dec], ref['cls'][dec]), f'{what}: wrong class on {int((cls.long() != ref["cls"])[dec].sum())} decided pixels'
    assert torch.equal(bits(fg), bits((cls > 0).float()[:, None])), f'{what}: foreground is not (class > 0)'
    assert torch.equal(bits(sel), bits(probs.gather(1, cls.long()[:, None]))), f'{what}: selected score is not probs[class]'
    assert bool((probs.gather(1, cls.long()[:, None]) >= probs).all()), f'{what}: class is not an argmax of the returned probabilities'
    first = torch.argmax(probs, 1)  # torch: first maximal index
    assert torch.equal(first, cls.long()), f'{what}: class is not the FIRST argmax of the returned probabilities'
    return ratio, undecided


# ---- 2. certainty mask -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_uncertainty(C, shape=(N, H, W), seed=2):
    """Uncertainty on the grid k / 8: every partial sum is exact in fp32."""
    n, h, w = shape
    return torch.randint(0, 9, (n, C, h, w), generator=torch.Generator().manual_seed(seed + C)).float() / 8


def grid_on_limit_cap(C, limit=.5):
    """Cap on the undecided share of a k / 8 grid case: the exact probability that C uniform draws from {0..8} sum to 8 C limit
    (only those pixels are undecided), plus four standard deviations of that share over the N H W pixels."""
    pmf = np.ones(1)
    for _ in range(C):
        pmf = np.convolve(pmf, np.full(9, 1 / 9))
    q = float(pmf[int(round(8 * C * limit))])
    return q + 4 * np.sqrt(q * (1 - q) / (N * H * W))


@functools.lru_cache(maxsize=None)
def certainty_scores(shape=(N, H, W), seed=3):
    """Scores whose bytes matter: random values of both signs, -0.0, 0.0, +-inf and -1 itself."""
    n, h, w = shape
    s = torch.randn(n, 1, h, w, generator=torch.Generator().manual_seed(seed))
    flat = s.view(-1)
    for i, v in enumerate((-0., 0., float('inf'), -float('inf'), -1., 1.)):
        flat[i::97][:3] = v
    return s


def certainty_reference(scores, unc, certainty_thresh, exact=False):
    """float64 mean against the fp32 limit the wrapper passes; decided where |mean - limit| > C 2^-23 max(1, limit) (``exact``:
    everywhere -- the caller knows the fp32 mean has no rounding)."""
    C = unc.shape[1]
    limit = float(np.float32(1 - certainty_thresh))
    mean = unc.double().mean(1, keepdim=True)
    decided = torch.ones_like(mean, dtype=torch.bool) if exact else (mean - limit).abs() > C * U * max(1., limit)
    expected = torch.where(mean < limit, scores.float(), torch.full_like(scores.float(), -1.))
    return dict(mean=mean, limit=limit, decided=decided, expected=expected, scores=scores.float())


def certainty_f32_standin(scores, unc, certainty_thresh):
    return torch.where(unc.float().mean(1, keepdim=True) < (1 - certainty_thresh), scores.float(), torch.full_like(scores.float(), -1.))


def judge_certainty(out, ref, what, cap):
    """Byte-for-byte on the decided pixels; an undecided pixel holds its score or -1.  Returns the undecided fraction."""
    got, exp, own = bits(out), bits(ref['expected']), bits(ref['scores'])
    dec = ref['decided']
    undecided = 1. - float(dec.double().mean())
    on_limit = float((ref['mean'] == ref['limit']).double().mean())
    print(f'{what}: undecided = {100 * undecided:.3f} %, mean == limit on {100 * on_limit:.2f} %')
    assert undecided <= cap, f'{what}: {100 * undecided:.2f} % undecided'
    assert torch.equal(got[dec], exp[dec]), f'{what}: {int((got != exp)[dec].sum())} decided pixels differ'
    assert bool(((got == own) | (got == bits(torch.tensor(-1.)))).all()), f'{what}: a value that is neither the score nor -1'
    return undecided


# ---- 3. gather -----------------------------------------------------------------------------------------------------------------
def gather_indices(P, shape=(N, H, W), seed=4):
    """P linear (b, y, x) indices: first and last pixel of the first and last image, duplicates, then random ones (unsorted)."""
    n, h, w = shape
    hw = h * w
    fixed = [0, hw - 1, (n - 1) * hw, n * hw - 1, 0, n * hw - 1, hw - 1, hw]
    rnd = torch.randint(0, n * hw, (max(P, 0),), generator=torch.Generator().manual_seed(seed + P)).tolist()
    idx = ([n * hw - 1] if P == 1 else (fixed + rnd)[:P])
    return torch.tensor(idx, dtype=torch.int32)


def gather_reference(maps, indices):
    n, C, h, w = maps.shape
    i = indices.long()
    b, rem = i // (h * w), i % (h * w)
    return maps[b, :, rem // w, rem % w].reshape(-1, C)


# ---- 4. bicubic ----------------------------------------------------------------------------------------------------------------
BICUBIC_CASES = (((1, 1, 1, 1), (4, 5)),  # every tap clamps
                 ((2, 2, 3, 2), (7, 9)),
                 ((1, 3, 19, 26), (75, 101)),
                 ((2, 2, 76, 102), (75, 101)),  # downscale
                 ((1, 1, 9, 9), (9, 31)))  # one axis unchanged


@functools.lru_cache(maxsize=None)
def bicubic_input(i):
    return torch.randn(BICUBIC_CASES[i][0], generator=torch.Generator().manual_seed(10 + i))


@functools.lru_cache(maxsize=None)
def bicubic_reference(i):
    return F.interpolate(bicubic_input(i).double(), BICUBIC_CASES[i][1], mode='bicubic', align_corners=False)


def bicubic_error(i, got):
    """Largest |got - float64 reference| of case i in units of 2^-23 max|input|."""
    got = torch.as_tensor(got).detach().cpu()
    assert got.shape == bicubic_reference(i).shape and got.dtype == torch.float32
    return float((got.double() - bicubic_reference(i)).abs().max() / (U * bicubic_input(i).abs().max().double()))


def bicubic_f32_standin(i):
    return F.interpolate(bicubic_input(i), BICUBIC_CASES[i][1], mode='bicubic', align_corners=False)


def bicubic_name(i):
    return '{}->{}'.format(*map(list, BICUBIC_CASES[i]))


def bicubic_bound(i):
    """Allowed ``bicubic_error`` of the kernel on case i: 4 x that of torch-CPU fp32 on the same case (committed measurement; fp32
    source coordinates make it grow with the map's size, so each case has its own)."""
    return BICUBIC_MARGIN * measured()['bicubic_cases'][bicubic_name(i)]


# ---- 5. fused decode -----------------------------------------------------------------------------------------------------------
DECODE_CASES = {
    # n, (h, w), (H, W), order, order_total, samples, buckets, iterations, offsets
    'A_max_coef': dict(n=2, hw=(17, 23), HW=(50, 70), order=64, total=64, samples=129, buckets=1, iterations=2, offsets=True),
    'B_200_samples_buckets': dict(n=3, hw=(9, 11), HW=(36, 44), order=5, total=8, samples=200, buckets=4, iterations=3, offsets=True),
    'C_one_sample': dict(n=1, hw=(5, 7), HW=(5, 7), order=1, total=6, samples=1, buckets=2, iterations=1, offsets=False),
    'D_65_samples_buckets': dict(n=2, hw=(17, 23), HW=(51, 69), order=6, total=6, samples=65, buckets=3, iterations=4, offsets=True),
    'D_no_refinement': dict(n=2, hw=(17, 23), HW=(51, 69), order=6, total=6, samples=65, buckets=1, iterations=0, offsets=True),
}
DECODE_KEYS = ('contours', 'contour_proposals', 'boxes', 'scores', 'locations', 'fourier')
DECODE_THRESH = .5


@functools.lru_cache(maxsize=None)
def decode_inputs(name):
    """Synthetic head maps of one case: scores uniform (half the pixels are proposals), Fourier maps randn * 4 / (k + 1) per order
    k, refinement uniform in +-3, offsets randint(-50, 5000)."""
    c = DECODE_CASES[name]
    n, (h, w), (H, W_) = c['n'], c['hw'], c['HW']
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    scores = torch.rand(n, 1, h, w, generator=g)
    loc = torch.randn(n, 2, h, w, generator=g)
    amp = (4. / (torch.arange(c['total']) + 1)).repeat_interleave(4).view(1, -1, 1, 1)
    fourier = torch.randn(n, 4 * c['total'], h, w, generator=g) * amp
    ref = (torch.rand(n, 2 * c['buckets'], H, W_, generator=g) * 2 - 1) * 3 if c['iterations'] > 0 else None
    offsets = torch.randint(-50, 5000, (n, 2), generator=g) if c['offsets'] else None
    return dict(scores=scores, locations=loc, fourier=fourier, refinement=ref, offsets=offsets)


@functools.lru_cache(maxsize=None)
def decode_reference(name):
    """The CPU restatement's flat result of one case (computed once): {key: [P, ...]} + 'b' + 'counts'."""
    import cpn_oracle as orc
    c, t = DECODE_CASES[name], decode_inputs(name)
    exp = orc.cpn_postprocess(t['scores'], t['locations'], t['refinement'], t['fourier'], input_size=c['HW'], order=c['order'],
                              samples=c['samples'], score_thresh=DECODE_THRESH, refinement_iterations=c['iterations'], nms=False,
                              offsets=None if t['offsets'] is None else t['offsets'].numpy(), scores_are_probabilities=True,
                              refinement_buckets=c['buckets'])
    counts = [len(s) for s in exp['scores']]
    out = {k: np.concatenate(exp[k]) for k in DECODE_KEYS}
    out['b'] = np.repeat(np.arange(c['n'], dtype=np.int32), counts)
    out['counts'] = counts
    return out


# ---- 6. the chain the model runs ---------------------------------------------------------------------------------------------
CHAIN = dict(order=3, samples=16, iterations=2, HW=(2 * H, 2 * W), certainty_thresh=.5)


@functools.lru_cache(maxsize=None)
def chain_inputs():
    """C = 4 logits on the grid 1/4 (two probabilities are equal or differ by a factor e^(1/4): every pixel decided or an exact
    tie), grid uncertainty, a 0/1 upper bound at map size."""
    g = torch.Generator().manual_seed(6)
    logits = torch.randint(-8, 9, (N, 4, H, W), generator=g).float() / 4
    t = dict(logits=logits, uncertainty=grid_uncertainty(4), upper=(torch.rand(N, 1, H, W, generator=g) > .25).float(),
             locations=torch.randn(N, 2, H, W, generator=g), fourier=torch.randn(N, 4 * CHAIN['order'], H, W, generator=g) * 2,
             refinement=(torch.rand(N, 2, *CHAIN['HW'], generator=g) * 2 - 1) * 3)
    return t


@functools.lru_cache(maxsize=None)
def chain_reference():
    import cpn_oracle as orc
    t = chain_inputs()
    exp = orc.cpn_postprocess(t['logits'], t['locations'], t['refinement'], t['fourier'], input_size=CHAIN['HW'],
                              order=CHAIN['order'], samples=CHAIN['samples'], refinement_iterations=CHAIN['iterations'], nms=False,
                              uncertainty=t['uncertainty'], certainty_thresh=CHAIN['certainty_thresh'],
                              scores_upper_bound=t['upper'])
    counts = [len(s) for s in exp['scores']]
    out = {k: np.concatenate(exp[k]) for k in DECODE_KEYS + ('classes', 'box_uncertainties')}
    out['counts'] = counts
    return out
