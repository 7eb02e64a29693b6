"""The fp32 head-map kernels of csrc/decode_nms.hip on their own, at their edges: class_scores_kernel, certainty_kernel,
gather_channels_kernel, the bicubic branch of resize_f32_kernel, and decode_kernel<false / true> where its loops wrap (more than 64
samples, more than 64 coefficients, the coefficient limit, bucketed refinement, a non-integer scale, a ragged last block).

References, bounds and cases come from tests/head_maps_oracle.py; tests/test_head_maps.py shows on the CPU that the bounds are
satisfiable.  Every test prints its worst error / bound and its undecided fraction.
"""
import numpy as np
import pytest
import torch

import head_maps_oracle as hm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def to(dev, t):
    return None if t is None else t.to(dev)


def assert_same_bits(got, exp, what):
    """Byte for byte (a -0.0 is not a 0.0): ``got`` a GPU tensor, ``exp`` the CPU restatement's array of the same dtype."""
    got, exp = got.detach().cpu().contiguous(), torch.as_tensor(np.ascontiguousarray(exp))
    assert got.shape == exp.shape and got.dtype == exp.dtype, f'{what}: {tuple(got.shape)} {got.dtype} != {tuple(exp.shape)} {exp.dtype}'
    bad = got.view(torch.int32) != exp.view(torch.int32)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} values differ in their bits'


# ---- 1. class scores ---------------------------------------------------------------------------------------------------------
def run_class_case(dev, name, logits, lower, upper):
    """Both variants of one case: with probabilities (judged against float64) and without (same bytes)."""
    from celldetection_amd import ops
    ref = hm.class_reference(logits, lower, upper)
    sel, cls, fg, probs = ops.class_scores(to(dev, logits), to(dev, lower), to(dev, upper), return_probs=True)
    assert cls.dtype == torch.int32 and cls.shape == logits.shape[:1] + logits.shape[2:] and probs.shape == logits.shape
    assert sel.shape == fg.shape == logits.shape[:1] + (1,) + logits.shape[2:]
    out = hm.judge_class_scores(sel, cls, fg, probs, ref, name)
    sel2, cls2, fg2, none = ops.class_scores(to(dev, logits), to(dev, lower), to(dev, upper), return_probs=False)
    assert none is None
    assert torch.equal(hm.bits(sel2), hm.bits(sel)) and torch.equal(cls2, cls) and torch.equal(hm.bits(fg2), hm.bits(fg)), \
        f'{name}: results depend on return_probs'
    return (sel, cls, fg, probs), ref, out


@pytest.mark.parametrize('scale', hm.CLASS_SCALES)
@pytest.mark.parametrize('C', hm.CLASS_C)
def test_class_scores_vs_fp64_softmax(dev, C, scale):
    worst = [run_class_case(dev, *case)[2] for case in hm.class_cases(C, scale)]
    print(f'C={C} scale={scale}: worst error / bound = {max(w[0] for w in worst):.3f}, worst undecided = '
          f'{100 * max(w[1] for w in worst):.3f} %')


def test_class_scores_one_pixel(dev):
    for case in hm.class_cases(4, 3, (1, 1, 1)):
        run_class_case(dev, *case)


def test_class_scores_designed_ties(dev):
    logits, lower, upper, expected = hm.tie_case()
    (sel, cls, fg, probs), ref, _ = run_class_case(dev, 'ties', logits, lower, upper)
    cls, fg, probs = cls.cpu(), fg.cpu(), probs.cpu()
    for name, (mask, want) in expected.items():
        assert bool(ref['decided'][mask].all()) and bool((cls[mask] == want).all()), name
        assert bool((fg[:, 0][mask] == float(want > 0)).all()), name
    pix = probs.permute(0, 2, 3, 1)
    assert bool((pix[expected['upper_0'][0]] == 0).all()) and bool((pix[expected['lower_1'][0]] == 1).all())
    m = expected['upper_frac_tie'][0]
    assert bool((pix[m][:, 1:3] == np.float32(.3)).all())


# ---- 2. certainty mask -------------------------------------------------------------------------------------------------------
def test_certainty_mask_exact_grid(dev):
    """Uncertainty on the grid k / 8: C = 4 has an exact mean, a few percent of the pixels sit on the limit (strict comparison:
    -1), and the result is compared byte for byte; C = 1, 3, 5 outside C 2^-23 of the limit."""
    from celldetection_amd import ops
    s = hm.certainty_scores()
    u = hm.grid_uncertainty(4)
    ref = hm.certainty_reference(s, u, .5, exact=True)
    assert float((ref['mean'] == ref['limit']).double().mean()) > .03
    hm.judge_certainty(ops.certainty_mask(s.to(dev), u.to(dev), .5), ref, 'grid C=4', 0.)
    u = hm.grid_uncertainty(1)  # one channel: the mean is the value itself, every pixel is judged (11 % sit on the limit)
    hm.judge_certainty(ops.certainty_mask(s.to(dev), u.to(dev), .5), hm.certainty_reference(s, u, .5, exact=True), 'grid C=1', 0.)
    for C in (3, 5):  # the division rounds: judged outside C 2^-23 of the limit, i.e. everywhere but on it
        u = hm.grid_uncertainty(C)
        ref = hm.certainty_reference(s, u, .5)
        assert torch.equal(ref['decided'], ref['mean'] != ref['limit'])
        hm.judge_certainty(ops.certainty_mask(s.to(dev), u.to(dev), .5), ref, f'grid C={C}', hm.grid_on_limit_cap(C))
    one = torch.full((1, 4, 1, 1), .5)
    for v, want in ((.5, -1.), (.375, 1.)):
        one[0, 0] = v
        out = ops.certainty_mask(torch.ones(1, 1, 1, 1, device=dev), one.to(dev), .5)
        assert out.shape == (1, 1, 1, 1) and out.item() == want


@pytest.mark.parametrize('thr', (.35, .65))
def test_certainty_mask_random(dev, thr):
    from celldetection_amd import ops
    s = hm.certainty_scores()
    g = torch.Generator().manual_seed(7)
    for C in (1, 4, 5):
        u = torch.rand(hm.N, C, hm.H, hm.W, generator=g)
        hm.judge_certainty(ops.certainty_mask(s.to(dev), u.to(dev), thr), hm.certainty_reference(s, u, thr),
                           f'random C={C} thr={thr}', .001)


# ---- 3. gather -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', (0, 1, 131))
@pytest.mark.parametrize('C', (1, 3, 5))
def test_gather_channels_exact(dev, C, P):
    from celldetection_amd import ops
    maps = torch.randn(hm.N, C, hm.H, hm.W, generator=torch.Generator().manual_seed(C))
    idx = hm.gather_indices(P)
    got = ops.gather_channels(maps.to(dev), idx.to(dev))
    assert got.shape == (P, C) and got.dtype == torch.float32
    assert torch.equal(hm.bits(got), hm.bits(hm.gather_reference(maps, idx)))


def test_gather_channels_one_pixel(dev):
    from celldetection_amd import ops
    maps = torch.randn(1, 5, 1, 1, generator=torch.Generator().manual_seed(0))
    got = ops.gather_channels(maps.to(dev), torch.zeros(3, dtype=torch.int32, device=dev))
    assert torch.equal(got.cpu(), maps.view(1, 5).expand(3, 5))


# ---- 4. bicubic ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(hm.BICUBIC_CASES)))
def test_bicubic_resize_vs_fp64(dev, i):
    from celldetection_amd.cpn import _equal_size
    shape, size = hm.BICUBIC_CASES[i]
    x = hm.bicubic_input(i).to(dev)
    got = _equal_size(x, torch.empty(1, 1, *size), mode='bicubic')
    e = hm.bicubic_error(i, got)
    print(f'bicubic {shape} -> {size}: error / bound = {e / hm.bicubic_bound(i):.3f} ({e:.2f} of {hm.bicubic_bound(i):.2f} x 2^-23 max|x|)')
    assert e <= hm.bicubic_bound(i)
    assert _equal_size(x, torch.empty(1, 1, *shape[2:]), mode='bicubic') is x  # same size: the input object


def test_bicubic_unchanged_axis_is_a_1d_resize(dev):
    from celldetection_amd.cpn import _equal_size
    x = hm.bicubic_input(4).to(dev)  # (1, 1, 9, 9) -> (9, 31): the row taps are (0, 1, 0, 0) exactly
    got = _equal_size(x, torch.empty(1, 1, 9, 31), mode='bicubic')
    rows = _equal_size(x.view(9, 1, 1, 9), torch.empty(1, 1, 1, 31), mode='bicubic')
    assert torch.equal(hm.bits(got), hm.bits(rows.view(1, 1, 9, 31)))
    # and against an independent 1-D reference: each row resized on its own in float64, within the case's bound
    rows64 = torch.nn.functional.interpolate(hm.bicubic_input(4).double().view(9, 1, 1, 9), (1, 31), mode='bicubic', align_corners=False)
    e = float((got.cpu().double() - rows64.view(1, 1, 9, 31)).abs().max() / (hm.U * hm.bicubic_input(4).abs().max().double()))
    print(f'bicubic rows against a float64 1-D resize: error / bound = {e / hm.bicubic_bound(4):.3f}')
    assert e <= hm.bicubic_bound(4)


# ---- 5. fused decode -----------------------------------------------------------------------------------------------------------
def decode(dev, name, indices, gathered=False, order=None, fourier=None):
    from celldetection_amd import ops
    c, t = hm.DECODE_CASES[name], hm.decode_inputs(name)
    loc, fou = to(dev, t['locations']), to(dev, t['fourier'] if fourier is None else fourier)
    if gathered:
        loc, fou = ops.gather_channels(loc, indices), ops.gather_channels(fou, indices)
    return ops.decode_proposals(indices, to(dev, t['scores']), loc, fou, to(dev, t['refinement']), size=c['HW'],
                                order=c['order'] if order is None else order, samples=c['samples'], iterations=c['iterations'],
                                offsets=t['offsets'], num_buckets=c['buckets'], gathered=gathered)


@pytest.mark.parametrize('name', list(hm.DECODE_CASES))
def test_fused_decode_at_loop_edges(dev, name):
    """Dense decode == CPU restatement bit for bit; a prefix of the proposals decodes to the same rows (no dependence on block
    neighbours or P % 4); the gathered variant (cpn_decode_gathered) equals the dense one on every key."""
    from celldetection_amd import ops
    t, ref = hm.decode_inputs(name), hm.decode_reference(name)
    idx, counts, _ = ops.compact_scores(t['scores'].to(dev), hm.DECODE_THRESH)
    assert counts == ref['counts']
    full = decode(dev, name, idx)
    for k in hm.DECODE_KEYS + ('b',):
        assert_same_bits(full[k], ref[k], f'{name}: {k}')
    print(f'{name}: {len(idx)} proposals (P % 4 = {len(idx) % 4}), bit-identical on {len(hm.DECODE_KEYS) + 1} keys')
    for k in (1, 2, 3, 5):
        part = decode(dev, name, idx[:k])
        for key, v in part.items():
            assert torch.equal(v, full[key][:k]), f'{name}: first {k} proposals differ in {key}'
    gathered = decode(dev, name, idx, gathered=True)
    for key, v in gathered.items():
        assert torch.equal(v, full[key]), f'{name}: gathered decode differs in {key}'
    part = decode(dev, name, idx[:3], gathered=True)
    for key, v in part.items():
        assert torch.equal(v, full[key][:3]), f'{name}: gathered decode of the first 3 proposals differs in {key}'


def test_decode_rejects_orders_beyond_the_limit(dev):
    """The decode entry points refuse these before they launch the decode kernel: order 65 needs 260 coefficients (the kernel holds
    256), and an order beyond the map's own cannot be cut out of it."""
    name = 'C_one_sample'
    idx = torch.arange(3, dtype=torch.int32, device=dev)
    wide = torch.zeros(1, 4 * 65, *hm.DECODE_CASES[name]['hw'])
    for gathered in (False, True):
        with pytest.raises(RuntimeError, match='order'):
            decode(dev, name, idx, gathered=gathered, order=65, fourier=wide)
        with pytest.raises(RuntimeError, match='order'):
            decode(dev, name, idx, gathered=gathered, order=7)  # order_total is 6


def test_decode_accepts_the_largest_order_of_a_wider_map(dev):
    """The positive control of the test above: order 64 of a 65-order map is decoded."""
    name = 'C_one_sample'
    wide = torch.zeros(1, 4 * 65, *hm.DECODE_CASES[name]['hw'])
    out = decode(dev, name, torch.arange(3, dtype=torch.int32, device=dev), order=64, fourier=wide)
    assert out['fourier'].shape == (3, 64, 4) and not bool(out['fourier'].any())


# ---- 6. the chain the model runs ---------------------------------------------------------------------------------------------
def test_class_certainty_compact_decode_gather_chain(dev):
    """class_scores -> certainty_mask -> compact_scores(.5) -> decode_proposals -> gather_channels as CPN.postprocess chains them, for
    a multi-class head with an uncertainty head and a score bound (no golden model has both)."""
    from celldetection_amd import ops
    t, ref = hm.chain_inputs(), hm.chain_reference()
    cref = hm.class_reference(t['logits'], None, t['upper'])
    assert bool(cref['decided'].all())
    scores, cls, fg, _ = ops.class_scores(t['logits'].to(dev), None, t['upper'].to(dev))
    select = ops.certainty_mask(fg, t['uncertainty'].to(dev), hm.CHAIN['certainty_thresh'])
    idx, counts, _ = ops.compact_scores(select, .5)
    assert counts == ref['counts']
    flat = ops.decode_proposals(idx, scores, t['locations'].to(dev), t['fourier'].to(dev), t['refinement'].to(dev),
                                size=hm.CHAIN['HW'], order=hm.CHAIN['order'], samples=hm.CHAIN['samples'],
                                iterations=hm.CHAIN['iterations'])
    classes = cls.reshape(-1)[idx.long()].cpu().numpy()
    np.testing.assert_array_equal(classes, ref['classes'])
    assert_same_bits(ops.gather_channels(t['uncertainty'].to(dev), idx), ref['box_uncertainties'], 'chain: box_uncertainties')
    for k in ('contours', 'contour_proposals', 'boxes', 'locations', 'fourier'):
        assert_same_bits(flat[k], ref[k], f'chain: {k}')
    lin = idx.long().cpu()
    pick = lambda m: m.gather(1, cref['cls'][:, None]).reshape(-1)[lin].numpy()
    ratio = np.abs(flat['scores'].cpu().numpy().astype(np.float64) - pick(cref['q'])) / pick(cref['tol'])
    print(f'chain: {sum(counts)} detections {counts}, classes {np.bincount(classes).tolist()}, scores worst error / bound = '
          f'{ratio.max():.3f}, undecided = 0 %')
    assert ratio.max() <= 1.
