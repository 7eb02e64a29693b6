"""CPU check of tests/head_maps_oracle.py: with torch-CPU fp32 standing in for the kernels of csrc/decode_nms.hip, every bound of
the GPU test (tests/test_gpu_head_maps.py) holds, every cap on undecided pixels holds and the designed ties resolve as stated -- the
bounds are satisfiable before a kernel meets them.  It also measures the two quantities the bounds leave open:

  exp_ulps       worst error of torch-CPU fp32 exp, in ulps, on the arguments x_c - max x of all class-score cases
                 (the kernel's allowance in the softmax bound is E = 2 x this + 1)
  bicubic_cases  worst error of torch-CPU fp32 bicubic interpolation on each bicubic case, in units of 2^-23 max|input|
                 (the kernel's bound on that case is 4 x this)

``python tests/test_head_maps.py`` writes them to tests/golden/head_maps_measured.json; the test measures again and holds the committed
file to the fresh measurement.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_maps_oracle as hm  # noqa: E402


def all_class_cases():
    for C in hm.CLASS_C:
        for scale in hm.CLASS_SCALES:
            yield from hm.class_cases(C, scale)
    yield from hm.class_cases(4, 3, (1, 1, 1))
    logits, lower, upper, _ = hm.tie_case()
    yield 'ties', logits, lower, upper


def measure():
    exp_cases = {name: hm.exp_error_ulps(hm.exp_arguments(logits)) for name, logits, _, _ in all_class_cases()}
    bic = {hm.bicubic_name(i): hm.bicubic_error(i, hm.bicubic_f32_standin(i)) for i in range(len(hm.BICUBIC_CASES))}
    return dict(exp_ulps=max(exp_cases.values()), bicubic_cases=bic,
                exp_ulps_by_scale={str(s): max(v for k, v in exp_cases.items() if f'_s{s}_' in k) for s in hm.CLASS_SCALES})


def test_committed_measurement_covers_a_fresh_one():
    """Another CPU's libm / vector width may round differently, so the committed figures are held with a factor: what the kernel is
    allowed (2 E + 1 ulps of exp; 4 x the bicubic error) has to cover the fresh measurement, and the committed figure may not be
    more than 4 x the fresh one (it would allow the kernel more than the reference's own error justifies)."""
    m, c = measure(), hm.measured()
    print(f'exp: measured {m["exp_ulps"]:.4f} ulp (committed {c["exp_ulps"]:.4f}); bicubic, x 2^-23 max|x|: measured '
          f'{m["bicubic_cases"]} (committed {c["bicubic_cases"]})')
    assert 0 < m['exp_ulps'] <= hm.exp_allowance(c['exp_ulps']) and c['exp_ulps'] <= 4 * m['exp_ulps']
    assert set(c['bicubic_cases']) == set(m['bicubic_cases'])
    for i in range(len(hm.BICUBIC_CASES)):
        fresh, kept = m['bicubic_cases'][hm.bicubic_name(i)], c['bicubic_cases'][hm.bicubic_name(i)]
        assert 0 < fresh <= hm.bicubic_bound(i) and kept <= 4 * fresh, hm.bicubic_name(i)
    assert c['exp_ulps'] < 2, 'a libm exp is good to an ulp or so; anything else is a mistake in the measurement'


@pytest.mark.parametrize('scale', hm.CLASS_SCALES)
@pytest.mark.parametrize('C', hm.CLASS_C)
def test_f32_softmax_is_within_the_bound(C, scale):
    for name, logits, lower, upper in hm.class_cases(C, scale):
        ref = hm.class_reference(logits, lower, upper)
        hm.judge_class_scores(*hm.class_f32_standin(logits, lower, upper), ref, name)


def test_one_pixel_and_designed_ties():
    for name, logits, lower, upper in hm.class_cases(4, 3, (1, 1, 1)):
        hm.judge_class_scores(*hm.class_f32_standin(logits, lower, upper), hm.class_reference(logits, lower, upper), name)
    logits, lower, upper, expected = hm.tie_case()
    ref = hm.class_reference(logits, lower, upper)
    sel, cls, fg, probs = hm.class_f32_standin(logits, lower, upper)
    hm.judge_class_scores(sel, cls, fg, probs, ref, 'ties')
    for name, (mask, want) in expected.items():
        assert mask.sum() > 50 and bool(ref['decided'][mask].all()), name
        assert bool((ref['cls'][mask] == want).all()) and bool((cls[mask] == want).all()), name
    m = expected['upper_0'][0]
    assert bool((probs.permute(0, 2, 3, 1)[m] == 0).all()) and bool((fg[:, 0][m] == 0).all())
    m = expected['lower_1'][0]
    assert bool((probs.permute(0, 2, 3, 1)[m] == 1).all())
    m = expected['upper_frac_tie'][0]
    assert bool((probs[:, 1][m] == np.float32(.3)).all()) and bool((probs[:, 2][m] == np.float32(.3)).all())


def test_the_class_judge_catches_a_wrong_kernel():
    """The judge must fail for the mistakes it is there for: a last-argmax tie rule, a wrong plane, a probability 40 ulps off."""
    logits, lower, upper, _ = hm.tie_case()
    ref = hm.class_reference(logits, lower, upper)
    sel, cls, fg, probs = hm.class_f32_standin(logits, lower, upper)
    last = probs.shape[1] - 1 - torch.argmax(probs.flip(1), 1)
    with pytest.raises(AssertionError):
        hm.judge_class_scores(probs.gather(1, last[:, None]), last.to(torch.int32), (last > 0).float()[:, None], probs, ref, 'last argmax')
    with pytest.raises(AssertionError):
        hm.judge_class_scores(sel, cls, fg, probs.roll(1, 3), ref, 'shifted plane')
    _, logits, lower, upper = hm.class_cases(3, .5)[0]
    ref = hm.class_reference(logits, lower, upper)
    sel, cls, fg, probs = hm.class_f32_standin(logits, lower, upper)
    off = probs * (1 + 40 * hm.U)
    with pytest.raises(AssertionError):
        hm.judge_class_scores(off.gather(1, cls.long()[:, None]), cls, fg, off, ref, '40 ulps off')


def test_certainty_mask_bounds():
    s = hm.certainty_scores()
    u = hm.grid_uncertainty(4)
    ref = hm.certainty_reference(s, u, .5, exact=True)
    on_limit = float((ref['mean'] == ref['limit']).double().mean())
    assert .03 < on_limit < .1  # the strict comparison is met by a few percent of the pixels
    assert bool((ref['expected'][ref['mean'] == ref['limit']] == -1).all())
    hm.judge_certainty(hm.certainty_f32_standin(s, u, .5), ref, 'grid C=4', 0.)
    u = hm.grid_uncertainty(1)  # the mean of one channel is exact too
    hm.judge_certainty(hm.certainty_f32_standin(s, u, .5), hm.certainty_reference(s, u, .5, exact=True), 'grid C=1', 0.)
    for C in (3, 5):
        u = hm.grid_uncertainty(C)
        ref = hm.certainty_reference(s, u, .5)
        assert torch.equal(ref['decided'], ref['mean'] != ref['limit'])  # undecided = on the limit, nothing else
        hm.judge_certainty(hm.certainty_f32_standin(s, u, .5), ref, f'grid C={C}', hm.grid_on_limit_cap(C))
    g = torch.Generator().manual_seed(7)
    for C in (1, 4, 5):
        u = torch.rand(hm.N, C, hm.H, hm.W, generator=g)
        for thr in (.35, .65):
            hm.judge_certainty(hm.certainty_f32_standin(s, u, thr), hm.certainty_reference(s, u, thr), f'random C={C} thr={thr}', .001)
    one = torch.full((1, 4, 1, 1), .5)
    out = hm.certainty_f32_standin(torch.ones(1, 1, 1, 1), one, .5)
    hm.judge_certainty(out, hm.certainty_reference(torch.ones(1, 1, 1, 1), one, .5, exact=True), 'one pixel on the limit', 0.)
    assert out.item() == -1


def test_gather_reference_and_indices():
    maps = torch.arange(hm.N * 5 * hm.H * hm.W, dtype=torch.float32).view(hm.N, 5, hm.H, hm.W)
    hw = hm.H * hm.W
    for P in (0, 1, 131):
        idx = hm.gather_indices(P)
        assert idx.dtype == torch.int32 and idx.shape == (P,)
        got = hm.gather_reference(maps, idx)
        assert got.shape == (P, 5)
        for p, lin in enumerate(idx.tolist()):
            b, pos = divmod(lin, hw)
            assert got[p].tolist() == [float((b * 5 + c) * hw + pos) for c in range(5)]
    idx = hm.gather_indices(131).tolist()
    assert {0, hw - 1, (hm.N - 1) * hw, hm.N * hw - 1} <= set(idx) and len(set(idx)) < len(idx)


def test_f32_bicubic_is_within_the_bound():
    for i, (shape, size) in enumerate(hm.BICUBIC_CASES):
        e = hm.bicubic_error(i, hm.bicubic_f32_standin(i))
        print(f'bicubic {shape} -> {size}: error {e:.3f} / bound {hm.bicubic_bound(i):.3f}')
        assert e <= hm.bicubic_bound(i)
    # one axis unchanged: the rows are 1-D resizes
    rows = torch.nn.functional.interpolate(hm.bicubic_input(4).double().view(9, 1, 1, 9), (1, 31), mode='bicubic', align_corners=False)
    assert torch.equal(rows.view(1, 1, 9, 31), hm.bicubic_reference(4))


def test_decode_cases_cross_their_edges():
    """Each case keeps at least 5 proposals (the prefix runs need them), A sits on the coefficient limit, the sample counts straddle
    one, two and four wave passes, and the totals are not all multiples of the block's 4 proposals."""
    import cpn_oracle  # noqa: F401  (conftest puts oracle/ on the path)
    totals = []
    for name, c in hm.DECODE_CASES.items():
        ref = hm.decode_reference(name)
        P = sum(ref['counts'])
        totals.append(P)
        assert P >= 5 and len(ref['b']) == P and ref['contours'].shape == (P, c['samples'], 2), name
        assert ref['fourier'].shape == (P, c['order'], 4) and np.isfinite(ref['contours']).all(), name
        if c['n'] > 1:
            assert min(ref['counts']) > 0, name
    assert hm.DECODE_CASES['A_max_coef']['order'] * 4 == 256
    assert sorted(c['samples'] for c in hm.DECODE_CASES.values()) == [1, 65, 65, 129, 200]
    assert any(P % 4 for P in totals)
    d, e = hm.decode_reference('D_no_refinement'), hm.decode_inputs('D_no_refinement')
    assert np.array_equal(d['contours'], d['contour_proposals']) and e['offsets'] is not None


def test_chain_reference():
    """The chain's inputs do what they are for: classes 1..3 occur, the certainty filter and the upper bound each remove pixels, and
    every pixel's class is decided (1/4-grid logits)."""
    import cpn_oracle  # noqa: F401
    t, ref = hm.chain_inputs(), hm.chain_reference()
    cref = hm.class_reference(t['logits'], None, t['upper'])
    assert bool(cref['decided'].all())
    fg = cref['cls'] > 0
    certain = hm.certainty_reference(fg.float()[:, None], t['uncertainty'], hm.CHAIN['certainty_thresh'], exact=True)
    keep = (certain['expected'][:, 0] > .5)
    assert ref['counts'] == keep.sum((1, 2)).tolist() and 0 < keep.sum() < fg.sum() < fg.numel()
    assert set(ref['classes'].tolist()) == {1, 2, 3}
    assert bool((cref['cls'][t['upper'][:, 0] == 0] == 0).all())
    np.testing.assert_array_equal(ref['classes'], cref['cls'][keep].numpy())
    sel64 = cref['q'].gather(1, cref['cls'][:, None])[:, 0][keep].numpy()
    tol = cref['tol'].gather(1, cref['cls'][:, None])[:, 0][keep].numpy()
    assert (np.abs(ref['scores'] - sel64) <= tol).all()


if __name__ == '__main__':
    with open(hm.MEASURED, 'w') as f:
        json.dump(measure(), f, indent=1, sort_keys=True)
        f.write('\n')
    print(open(hm.MEASURED).read())
