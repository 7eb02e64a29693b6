"""GPU tests of the CPN training objective (``cda.CPNObjective``, csrc/cpn_objective.hip) against ``tests/objective_oracle.py`` on
the cases of ``tests/golden/objective.npz`` and on edge cases of the kernels.

Bounds.  Contours, boxes and proposal indices are equal bit for bit (float32 arithmetic in the reference's order).  A term lies
within 1 float32 ulp of the oracle's float64 value: both are float64 sums of the same float32 elements (n < 2^20, so the two
summation orders differ by far less than a float32 ulp) and the kernel rounds to float32 once.  A gradient element lies within
2^-23 * A of the oracle's (A: the summed magnitude of its contributions; float64 sums, one rounding to float32) and is exactly 0
where nothing contributes.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objective_oracle as oracle  # noqa: E402

import celldetection_amd as cda  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = oracle.load_fixture()
MAPS = ('scores', 'locations', 'refinement', 'fourier')


def make_objective(config, S):
    return cda.CPNObjective(config['order'], S, classes=config['classes'], refinement=config['refine'],
                            refinement_iterations=config['iterations'], refinement_buckets=config['buckets'],
                            order_weights=config['order_weights'], weights=config['weights'])


def run_gpu(maps, targets, config, grad=MAPS, detail=True, grad_output=None):
    """-> dict(loss, losses, grads name -> numpy or None, detail, leaves)."""
    dev = torch.device('cuda')
    leaves = {k: (None if maps[k] is None else torch.tensor(maps[k], device=dev, requires_grad=k in grad)) for k in MAPS}
    tg = {k: torch.as_tensor(v).to(dev) for k, v in targets.items()}
    obj = make_objective(config, targets['sampling'].shape[1])
    obj.full_detail = detail
    loss, losses = obj(leaves['scores'], leaves['locations'], leaves['refinement'], leaves['fourier'], tg, size=config['size'])
    if grad:
        (loss if grad_output is None else loss * grad_output).backward()
    grads = {k: (None if v is None or v.grad is None else v.grad.cpu().numpy()) for k, v in leaves.items()}
    return dict(loss=loss, losses=losses, grads=grads, detail=obj.last_detail, leaves=leaves, objective=obj)


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def check_against_oracle(got, want, name='', expect=MAPS):
    d, w = got['detail'], want['detail']
    if d is not None:
        for j in range(3):
            assert np.array_equal(d['index'][j].cpu().numpy(), w['index'][j]), name
        assert np.array_equal(d['proposals'].cpu().numpy(), w['proposals']), name
        assert np.array_equal(d['boxes'].cpu().numpy(), w['boxes']), name
        assert len(d['refined']) == len(w['refined']), name
        for a, b in zip(d['refined'], w['refined']):
            assert np.array_equal(a.cpu().numpy(), b), name
    total = np.float32(0)
    for k in oracle.KEYS:
        v, n = want['terms'][k]
        t = got['losses'][k]
        assert (t is None) == (v is None), (name, k)
        if v is None:
            continue
        assert n < 2 ** 20 and t.dtype == torch.float32 and t.is_cuda and t.ndim == 0
        t = float(t)
        print(f'{name} {k}: {t!r} oracle {v!r} n {n}')
        assert abs(t - v) <= ulp32(v), (name, k, t, v)
        total = np.float32(total + np.float32(t))
    assert np.float32(got['loss'].item()).tobytes() == total.tobytes(), (name, got['loss'].item(), total)
    for k in MAPS:
        g = got['grads'][k]
        if want['grads'][k] is None or k not in expect:
            assert g is None, (name, k)
            continue
        assert g is not None, (name, k)
        v, m, a = want['grads'][k]
        nan = np.isnan(v)
        assert np.array_equal(np.isnan(g), nan), (name, k)
        err = np.where(nan, 0., np.abs(np.where(nan, 0., g.astype(np.float64)) - np.where(nan, 0., v)))
        bound = np.where(nan, 0., 2. ** -23 * a)
        worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.
        print(f'{name} grad {k}: largest error / bound {worst:.3f}, {int((m > 0).sum())} of {m.size} elements hit')
        assert (err <= bound).all(), (name, k, worst)
        assert (g[(m == 0) & ~nan] == 0).all(), (name, k)


@pytest.mark.parametrize('name', list(CASES))
def test_fixture_case_equals_the_oracle(name):
    case = CASES[name]
    got = run_gpu(case['maps'], case['targets'], case['config'])
    check_against_oracle(got, oracle.run_case(case), name)
    # the recorded boxes and proposals of the reference itself
    assert np.array_equal(got['detail']['proposals'].cpu().numpy(), case['rec']['proposals']), name
    assert np.array_equal(got['detail']['boxes'].cpu().numpy(), case['rec']['boxes']), name


@pytest.mark.parametrize('name', list(CASES))
def test_contours_equal_the_inference_ops(name):
    """The proposals and the last refined set are the bits of ``ops.fouriers2contours`` and ``ops.local_refinement``."""
    case = CASES[name]
    config, maps, targets = case['config'], case['maps'], case['targets']
    got = run_gpu(maps, targets, config, grad=())
    d = got['detail']
    b, y, x = d['index']
    if not len(b):
        return
    H, W = config['size']
    fourier, locations = got['leaves']['fourier'].detach(), got['leaves']['locations'].detach()
    N, _, h, w = fourier.shape
    sel = fourier.view(N, -1, 4, h, w)[b, :config['order'], :, y, x]
    loc = locations[b, :, y, x] + torch.stack((x, y), 1).float()
    scale = (torch.tensor([W, H], dtype=torch.float32) / torch.tensor([w, h], dtype=torch.float32)).cuda()
    hi = torch.tensor([W - 1, H - 1], dtype=torch.float32).cuda()
    refine = config['refine'] and config['iterations'] > 0
    linspace = np.array_equal(targets['sampling'], np.stack([torch.linspace(0, 1.0, targets['sampling'].shape[1]).numpy()] * N))
    for n in range(N):
        mine = b == n
        if not mine.any():
            continue
        con = cda.ops.fouriers2contours(sel[mine], loc[mine], sampling=torch.as_tensor(targets['sampling'][n]))[0] * scale
        if not refine:
            assert torch.equal(torch.minimum(torch.clamp(con, min=0), hi), d['proposals'][mine]), name
            continue
        assert torch.equal(con, d['proposals'][mine]), name
        if config['buckets'] > 1 and not linspace:
            continue  # ops.local_refinement builds its bucket tables for the default sampling only
        for it in (1, config['iterations']):
            ref = cda.ops.local_refinement(con, got['leaves']['refinement'].detach(), it, b[mine], num_buckets=config['buckets'])
            assert torch.equal(torch.minimum(torch.clamp(ref, min=0), hi), d['refined'][it - 1][mine]), (name, it)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('name', ['base', 'buckets4_random', 'classes4', 'no_refinement'])
def test_two_runs_are_bit_identical(name):
    case = CASES[name]
    one = run_gpu(case['maps'], case['targets'], case['config'])
    two = run_gpu(case['maps'], case['targets'], case['config'])
    assert _same_bits(one['loss'], two['loss'])
    for k in oracle.KEYS:
        assert (one['losses'][k] is None) == (two['losses'][k] is None)
        if one['losses'][k] is not None:
            assert _same_bits(one['losses'][k], two['losses'][k]), k
    for k in MAPS:
        if one['leaves'][k] is not None:
            assert _same_bits(one['leaves'][k].grad, two['leaves'][k].grad), k


def synthetic(seed, N, size, head, order=2, S=4, K=3, buckets=1, iterations=2, labels=None):
    rng = np.random.RandomState(seed)
    (H, W), (h, w) = size, head
    f16 = lambda a: np.asarray(a, np.float16).astype(np.float32)
    maps = dict(scores=f16(rng.randn(N, 1, h, w)), locations=f16(rng.randn(N, 2, h, w)),
                fourier=f16(rng.randn(N, 4 * order, h, w) * 2),
                refinement=(np.round(rng.randn(N, 2 * buckets, H, W) * 6) / 4).astype(np.float32))
    centre = np.stack((rng.uniform(0, W, (N, K)), rng.uniform(0, H, (N, K))), -1)
    targets = dict(labels=rng.randint(1, K + 1, (N, H, W)).astype(np.int64) if labels is None else labels,
                   fourier=f16(rng.randn(N, K, order, 4)), locations=f16(centre),
                   sampled_contours=(np.round((centre[:, :, None] + rng.randn(N, K, S, 2) * 4) * 4) / 4).astype(np.float32),
                   sampling=np.sort(rng.uniform(0, 1, (N, S)), 1).astype(np.float32))
    config = dict(order=order, classes=2, refine=True, iterations=iterations, buckets=buckets, order_weights=True, weights={},
                  size=size)
    return dict(maps=maps, targets=targets, config=config)


def test_all_foreground_more_than_one_block():
    case = synthetic(1, 2, (64, 64), (64, 64))
    got = run_gpu(case['maps'], case['targets'], case['config'])
    assert got['detail']['boxes'].shape[0] == 2 * 64 * 64
    assert got['losses']['score'] is not None
    check_against_oracle(got, oracle.run_case(case), 'all foreground')


def test_many_proposals_on_one_refinement_pixel():
    """200 proposals whose contours all collapse onto one pixel of the refinement map: 200 * S contributions per iteration for
    one element, summed in list order."""
    case = synthetic(2, 1, (10, 20), (10, 20), order=1, S=4, iterations=2)
    case['config']['order_weights'] = False
    case['maps']['fourier'][:] = 0
    yy, xx = np.mgrid[:10, :20]
    case['maps']['locations'][0, 0] = 7.25 - xx  # every absolute location is (7.25, 3.5): rounds to the pixel (7, 4)
    case['maps']['locations'][0, 1] = 3.5 - yy
    case['maps']['refinement'][0, :, 4, 7] = .25  # ... and stays there in the second iteration
    got = run_gpu(case['maps'], case['targets'], case['config'])
    want = oracle.run_case(case)
    assert got['detail']['boxes'].shape[0] == 200
    m = want['grads']['refinement'][1]
    assert m[0, 0, 4, 7] >= 200 * 4 and (m > 0).sum() <= 4
    check_against_oracle(got, want, 'one pixel')
    again = run_gpu(case['maps'], case['targets'], case['config'])
    assert _same_bits(got['leaves']['refinement'].grad, again['leaves']['refinement'].grad)


def test_no_proposals_leaves_the_score_term():
    case = synthetic(3, 2, (16, 20), (8, 10), labels=np.zeros((2, 16, 20), np.int64))
    got = run_gpu(case['maps'], case['targets'], case['config'])
    assert [k for k, v in got['losses'].items() if v is not None] == ['score']
    assert _same_bits(got['loss'], got['losses']['score'])
    for k in ('locations', 'refinement', 'fourier'):
        assert not got['grads'][k].any()
    assert got['grads']['scores'].all()
    check_against_oracle(got, oracle.run_case(case), 'no proposals')


def test_grad_output_scales_exactly_and_unused_maps_get_no_gradient():
    case = CASES['base']
    full = run_gpu(case['maps'], case['targets'], case['config'])
    half = run_gpu(case['maps'], case['targets'], case['config'], grad_output=.5)
    for k in MAPS:
        assert np.array_equal(half['grads'][k], full['grads'][k] * np.float32(.5)), k
    only = run_gpu(case['maps'], case['targets'], case['config'], grad=('fourier',))
    assert _same_bits(only['loss'], full['loss'])
    assert np.array_equal(only['grads']['fourier'], full['grads']['fourier'])
    assert all(only['grads'][k] is None for k in ('scores', 'locations', 'refinement'))
    with torch.no_grad():
        none = run_gpu(case['maps'], case['targets'], case['config'], grad=())
    assert _same_bits(none['loss'], full['loss']) and not none['loss'].requires_grad


def test_torch_op_equals_the_python_call():
    import celldetection_amd.torch_ops  # noqa: F401  (registers the operators)
    case = CASES['base']
    full = run_gpu(case['maps'], case['targets'], case['config'])
    dev = torch.device('cuda')
    m = {k: torch.tensor(case['maps'][k], device=dev) for k in MAPS}
    t = {k: torch.as_tensor(v).to(dev) for k, v in case['targets'].items()}
    out, gs, gl, gf, gr = torch.ops.celldetection_amd.cpn_objective(
        m['scores'], m['locations'], m['refinement'], m['fourier'], t['labels'], t['fourier'], t['locations'], t['sampled_contours'],
        t['sampling'], 32, 40, 2, 4, 1, True)
    assert _same_bits(out[8], full['loss'].detach())
    for i, k in enumerate(oracle.KEYS):
        assert bool(torch.isnan(out[i])) == (full['losses'][k] is None) and (full['losses'][k] is None or _same_bits(out[i], full['losses'][k]))
    for g, k in ((gs, 'scores'), (gl, 'locations'), (gf, 'fourier'), (gr, 'refinement')):
        assert np.array_equal(g.cpu().numpy(), full['grads'][k]), k


def test_a_map_that_is_not_contiguous_is_copied():
    case = CASES['base']
    full = run_gpu(case['maps'], case['targets'], case['config'])
    dev = torch.device('cuda')
    leaves = {k: torch.tensor(case['maps'][k], device=dev) for k in MAPS}
    fourier = leaves['fourier'].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_()
    assert not fourier.is_contiguous()
    obj = make_objective(case['config'], 8)
    loss, _ = obj(leaves['scores'], leaves['locations'], leaves['refinement'], fourier,
                  {k: torch.as_tensor(v).to(dev) for k, v in case['targets'].items()}, size=case['config']['size'])
    loss.backward()
    assert _same_bits(loss.detach(), full['loss'].detach())
    assert np.array_equal(fourier.grad.cpu().numpy(), full['grads']['fourier'])


def test_argument_errors_on_the_gpu():
    case = CASES['base']
    dev = torch.device('cuda')
    maps = {k: torch.tensor(case['maps'][k], device=dev) for k in MAPS}
    tg = {k: torch.as_tensor(v).to(dev) for k, v in case['targets'].items()}
    obj = make_objective(case['config'], 8)
    call = lambda t, **kw: obj(kw.get('scores', maps['scores']), maps['locations'], maps['refinement'], maps['fourier'], t, size=(32, 40))
    big = dict(tg, labels=tg['labels'].clone())
    big['labels'][0, 0, 0] = 2 ** 24 + 1
    with pytest.raises(ValueError, match='2\\^24'):
        call(big)
    rows = dict(tg, labels=tg['labels'].clone())
    rows['labels'][1, 3, 3] = tg['fourier'].shape[1] + 1
    with pytest.raises(ValueError, match='larger than the number of target rows'):
        call(rows)
    with pytest.raises(ValueError, match='shape'):
        call(dict(tg, locations=tg['locations'][:, :-1]))
    with pytest.raises(ValueError, match='GPU'):
        call(tg, scores=maps['scores'].cpu())
    with pytest.raises(RuntimeError, match='GPU'):
        call(dict(tg, labels=tg['labels'].cpu()))
    with pytest.raises(NotImplementedError, match='boxes'):
        call(dict(tg, boxes=torch.zeros((2, 5, 4), device=dev)))


def test_end_to_end_from_label_images():
    """label image -> CPNTargetGenerator (two images with different K) -> collate_cpn_targets -> objective -> oracle."""
    H, W, order, S = 32, 40, 3, 8
    yy, xx = np.mgrid[:H, :W]
    images = []
    for discs in (((8, 9, 6), (20, 28, 7), (24, 8, 5)), ((10, 12, 7), (21, 27, 8))):
        lab = np.zeros((H, W), np.int32)
        for i, (cy, cx, r) in enumerate(discs):
            lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = i + 1
        images.append(lab)
    np.random.seed(5)
    gens = []
    for lab in images:
        gen = cda.CPNTargetGenerator(samples=S, order=order)
        gen.feed(torch.as_tensor(lab[..., None]).cuda())
        gens.append(gen)
    tg = cda.collate_cpn_targets(gens)
    assert tg['fourier'].shape == (2, 3, order, 4) and tg['sampled_contours'].shape == (2, 3, S, 2)
    assert tg['labels'].shape == (2, H, W) and tg['sampling'].dtype == torch.float32 and tg['sampling'].shape == (2, S)
    assert not tg['fourier'][1, 2].any() and tg['fourier'][1, 1].any()  # the second image is padded with a zero row
    case = synthetic(7, 2, (H, W), (H // 2, W // 2), order=order, S=S, iterations=3)
    case['targets'] = {k: v.cpu().numpy() for k, v in tg.items()}
    got = run_gpu(case['maps'], case['targets'], case['config'])
    assert got['detail']['boxes'].shape[0] > 10 and (case['targets']['labels'] < 0).any()
    check_against_oracle(got, oracle.run_case(case), 'end to end')
