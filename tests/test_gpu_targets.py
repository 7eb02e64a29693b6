"""CPN training targets on the MI355X: celldetection_amd.labels2distances, mask_labels_by_distance_, filter_instances_ and
CPNTargetGenerator against the reference's recorded results (tests/golden/targets.npz) and against the numpy restatement of
tests/targets_oracle.py, which the CPU tests pin to that fixture.  Distances are compared bit by bit and labels value by
value; the only bounds are those of the Fourier tests (tests/test_fourier.py) and the float32 reasoning written at their use."""
import os

import numpy as np
import pytest
import torch

import celldetection_amd as cda
import fourier_oracle
import targets_oracle as oracle
from celldetection_amd.targets import MAX_STEPS
from test_fourier import constants, within
from test_instance_eval import disc_labels
from test_targets import BG, FG, distance_cases, filter_cases, generator_cases

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(a, what='', mask=True, **kw):
    """cda.labels2distances (and the masking) on the device copy of ``a`` against the oracle -> the stats."""
    x = gpu(a)
    dist, lab, st = cda.labels2distances(x, return_stats=True, **kw)
    exp_d, exp_l = oracle.labels2distances(a, **kw)
    assert dist.is_cuda and dist.dtype == torch.float32 and lab.dtype == x.dtype and tuple(lab.shape) == exp_l.shape, what
    got = dist.cpu().numpy()
    assert same_bits(got, exp_d), (what, f'{int((got != exp_d).sum())} distances differ, first at {np.argwhere(got != exp_d)[:3].tolist()}')
    assert np.array_equal(lab.cpu().numpy(), exp_l), what
    assert np.array_equal(x.cpu().numpy(), a), what  # the input is left untouched
    assert st['launches'] == len(st['active_tiles']) == len(st['changed_pixels']) and st['changed_pixels'][-1] == 0, (what, st)
    if mask:
        red = cda.mask_labels_by_distance_(lab, dist, BG, FG, return_reduced=True)
        exp_m, exp_r = oracle.mask_labels_by_distance(exp_l, exp_d, BG, FG)
        assert np.array_equal(lab.cpu().numpy(), exp_m) and np.array_equal(red.cpu().numpy(), exp_r), what
    return st


def test_fixture_cases_equal_the_reference():
    for key, a, dt, inst, prot, dist, lab, masked, reduced in distance_cases():
        d, l = cda.labels2distances(gpu(a), distance_type=dt, per_instance=inst, protected_size=prot)
        assert same_bits(d.cpu().numpy(), dist), key
        assert np.array_equal(l.cpu().numpy(), lab), key
        r = cda.mask_labels_by_distance_(l, d, BG, FG, return_reduced=True)
        assert np.array_equal(l.cpu().numpy(), masked) and np.array_equal(r.cpu().numpy(), reduced), key
        assert cda.mask_labels_by_distance_(gpu(lab), gpu(dist), BG, FG) is None


@pytest.mark.parametrize('channels', (1, 2, 3, 11))
def test_sizes_and_channel_counts(channels):
    for h, w in ((1, 1), (1, 7), (31, 33), (32, 32), (33, 65), (67, 129)):
        a = disc_labels(h, w, max(h * w // 120, 1), channels, seed=h + channels, rmax=9.)
        if h == 1:
            a[:] = 0
            a[0, : w // 2 + 1, 0] = 7
            a[0, w // 4:, channels - 1] = 9 if channels > 1 else 7  # two runs sharing a stretch (one channel: one run)
        for inst in (True, False):
            if not inst and (oracle.owner_image(a) != 0).all():
                continue
            for dt in ((1, 2, 3) if (h, w) == (33, 65) else (2,)):
                check(a, f'{h} x {w} x {channels}, per_instance {inst}, type {dt}', distance_type=dt, per_instance=inst)


def seam_image():
    """70 x 100: objects across every tile seam (32, 64 | 32, 64, 96), on the corners and along the borders."""
    a = np.zeros((70, 100, 2), np.int32)
    v = 1
    for y in (0, 26, 58):
        for x in (0, 25, 57, 89):
            a[y:y + 12, x:x + 11, v % 2] = v
            v += 1
    a[28:36, :, 0][a[28:36, :, 0] == 0] = v  # a band along the first horizontal seam, over the whole width
    a[:, 60:68, 1][a[:, 60:68, 1] == 0] = v + 1  # and one along a vertical seam: overlaps where they cross other objects
    return a


def test_objects_on_tile_seams_and_borders():
    a = seam_image()
    assert ((a > 0).sum(2) > 1).any()
    for inst in (True, False):
        for prot in (36, 0):
            check(a, f'seams, per_instance {inst}', per_instance=inst, protected_size=prot)


def spiral(h, w, width=3, gap=3):
    """One connected object over the whole image: a band of ``width`` pixels winding inwards, every winding a rectangle that is
    open at its top left corner and joined to the next one there."""
    m = np.zeros((h, w), bool)
    step = width + gap
    k = 0
    while h - 2 * k * step >= 3 * width and w - 2 * k * step >= 3 * width:
        t, l, b, r = k * step, k * step, h - k * step, w - k * step  # half-open
        m[t:t + width, l + step:r] = True  # top, open at the left
        m[t:b, r - width:r] = True
        m[b - width:b, l:r] = True
        m[t + step:b, l:l + width] = True  # left, open at the top
        m[t + step:t + step + width, l:l + 2 * step] = True  # the left side runs into the top of the next winding
        k += 1
    return m


def test_large_objects_need_several_launches():
    a = np.zeros((130, 257, 1), np.int32)
    a[15:115, 70:170] = 3  # inradius 50 > the halo: several launches
    for inst in (True, False):
        st = check(a, f'square, per_instance {inst}', per_instance=inst)
        assert st['launches'] >= 50 // MAX_STEPS and st['launches'] > 1, st
    d, _ = cda.labels2distances(gpu(a))
    assert float(d[64, 120]) == 1. and float(d[15, 70]) == np.float32(62587) / np.float32(50 * 62587)
    a = np.zeros((130, 257, 1), np.int32)
    a[spiral(130, 257), 0] = 9
    st = check(a, 'spiral')
    assert st['launches'] > 1 and st['active_tiles'][0] == 5 * 9, st
    a[a == 0] = 4  # the complement as a second object; nothing without an owner: fg mode raises, instance mode works
    check(a, 'spiral and complement')
    with pytest.raises(ValueError, match='without an owner'):
        cda.labels2distances(gpu(a), per_instance=False)
    b = np.concatenate((a, a), 2)  # everything overlaps: every pixel is a zero pixel
    d, l = cda.labels2distances(gpu(b), per_instance=False)
    assert not d.any() and (l == -1).all()


def many_small(values=None):
    """256 x 512: 2048 cells of 8 x 8, cell k holding an object of 1 + k % 40 pixels (both sides of the protected size)."""
    a = np.zeros((256, 512, 1), np.int32)
    for k in range(2048):
        n = 1 + k % 40
        cell = np.zeros(49, np.int32)
        cell[:n] = k + 1 if values is None else values[k]
        y, x = (k // 64) * 8, (k % 64) * 8
        a[y:y + 7, x:x + 7, 0] = cell.reshape(7, 7)
    return a


def test_two_thousand_small_objects_sparse_and_large_labels():
    a = many_small()
    sizes = np.bincount(a[a > 0])
    assert len(sizes) - 1 >= 2000 and {35, 36, 37} <= set(sizes.tolist())
    check(a, '2048 objects')
    check(a, '2048 objects, protected 10', protected_size=10)
    values = 2 ** 31 - 1 - 1000003 * np.arange(2048, dtype=np.int64) % (2 ** 30)  # near 2^31 and sparse
    assert values.max() == 2 ** 31 - 1 and len(np.unique(values)) == 2048 and values.min() > 2 ** 29
    check(many_small(values.astype(np.int32)), 'labels near 2^31')
    check(many_small((1 + 7919 * np.arange(2048)).astype(np.int32)), 'sparse labels', per_instance=False)


def test_input_kinds_and_repeatability():
    a = disc_labels(67, 129, 40, 3, seed=4, rmax=12.)
    assert a.max() < 127
    exp_d, exp_l = oracle.labels2distances(a)
    for dt in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
        x = gpu(a).to(dt)
        keep = x.clone()
        d, l = cda.labels2distances(x)
        assert l.dtype == dt and same_bits(d.cpu().numpy(), exp_d) and torch.equal(x, keep), dt
        if dt != torch.uint8:
            assert np.array_equal(l.cpu().numpy(), exp_l), dt
        else:
            assert np.array_equal(l.cpu().numpy(), exp_l.astype(np.uint8)), dt
    d2, l2 = cda.labels2distances(gpu(a))
    assert torch.equal(d, d2)  # the same image twice: bit-identical
    flat = gpu(a[..., 0])
    d3, l3 = cda.labels2distances(flat)
    assert tuple(l3.shape) == (67, 129, 1) and same_bits(d3.cpu().numpy(), oracle.labels2distances(a[..., :1])[0])
    view = gpu(np.concatenate((a, a), 1))[:, 129:]  # not contiguous
    assert same_bits(cda.labels2distances(view)[0].cpu().numpy(), exp_d)
    with pytest.raises(ValueError, match='fit int32'):
        cda.labels2distances(gpu(a).to(torch.int64) + 2 ** 31)
    import celldetection_amd.torch_ops  # noqa: F401
    d4, l4 = torch.ops.celldetection_amd.labels2distances(gpu(a), 2, True, 36)
    assert torch.equal(d4, d2) and torch.equal(l4, l2)
    # mask_labels_by_distance_ in place on other dtypes and thresholds
    for dt in (torch.int64, torch.int16):
        l = gpu(exp_l).to(dt)
        assert cda.mask_labels_by_distance_(l, d2, .3, .9) is None
        assert l.dtype == dt and np.array_equal(l.cpu().numpy(), oracle.mask_labels_by_distance(exp_l, exp_d, .3, .9)[0])
    for m in oracle.MASK_MUTANTS:
        assert (oracle.mask_labels_by_distance(exp_l, exp_d, BG, FG, mutant=m)[0] != oracle.mask_labels_by_distance(exp_l, exp_d, BG, FG)[0]).any()


def test_filter_instances():
    for name, a, kw, res in filter_cases():
        for dt in (torch.int32, torch.int64):
            x = gpu(a).to(dt)
            out = cda.filter_instances_(x, **kw)
            assert out is x, name
            got = x.cpu().numpy()
            assert np.array_equal(got, oracle.filter_instances(a, **kw)), name  # the stated pairing: largest to largest
            assert oracle.same_partition(got, res) and np.array_equal(np.unique(got), np.unique(res)), name
            if not kw['continuous'] or 'gap_free' in name:
                assert np.array_equal(got, res), name
            if kw['continuous']:
                pos = np.unique(got[got > 0])
                assert np.array_equal(pos, np.arange(1, len(pos) + 1)), name
    a = disc_labels(90, 120, 50, 2, seed=9) * 5
    x = gpu(a)[:, 10:100]  # a view: rewritten in place through a copy
    cda.filter_instances_(x, partials_border=2, min_area=20, max_area=300)
    assert np.array_equal(x.cpu().numpy(), oracle.filter_instances(a[:, 10:100], partials_border=2, min_area=20, max_area=300))
    with pytest.raises(ValueError, match='does not fit'):
        cda.filter_instances_(gpu(a).to(torch.uint8), constant=-1)


def perimeter(points):
    p = np.asarray(points, np.float64).reshape(-1, 2)
    closed = np.concatenate((p, p[:1])) if not fourier_oracle.is_closed(p) else p
    return len(closed) - 1, float((np.sqrt((np.diff(closed, axis=0) ** 2).sum(1)) + 1e-6).sum())


def test_generator_against_the_reference():
    c_f, c_l = constants()
    for name, a, ckw, fkw, seed, exact, rec in generator_cases():
        gen = cda.CPNTargetGenerator(**ckw)
        x = gpu(a)
        gen.feed(x, **fkw)
        np.random.seed(seed)
        np_ = lambda t: t.cpu().numpy()
        K, S, order = len(rec['fourier']), ckw['samples'], ckw['order']
        assert gen.labels.data_ptr() == x.data_ptr()  # filtered and flagged in place
        assert np.array_equal(gen.sampling, rec['sampling']) and gen.sampling is gen.sampling, name
        if not exact:  # labels moved: the reference's pairing is unspecified, the partition is not
            assert oracle.same_partition(np_(gen.labels), rec['labels']), name
            assert oracle.same_partition(np_(gen.reduced_labels), rec['reduced_labels']), name
            assert same_bits(np_(gen.distances), rec['distances']), name  # distances do not depend on the names
            continue
        assert np.array_equal(np_(gen.labels), rec['labels']), name
        assert same_bits(np_(gen.distances), rec['distances']), name
        assert np.array_equal(np_(gen.labels_red), rec['labels_red']), name
        assert np.array_equal(np_(gen.reduced_labels), rec['reduced_labels']), name
        ids, offsets, points = gen.packed_contours
        assert np.array_equal(np_(ids), rec['contour_ids']) and np.array_equal(np_(offsets), rec['contour_offsets']), name
        assert np.array_equal(np_(points), rec['contour_points']), name
        con = gen.contours
        assert list(con) == rec['contour_ids'].tolist() and all(c.shape[1:] == (1, 2) for c in con.values()), name
        # the composition adds nothing: bit-equal to the existing functions on the same contours
        f, l = cda.contours2fourier(con, order=order)
        assert gen.fourier.dtype == torch.float32 and torch.equal(gen.fourier, f) and torch.equal(gen.locations, l), name
        s, _ = cda.ops.fouriers2contours(f, l, samples=S, sampling=torch.as_tensor(gen.sampling))
        assert tuple(gen.sampled_contours.shape) == (K, S, 2) and torch.equal(gen.sampled_contours, s), name
        res = torch.stack(cda.resample_contours([c[:, 0] for c in con.values()], S))
        assert gen.resampled_contours.dtype == torch.float64 and tuple(gen.resampled_contours.shape) == (K, S, 2), name
        assert torch.equal(gen.resampled_contours[ids.long() - 1], res), name
        size = gen.sampled_contours.max(1).values - gen.sampled_contours.min(1).values
        assert torch.equal(gen.sampled_sizes, size) and tuple(size.shape) == (K, 2), name
        # against the reference's recorded values, by the bounds the existing tests hold these functions to
        assert np.array_equal(np_(gen.resampled_contours), rec['resampled_contours']), name  # exact, as test_gpu_label_contours
        f64, l64 = cda.fourier.efd_packed(points, offsets, order)
        assert torch.equal(gen.fourier[ids.long() - 1], f64.float()) and torch.equal(gen.locations[ids.long() - 1], l64.float())
        split = np.split(np_(points), np_(offsets)[1:-1])
        for k in range(len(split)):
            N, T = perimeter(split[k])
            row = int(ids[k]) - 1
            if k < 4 and N >= 2:  # the float64 result against the 40-digit truth, the bound of tests/test_fourier.py
                ref = fourier_oracle.truth(split[k], order, 1e-6, not fourier_oracle.is_closed(split[k]))
                within(np_(f64[k]), np_(l64[k]), ref, f'{name} contour {k}')
            # both float32 values are roundings of float64 values within c U of the truth: <= 2 c U + one float32 ulp apart
            U = 2. ** -53 * N * T
            got_f, ref_f = np_(gen.fourier[row]).astype(np.float64), rec['fourier'][row].astype(np.float64)
            assert (np.abs(got_f - ref_f) <= 2 * c_f * U + 2. ** -23 * np.abs(ref_f)).all(), (name, k)
            got_l, ref_l = np_(gen.locations[row]).astype(np.float64), rec['locations'][row].astype(np.float64)
            assert (np.abs(got_l - ref_l) <= 2 * c_l * U + 2. ** -23 * np.abs(ref_l)).all(), (name, k)
            # sampled contour = location + sum over order of 4 products, in float32 here and float64 there, from coefficients one
            # float32 ulp apart at most: (4 order + 2) roundings of 2^-24 each on terms bounded by |location| + sum |coefficient|,
            # plus the ulp of every input: 2^-23 (4 order + 4) (|location| + sum |coefficient|)
            scale = np.abs(ref_l).max() + np.abs(ref_f).sum()
            diff = np.abs(np_(gen.sampled_contours[row]).astype(np.float64) - rec['sampled_contours'][row]).max()
            assert diff <= 2. ** -23 * (4 * order + 4) * scale, (name, k, diff)
        print(f'{name}: {K} rows, {len(split)} contours')
    two = {name: (a, ckw, fkw) for name, a, ckw, fkw, *_ in generator_cases() if name.startswith('gen_two_pieces')}
    out = {}
    for name, (a, ckw, fkw) in two.items():
        gen = cda.CPNTargetGenerator(**ckw)
        gen.feed(gpu(a), **fkw)
        out[name] = (gen.labels.cpu().numpy(), gen.distances.cpu().numpy())
    flag, keep = out['gen_two_pieces_flag'], out['gen_two_pieces_keep']
    assert (flag[0] == -1).sum() > (keep[0] == -1).sum() and (flag[1][flag[0][..., 0] == -1] == 0).all()
    assert (keep[1][flag[0][..., 0] == -1] > 0).all()  # flagging happened before the distances were taken


def test_round_trip_from_a_model():
    """model -> contours2labels -> flat -> CPNTargetGenerator.feed -> sampled_contours -> contours2labels on one 256 x 256 tile:
    the objects above the protected size come back (F1 at IoU 0.5 = 1.0 against the fed labels).  The label image is flattened
    first because LabelMatcher takes at most 8 channels and the synthetic model's contours overlap in more."""
    from celldetection_amd.synth import synth_state_dict
    from model_specs import G, MODEL_SPECS
    spec = MODEL_SPECS['CpnU22']
    g = np.load(os.path.join(G, 'model_CpnU22.npz'))
    model = getattr(cda.models, spec['cls'])(**spec['kwargs'])
    overrides = {k[len('override.'):]: torch.as_tensor(g[k]) for k in g.files if k.startswith('override.')}
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=int(g['seed']) if 'seed' in g.files else 0, overrides=overrides))
    model = model.to(DEV)
    x = torch.as_tensor(g['x'])
    reps = (-(-256 // x.shape[2]), -(-256 // x.shape[3]))
    x = x.repeat(1, 1, *reps)[:1, :, :256, :256].contiguous().to(DEV)
    model.precision = 'fp32'
    y = model(x)
    size = (256, 256)
    labels = cda.resolve_label_channels(cda.contours2labels(y['contours'][0], size))  # the flat image: what is saved and annotated
    assert labels.is_cuda and tuple(labels.shape) == size and int(labels.max()) >= 1
    gen = cda.CPNTargetGenerator(samples=128, order=25)
    gen.feed(labels, min_area=37)  # only objects above the protected size stay
    fed = gen.labels
    assert fed.data_ptr() == labels.data_ptr()
    assert tuple(gen.distances.shape) == size and tuple(gen.reduced_labels.shape) == size and gen.sampled_contours.is_cuda
    ids = gen.packed_contours[0].long()
    kept = torch.unique(fed[fed > 0])
    assert len(ids) >= 1 and torch.equal(kept, ids)  # what is left after filtering and flagging has a contour each (gaps: flagged)
    assert int((gen.sampled_contours[ids - 1].flatten(1).abs().sum(1) == 0).sum()) == 0
    again = cda.contours2labels(gen.sampled_contours[ids - 1], size)
    # epsilon=0: with the default 1e-12 in every denominator no score can reach 1.0 exactly, however perfect the match
    m = cda.LabelMatcher(again, fed.clamp(min=0), iou_thresh=.5, epsilon=0)
    f1 = m.f1
    print(f'{len(ids)} objects above the protected size: F1 at IoU 0.5 of the decoded sampled contours against the fed labels = {f1!r} '
          f'(tp {m.true_positives}, fp {m.false_positives}, fn {m.false_negatives})')
    assert f1 == 1.
    assert m.true_positives == len(ids) and m.false_positives == 0 and m.false_negatives == 0
