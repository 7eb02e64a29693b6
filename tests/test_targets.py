"""CPN training targets, the part that needs no GPU: the numpy restatement of tests/targets_oracle.py against the results the
reference's own labels2distances, mask_labels_by_distance_, filter_instances_ and CPNTargetGenerator returned
(tests/golden/targets.npz, written by tests/golden/make_golden_targets.py), hand-worked values, the oracle's three statements of
the chamfer transform against each other, and the C ABI, bindings, exports and argument errors of celldetection_amd.targets."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import celldetection_amd as cda
import targets_oracle as oracle
from celldetection_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG, FG = .5, .75
HV, DIAG = 62587, 89738
_cache = {}


def fixture():
    if 'z' not in _cache:
        with np.load(os.path.join(ROOT, 'tests', 'golden', 'targets.npz')) as z:
            _cache['z'] = {k: z[k] for k in z.files}
    return _cache['z']


def distance_cases():
    """-> (key, labels, distance_type, per_instance, protected_size, distances, labels_out, masked, reduced)."""
    z = fixture()
    for key in z['distance_cases'].tolist():
        dt, inst, prot = z[f'{key}.params'].tolist()
        yield (key, z[f'{key}.labels'], dt, bool(inst), prot, z[f'{key}.distances'], z[f'{key}.labels_out'], z[f'{key}.masked'],
               z[f'{key}.reduced'])


def filter_cases():
    """-> (name, labels, keywords, result)."""
    z = fixture()
    for name in z['filter_cases'].tolist():
        p = z[f'filter.{name}.params'].tolist()
        kw = dict(partials=bool(p[0]), partials_border=p[1], min_area=None if p[2] < 0 else p[2], max_area=None if p[3] < 0 else p[3],
                  constant=p[4], continuous=bool(p[5]))
        yield name, z[f'filter.{name}.labels'], kw, z[f'filter.{name}.result']


def generator_cases():
    """-> (name, input, constructor keywords, feed keywords, seed, exact, dict of recorded properties)."""
    z = fixture()
    for name in z['generator_cases'].tolist():
        p = f'gen.{name}'
        i, f = z[f'{p}.ints'].tolist(), z[f'{p}.floats'].tolist()
        ckw = dict(samples=i[0], order=i[1], random_sampling=bool(i[2]), remove_partials=bool(i[3]), flag_fragmented=bool(i[4]),
                   flag_fragmented_constant=i[5], min_fg_dist=f[0], max_bg_dist=f[1])
        fkw = dict(border=i[6], min_area=i[7], max_area=None if i[8] < 0 else i[8])
        rec = {k[len(p) + 1:]: v for k, v in z.items() if k.startswith(p + '.')}
        yield name, z[f'{p}.input'], ckw, fkw, i[9], bool(i[10]), rec


def oracle_feed(a, ckw, fkw):
    """CPNTargetGenerator.feed by the oracle's rules, contours aside: -> (labels before flagging, distances and masking of a
    labels image, as functions)."""
    lab = a[..., None] if a.ndim == 2 else a
    return oracle.filter_instances(lab, partials=ckw['remove_partials'], partials_border=fkw['border'], min_area=fkw['min_area'],
                                   max_area=fkw['max_area'], constant=-1, continuous=True)


def test_oracle_reproduces_every_recorded_distance_result():
    n = 0
    for key, a, dt, inst, prot, dist, lab, masked, reduced in distance_cases():
        d, l = oracle.labels2distances(a, dt, per_instance=inst, protected_size=prot)
        assert d.dtype == np.float32 and np.array_equal(d, dist), key
        assert np.array_equal(l, lab), key
        m, r = oracle.mask_labels_by_distance(lab, dist, BG, FG)
        assert np.array_equal(m, masked) and np.array_equal(r, reduced), key
        n += 1
    assert n == 29  # 8 anchors in two modes, the square with protected_size 0, two disc images in 3 types x 2 modes
    kinds = {(dt, inst) for _, _, dt, inst, *_ in distance_cases()}
    assert kinds == {(dt, inst) for dt in (1, 2, 3) for inst in (True, False)}


def test_every_mutant_differs_on_both_disc_images():
    for name in ('discs_c3', 'discs_c2'):
        cases = {key: rest for key, *rest in distance_cases() if key.startswith(name) and '.d2.' in key}
        a, _, _, _, dist, lab, masked, _ = cases[f'{name}.inst.d2.p36']
        for m in oracle.DISTANCE_MUTANTS:
            assert (oracle.labels2distances(a, mutant=m)[0] != dist).any(), (name, m)
        for m in oracle.MASK_MUTANTS:
            assert (oracle.mask_labels_by_distance(lab, dist, BG, FG, mutant=m)[0] != masked).any(), (name, m)
        a, _, _, _, dist, *_ = cases[f'{name}.fg.d2.p36']
        for m in oracle.FG_MUTANTS:
            assert (oracle.labels2distances(a, per_instance=False, mutant=m)[0] != dist).any(), (name, m)
    # counting per channel cannot differ where every label lives in one channel: the two-channel case tells it apart
    cases = {name: rest for name, *rest in filter_cases()}
    a, kw, res = cases['two_channel_counts']
    assert np.array_equal(oracle.filter_instances(a, **kw), res)
    for m in oracle.FILTER_MUTANTS:
        assert not np.array_equal(oracle.filter_instances(a, mutant=m, **kw), res)
    assert set(oracle.MUTANTS) == set(oracle.DISTANCE_MUTANTS + oracle.FG_MUTANTS + oracle.MASK_MUTANTS + oracle.FILTER_MUTANTS)
    assert len(oracle.MUTANTS) == 9


def test_hand_worked_anchor_values():
    f32 = np.float32
    s = f32(2. ** -16)
    cases = {key: rest for key, *rest in distance_cases()}
    # one pixel: the ring of zeros is one straight step away; 1 pixel <= 36: not normalised; 0.955 < 1: not clipped
    dist = cases['one_pixel.inst.d2.p36'][4]
    assert dist[2, 2] == f32(HV) * s and dist.sum() == dist[2, 2] and abs(float(dist[2, 2]) - .955) < 1e-5
    # 6 x 6 = 36 pixels is NOT more than the protected size: raw distances HV, 2 HV, 3 HV from the edge inwards, clipped to 1
    dist = cases['square_6x6.inst.d2.p36'][4]
    assert dist[2, 3] == f32(HV) * s and dist[3, 4] == 1. and dist[4, 5] == 1. and dist[2:8, 3:9].min() == f32(HV) * s
    # with protected_size 0 the same square is normalised by its maximum 3 HV
    dist = cases['square_6x6.inst.d2.p0'][4]
    assert dist[2, 3] == f32(HV) * s / (f32(3 * HV) * s) and dist[3, 4] == f32(2 * HV) * s / (f32(3 * HV) * s) and dist[4, 5] == 1.
    # 7 x 6 = 42 pixels: normalised; the middle row is 3 straight steps from the nearest edge
    dist = cases['rect_7x6.inst.d2.p36'][4]
    assert dist[1, 3] == f32(HV) * s / (f32(3 * HV) * s) and dist[4, 5] == 1. and dist[4, 6] == 1. and dist[3, 5] == 1.
    assert (dist[1:8, 3:9] > 0).all() and dist.sum() == dist[1:8, 3:9].sum()
    # image border and corner: outside counts as zero in instance mode, and does not in fg mode
    inst, fg = cases['border_corner.inst.d2.p36'][4], cases['border_corner.fg.d2.p36'][4]
    assert inst[0, 0] == f32(HV) * s  # 30 pixels: raw
    t = oracle.closed_form(np.pad(np.ones((5, 6), bool), ((0, 1), (0, 1))))  # fg mode: zeros only below and right of the 5 x 6 block
    assert fg[0, 0] == 1. and fg[4, 5] == f32(HV) * s / (f32(t.max()) * s) and t[0, 0] == t.max() == 5 * HV
    # two overlapping discs: overlap pixels have distance 0 and -1 in every channel of the labels
    a, dt, _, _, dist, lab, masked, reduced = cases['two_discs_overlap.inst.d2.p36']
    over = (a > 0).sum(2) > 1
    assert over.sum() > 10 and (dist[over] == 0).all() and (lab[over] == -1).all() and (lab[~over] == a[~over]).all()
    assert (reduced[over] == -1).all()  # -1 stays -1 under the masking
    # the neighbours of the overlap are one step from a zero pixel
    own = oracle.owner_image(a)
    assert dist[own == 1].max() == 1. and dist[own == 2].max() == 1.
    # one label in two channels: one object with one maximum over both pieces; the doubled pixels are overlap
    a, _, _, _, dist, lab, *_ = cases['one_label_two_channels.inst.d2.p36']
    own = oracle.owner_image(a)
    assert (own[5:8, 7:9] == 0).all() and (lab[5:8, 7:9] == -1).all() and (dist == 1.).sum() >= 1
    m = np.pad(own == 4, 1)
    t = oracle.closed_form(m)[1:-1, 1:-1]
    assert np.array_equal(dist[own == 4], (t.astype(f32) * s / (f32(t.max()) * s))[own == 4])
    # a label in two pieces: normalised by the maximum over both
    a, _, _, _, dist, *_ = cases['two_pieces.inst.d2.p36']
    assert dist[4, 4] == 1. and dist[9, 13] == 1. and dist[1, 1] == f32(HV) * s / (f32(4 * HV) * s)
    assert dist[10, 3] == 1. and dist[9, 2] == f32(HV) * s  # label 5: 16 pixels, raw, 2 HV clipped
    # negatives own nothing, are zero pixels for their neighbours and stay in the labels
    a, _, _, _, dist, lab, masked, reduced = cases['negatives.inst.d2.p36']
    assert (dist[a.max(2) <= 0] == 0).all() and np.array_equal(lab, a)
    assert (masked[0, :, 1] == -2).all() and (reduced[0] == 0).all()
    # masking on the 7 x 6 rectangle: d = 1/3 <= 0.5 -> 0, d = 2/3 in (0.5, 0.75) -> -1, d = 1 stays
    _, _, _, _, dist, lab, masked, reduced = cases['rect_7x6.inst.d2.p36']
    assert reduced[1, 3] == 0 and reduced[2, 4] == -1 and reduced[4, 5] == 1 and set(np.unique(reduced)) == {-1, 0, 1}


def test_two_pass_oracle_equals_literal_and_closed_form():
    rng = np.random.default_rng(0)
    for k in range(40):
        h, w = rng.integers(1, 14, 2)
        m = rng.random((h, w)) < rng.choice([.5, .8, .95, 1.])
        for dt in (1, 2, 3):
            assert np.array_equal(oracle.chamfer(m, dt), oracle.chamfer_literal(m, dt)), (k, dt)
            assert np.array_equal(oracle.chamfer(np.pad(m, 1), dt), oracle.closed_form(np.pad(m, 1), dt)), (k, dt)
    assert oracle.weights(2) == (HV, DIAG) and oracle.weights(1) == (65536, 131072) and oracle.weights(3) == (65536, 65536)
    seen = set()
    for key, a, dt, inst, prot, dist, *_ in distance_cases():
        name = key.split('.')[0]
        own = oracle.owner_image(a)
        if inst and (name, dt) not in seen and dt == 2:  # per object on its padded box
            seen.add((name, dt))
            for v in np.unique(own[own > 0]):
                m = np.pad(own == v, 1)
                assert np.array_equal(oracle.chamfer(m, dt), oracle.closed_form(m, dt)), (key, v)
        if not inst and (dt == 2 or a.size < 4000):  # the whole image at once
            assert np.array_equal(oracle.chamfer(own != 0, dt), oracle.closed_form(own != 0, dt)), key


def test_filter_oracle_against_the_reference():
    moved = 0
    for name, a, kw, res in filter_cases():
        got = oracle.filter_instances(a, **kw)
        assert oracle.same_partition(got, res), name
        assert np.array_equal(np.unique(got), np.unique(res)), name
        if not kw['continuous'] or 'gap_free' in name:
            assert np.array_equal(got, res), name
        else:
            moved += 1
            pos = np.unique(got[got > 0])
            assert np.array_equal(pos, np.arange(1, len(pos) + 1)), name
            keep = (a > 0) & (a <= len(pos)) & (got > 0)  # labels <= n stay
            assert np.array_equal(got[keep], a[keep]) and np.array_equal(res[keep], a[keep]), name
    assert moved >= 2
    cases = {name: (a, kw, res) for name, a, kw, res in filter_cases()}
    a, _, r0 = cases['partials_border0']
    assert np.array_equal(a, r0) and (cases['partials_border1'][2] != a).any()
    assert (cases['partials_border3'][2] != cases['partials_border1'][2]).any()
    assert (cases['min_area_at'][2] != cases['min_area_above'][2]).any() and (cases['max_area_at'][2] != cases['max_area_below'][2]).any()


def test_generator_oracle_against_the_reference():
    for name, a, ckw, fkw, seed, exact, rec in generator_cases():
        lab = oracle_feed(a, ckw, fkw)
        flagged = rec['labels']
        if exact:
            keep = flagged == lab  # what the contours flagged is the rest
            assert (flagged[~keep] == ckw['flag_fragmented_constant']).all(), name
            assert ckw['flag_fragmented'] or keep.all(), name
        else:
            assert oracle.same_partition(np.where(flagged > 0, flagged, 0), np.where(flagged > 0, lab, 0)), name
        d, l = oracle.labels2distances(flagged, 2)
        assert np.array_equal(d, rec['distances']), name
        m, r = oracle.mask_labels_by_distance(l, d, ckw['max_bg_dist'], ckw['min_fg_dist'])
        assert np.array_equal(m, rec['labels_red']) and np.array_equal(r, rec['reduced_labels']), name
        np.random.seed(seed)
        s = np.random.uniform(0., 1., ckw['samples']) if ckw['random_sampling'] else np.linspace(0., 1., ckw['samples'])
        s.sort()
        assert np.array_equal(s, rec['sampling']), name
    rec = {name: rec for name, *_, rec in generator_cases()}
    assert (rec['gen_two_pieces_flag']['labels'] != rec['gen_two_pieces_keep']['labels']).any()
    assert (rec['gen_two_pieces_flag']['distances'] != rec['gen_two_pieces_keep']['distances']).any()


def test_abi_header_bindings_and_exports_agree():
    names = ('cpn_label_distances_workspace_bytes', 'cpn_label_distances_table_bytes', 'cpn_label_distances_classify',
             'cpn_label_distances_step', 'cpn_label_distances_reduce', 'cpn_label_distances_finalise', 'cpn_label_distances_mask',
             'cpn_label_remap')
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    define = lambda what: int(re.search(r'#define\s+%s\s+(\d+)' % what, hdr).group(1))
    t = cda.targets
    assert define('CPN_LABEL_DISTANCES_MAX_STEPS') == t.MAX_STEPS
    assert (define('CPN_DIST_L1'), define('CPN_DIST_L2'), define('CPN_DIST_C')) == (t.DIST_L1, t.DIST_L2, t.DIST_C) == \
        (oracle.DIST_L1, oracle.DIST_L2, oracle.DIST_C)
    kernel = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'label_distances.hip')).read()
    assert not re.search(r'atomic\w*\s*\(\s*[^,]*,\s*\(?\s*(double|float)', kernel) and 'unsafeAtomicAdd' not in kernel
    assert str(HV) in kernel and str(DIAG) in kernel and str(HV) in hdr and str(DIAG) in hdr
    from celldetection_amd import build
    assert build.SOURCES['label_distances.hip'] == build.SOURCES['overlay.hip'] == \
        ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt']
    # argument checks answer before anything touches a device (the buffers are never dereferenced)
    buf = ctypes.create_string_buffer(4096)
    status = (ctypes.c_int64 * 2)()
    assert lib.cpn_label_distances_workspace_bytes(100, 100) >= 3 * 100 * 100 * 4
    assert lib.cpn_label_distances_workspace_bytes(-1, 4) == 0 and lib.cpn_label_distances_workspace_bytes(4, t.MAX_SIDE + 1) == 0
    assert lib.cpn_label_distances_table_bytes(1024) == 1024 * 12 and lib.cpn_label_distances_table_bytes(1000) == 0
    big = 1 << 40
    assert lib.cpn_label_distances_classify(buf, 0, 4, 4, 2, 1, buf, big, status, None) == _lib.E_INVALID
    assert lib.cpn_label_distances_classify(buf, 1, 4, 4, 4, 1, buf, big, status, None) == _lib.E_INVALID
    assert b'distance_type' in lib.cpn_last_error()
    assert lib.cpn_label_distances_classify(buf, 1, 4, 4, 2, 1, buf, 8, status, None) == _lib.E_WORKSPACE
    assert lib.cpn_label_distances_classify(buf, 1, 4, 40000, 2, 1, buf, big, status, None) == _lib.E_UNSUPPORTED
    assert lib.cpn_label_distances_step(4, 4, 0, 2, 1, 0, buf, big, status, None) == _lib.E_INVALID and b'steps' in lib.cpn_last_error()
    assert lib.cpn_label_distances_step(4, 4, 9, 2, 1, 0, buf, big, status, None) == _lib.E_INVALID
    assert lib.cpn_label_distances_step(4, 4, 8, 2, 1, -1, buf, big, status, None) == _lib.E_INVALID
    assert lib.cpn_label_distances_reduce(4, 4, buf, big, buf, 100, status, None) == _lib.E_INVALID
    assert lib.cpn_label_distances_finalise(buf, 1, 4, 4, 1, -1, buf, big, buf, 64, buf, buf, None) == _lib.E_INVALID
    assert lib.cpn_label_distances_finalise(buf, 1, 0, 4, 1, 36, buf, big, buf, 64, buf, buf, None) == 0
    assert lib.cpn_label_distances_mask(buf, 0, 4, buf, .5, .75, None, None) == _lib.E_INVALID
    assert lib.cpn_label_distances_mask(buf, 1, 0, buf, .5, .75, None, None) == 0
    assert lib.cpn_label_remap(buf, -1, buf, buf, 1, None) == _lib.E_INVALID and lib.cpn_label_remap(buf, 0, buf, buf, 1, None) == 0


def test_names_are_exported():
    names = {'targets', 'labels2distances', 'mask_labels_by_distance_', 'filter_instances_', 'CPNTargetGenerator'}
    assert names <= set(cda.__all__)
    t = cda.targets
    assert cda.labels2distances is t.labels2distances and cda.CPNTargetGenerator is t.CPNTargetGenerator
    assert cda.mask_labels_by_distance_ is t.mask_labels_by_distance_ and cda.filter_instances_ is t.filter_instances_
    for phrase in ('overlap_zero=False', 'sentinel', 'set iteration', 'drops the first unique value'):
        assert phrase in t.__doc__, phrase
    import celldetection_amd.torch_ops  # noqa: F401  (registers the operators)
    assert hasattr(torch.ops.celldetection_amd, 'labels2distances')


def test_no_cpu_fallback_and_argument_errors():
    a = torch.zeros((8, 9, 2), dtype=torch.int32)
    d = torch.zeros((8, 9))
    gen = cda.CPNTargetGenerator(samples=8, order=3)
    for call in (lambda: cda.labels2distances(a), lambda: cda.labels2distances(a[..., 0]), lambda: cda.filter_instances_(a),
                 lambda: cda.mask_labels_by_distance_(a, d, .5, .75), lambda: gen.feed(a)):
        with pytest.raises(RuntimeError, match='MI355X'):
            call()
    for bad in (a.float(), a.bool()):
        with pytest.raises(TypeError, match='integers'):
            cda.labels2distances(bad)
        with pytest.raises(TypeError, match='integers'):
            cda.filter_instances_(bad)
    with pytest.raises(TypeError, match='Tensor'):
        cda.labels2distances(np.zeros((8, 9, 2), np.int32))
    for bad in (a[0, 0], a[None]):
        with pytest.raises(ValueError, match=r'\[H, W, C\]'):
            cda.labels2distances(bad)
    with pytest.raises(NotImplementedError, match='overlap_zero'):
        cda.labels2distances(a, overlap_zero=False)
    with pytest.raises(NotImplementedError, match='overlap_zero'):
        cda.labels2distances(a, overlap_zero=False, per_instance=False)
    for dt in (0, 4, 6, 'l2', True):
        with pytest.raises(ValueError, match='distance_type'):
            cda.labels2distances(a, distance_type=dt)
    with pytest.raises(ValueError, match='protected_size'):
        cda.labels2distances(a, protected_size=-1)
    with pytest.raises(ValueError, match='distances must be'):
        cda.mask_labels_by_distance_(a, torch.zeros((8, 8)), .5, .75)
    with pytest.raises(ValueError, match='order'):
        cda.CPNTargetGenerator(samples=8, order=0)
    # the host part of filter_instances_: the table of values
    tab = cda.targets._filter_table
    uni, cnt = np.array([-1, 0, 2, 5, 9]), np.array([3, 50, 4, 7, 2])
    assert tab(uni, cnt, None, 4, None, -1, False).tolist() == [-1, 0, 2, 5, -1]
    assert tab(uni, cnt, None, 4, None, -1, True).tolist() == [-1, 0, 2, 1, -1]
    assert tab(uni, cnt, None, None, None, -1, True).tolist() == [-1, 0, 2, 1, 3]
    assert tab(uni, cnt, np.array([0, 5]), None, 6, -1, False).tolist() == [-1, 0, 2, -1, 9]
    assert tab(uni, cnt, np.array([-1, 0]), 1, 3, 7, False).tolist() == [7, 0, 7, 7, 9]  # -1 on the border becomes 7: 3 elements, kept
