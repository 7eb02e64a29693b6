"""CPU tests of the CPN training objective: ``tests/objective_oracle.py`` against the reference's recorded results
(``tests/golden/objective.npz``, written by ``tests/golden/make_golden_objective.py``), the wrong rules that the fixture has to tell
apart, the ABI and the argument checks of ``cda.CPNObjective`` / ``cda.collate_cpn_targets`` that need no device.

Bounds (``objective_oracle.term_bound``): the oracle's contours and boxes equal the recorded ones bit for bit; L1 terms lie within
(n + 8) * 2^-24 relative of the recorded float32 values; the score and iou terms within the cap (n + 64) * 2^-24, with the
measured ratio in ``tests/golden/objective_measured.json`` (``python tests/test_objective.py`` writes it, the test measures again);
a gradient element with m contributions of summed magnitude A lies within (m + 8) * 2^-24 * A and is exactly 0 where m = 0.
"""
import ctypes
import json
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, ROOT]
import objective_oracle as oracle  # noqa: E402

import celldetection_amd as cda  # noqa: E402
from celldetection_amd import _lib  # noqa: E402

MEASURED = os.path.join(HERE, 'golden', 'objective_measured.json')
CASES = oracle.load_fixture()
RESULTS = {}


def result(name):
    if name not in RESULTS:
        RESULTS[name] = oracle.run_case(CASES[name])
    return RESULTS[name]


def measure():
    """Largest |oracle - recorded| / (2^-24 * |recorded|) of the score and iou terms over the fixture, and where."""
    out = {}
    for key in ('score', 'iou'):
        worst = (0., None, 0)
        for name, case in CASES.items():
            v, n = result(name)['terms'][key]
            r = float(case['rec']['term_' + key])
            if v is None or r == 0:
                continue
            ratio = abs(v - r) / (2. ** -24 * abs(r))
            if ratio >= worst[0]:
                worst = (ratio, name, n)
        out[key] = dict(ratio=worst[0], case=worst[1], n=worst[2])
    return out


def test_fixture_holds_the_cases_of_the_issue():
    cfg = {k: c['config'] for k, c in CASES.items()}
    shape = lambda k, m: CASES[k]['maps'][m].shape
    assert cfg['base']['size'] == (32, 40) and shape('base', 'scores') == (2, 1, 16, 20) and cfg['base']['order'] == 3
    assert CASES['base']['targets']['sampling'].shape == (2, 8)
    assert cfg['nearest']['size'] == (35, 41) and shape('nearest', 'scores')[2:] == (18, 21)
    assert cfg['stride4']['size'] == (32, 40) and shape('stride4', 'scores')[2:] == (8, 10)
    assert {cfg[k]['order'] for k in CASES} >= {1, 3, 8}
    assert {c['targets']['sampling'].shape[1] for c in CASES.values()} >= {1, 8, 32, 65}
    assert cfg['buckets4']['buckets'] == 4 and shape('buckets4', 'refinement')[1] == 8
    assert cfg['classes4']['classes'] == 4 and 'classes' in CASES['classes4']['targets'] and shape('classes4', 'scores')[1] == 4
    assert not cfg['no_refinement']['refine'] and CASES['no_refinement']['maps']['refinement'] is None
    assert shape('order_core', 'fourier')[1] == 20 and cfg['order_core']['order'] == 3
    assert not CASES['no_foreground']['targets']['labels'][0].any() and CASES['no_foreground']['targets']['labels'][1].any()
    assert (CASES['all_foreground']['targets']['labels'][0] > 0).all()
    assert (CASES['negative']['targets']['labels'] == -1).sum() > 20
    assert not cfg['order_weights_off']['order_weights'] and cfg['weights']['weights']['contour'] == 1.5
    # contours that leave the image on every side; boxes thinner than 1, and a case where every box is
    p, (H, W) = result('outside')['detail']['refined'], cfg['outside']['size']
    raw = CASES['outside']['rec']['proposals']
    assert raw[..., 0].min() < 0 and raw[..., 1].min() < 0 and raw[..., 0].max() > W - 1 and raw[..., 1].max() > H - 1 and len(p) == 4
    thin = lambda k: ((CASES[k]['rec']['boxes'][:, 2] - CASES[k]['rec']['boxes'][:, 0] < 1) |
                      (CASES[k]['rec']['boxes'][:, 3] - CASES[k]['rec']['boxes'][:, 1] < 1))
    assert 0 < thin('thin').sum() < len(thin('thin')) and thin('all_thin').all() and len(thin('all_thin')) > 10
    assert float(CASES['all_thin']['rec']['term_iou']) == 0. and not CASES['all_thin']['rec']['none_iou']
    assert [k for k in oracle.KEYS if not CASES['no_proposals']['rec']['none_' + k]] == ['score']
    assert os.path.getsize(os.path.join(HERE, 'golden', 'objective.npz')) < 1 << 20


@pytest.mark.parametrize('name', list(CASES))
def test_oracle_equals_the_reference(name):
    case, res = CASES[name], result(name)
    rec, d = case['rec'], res['detail']
    assert d['proposals'].dtype == np.float32 and np.array_equal(d['proposals'], rec['proposals'])
    assert np.array_equal(d['boxes'], rec['boxes'])
    assert np.array_equal(d['refined'][-1] if d['refined'] else d['proposals'], rec['contours'])
    for k in oracle.KEYS:
        v, n = res['terms'][k]
        assert (v is None) == bool(rec['none_' + k]), k
        if v is not None:
            r = float(rec['term_' + k])
            assert abs(v - r) <= oracle.term_bound(k, n) * abs(r), (k, v, r, n)
    assert abs(res['loss'] - float(rec['loss'])) <= 8 * 2. ** -24 * abs(float(rec['loss'])) + \
        sum(oracle.term_bound(k, n) * abs(v) for k, (v, n) in res['terms'].items() if v is not None)
    for k in ('scores', 'locations', 'fourier', 'refinement'):
        if res['grads'][k] is None:
            assert 'grad_' + k not in rec
            continue
        v, m, a = res['grads'][k]
        r = rec['grad_' + k].astype(np.float64)
        nan = np.isnan(r)
        assert np.array_equal(np.isnan(v), nan), k
        assert (np.abs(v - r)[~nan] <= ((m + 8) * 2. ** -24 * a)[~nan]).all(), k
        assert (r[(m == 0) & ~nan] == 0).all() and (v[(m == 0) & ~nan] == 0).all(), k
    assert not oracle.departs(res, rec)


def test_order_one_with_order_weights_is_the_reference_nan():
    """``order_weighting(1)`` is 0 / 0 there: the fourier term counts as 0, its gradient is NaN at every proposal."""
    rec = CASES['order1']['rec']
    b, y, x = result('order1')['detail']['index']
    assert float(rec['term_fourier']) == 0. and np.isnan(rec['grad_fourier'][b, :, y, x]).all()
    assert np.isnan(rec['grad_fourier']).sum() == 4 * len(b)
    assert not np.isnan(CASES['order1_plain']['rec']['grad_fourier']).any()
    assert torch.isnan(cda.objective.order_weighting(1)).all()
    assert np.array_equal(cda.objective.order_weighting(5).numpy()[:, 0], oracle.order_weighting(5))


@pytest.mark.parametrize('rule', oracle.WRONG_RULES)
def test_wrong_rule_fails_on_the_fixture(rule):
    order = ['nearest', 'thin', 'base'] + [k for k in CASES if k not in ('nearest', 'thin', 'base')]
    caught = next((name for name in order if oracle.departs(oracle.run_case(CASES[name], (rule,)), CASES[name]['rec'])), None)
    assert caught is not None, rule
    assert len(oracle.WRONG_RULES) >= 8


def test_score_and_iou_terms_hold_their_cap_and_the_committed_measurement():
    now = measure()
    with open(MEASURED) as f:
        committed = json.load(f)
    for key in ('score', 'iou'):
        print(key, now[key])
        assert now[key]['ratio'] <= now[key]['n'] + 64
        assert committed[key]['case'] == now[key]['case'] and abs(committed[key]['ratio'] - now[key]['ratio']) <= .5, (key, committed, now)


def test_abi_header_bindings_and_exports_agree():
    names = ('cpn_objective_head_workspace_bytes', 'cpn_objective_head', 'cpn_objective_workspace_bytes', 'cpn_objective_proposals')
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    assert 'Training objective' in hdr and lib.cpn_abi_version() == _lib.ABI_VERSION
    define = lambda what: int(re.search(r'#define\s+%s\s+(\d+)' % what, hdr).group(1))
    assert define('CPN_OBJECTIVE_MAX_ITERATIONS') == _lib.OBJECTIVE_MAX_ITERATIONS
    assert define('CPN_OBJECTIVE_META_WORDS') == _lib.OBJECTIVE_META_WORDS
    assert (define('CPN_OBJECTIVE_FLAG_LABEL_RANGE'), define('CPN_OBJECTIVE_FLAG_LABEL_ROWS'), define('CPN_OBJECTIVE_FLAG_CLASS_RANGE')) == \
        (_lib.OBJECTIVE_FLAG_LABEL_RANGE, _lib.OBJECTIVE_FLAG_LABEL_ROWS, _lib.OBJECTIVE_FLAG_CLASS_RANGE)
    # the struct of the header and the ctypes mirror list the same fields in the same order
    body = re.search(r'typedef struct CpnObjectiveArgs \{(.*?)\} CpnObjectiveArgs;', hdr, re.S).group(1)
    fields = [f.strip(' *') for decl in body.split(';') if decl.strip() for f in decl.strip().split(' ', 2 if decl.strip().startswith('const') else 1)[-1].split(',')]
    assert fields == [f[0] for f in _lib.ObjectiveArgs._fields_], fields
    assert ctypes.sizeof(_lib.ObjectiveArgs) == 21 * 8 + 7 * 8 + 14 * 4
    kernel = open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'cpn_objective.hip')).read()
    assert not re.search(r'atomic\w*\s*\(\s*[^,]*,\s*\(?\s*(double|float)', kernel) and 'unsafeAtomicAdd' not in kernel
    assert '#include "decode_device.h"' in kernel
    assert '#include "decode_device.h"' in open(os.path.join(ROOT, 'celldetection_amd', 'csrc', 'decode_nms.hip')).read()
    from celldetection_amd import build
    assert build.SOURCES['cpn_objective.hip'] == build.SOURCES['decode_nms.hip'] == ['-ffp-contract=off']
    assert 'decode_device.h' in build.HEADERS


def test_argument_checks_answer_before_a_device_is_touched():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    addr = ctypes.addressof(buf)

    def args(**kw):
        a = _lib.ObjectiveArgs()
        for k in ('scores', 'locations', 'refinement', 'fourier', 'labels', 't_fourier', 't_locations', 't_contours', 'cos_table',
                  'sin_table'):
            setattr(a, k, addr)
        for k, v in dict(N=2, score_channels=1, h=8, w=10, H=16, W=20, order_total=3, order=3, samples=8, K=5, iterations=4,
                         buckets=1).items():
            setattr(a, k, v)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    big = 1 << 40
    head = lambda a, ws=big: lib.cpn_objective_head(ctypes.byref(a), addr, addr, addr, ws, None)
    assert lib.cpn_objective_head_workspace_bytes(2, 8, 10) >= 2 * 8 * 10 * 8
    assert lib.cpn_objective_head_workspace_bytes(0, 8, 10) == 0 and lib.cpn_objective_head_workspace_bytes(1 << 15, 1 << 8, 1 << 8) == 0
    assert lib.cpn_objective_workspace_bytes(ctypes.byref(args()), 100) > 100 * 9 * 8
    assert lib.cpn_objective_workspace_bytes(ctypes.byref(args(order=4)), 100) == 0
    for bad, text in ((dict(N=0), b'positive'), (dict(h=17), b'head grid'), (dict(order=4), b'order'), (dict(order=65, order_total=65), b'order'),
                      (dict(samples=0), b'samples'), (dict(iterations=65), b'iterations'), (dict(buckets=0), b'buckets'),
                      (dict(scores=None), b'must be given'), (dict(t_contours=None), b'targets'), (dict(buckets=4), b'bucket tables'),
                      (dict(refinement=None, g_refinement=addr), b'refinement map')):
        assert head(args(**bad)) == _lib.E_INVALID and text in lib.cpn_last_error(), (bad, lib.cpn_last_error())
        assert lib.cpn_objective_proposals(ctypes.byref(args(**bad)), addr, 1, addr, 0, addr, addr, big, addr, None) == _lib.E_INVALID
    assert head(args(N=1 << 15, h=1 << 8, w=1 << 8, H=1 << 8, W=1 << 8)) == _lib.E_UNSUPPORTED
    assert head(args(), ws=8) == _lib.E_WORKSPACE
    a = args()
    assert lib.cpn_objective_proposals(ctypes.byref(a), addr, -1, addr, 0, addr, addr, big, addr, None) == _lib.E_INVALID
    assert lib.cpn_objective_proposals(ctypes.byref(a), addr, 1, addr, 0, addr, addr, 8, addr, None) == _lib.E_WORKSPACE
    assert lib.cpn_objective_proposals(ctypes.byref(args(g_refinement=addr)), addr, 1 << 30, addr, 0, addr, addr, big, addr, None) == \
        _lib.E_UNSUPPORTED


def cpu_call(obj=None, **change):
    obj = obj or cda.CPNObjective(3, 8)
    t = dict(scores=torch.zeros(2, 1, 8, 10), locations=torch.zeros(2, 2, 8, 10), refinement=torch.zeros(2, 2, 16, 20),
             fourier=torch.zeros(2, 12, 8, 10))
    tg = dict(labels=torch.zeros((2, 16, 20), dtype=torch.int64), fourier=torch.zeros(2, 5, 3, 4), locations=torch.zeros(2, 5, 2),
              sampled_contours=torch.zeros(2, 5, 8, 2), sampling=torch.zeros(2, 8))
    size = change.pop('size', (16, 20))
    extra = {k: change.pop(k) for k in ('uncertainty',) if k in change}
    for k, v in change.items():
        (t if k in t else tg)[k[2:] if k.startswith('t_') else k] = v
    return obj(t['scores'], t['locations'], t['refinement'], t['fourier'], tg, size=size, **extra)


def test_names_attributes_and_errors_without_a_device():
    assert {'objective', 'CPNObjective', 'collate_cpn_targets'} <= set(cda.__all__)
    assert cda.CPNObjective is cda.objective.CPNObjective and cda.collate_cpn_targets is cda.objective.collate_cpn_targets
    obj = cda.CPNObjective(5, 32)
    assert (obj.order, obj.samples, obj.classes, obj.refinement, obj.refinement_iterations, obj.refinement_buckets) == (5, 32, 2, True, 4, 1)
    assert obj.weights == oracle.DEFAULT_WEIGHTS == cda.objective.DEFAULT_WEIGHTS and obj.order_weights.shape == (5, 1)
    assert cda.CPNObjective(5, 32, order_weights=False).order_weights == 1. and cda.CPNObjective(5, 32, classes=4).score_channels == 4
    assert cda.objective.LOSS_KEYS == oracle.KEYS
    import celldetection_amd.torch_ops  # noqa: F401  (registers the operators)
    assert hasattr(torch.ops.celldetection_amd, 'cpn_objective')
    for kw in (dict(uncertainty_head=True), dict(certainty_thresh=.5), dict(functional=True), dict(objectives={})):
        with pytest.raises(NotImplementedError):
            cda.CPNObjective(5, 32, **kw)
    for kw in (dict(order=0), dict(order=65), dict(samples=0), dict(refinement_buckets=0), dict(weights=dict(bogus=1.)),
               dict(order_weights=torch.ones(4, 1))):
        with pytest.raises(ValueError):
            cda.CPNObjective(**dict(dict(order=5, samples=32), **kw))
    # no CPU fallback: RuntimeError naming the GPU (a ValueError too: the tensors are not on the GPU)
    with pytest.raises(RuntimeError, match='GPU'):
        cpu_call()
    with pytest.raises(ValueError, match='GPU'):
        cpu_call()
    for change in (dict(uncertainty=torch.zeros(2, 4, 8, 10)), dict(t_boxes=torch.zeros(2, 5, 4)),
                   dict(t_hires_sampled_contours=torch.zeros(2, 5, 16, 2))):
        with pytest.raises(NotImplementedError):
            cpu_call(**change)
    for change in (dict(scores=torch.zeros(2, 2, 8, 10)), dict(locations=torch.zeros(2, 2, 8, 11)), dict(fourier=torch.zeros(2, 8, 8, 10)),
                   dict(fourier=torch.zeros(2, 13, 8, 10)), dict(refinement=torch.zeros(2, 4, 16, 20)), dict(size=(16, 21)),
                   dict(size=(4, 20), t_labels=torch.zeros((2, 4, 20), dtype=torch.int64), refinement=torch.zeros(2, 2, 4, 20)),
                   dict(t_sampling=torch.zeros(2, 9)), dict(t_fourier=torch.zeros(2, 5, 4, 4)), dict(t_locations=torch.zeros(2, 4, 2)),
                   dict(t_sampled_contours=torch.zeros(2, 5, 9, 2)), dict(t_classes=torch.zeros((2, 4), dtype=torch.int64)),
                   dict(refinement=None)):
        with pytest.raises(ValueError) as e:
            cpu_call(**change)
        assert not isinstance(e.value, RuntimeError), change  # the shapes are refused before the device is looked at
    with pytest.raises(TypeError):
        cpu_call(t_labels=torch.zeros(2, 16, 20))
    with pytest.raises(TypeError):
        cpu_call(scores=torch.zeros(2, 1, 8, 10, dtype=torch.float64))
    # the inference engine keeps refusing to train (tests/test_host_logic.py pins model.train())
    model = cda.models.CpnU22(3, backbone_kwargs={'backbone_kwargs': {'base_channels': 8}})
    with pytest.raises(NotImplementedError):
        model.train()


def test_collate_pads_along_k_and_stacks_the_rest():
    pad = cda.objective._pad_and_stack
    rng = np.random.RandomState(0)
    ks, order, S, (H, W) = (3, 0, 5), 2, 4, (6, 7)
    items = [SimpleNamespace(labels=torch.as_tensor(rng.randint(-1, 4, (H, W)).astype(np.int32)),
                             fourier=torch.as_tensor(rng.randn(k, order, 4).astype(np.float32)),
                             locations=torch.as_tensor(rng.randn(k, 2).astype(np.float32)),
                             contours=torch.as_tensor(rng.randn(k, S, 2).astype(np.float32)),
                             sampling=np.sort(rng.uniform(0, 1, S))) for k in ks]
    call = lambda its: pad([i.labels for i in its], [i.fourier for i in its], [i.locations for i in its], [i.contours for i in its],
                           [i.sampling for i in its])
    out = call(items)
    assert list(out) == ['labels', 'fourier', 'locations', 'sampled_contours', 'sampling']
    assert out['labels'].shape == (3, H, W) and out['labels'].dtype == torch.int32
    assert out['fourier'].shape == (3, 5, order, 4) and out['locations'].shape == (3, 5, 2) and out['sampled_contours'].shape == (3, 5, S, 2)
    assert out['sampling'].dtype == torch.float32 and out['sampling'].shape == (3, S)
    for n, (k, it) in enumerate(zip(ks, items)):
        assert torch.equal(out['labels'][n], it.labels)
        for key, src in (('fourier', it.fourier), ('locations', it.locations), ('sampled_contours', it.contours)):
            assert torch.equal(out[key][n, :k], src) and not out[key][n, k:].any()
        assert np.array_equal(out['sampling'][n].numpy(), it.sampling.astype(np.float32))
    items[1].contours = torch.zeros(0, S + 1, 2)
    with pytest.raises(ValueError, match='sampled_contours'):
        call(items)
    with pytest.raises(ValueError):
        call([])
    with pytest.raises(ValueError, match='fed'):
        cda.collate_cpn_targets([cda.CPNTargetGenerator(samples=4, order=2)])
    fed = SimpleNamespace(reduced_labels=items[0].labels, fourier=items[0].fourier, locations=items[0].locations,
                          sampled_contours=items[0].contours, sampling=items[0].sampling)
    with pytest.raises(RuntimeError, match='GPU'):
        cda.collate_cpn_targets([fed])


if __name__ == '__main__':
    with open(MEASURED, 'w') as f:
        json.dump(measure(), f, indent=1)
        f.write('\n')
    print(open(MEASURED).read())
