"""No result of a plan depends on what the activation arena held before the run.

The product arena is uninitialised memory, placed by a liveness-based first fit (csrc/plan_shapes.hip) and reused from run to run:
a kernel that reads a region no op of this run has written gets plausible activations of another layer, finite and the same
from run to run.  Here every plan runs with its arena, the bytes past it and its external outputs pre-filled with each of the
three byte patterns of tests/read_guards.py (NaN, zero and plausible data in every storage type), and once more into the arena a
run at ANOTHER size left behind: all external outputs are finite and the same bits in the four runs.  No tolerance: the runs are
the same code on the same operands, and every reduction of this project has a fixed order.

Two positive controls show that the poison was where the plan leaves bytes unwritten: the interior of the resized map of an fp8
FPN plan in ring mode, and the input tensor's storage beyond the padded stem layout.  A last test goes through the public path
(CPN.forward with score-gated heads and the post-processing, which read the arena after the run).

Results allowed to differ between the runs (they are not compared): none of the external outputs.  Arena regions the header
documents as unwritten -- the ring interior, the tail of the stem record's storage -- are internal and are what the controls
inspect.
"""
import os
from ctypes import byref, c_int32, c_int64, c_void_p

import pytest
import torch

import read_guards as rg
from model_specs import ALL_SPECS
from celldetection_amd import _lib

pytestmark = pytest.mark.gpu
WS_GUARD = 4096
N = 2
FPN_SCALE = .01  # constant fp8 activation scale, as test_fp8_resize_ring_mode
MODELS = {  # name in tests/model_specs.py -> the sizes: one where the fused alternatives run, one odd size where they do not
    'CpnU22': ((64, 96), (75, 101)),
    'CpnResNeXt101UNet': ((64, 96), (75, 101)),
    'CpnResNet18FPN': ((64, 96), (75, 101)),
    'CpnResNet50FPN': ((64, 96), (75, 101)),
    'CpnU22_classes4': ((64, 96), (75, 101)),
    'CpnU22_uncertainty': ((64, 96), (75, 101)),
    'CpnResNet18FPN_bicubic_lowres': ((64, 96), (75, 101)),   # (the head's output maps are resized after the plan has run)
    'CpnResNet18FPN_bicubic': ((64, 96), (75, 101)),          # the bicubic resize as an op of the plan: bf16 and fp32 plans only
}
FPN = ('CpnResNet18FPN', 'CpnResNet50FPN', 'CpnResNet18FPN_bicubic_lowres')
PRECISIONS = ('bf16', 'fp8', 'fp32')
CODE = dict(bf16=_lib.PRECISION_BF16, fp8=_lib.PRECISION_FP8, fp32=_lib.PRECISION_F32)
NO_FP8 = ('CpnResNet18FPN_bicubic',)  # pack.py: bicubic weights are negative in places, the result leaves the e4m3 range of its source
CASES = [(m, p, s, None) for m in MODELS for p in PRECISIONS for s in MODELS[m] if not (p == 'fp8' and m in NO_FP8)] + \
        [(m, p, s, '2') for m in FPN for p in PRECISIONS for s in MODELS[m]]


def case_id(c):
    m, p, (h, w), bl = c
    return f'{m}-{p}-{h}x{w}' + (f'-BLPHASE{bl}' if bl else '')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault():
    """A faulted device runs nothing more: the session ends instead of starting the remaining tests on it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'GPU fault, nothing more is started: {e}', 3)


@pytest.fixture
def blphase():
    """Sets CPN_BLPHASE for the test and restores the environment afterwards."""
    before = os.environ.pop('CPN_BLPHASE', None)

    def set_to(value):
        os.environ.pop('CPN_BLPHASE', None)
        if value is not None:
            os.environ['CPN_BLPHASE'] = value
    yield set_to
    os.environ.pop('CPN_BLPHASE', None)
    if before is not None:
        os.environ['CPN_BLPHASE'] = before


_models = {}


def build_model(name):
    import celldetection_amd as cda
    from celldetection_amd.synth import synth_state_dict
    if name not in _models:
        spec = ALL_SPECS[name]
        model = getattr(cda.models, spec['cls'])(**spec['kwargs'])
        model.load_state_dict(synth_state_dict(model.state_dict(), seed=0))
        _models[name] = model
    return _models[name]


class PackedPlan:
    """A model's plan for one precision, packed and created; run() executes it into caller-prepared memory."""

    def __init__(self, name, prec, dev):
        from celldetection_amd import graph
        model = build_model(name)
        plan = model.plan_for(prec)
        kw = dict(act_scales=[FPN_SCALE] * len(plan.tensors)) if prec == 'fp8' else {}
        self.tens, self.ops, self.wblob, self.bblob = graph.pack(plan, model.state_dict(), dev, precision=prec, **kw)[:4]
        self.prec, self.dev, self.lib = prec, dev, _lib.load()
        self.handle = c_void_p()
        _lib.check(self.lib.cpn_plan_create(self.handle, self.tens, len(self.tens), self.ops, len(self.ops), _lib.ptr(self.wblob),
                                            self.wblob.numel() * self.wblob.element_size(), _lib.ptr(self.bblob), self.bblob.numel(),
                                            CODE[prec]), 'plan_create')
        # channels of every external output: the widest conv that writes it (0: no op writes it)
        self.channels = [max([max(o.cout_real, o.fuse_cout) for o in self.ops if o.dst < 0 and o.out_index == i and o.op == _lib.OP_CONV] + [0])
                         for i in range(_lib.NUM_OUTPUTS)]
        assert self.channels[_lib.OUT_SCORES] > 0

    def close(self):
        self.lib.cpn_plan_destroy(self.handle)

    def need(self, h, w):
        total = self.lib.cpn_plan_workspace_bytes(self.handle, N, h, w)
        assert total > 0, self.lib.cpn_last_error().decode()
        return int(total)

    def outputs(self, h, w, pattern):
        outs = []
        for i in range(_lib.NUM_OUTPUTS):
            oh, ow = c_int32(), c_int32()
            _lib.check(self.lib.cpn_plan_output_dims(self.handle, h, w, i, byref(oh), byref(ow)), 'output_dims')
            count = N * self.channels[i] * oh.value * ow.value
            assert count > 0 or self.channels[i] == 0, f'output {i} has no pixels'
            outs.append(torch.full((max(count, 1) * 4 + WS_GUARD,), pattern, dtype=torch.uint8, device=self.dev))
        return outs

    def tensor_span(self, h, w, t):
        off, th, tw, ch = c_int64(), c_int32(), c_int32(), c_int32()
        _lib.check(self.lib.cpn_plan_tensor_info(self.handle, N, h, w, t, byref(off), byref(th), byref(tw), byref(ch)), 'tensor_info')
        return off.value, (N, th.value, tw.value, ch.value)

    def run(self, x, ws, pattern):
        """One cpn_plan_run of the batch x into the arena ``ws`` (used as it is) and outputs filled with ``pattern`` ->
        ({output name: fp32 tensor on the CPU}, arena bytes on the CPU).  The bytes past the workspace and past every output are
        intact, the range flag is 0."""
        h, w = x.shape[-2:]
        total = self.need(h, w)
        assert ws.numel() >= total + WS_GUARD
        tail = ws[total:total + WS_GUARD].cpu()
        outs = self.outputs(h, w, pattern)
        flag = torch.zeros(1, dtype=torch.int32, device=self.dev)
        _lib.check(self.lib.cpn_plan_run(self.handle, _lib.ptr(x), 0, N, h, w, _lib.ptr(ws), total,
                                         (c_void_p * _lib.NUM_OUTPUTS)(*[o.data_ptr() for o in outs]), _lib.ptr(flag), _lib.stream_ptr()), 'plan_run')
        torch.cuda.synchronize()
        host = ws.cpu()
        assert torch.equal(host[total:total + WS_GUARD], tail), 'the plan wrote past the workspace size it asked for'
        assert int(flag.item()) == 0, 'range flag'
        got = {}
        for i, o in enumerate(outs):
            if self.channels[i]:
                o = o.cpu()
                assert bool((o[-WS_GUARD:] == pattern).all()), f'the plan wrote past external output {i}'
                got[f'output {i}'] = o[:-WS_GUARD].view(torch.float32)
        return got, host


_plans = {}


@pytest.fixture(scope='module')
def packed(dev):
    def get(name, prec, bl):
        key = (name, prec, bl)
        if key not in _plans:
            _plans[key] = PackedPlan(name, prec, dev)
        return _plans[key]
    yield get
    for p in _plans.values():
        p.close()
    _plans.clear()


def batch(dev, h, w):
    return torch.rand(N, 3, h, w, generator=torch.Generator().manual_seed(h * 1000 + w)).to(dev)


def poisoned_runs(plan, x):
    """The three runs into a pre-filled arena -> ({pattern: outputs}, {pattern: arena bytes})."""
    h, w = x.shape[-2:]
    res, arenas = {}, {}
    for pattern in rg.PATTERNS:
        ws = torch.full((plan.need(h, w) + WS_GUARD,), pattern, dtype=torch.uint8, device=x.device)
        res[pattern], arenas[pattern] = plan.run(x, ws, pattern)
    return res, arenas


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_outputs_do_not_depend_on_the_arena(dev, packed, blphase, case):
    name, prec, (h, w), bl = case
    blphase(bl)
    plan = packed(name, prec, bl)
    x = batch(dev, h, w)
    res, _ = poisoned_runs(plan, x)
    # a fourth run into the arena a run at another size left behind, with no refill
    oh, ow = [s for s in MODELS[name] if s != (h, w)][0]
    ws = torch.full((max(plan.need(h, w), plan.need(oh, ow)) + WS_GUARD,), rg.NAN, dtype=torch.uint8, device=dev)
    plan.run(batch(dev, oh, ow), ws, rg.NAN)
    res[f'after a {oh}x{ow} run'], _ = plan.run(x, ws, rg.NAN)
    rg.same_bits_across(res)
    # (synthetic weights saturate the sigmoid of some score heads to 0 / 1; the location and Fourier maps are not bounded)
    assert any(v.unique().numel() > 8 for k, v in res[rg.ZERO].items() if k != f'output {_lib.OUT_SCORES}'), \
        'every head map is (nearly) constant: the case checks nothing'


def never_written(arenas, lo, hi):
    """Bytes of [lo, hi) that hold the fill pattern after each of the three runs."""
    keep = torch.ones(hi - lo, dtype=torch.bool)
    for pattern, host in arenas.items():
        keep &= host[lo:hi] == pattern
    return keep


@pytest.mark.parametrize('name', ['CpnResNet18FPN', 'CpnResNet50FPN'])
def test_control_ring_interior_keeps_the_poison(dev, packed, blphase, name):
    """fp8 FPN plan in ring mode (CPN_BLPHASE=2, 64x96: the resize is an exact x2): the resize writes only the pixels within 7 of
    the border.  Of the interior, whatever the first fit did not place on an earlier, dead tensor still holds the fill after the
    run -- 0xFF after the 0xFF run: the poison was in place where the plan leaves bytes unwritten, and the outputs agree anyway."""
    blphase('2')
    plan = packed(name, 'fp8', '2')
    h, w, ring = 64, 96, 7
    (ri,) = [i for i, o in enumerate(plan.ops) if o.op == _lib.OP_BILINEAR]
    off, shape = plan.tensor_span(h, w, plan.ops[ri].dst)
    assert shape[1:3] == (h, w)
    res, arenas = poisoned_runs(plan, batch(dev, h, w))
    rg.same_bits_across(res)
    size = shape[0] * shape[1] * shape[2] * shape[3]
    kept = never_written(arenas, off, off + size).view(shape)
    interior = kept[:, ring:h - ring, ring:w - ring]
    share = interior.float().mean().item()
    print(f'{name} fp8 ring mode {h}x{w}: {100 * share:.1f} % of the interior bytes of the resized map still hold the fill after the run')
    assert share > 0, 'the interior of the resize destination was written: the plan did not run the resize in ring mode'
    ff = arenas[rg.NAN][off:off + size].view(shape)[:, ring:h - ring, ring:w - ring]
    assert bool((ff[interior] == rg.NAN).all())


@pytest.mark.parametrize('name', ['CpnResNet18FPN'])
def test_control_stem_record_tail_keeps_the_poison(dev, packed, blphase, name):
    """bf16 run on the stem fast path: the padded [H + 6][W + 8][4] input record lies inside the input tensor's storage and does not
    fill it.  Of the rest of that storage, whatever the first fit did not hand to a later tensor still holds the fill after the run.
    (In the plan of CpnResNeXt101UNet at this size later tensors take all of it: no byte is left to inspect, so the FPN plan is the
    control.)"""
    blphase(None)
    plan = packed(name, 'bf16', None)
    h, w = 64, 96
    stems = [o for o in plan.ops if o.op == _lib.OP_INPUT_STEM]
    assert len(stems) == 1, 'the plan has no stem fast path'
    t = stems[0].dst
    off, shape = plan.tensor_span(h, w, t)
    record, storage = (h + 6) * (w + 8) * 8, h * w * shape[3] * 2
    assert record <= storage, 'the padded layout does not fit: the generic stem runs at this size'   # the rule of csrc/plan_shapes.hip
    res, arenas = poisoned_runs(plan, batch(dev, h, w))
    rg.same_bits_across(res)
    # the record holds N images back to back from the start of the storage
    lo, hi = off + N * record, off + N * storage
    kept = never_written(arenas, lo, hi)
    print(f'{name} bf16 stem fast path {h}x{w}: {int(kept.sum())} of {hi - lo} bytes behind the stem record still hold the fill after the run')
    assert int(kept.sum()) > 0
    assert bool((arenas[rg.NAN][lo:hi][kept] == rg.NAN).all())
    # the record itself was written: its zero borders and the pixels do not keep all three fills
    assert never_written(arenas, off, off + N * record).float().mean().item() < .01


def public_model(dev, name):
    import celldetection_amd as cda
    if name == 'CpnResNet18FPN':  # full width, bench.py's synthetic weights with live heads, as tests/test_gpu_sparse_heads.py
        import test_gpu_sparse_heads as ts
        model = cda.models.CpnResNet18FPN(3)
        model.load_state_dict(ts._model(dev).state_dict())
        return model.to(dev).eval(), torch.rand(N, 3, 96, 160, generator=torch.Generator().manual_seed(1))
    import cpn_oracle as orc
    from celldetection_amd.synth import calibrate_heads, synth_state_dict
    spec = ALL_SPECS[name]
    model = getattr(cda.models, spec['cls'])(**spec['kwargs'])
    x = torch.rand(N, 3, 64, 96, generator=torch.Generator().manual_seed(7))
    sd, _ = calibrate_heads(synth_state_dict(model.state_dict(), seed=0), lambda s: orc.core_forward(s, x))  # some detections
    model.load_state_dict(sd)
    return model.to(dev).eval(), x


@pytest.mark.parametrize('name,gated', [('CpnU22', False), ('CpnResNet18FPN', True)])
def test_public_forward_does_not_depend_on_the_arena(dev, monkeypatch, name, gated):
    """CPN.forward with the default sparse_heads='auto' and CPN_HIP_GRAPH=0: the engine is handed arenas pre-filled with each pattern
    (_Engine.workspace keeps an arena that is large enough) and must return the same detections.  CpnU22: the post-processing reads
    the head maps; its heads are 64 wide and do not qualify for the score gate (graph.build_plan), so 'auto' runs the dense plan.
    CpnResNet18FPN: the score-gated location / Fourier heads read their source in the arena after the conv graph has run."""
    monkeypatch.setenv('CPN_HIP_GRAPH', '0')
    model, x = public_model(dev, name)
    assert model.sparse_heads == 'auto'
    h, w = x.shape[-2:]
    eng = model.engine(dev, _forward_path=True)
    assert bool(eng.sparse) == gated
    need = int(_lib.load().cpn_plan_workspace_bytes(eng.handle, N, h, w))
    res = {}
    for pattern in rg.PATTERNS:
        arenas = [torch.full((need + WS_GUARD,), pattern, dtype=torch.uint8, device=dev) for _ in range(2)]
        eng._ws_ring, eng._ws = list(arenas), arenas[0]
        y = model(x.to(dev))
        torch.cuda.synchronize()
        assert model.engine(dev, _forward_path=True) is eng and (eng.last_sparse is not None) == gated
        if gated:
            assert eng.last_sparse['ws'].data_ptr() in [a.data_ptr() for a in arenas], 'the run did not use the arena it was handed'
        assert any(bool((a[:need] != pattern).any()) for a in arenas), 'the run did not use the arena it was handed'
        for a in arenas:
            assert bool((a[need:] == pattern).all()), 'the run wrote past the workspace size it asked for'
        res[pattern] = {f'{k}[{i}]': t for k, v in y.items() if isinstance(v, (list, tuple)) for i, t in enumerate(v) if isinstance(t, torch.Tensor)}
        assert sum(t.shape[0] for k, t in res[pattern].items() if k.startswith('scores[')) > 0, 'no detections: the case checks nothing'
    rg.same_bits_across(res)
