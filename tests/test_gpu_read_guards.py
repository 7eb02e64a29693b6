"""No kernel result depends on bytes next to its operands.

Every case runs once per byte pattern of tests/read_guards.py with its operands embedded between bands of that pattern: 0xFF (NaN
in every float type) and 0x00 everywhere, 0x3C (plausible data, which survives an fmax or a clamp that drops a NaN) where the kernel
takes a maximum or clamps -- pool, ReLU epilogues, the objective.  The results of the runs are finite and the same bits, every
operand and its bands come back unwritten (operands a call is documented to update are compared by value), the existing output
guard bands are intact, and the entry points -- wrapped on the loaded library handle for the duration of the call -- received the
pointers of the embedded views: no kernel was fed a copy.  No tolerance appears: the runs are the same code on the same operands.

The cases are the smallest ragged entries of the existing tables; nothing here invents a shape.  The conv, sub-pixel, stem, pair,
bridge and graph-op runners of the neighbouring test files take the pattern as ``embed=`` and keep every assertion they make
without it: a conv case here is also judged against its fp64 bound.

Where a public function copies an operand by design, the case says so and gives it the form it does not copy:
  * ``cda.nn`` rounds fp32 activations to bf16 and makes other layouts channels-last on the way in: the cases pass bf16 channels-last
    activations and gradients (``stem_conv2d`` and the fp32 family of ``bilinear_resize``: fp32 NCHW, what they read), contiguous
    fp32 parameters;
  * ``stem_conv2d`` reads the image into the padded stem record first; the image pointer is what the library receives.

Results exempted from the comparison: none.
"""
import contextlib

import numpy as np
import pytest
import torch

import conv_tiles as ct
import graph_ops_oracle as go
import head_maps_oracle as hm
import read_guards as rg
import train_tiles as tt
from celldetection_amd import _lib

pytestmark = pytest.mark.gpu
CL = torch.channels_last
BF16, F32 = torch.bfloat16, torch.float32
TWO = (rg.NAN, rg.ZERO)
THREE = rg.PATTERNS


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


def across(patterns, run):
    """run(pattern) -> {name: result} once per pattern; all finite and the same bits."""
    rg.same_bits_across({p: run(p) for p in patterns})


def test_control_a_kernel_that_reads_the_band_is_flagged(dev):
    """The judge on the GPU: cpn_maxpool2d with a 1/1/0 window (a copy) is told that its one image has a row more than the embedded
    operand holds.  That row is the first row of the band after the operand -- inside the buffer, whose bands hold at least a row --
    so the kernel reads exactly what a loop that runs one row too far would read.  The runs differ under 0xFF (NaN in the result)
    and under 0x3C, the operand and its bands stay unwritten, and the same call with the true height passes."""
    import conv_bounds as cb
    lib = _lib.load()
    h, w, c = 5, 7, 32
    x = randn(1, h, w, c, seed=40).to(BF16)

    def run(pattern, rows):
        e = rg.Embedding(pattern)
        src = e('src', x.to(dev))
        out, buf, guard = cb.guarded_nhwc_bf16(1, rows, w, c, dev)
        with e.watch(lib, 'cpn_maxpool2d'):
            _lib.check(lib.cpn_maxpool2d(_lib.ptr(src), _lib.ptr(out), 1, rows, w, c, 1, 1, 0, _lib.stream_ptr()), 'maxpool2d')
        torch.cuda.synchronize()
        cb.assert_guards('maxpool', buf, guard, cb.BF16_GUARD)
        e.check()
        return {'output': out.cpu().float()}

    across(THREE, lambda pattern: run(pattern, h))
    with pytest.raises(AssertionError, match=r'output: 224 (non-finite values in run 0xFF, first at|of 1344 elements differ .* first at index) \(0, 5, 0, 0\)'):
        rg.same_bits_across({p: run(p, h + 1) for p in (rg.NAN, rg.ZERO)})
    with pytest.raises(AssertionError, match=r'output: 224 of 1344 elements differ between runs 0x00 and 0x3C.*first at index \(0, 5, 0, 0\)'):
        rg.same_bits_across({p: run(p, h + 1) for p in (rg.ZERO, rg.PLAUSIBLE)})


# ======================================================================================================================================
# cpn_conv2d / cpn_conv2d_fp8: one case per kernel instantiation (tests/conv_tiles.py: every entry has partial tiles), with the
# second epilogues entered there (+res, +res_up, +concat_up, +f32, +fused); the source forms the table does not hold -- nearest
# resized first source, grouped, padded channels -- from CONV_CASES at their smallest entries
# ======================================================================================================================================
def conv_patterns(cfg):
    """0x3C as well where the epilogue clamps: ReLU (the default activation of the runners) and the bounded head activations."""
    return THREE if cfg.get('act', 'relu') != 'none' or cfg.get('fuse_cout') else TWO


@pytest.mark.parametrize('key', [k for k in ct.TABLE if 'bridge' not in ct.TABLE[k]])
def test_conv_instantiation(dev, key, monkeypatch):
    import test_gpu_kernels as tk
    unit, mode, th, bn, _ = ct.parse_key(key)
    for name, value in ct.ENV.get(key, {}).items():
        monkeypatch.setenv(name, value)
    assert ct.query(key)[:3] == (mode, th, bn), f'{key}: the library runs another kernel here'
    cfg = ct.TABLE[key]

    def run(pattern):
        if unit == 'e4m3':
            out = tk.run_conv_fp8(dev, key, **cfg, embed=pattern, reference=False)
            assert out.dtype != torch.uint8 or not bool(((out & 0x7f) == 0x7f).any()), f'{key}: NaN codes in the e4m3 output'
            return {'output': out}
        got, _, _ = tk.run_conv(dev, **cfg, embed=pattern, reference=False)
        return {'output': got}
    across(conv_patterns(cfg), run)


CONV_FORMS = ('3x3_bridge_up0', '3x3_grouped_cpg8', '3x3_grouped_cpg64_s2', '3x3_grouped_cpg1', '3x3_concat_up_pad', '1x1_fpn_lateral',
              '7x7_stem_s2', 'fused_head_small', '3x3_bilinear_src_32', '3x3_narrow16_rows24_res', '5x5_narrow16_f32_out', 'final_fourier')


@pytest.mark.parametrize('name', CONV_FORMS)
def test_conv_source_forms(dev, name):
    """Judged against the fp64 bound as well (run_conv's check), under every pattern."""
    import test_gpu_kernels as tk
    cfg = tk.CONV_CASES[name]

    def run(pattern):
        got, chk, _ = tk.run_conv(dev, **cfg, embed=pattern)
        chk(name, got)
        return {'output': got}
    across(conv_patterns(cfg), run)


@pytest.mark.parametrize('name', ['1x1_odd_chunks_res', '3x3_odd_channels', '3x3_concat_up', '3x3_grouped_cpg8', '7x7_stem_s2'])
def test_conv_fp8_source_forms(dev, name):
    import test_gpu_kernels as tk
    cfg = tk.FP8_CASES[name]
    across(conv_patterns(cfg), lambda pattern: {'output': tk.run_conv_fp8(dev, name, **cfg, embed=pattern, reference=False)})


@pytest.mark.parametrize('name', ['sp_padded_channels', 'sp_partial_tiles', 'sp_no_bias'])
def test_subpixel_triple(dev, name):
    import test_gpu_kernels as tk
    across(THREE, lambda pattern: tk.test_subpixel_decoder_conv(dev, name, embed=pattern))


@pytest.mark.parametrize('case', [(1, 75, 101, 3, 64, 0), (1, 7, 9, 3, 64, 0)], ids=['75x101', '7x9'])
def test_stem_fast_path(dev, case):
    import test_gpu_kernels as tk
    across(THREE, lambda pattern: tk.test_stem_fast_path(dev, *case, embed=pattern))


def test_conv_pair(dev):
    """'gen_w63_ragged': ragged width and height, the generic strip kernel."""
    import test_gpu_conv_pair as tp

    def run(pattern):
        fused, two, _ = tp.run_pair(dev, **tp.PAIR_CASES['gen_w63_ragged'], embed=pattern)
        return dict(pair=fused, two_launches=two)
    across(THREE, run)


def test_conv_bridge(dev):
    import test_gpu_conv_bridge as tb
    across(THREE, lambda pattern: tb.test_conv_bridge_kernel(dev, 'bridge_partial_tiles', embed=pattern))


# ======================================================================================================================================
# graph ops at the ragged cases of tests/graph_ops_oracle.py
# ======================================================================================================================================
def test_maxpool(dev):
    import test_gpu_graph_ops as tg
    for name, x, pools in go.pool_cases('bf16'):
        for k, s, p in pools:
            across(THREE, lambda pattern: {f'{name} {k}/{s}/{p}': tg.direct_pool(dev, x, k, s, p, embed=pattern).float()})


def test_resize_bilinear(dev):
    import test_gpu_graph_ops as tg
    for case in go.RESIZE_CASES:
        _, s = go.resize_source('bf16', case, True, 'interval')
        across(TWO, lambda pattern: {go.resize_name(case): tg.direct_resize(dev, s, case[1], embed=pattern).float()})


def test_convert_input(dev):
    import test_gpu_graph_ops as tg
    for c in (1, 3, 4):
        for src in go.input_sources(c):
            for cpad, stem in ((8, False), (32, False), (4, True)):
                def run(pattern):
                    got, flag = tg.direct_input(dev, src, cpad, stem=stem, embed=pattern)
                    return {f'C={c} {src.dtype} cpad={cpad} stem={stem}': got.float(), 'range flag': np.array([flag])}
                across(TWO, run)
    for name, src, expected in go.range_flag_sources():  # (the offending value is the very last element: the flag reads no further)
        if expected == 0:
            for pattern in THREE:
                assert tg.direct_input(dev, src, 8, embed=pattern)[1] == 0, f'{name}: the range flag saw the band (0x{pattern:02X})'


@pytest.mark.parametrize('mode', ['bilinear', 'bicubic'])
def test_resize_f32(dev, mode):
    """cpn_resize_f32 through cpn._equal_size, which passes a contiguous fp32 map as it is."""
    from celldetection_amd.cpn import _equal_size
    lib = _lib.load()
    for i, (shape, size) in enumerate(hm.BICUBIC_CASES):
        def run(pattern):
            e = rg.Embedding(pattern)
            x = e('x', hm.bicubic_input(i).to(dev))
            with e.watch(lib, 'cpn_resize_f32'):
                out = _equal_size(x, torch.empty(1, 1, *size), mode=mode)
            torch.cuda.synchronize()
            e.check()
            return {f'{shape}->{size}': out}
        across(TWO, run)


# ======================================================================================================================================
# head-map kernels at the edge cases of tests/head_maps_oracle.py (the public ops pass contiguous fp32 / int32 operands as they are)
# ======================================================================================================================================
HEAD_ENTRY_POINTS = ('cpn_class_scores', 'cpn_certainty_mask', 'cpn_gather_channels', 'cpn_compact', 'cpn_decode')


def head_run(dev, pattern, operands, call):
    """operands: {name: CPU tensor | None}; call(**embedded device tensors) -> {name: result}."""
    e = rg.Embedding(pattern)
    on = {k: (None if v is None else e(k, v.to(dev).contiguous())) for k, v in operands.items()}
    with e.watch(_lib.load(), *HEAD_ENTRY_POINTS):
        out = call(**on)
    torch.cuda.synchronize()
    e.check()
    return out


@pytest.mark.parametrize('C', (2, 7, 33))
def test_class_scores(dev, C):
    from celldetection_amd import ops
    for name, logits, lower, upper in hm.class_cases(C, 3) + hm.class_cases(C, 3, (1, 1, 1)):
        def call(logits, lower, upper):
            sel, cls, fg, probs = ops.class_scores(logits, lower, upper, return_probs=True)
            return dict(selected=sel, classes=cls, foreground=fg, probabilities=probs)
        across(THREE, lambda pattern: head_run(dev, pattern, dict(logits=logits, lower=lower, upper=upper), call))


@pytest.mark.parametrize('C', (1, 4, 5))
def test_certainty_mask(dev, C):
    """The scores hold +-inf on purpose (their bytes pass through): compared for their bits, not for finiteness."""
    from celldetection_amd import ops
    s, u = hm.certainty_scores(), hm.grid_uncertainty(C)
    res = {p: head_run(dev, p, dict(scores=s, uncertainty=u), lambda scores, uncertainty: dict(mask=ops.certainty_mask(scores, uncertainty, .5)))
           for p in THREE}
    rg.same_bits_across(res, finite=False)
    assert not bool(res[rg.ZERO]['mask'].isnan().any())


@pytest.mark.parametrize('C,P', [(1, 131), (3, 1), (5, 131)])
def test_gather_channels(dev, C, P):
    from celldetection_amd import ops
    maps = torch.randn(hm.N, C, hm.H, hm.W, generator=torch.Generator().manual_seed(C))
    across(TWO, lambda pattern: head_run(dev, pattern, dict(maps=maps, indices=hm.gather_indices(P)),
                                         lambda maps, indices: dict(gathered=ops.gather_channels(maps, indices))))


@pytest.mark.parametrize('name', list(hm.DECODE_CASES))
def test_compact_and_decode(dev, name):
    from celldetection_amd import ops
    c, t = hm.DECODE_CASES[name], hm.decode_inputs(name)

    def call(scores, locations, fourier, refinement):
        idx, counts, _ = ops.compact_scores(scores, hm.DECODE_THRESH)
        flat = ops.decode_proposals(idx, scores, locations, fourier, refinement, size=c['HW'], order=c['order'], samples=c['samples'],
                                    iterations=c['iterations'], offsets=t['offsets'], num_buckets=c['buckets'])
        return dict(flat, indices=idx, counts=np.array(counts))
    across(THREE, lambda pattern: head_run(dev, pattern, {k: t[k] for k in ('scores', 'locations', 'fourier', 'refinement')}, call))


# ======================================================================================================================================
# cda.nn: forward, input gradient, weight and bias gradient all count as results
# ======================================================================================================================================
def act(t):
    """bf16 channels-last: the form cda.nn reads without a copy."""
    return t.to(BF16).contiguous(memory_format=CL)


def nn_run(dev, pattern, fn, inputs, grads_for, updated=(), seed=None, grad_format=None):
    """fn(**embedded inputs) -> output(s); one backward from seeded, embedded output gradients.  inputs: {name: CPU tensor | other};
    grads_for: the names that require a gradient; updated: inputs the call is documented to update (returned as results).
    -> {output i, d name, name (updated)}"""
    e = rg.Embedding(pattern)
    on = {}
    for k, v in inputs.items():
        if isinstance(v, torch.Tensor):
            v = e(k, v.to(dev), updated=k in updated)
            if k in grads_for:
                v.requires_grad_(True)
        on[k] = v
    if seed is not None:
        torch.manual_seed(seed)
    with e.watch(_lib.load(), *_lib.EXPORTED_SYMBOLS):
        out = fn(**on)
        outs = out if isinstance(out, (tuple, list)) else (out,)
        outs = [o for o in outs if isinstance(o, torch.Tensor) and o.requires_grad]
        g = torch.Generator().manual_seed(11)
        gouts = []
        for i, o in enumerate(outs):
            go_ = torch.randn(o.shape, generator=g).to(o.dtype)
            go_ = go_.contiguous() if o.dim() != 4 or o.is_contiguous() else go_.contiguous(memory_format=CL)
            gouts.append(e(f'grad_output {i}', go_.to(dev)))
        if outs:
            torch.autograd.backward(outs, gouts)
    torch.cuda.synchronize()
    e.check()
    res = {f'output {i}': o.detach() for i, o in enumerate(out if isinstance(out, (tuple, list)) else (out,)) if isinstance(o, torch.Tensor)}
    for k in grads_for:
        assert on[k].grad is not None, f'{k} received no gradient'
        res[f'd {k}'] = on[k].grad
    for k in updated:
        res[k] = on[k].detach()
    return res


def randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('hw', [(5, 7), (3, 65)], ids=str)
def test_nn_stem_conv2d(dev, hw):
    """test_gpu_stem.SHAPES.  The image is fp32 NCHW (what the stem reads) and gets no gradient."""
    from celldetection_amd import nn
    x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(1))
    inputs = dict(x=x, weight=randn(64, 3, 7, 7, seed=2) / 12, bias=randn(64, seed=3))
    across(TWO, lambda p: nn_run(dev, p, nn.stem_conv2d, inputs, ('weight', 'bias')))


@pytest.mark.parametrize('geometry', [(3, 2, 1), (2, 2, 0)], ids=str)
@pytest.mark.parametrize('hw', [(2, 2), (5, 7), (33, 70)], ids=str)
def test_nn_max_pool2d(dev, hw, geometry):
    """test_gpu_stem.POOL_SIZES x GEOMETRIES; all values negative, so that a padded or stray zero would win the maximum."""
    from celldetection_amd import nn
    k, s, pad = geometry
    x = act(-randn(2, 24, *hw, seed=4).abs() - .5)
    across(THREE, lambda p: nn_run(dev, p, lambda x: nn.max_pool2d(x, k, s, pad), dict(x=x), ('x',)))


@pytest.mark.parametrize('case', [(5, 7, 32, 32, 3), (5, 7, 96, 64, 7), (17, 33, 64, 160, 7)], ids=str)
@pytest.mark.parametrize('fork', [False, True], ids=['conv2d', 'conv2d_fork'])
def test_nn_conv2d(dev, case, fork):
    """test_gpu_conv_train.CASES."""
    from celldetection_amd import nn
    h, w, cin, cout, k = case
    inputs = dict(x=act(randn(2, cin, h, w, seed=5)), weight=randn(cout, cin, k, k, seed=6) / (k * cin ** .5), bias=randn(cout, seed=7))
    across(TWO, lambda p: nn_run(dev, p, nn.conv2d_fork if fork else nn.conv2d, inputs, ('x', 'weight', 'bias')))


@pytest.mark.parametrize('key', [f'{route}/k{k}/tiles' for route in tt.ROUTES for k in tt.KS[route]])
def test_nn_weight_gradient_with_a_partial_last_slab(dev, key):
    """The 'tiles' entry of every weight-gradient slab kernel of tests/train_tiles.py at 8 rows per slab: 15 (resized: 18) image rows, the last slab
    holds 7 (2)."""
    ops = tt._draw(key, 'normal')
    info = tt.info(key, 8)
    rows = tt.TABLE[key]['n'] * tt.TABLE[key]['h']
    assert info['slabs'] > 1 and rows % info['slab_rows'], f'{key}: the last slab is whole {info}'

    def run(pattern):
        e = rg.Embedding(pattern)
        on = {k: e(k, act(v).to(dev)) for k, v in ops.items()}
        with e.watch(_lib.load(), *_lib.EXPORTED_SYMBOLS), cuda_operands(on):
            dw, db = tt.weight_grad(key, on, 8)
        torch.cuda.synchronize()
        e.check()
        return dict(dW=dw, db=db)
    across(TWO, run)


@contextlib.contextmanager
def cuda_operands(on):
    """train_tiles.weight_grad moves its operands with .cuda(): a no-op on tensors that are there already."""
    assert all(t.is_cuda and t.cuda() is t for t in on.values())
    yield


@pytest.mark.parametrize('residual', [False, True], ids=['plain', 'residual'])
@pytest.mark.parametrize('shape', [(5, 7, 24), (3, 40, 96), (17, 33, 160)], ids=str)
def test_nn_batch_norm(dev, shape, residual):
    """test_gpu_batch_norm.SHAPES, training mode with the fused ReLU: the running statistics are documented updates, compared by
    value."""
    from celldetection_amd import nn
    h, w, c = shape
    inputs = dict(x=act(randn(3, c, h, w, seed=8) * 2 + .3), running_mean=randn(c, seed=9), running_var=randn(c, seed=30).abs() + .5,
                  weight=randn(c, seed=10), bias=randn(c, seed=11))
    wanted = ('x', 'weight', 'bias')
    if residual:
        inputs['residual'] = act(randn(3, c, h, w, seed=12))
        wanted += ('residual',)

    def fn(**kw):
        return nn.batch_norm(kw['x'], kw['running_mean'], kw['running_var'], kw['weight'], kw['bias'], training=True, activation='relu',
                             residual=kw.get('residual'))
    across(THREE, lambda p: nn_run(dev, p, fn, inputs, wanted, updated=('running_mean', 'running_var')))


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('case', [(2, 5, 7, 32, 8), (2, 6, 9, 64, 32), (2, 17, 33, 160, 32)], ids=str)
def test_nn_grouped_conv2d(dev, case, stride):
    """test_grouped_conv.GPU_SHAPES."""
    from celldetection_amd import nn
    n, h, w, c, cpg = case
    inputs = dict(x=act(randn(n, c, h, w, seed=13)), weight=randn(c, cpg, 3, 3, seed=14) / (3 * cpg ** .5), bias=randn(c, seed=15))
    across(TWO, lambda p: nn_run(dev, p, lambda x, weight, bias: nn.grouped_conv2d(x, weight, bias, stride=stride, groups=c // cpg),
                                 inputs, ('x', 'weight', 'bias')))


@pytest.mark.parametrize('case', [(32, 64, 9, 11), (96, 32, 6, 8), (64, 288, 1, 2)], ids=str)
def test_nn_strided_conv1x1(dev, case):
    """test_gpu_bottleneck.STRIDED."""
    from celldetection_amd import nn
    cin, cout, h, w = case
    inputs = dict(x=act(randn(2, cin, h, w, seed=16)), weight=randn(cout, cin, 1, 1, seed=17) / cin ** .5, bias=randn(cout, seed=18))
    across(TWO, lambda p: nn_run(dev, p, nn.strided_conv1x1, inputs, ('x', 'weight', 'bias')))


@pytest.mark.parametrize('case', [(5, 7, 2, 3, 64, 32, 32, 3), (9, 10, 3, 3, 64, 32, 32, 1), (17, 33, 9, 17, 96, 32, 160, 3)], ids=str)
def test_nn_cat_conv2d(dev, case):
    """test_gpu_cat_conv.CASES: the first two resize by 5/2 x 7/3 and 3 x 10/3, not by 2."""
    from celldetection_amd import nn
    H, W, h, w, c0, c1, cout, k = case
    inputs = dict(lateral=act(randn(2, c0, H, W, seed=19)), top=act(randn(2, c1, h, w, seed=20)),
                  weight=randn(cout, c0 + c1, k, k, seed=21) / (k * (c0 + c1) ** .5), bias=randn(cout, seed=22))
    across(TWO, lambda p: nn_run(dev, p, nn.cat_conv2d, inputs, ('lateral', 'top', 'weight', 'bias')))


@pytest.mark.parametrize('case', [(5, 7, 32, 2), (3, 40, 96, 1), (17, 33, 256, 17)], ids=str)
def test_nn_dropout_conv1x1(dev, case):
    """test_gpu_readout_tail.CASES, training with p = 0.5; the generator is seeded before every run so that the masks agree."""
    from celldetection_amd import nn
    h, w, cin, cout = case
    inputs = dict(x=act(randn(2, cin, h, w, seed=23)), weight=randn(cout, cin, 1, 1, seed=24) / cin ** .5, bias=randn(cout, seed=25))
    across(TWO, lambda p: nn_run(dev, p, lambda x, weight, bias: nn.dropout_conv1x1(x, weight, bias, p=.5, training=True), inputs,
                                 ('x', 'weight', 'bias'), seed=1234))


@pytest.mark.parametrize('family', ['bf16 channels-last', 'fp32 NCHW'])
@pytest.mark.parametrize('shape', [(13, 14, 7, 7), (46, 6, 14, 3), (15, 27, 5, 9)], ids=str)
def test_nn_bilinear_resize_and_adjoint(dev, shape, family):
    """test_gpu_bilinear_resize.SHAPES; the backward of ``bilinear_resize`` is ``bilinear_resize_backward``, the adjoint."""
    from celldetection_amd import nn
    H, W, h, w = shape
    x = act(randn(2, 32, h, w, seed=26)) if family.startswith('bf16') else randn(2, 3, h, w, seed=26)
    across(TWO, lambda p: nn_run(dev, p, lambda x: nn.bilinear_resize(x, (H, W)), dict(x=x), ('x',)))


@pytest.mark.parametrize('case', [(13, 14, 7, 7, 64, 64, 3), (15, 27, 5, 9, 96, 32, 3), (13, 14, 7, 7, 32, 32, 7)], ids=str)
def test_nn_resized_conv2d(dev, case):
    """test_gpu_bilinear_resize.CASES."""
    from celldetection_amd import nn
    H, W, h, w, c, cout, k = case
    inputs = dict(x=act(randn(2, c, h, w, seed=27)), weight=randn(cout, c, k, k, seed=28) / (k * c ** .5), bias=randn(cout, seed=29))
    across(TWO, lambda p: nn_run(dev, p, lambda x, weight, bias: nn.resized_conv2d(x, weight, bias, size=(H, W)), inputs,
                                 ('x', 'weight', 'bias')))


# ======================================================================================================================================
# the optimizer and the objective
# ======================================================================================================================================
@pytest.mark.parametrize('kind', ['float32', 'bfloat16', 'mixed'])
def test_adamw_step(dev, kind):
    """One step over test_gpu_optim.EDGES with parameters, gradients and both moments embedded.  Parameters and moments are
    documented updates: compared by value.  The addresses travel in the CpnOptimTensor table (cpn_optim_upload)."""
    import celldetection_amd as cda
    import test_gpu_optim as to

    def run(pattern):
        dtypes = to.LISTS[kind]
        host = to._host(to.EDGES, dtypes, seed=1)
        e = rg.Embedding(pattern)
        params, states = [], []
        for i, (h, dt) in enumerate(zip(host, dtypes)):
            p = torch.nn.Parameter(e(f'p{i}', to._dev(h['p'], dt), updated=True))
            p.grad = e(f'g{i}', to._dev(h['g'], dt))
            params.append(p)
            states.append((e(f'm{i}', to._dev(h['m']), updated=True), e(f'v{i}', to._dev(h['v']), updated=True)))
        opt = cda.optim.AdamW(params, max_grad_norm=1., **to.HYPER)
        for p, (m, v) in zip(params, states):
            opt.state[p] = dict(step=torch.tensor(6., dtype=F32), exp_avg=m, exp_avg_sq=v)
        with e.watch(_lib.load(), *_lib.EXPORTED_SYMBOLS):
            opt.step()
        torch.cuda.synchronize()
        e.check()
        res = {'grad norm': opt.last_grad_norm.detach().reshape(1) if isinstance(opt.last_grad_norm, torch.Tensor) else np.array([float(opt.last_grad_norm)])}
        for i, (p, (m, v)) in enumerate(zip(params, states)):
            assert opt.state[p]['exp_avg'].data_ptr() == m.data_ptr(), 'the step replaced a moment instead of updating it'
            res.update({f'p{i}': p.detach(), f'm{i}': m, f'v{i}': v})
        return res
    across(TWO, run)


def test_objective(dev):
    """The smallest fixture case with the four maps embedded; the losses clamp and take maxima: all three patterns."""
    import test_gpu_objective as tj
    name = min(tj.CASES, key=lambda k: sum(np.asarray(v).size for v in tj.CASES[k]['maps'].values() if v is not None))
    case = tj.CASES[name]
    config, targets = case['config'], case['targets']

    def run(pattern):
        e = rg.Embedding(pattern)
        leaves = {k: (None if case['maps'][k] is None else e(k, torch.tensor(case['maps'][k], device=dev)).requires_grad_(True)) for k in tj.MAPS}
        tg = {k: torch.as_tensor(v).to(dev) for k, v in targets.items()}
        obj = tj.make_objective(config, targets['sampling'].shape[1])
        with e.watch(_lib.load(), *_lib.EXPORTED_SYMBOLS):
            loss, losses = obj(leaves['scores'], leaves['locations'], leaves['refinement'], leaves['fourier'], tg, size=config['size'])
            loss.backward()
        torch.cuda.synchronize()
        e.check()
        res = {'loss': loss.detach().reshape(1)}
        res.update({f'loss {k}': v.detach().reshape(1) for k, v in losses.items() if v is not None})
        res.update({f'd {k}': v.grad for k, v in leaves.items() if v is not None and v.grad is not None})
        assert any(k.startswith('d ') for k in res)
        return res
    res = {p: run(p) for p in THREE}
    # (the oracle's gradients hold NaN where the reference's do -- test_gpu_objective.check_against_oracle: bits, not finiteness)
    rg.same_bits_across(res, finite=False)
    assert np.isfinite(res[rg.ZERO]['loss'].cpu().numpy()).all()
