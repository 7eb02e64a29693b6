"""The kernels between the convs of every plan, on their own and in all three precisions: input conversion (input_kernel,
input_fp8_kernel, input_f32_kernel, input_stem_kernel), max-pool, bilinear / bicubic resize, the activation op and the calibration
abs-max (csrc/misc_kernels.hip, csrc/misc_fp8.hip, csrc/conv_f32.hip, csrc/stem.hip).

References, bounds and cases come from tests/graph_ops_oracle.py; tests/test_graph_ops.py shows on the CPU that the bounds are
satisfiable.  The bf16 kernels are called through their C entry points into guarded buffers; the fp8 and fp32 kernels (and the bf16
activation, bicubic and abs-max) through hand-written conv-free plans whose tensors are read back from an oversized workspace filled
with a sentinel: the bytes past cpn_plan_workspace_bytes must be intact.  Every test prints its worst error / bound.
"""
from ctypes import byref, c_int32, c_int64, c_void_p

import pytest
import torch

import conv_bounds as cb
import graph_ops_oracle as go
import read_guards as rg
from celldetection_amd import _lib

pytestmark = pytest.mark.gpu
SC = 2.0 ** -9  # fp8 scale of the exact cases: code values times a power of two are exact inputs, 448 * SC < 1
WS_GUARD, WS_SENTINEL = 4096, 0xA5


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


def feed(prec, values):
    """The plan input that makes the input op store ``values`` (fp8: as code values at scale SC)."""
    return values * SC if prec == 'fp8' else values


def stored(prec, values):
    return go.encode(prec, go.nhwc(values))


def nchw(t):
    return t.float().permute(0, 3, 1, 2)


def in_range(x):
    v = x.float() / 255 if x.dtype == torch.uint8 else x
    return bool(((v >= 0) & (v <= 1)).all())


def run_plan(dev, plan, x, read, stats=False):
    """Runs a conv-free plan on the NCHW source x (f32 | u8) -> ({tensor id: stored NHWC tensor on the CPU}, range flag[, abs-max])."""
    lib = _lib.load()
    n, c, h, w = x.shape
    assert c == plan.in_channels
    nt = len(plan.tensors)
    handle = c_void_p()
    _lib.check(lib.cpn_plan_create(handle, plan.tensors, nt, plan.ops, nt, None, 0, None, 0, go.PRECISION_CODE[plan.prec]), 'plan_create')
    try:
        total = lib.cpn_plan_workspace_bytes(handle, n, h, w)
        assert total > 0, lib.cpn_last_error().decode()
        ws = torch.full((total + WS_GUARD,), WS_SENTINEL, dtype=torch.uint8, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        absmax = torch.zeros(nt, dtype=torch.float32, device=dev)
        src = x.contiguous().to(dev)
        args = (handle, _lib.ptr(src), 1 if x.dtype == torch.uint8 else 0, n, h, w, _lib.ptr(ws), total, None, _lib.ptr(flag))
        if stats:
            _lib.check(lib.cpn_plan_run_stats(*args, _lib.ptr(absmax), _lib.stream_ptr()), 'plan_run_stats')
        else:
            _lib.check(lib.cpn_plan_run(*args, _lib.stream_ptr()), 'plan_run')
        torch.cuda.synchronize()
        host = ws.cpu()
        assert bool((host[total:] == WS_SENTINEL).all()), 'the plan wrote past the workspace size it asked for'
        spans, out = [], {}
        for t in range(nt):
            off, th, tw, ch = c_int64(), c_int32(), c_int32(), c_int32()
            _lib.check(lib.cpn_plan_tensor_info(handle, n, h, w, t, byref(off), byref(th), byref(tw), byref(ch)), 'tensor_info')
            spans.append((off.value, off.value + n * th.value * tw.value * ch.value * go.ELEM[plan.prec], (n, th.value, tw.value, ch.value)))
        for t in read:
            a, b, shape = spans[t]
            assert b <= total and all(b <= a2 or b2 <= a for a2, b2, _ in spans[t + 1:]), f'tensor {t} is overwritten by a later op'
            out[t] = host[a:b].clone().view(go.STORE[plan.prec]).view(shape)
        return (out, int(flag.item())) + ((absmax.cpu(),) if stats else ())
    finally:
        lib.cpn_plan_destroy(handle)


def plan_result(dev, prec, ops, x, scales=None, read=None):
    """The last tensor (or ``read``) of the plan input -> ops at full channel width."""
    plan = go.Plan(prec, x.shape[1], ops, [SC] * (len(ops) + 1) if scales is None else scales)
    out, flag = run_plan(dev, plan, x, [len(ops)] if read is None else read)
    assert flag == int(not in_range(x)), 'range flag'
    return out[len(ops)] if read is None else out


# ---- the bf16 entry points, into guarded buffers -------------------------------------------------------------------------------------
# (``embed``: a byte pattern of tests/read_guards.py; the source then lies between bands of that pattern, which must come back intact
# around the unchanged source, and the library must have received exactly that pointer)
def direct_pool(dev, x, k, s, p, embed=None):
    lib = _lib.load()
    n, c, h, w = x.shape
    ho, wo = go.chain_size((h, w), ((k, s, p),))
    e = rg.Embedding(embed)
    src = e('src', stored('bf16', x).to(dev))
    out, buf, guard = cb.guarded_nhwc_bf16(n, ho, wo, c, dev)
    with e.watch(lib, 'cpn_maxpool2d'):
        _lib.check(lib.cpn_maxpool2d(_lib.ptr(src), _lib.ptr(out), n, h, w, c, k, s, p, _lib.stream_ptr()), 'maxpool2d')
    torch.cuda.synchronize()
    e.check()
    cb.assert_guards(f'maxpool {k}/{s}/{p}', buf, guard, cb.BF16_GUARD)
    return out.cpu()


def direct_resize(dev, x, size, embed=None):
    lib = _lib.load()
    n, c, h, w = x.shape
    e = rg.Embedding(embed)
    src = e('src', stored('bf16', x).to(dev))
    out, buf, guard = cb.guarded_nhwc_bf16(n, size[0], size[1], c, dev)
    with e.watch(lib, 'cpn_resize_bilinear'):
        _lib.check(lib.cpn_resize_bilinear(_lib.ptr(src), _lib.ptr(out), n, h, w, size[0], size[1], c, _lib.stream_ptr()), 'resize_bilinear')
    torch.cuda.synchronize()
    e.check()
    cb.assert_guards(f'resize {h}x{w}->{size}', buf, guard, cb.BF16_GUARD)
    return out.cpu()


def direct_input(dev, x, cpad, stem=False, embed=None):
    """-> (stored tensor with its padded channels | the stem record, range flag)"""
    lib = _lib.load()
    n, c, h, w = x.shape
    e = rg.Embedding(embed)
    src = e('src', x.contiguous().to(dev))
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    dtype = 1 if x.dtype == torch.uint8 else 0
    with e.watch(lib, 'cpn_convert_input_stem', 'cpn_convert_input'):
        if stem:
            out, buf, guard = cb.guarded_nhwc_bf16(n, h + 6, w + 8, 4, dev)
            _lib.check(lib.cpn_convert_input_stem(_lib.ptr(src), dtype, _lib.ptr(out), n, c, h, w, _lib.ptr(flag), _lib.stream_ptr()), 'input_stem')
        else:
            out, buf, guard = cb.guarded_nhwc_bf16(n, h, w, cpad, dev)
            _lib.check(lib.cpn_convert_input(_lib.ptr(src), dtype, _lib.ptr(out), n, c, h, w, cpad, _lib.ptr(flag), _lib.stream_ptr()), 'input')
    torch.cuda.synchronize()
    e.check()
    cb.assert_guards('input conversion', buf, guard, cb.BF16_GUARD)
    return out.cpu(), int(flag.item())


# ---- max-pool: byte for byte ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', go.PRECISIONS)
def test_maxpool_is_exact(dev, prec):
    runs = 0
    for name, x, pools in go.pool_cases(prec) + [('identity', go.identity_values(prec), ((1, 1, 0),))]:
        for k, s, p in pools:
            exp = stored(prec, go.pool_ref(x, k, s, p))
            go.judge_exact(f'{prec} plan max-pool {name} {k}/{s}/{p}', prec, plan_result(dev, prec, [('pool', k, s, p)], feed(prec, x)), exp)
            if prec == 'bf16':
                go.judge_exact(f'cpn_maxpool2d {name} {k}/{s}/{p}', prec, direct_pool(dev, x, k, s, p), exp)
            runs += 1
    print(f'{prec} max-pool: {runs} cases byte for byte (worst error / bound 0)')


# ---- input conversion: byte for byte -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', go.PRECISIONS)
def test_input_conversion_is_exact(dev, prec):
    runs = 0
    for scale in (go.FP8_INPUT_SCALES if prec == 'fp8' else (None,)):
        for c in (1, 3, 4):
            for src in go.input_sources(c, scale):
                plan = go.Plan(prec, c, [], [scale or 1.])
                out, flag = run_plan(dev, plan, src, [0])
                exp = go.encode(prec, go.nhwc(go.input_ref(prec, src, scale).float(), plan.channels))
                go.judge_exact(f'{prec} plan input C={c} {src.dtype} scale={scale}', prec, out[0], exp)  # (padded channels: zero)
                assert flag == 0
                runs += 1
                for cpad in ((8, 32) if prec == 'bf16' else ()):
                    got, flag = direct_input(dev, src, cpad)
                    go.judge_exact(f'cpn_convert_input C={c} Cpad={cpad} {src.dtype}', prec, got, go.encode(prec, go.nhwc(go.input_ref(prec, src).float(), cpad)))
                    assert flag == 0
    print(f'{prec} input conversion: {runs} plan cases byte for byte (worst error / bound 0)')


def test_stem_input_record_is_exact(dev):
    for c in (1, 3, 4):
        for src in go.input_sources(c):
            got, flag = direct_input(dev, src, 4, stem=True)
            go.judge_exact(f'cpn_convert_input_stem C={c} {src.dtype}', 'bf16', got, go.stem_ref(src))
            assert flag == 0
    print('stem input record: 6 cases byte for byte, borders zero')


@pytest.mark.parametrize('prec', go.PRECISIONS)
def test_range_flag(dev, prec):
    for name, src, expected in go.range_flag_sources():
        assert run_plan(dev, go.Plan(prec, 3, [], [1. / 448.]), src, [0])[1] == expected, f'{prec} plan {name}'
        if prec == 'bf16':
            assert direct_input(dev, src, 8)[1] == expected, f'cpn_convert_input {name}'
            assert direct_input(dev, src, 4, stem=True)[1] == expected, f'cpn_convert_input_stem {name}'
    print(f'{prec} range flag: {len(go.range_flag_sources())} cases')


# ---- abs-max: bit for bit ------------------------------------------------------------------------------------------------------------
def test_absmax_is_exact(dev):
    for shape in ((1, 32, 3, 5), (2, 32, 9, 11), (3, 64, 37, 41)):  # 480, 6336 and 291 264 values: no multiple of 256 | several blocks
        x = go.encode('bf16', torch.rand(shape, generator=torch.Generator().manual_seed(shape[2])) * 1.8 - .9).float()
        x[-1, -1, -1, -1] = -0.99609375  # the maximum is attained at a negative value, in the last element
        assert torch.Size(shape).numel() % 256 and float(x.abs().max()) == 0.99609375 and int((x.abs() == 0.99609375).sum()) == 1
        plan = go.Plan('bf16', shape[1], [('pool', 1, 1, 0)])
        out, flag, absmax = run_plan(dev, plan, x, [0, 1], stats=True)
        for t in (0, 1):
            ref = out[t].float().abs().max().reshape(1)
            assert torch.equal(absmax[t:t + 1].view(torch.int32), ref.view(torch.int32)) and float(ref) == 0.99609375, (shape, t, absmax)
    print('abs-max: 3 sizes bit for bit')


# ---- bilinear at dyadic ratios on grid values: byte for byte -------------------------------------------------------------------------
@pytest.mark.parametrize('prec', go.PRECISIONS)
def test_bilinear_dyadic_is_exact(dev, prec):
    for case in go.DYADIC_CASES:
        src, size, chain = case
        if chain is not None:
            x, s = go.resize_source(prec, case, False, 'grid')
            got = plan_result(dev, prec, go.pool_ops(chain) + [('resize', 0)], feed(prec, x))
            go.judge_exact(f'{prec} plan bilinear {go.resize_name(case)}', prec, got, stored(prec, go.bilinear_ref(s, size)[0]))
        if prec == 'bf16':
            _, s = go.resize_source(prec, case, True, 'grid')
            go.judge_exact(f'cpn_resize_bilinear {go.resize_name(case)}', prec, direct_resize(dev, s, size), stored(prec, go.bilinear_ref(s, size)[0]))
    print(f'{prec} bilinear, same size / x2 / x4 on grid values: byte for byte (worst error / bound 0)')


# ---- bilinear at the other ratios: the interval ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', go.PRECISIONS)
def test_bilinear_is_within_the_interval(dev, prec):
    for case in go.RESIZE_CASES:
        src, size, chain = case
        x, s = go.resize_source(prec, case, chain is None, 'interval')
        ref, e = go.bilinear_ref(s, size)
        lo, hi = go.interval(prec, ref, e)
        line = f'{prec} bilinear {go.resize_name(case)}:'
        if chain is not None:
            got = plan_result(dev, prec, go.pool_ops(chain) + [('resize', 0)], feed(prec, x))
            line += f' plan worst error / bound {go.judge_interval(line + " plan", nchw(got), lo, hi, ref, prec, e):.3f}'
        if prec == 'bf16':
            line += f' entry point worst error / bound {go.judge_interval(line + " entry point", nchw(direct_resize(dev, s, size)), lo, hi, ref, prec, e):.3f}'
        elif chain is None:
            continue
        if prec != 'fp32':
            share, more = go.interval_widths(prec, lo, hi)
            line += f', two-valued intervals {100 * share:.2f} %'
        print(line)


@pytest.mark.parametrize('prec', ('bf16', 'fp32'))
def test_bicubic_is_within_the_bound(dev, prec):
    for case in go.RESIZE_CASES:
        src, size, chain = case
        if chain is None:
            continue
        x, s = go.resize_source(prec, case, False, 'bicubic')
        got = nchw(plan_result(dev, prec, go.pool_ops(chain) + [('resize', 1)], x))
        ref, (lo, hi) = go.bicubic_interval(prec, case, s)
        e = go.bicubic_bound(prec, case) * 2 * go.U * float(s.abs().max())
        r = go.judge_interval(f'{prec} bicubic {go.resize_name(case)}', got, lo, hi, ref, prec, e)
        print(f'{prec} bicubic {go.resize_name(case)}: worst error / bound {r:.3f} (bound {go.bicubic_bound(prec, case):.2f} x 2^-23 max|x|)')


# ---- activations: the interval -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', list(go.ACTS))
@pytest.mark.parametrize('prec', go.PRECISIONS)
def test_activation_is_within_the_interval(dev, prec, kind):
    for pair in (go.FP8_ACT_SCALES if prec == 'fp8' else (None,)):
        x, args = go.act_inputs(prec, pair)
        plan = go.Plan(prec, go.C, [('act', kind)], pair)
        out, flag = run_plan(dev, plan, x, [0, 1])
        assert flag == 1
        # the argument tensor holds what the reference assumes: every finite pattern (fp8: every finite code)
        go.judge_exact(f'{prec} {kind} arguments', prec, out[0], stored(prec, go.identity_values('fp8') if prec == 'fp8' else x))
        ref, lo, hi, e = go.act_interval(prec, kind, args, pair)
        r = go.judge_interval(f'{prec} {kind} {pair or ""}', nchw(out[1]), lo, hi, ref, prec, e)
        print(f'{prec} {kind} {pair or ""}: worst error / bound {r:.3f} over {args.numel()} arguments')


# ---- grid-stride laps: more than 256 x 16 x 256 thread items, so the second lap exists and is ragged -------------------------------------
def test_second_lap_input_and_pool(dev):
    v = go.lap_values('bf16')
    got, flag = direct_input(dev, v, go.C)
    go.judge_exact('cpn_convert_input, second lap', 'bf16', got, stored('bf16', v))
    go.judge_exact('cpn_maxpool2d, second lap', 'bf16', direct_pool(dev, v, 1, 1, 0), stored('bf16', v))
    del got
    v = go.lap_values('fp8')
    out = plan_result(dev, 'fp8', [('pool', 1, 1, 0)], feed('fp8', v), read=[0, 1])
    go.judge_exact('fp8 input, second lap', 'fp8', out[0], stored('fp8', v))
    go.judge_exact('fp8 max-pool, second lap', 'fp8', out[1], stored('fp8', v))
    print(f'second lap: bf16 / fp8 input conversion and max-pool over {v.numel()} elements byte for byte')


@pytest.mark.parametrize('prec', go.PRECISIONS)
def test_second_lap_activation(dev, prec):
    v = go.lap_values('fp8' if prec == 'fp8' else 'bf16')
    # relu of positive values is the identity; the fp8 scales are powers of two (SC -> 2 SC: every product is exact)
    got = plan_result(dev, prec, [('act', 'relu')], feed(prec, v), scales=(SC, 2 * SC))
    go.judge_exact(f'{prec} activation, second lap', prec, got, stored(prec, v / 2 if prec == 'fp8' else v))
    print(f'second lap: {prec} activation over {v.numel()} elements byte for byte')


def test_second_lap_bilinear(dev):
    x = go.grid_values((2, go.C, 65, 65), 77)
    got = direct_resize(dev, x, (260, 260))
    go.judge_exact('cpn_resize_bilinear 65x65->260x260, second lap', 'bf16', got, stored('bf16', go.bilinear_ref(x, (260, 260))[0]))
    print(f'second lap: bf16 bilinear x4 over {got.numel()} elements byte for byte')


# ---- fp8 ring mode: the resize in front of the FPN refinement head writes only the frame the frame conv reads ------------------------------
def test_fp8_resize_ring_mode(dev):
    """The tiny fp8 CpnResNet18FPN of test_plan_validation.py: the resize op's destination after a default run, a run with
    CPN_BLPHASE=0 (the whole map) and one with CPN_BLPHASE=2 (ring mode wherever the resize is an exact x2).  The pixels within
    ``ring`` = 7 of the border are the same bytes in all three, ring mode does not write the interior, and the whole map satisfies
    the interval judge.  (Only the refinement head's convs follow the resize, into external outputs: both tensors stay intact.)"""
    import os
    from ctypes import c_void_p as vp
    import celldetection_amd as cda
    from celldetection_amd import graph
    lib = _lib.load()
    model = cda.models.CpnResNet18FPN(3, backbone_kwargs=dict(backbone_kwargs={'base_channel': 8}, fpn_channels=16))
    plan = model.plan_for('fp8')
    tens, ops, wblob, bblob = graph.pack(plan, model.state_dict(), dev, precision='fp8', act_scales=[.01] * len(plan.tensors))[:4]
    (ri,) = [i for i, o in enumerate(ops) if o.op == _lib.OP_BILINEAR]
    src_t, dst_t, ring, n = ops[ri].src0, ops[ri].dst, 7, 2
    assert all(o.dst < 0 for o in ops[ri + 1:]), 'an op after the resize writes a tensor: the destination may not be intact'
    channels = [max([max(o.cout_real, o.fuse_cout) for o in ops if o.dst < 0 and o.out_index == i and o.op == _lib.OP_CONV] + [1]) for i in range(_lib.NUM_OUTPUTS)]
    handle = c_void_p()
    _lib.check(lib.cpn_plan_create(handle, tens, len(tens), ops, len(ops), _lib.ptr(wblob), wblob.numel() * wblob.element_size(),
                                   _lib.ptr(bblob), bblob.numel(), _lib.PRECISION_FP8), 'plan_create')
    before = os.environ.pop('CPN_BLPHASE', None)
    try:
        for h, w in ((64, 96), (48, 68)):
            x = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(h)).to(dev)
            maps = {}
            for switch in (None, '0', '2'):
                os.environ.pop('CPN_BLPHASE', None)
                if switch is not None:
                    os.environ['CPN_BLPHASE'] = switch
                total = lib.cpn_plan_workspace_bytes(handle, n, h, w)
                assert total > 0, lib.cpn_last_error().decode()
                outs = []
                for i in range(_lib.NUM_OUTPUTS):
                    oh, ow = c_int32(), c_int32()
                    _lib.check(lib.cpn_plan_output_dims(handle, h, w, i, byref(oh), byref(ow)), 'output_dims')
                    outs.append(torch.zeros(n * channels[i] * max(oh.value * ow.value, 1), dtype=torch.float32, device=dev))
                ws = torch.full((total + WS_GUARD,), WS_SENTINEL, dtype=torch.uint8, device=dev)
                flag = torch.zeros(1, dtype=torch.int32, device=dev)
                _lib.check(lib.cpn_plan_run(handle, _lib.ptr(x), 0, n, h, w, _lib.ptr(ws), total, (vp * _lib.NUM_OUTPUTS)(*[o.data_ptr() for o in outs]),
                                            _lib.ptr(flag), _lib.stream_ptr()), 'plan_run')
                torch.cuda.synchronize()
                host = ws.cpu()
                assert bool((host[total:] == WS_SENTINEL).all()) and int(flag.item()) == 0
                got = {}
                for t in (src_t, dst_t):
                    off, th, tw, ch = c_int64(), c_int32(), c_int32(), c_int32()
                    _lib.check(lib.cpn_plan_tensor_info(handle, n, h, w, t, byref(off), byref(th), byref(tw), byref(ch)), 'tensor_info')
                    got[t] = host[off.value:off.value + n * th.value * tw.value * ch.value].clone().view(n, th.value, tw.value, ch.value)
                assert tuple(got[dst_t].shape[1:3]) == (h, w) and tuple(got[src_t].shape[1:3]) == (h // 2, w // 2)
                maps[switch] = got
            frame = torch.ones(h, w, dtype=torch.bool)
            frame[ring:h - ring, ring:w - ring] = False
            whole = maps['0'][dst_t]
            for switch in (None, '2'):
                assert torch.equal(maps[switch][src_t], maps['0'][src_t])
                assert torch.equal(maps[switch][dst_t][:, frame], whole[:, frame]), f'{h}x{w} CPN_BLPHASE={switch}: the ring differs from the whole map'
            # (the arena placed the destination on dead tensors: what ring mode leaves alone is their data, not the sentinel)
            assert not torch.equal(maps['2'][dst_t][:, ~frame], whole[:, ~frame]), 'CPN_BLPHASE=2 did not run the resize in ring mode'
            src = nchw(maps['0'][src_t].view(torch.float8_e4m3fn))
            assert src.unique().numel() > 8, 'the source map is (nearly) constant: the case checks nothing'
            ref, e = go.bilinear_ref(src, (h, w))
            lo, hi = go.interval('fp8', ref, e)
            r = go.judge_interval(f'fp8 FPN resize {h}x{w}', nchw(whole.view(torch.float8_e4m3fn)), lo, hi, ref, 'fp8', e)
            default_ring = not torch.equal(maps[None][dst_t][:, ~frame], whole[:, ~frame])
            print(f'fp8 ring mode {h}x{w}: ring bytes identical (default run in ring mode: {default_ring}); whole map worst error / bound {r:.3f}, '
                  f'{src.unique().numel()} distinct source codes')
    finally:
        os.environ.pop('CPN_BLPHASE', None)
        if before is not None:
            os.environ['CPN_BLPHASE'] = before
        lib.cpn_plan_destroy(handle)
