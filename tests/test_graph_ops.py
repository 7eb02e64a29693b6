"""CPU check of tests/graph_ops_oracle.py: with torch-CPU fp32 arithmetic followed by the precision's rounding standing in for the
kernels, every judge of the GPU test (tests/test_gpu_graph_ops.py) accepts, every cap on two-valued intervals holds, and the
hand-written conv-free plans the GPU test runs are accepted and sized as expected by the native planner (host code, no kernel) -- the
bounds are satisfiable before a kernel meets them.  It also measures the constants the bounds leave open:

  lib_ulps       worst error in ulps of torch-CPU fp32 exp / erf / tanh / log1p / expm1 against float64 on the arguments the
                 activation cases hand them (the kernel is allowed L = 2 x this + 1)
  bicubic_cases  worst error of torch-CPU fp32 bicubic interpolation on each bicubic case, in units of 2^-23 max|input|
                 (the kernel's bound on that case is 4 x this)

``python tests/test_graph_ops.py`` writes them to tests/golden/graph_ops_measured.json; the test measures again and holds the
committed file to the fresh measurement.
"""
import json
import os
import sys
from ctypes import byref, c_int32, c_int64, c_void_p

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import conv_bounds as cb  # noqa: E402
import graph_ops_oracle as go  # noqa: E402
from celldetection_amd import _lib  # noqa: E402

PLAN_RESIZE = [c for c in go.RESIZE_CASES if c[2] is not None]
BICUBIC = [(p, c) for p in ('bf16', 'fp32') for c in PLAN_RESIZE]


def act_arguments():
    yield go.act_inputs('bf16')[1]
    yield go.act_inputs('fp32')[1]
    for pair in go.FP8_ACT_SCALES:
        yield go.act_inputs('fp8', pair)[1]


def measure():
    args = [go.lib_arguments(x) for x in act_arguments()]
    ulps = {f: max(go.lib_error_ulps(f, a[f]) for a in args) for f in go.LIB_FUNCTIONS}
    bic = {}
    for prec, case in BICUBIC:
        x = go.resize_source(prec, case, False, 'bicubic')[1]
        bic[f'{prec}_{go.resize_name(case)}'] = go.bicubic_error(x, case[1], F.interpolate(x, case[1], mode='bicubic', align_corners=False))
    return dict(lib_ulps=ulps, bicubic_cases=bic)


def test_committed_measurement_covers_a_fresh_one():
    """Another CPU's libm / vector width may round differently, so the committed figures are held with a factor: what the kernel is
    allowed (2 L + 1 ulps; 4 x the bicubic error) has to cover the fresh measurement, and a committed figure may not be more than
    4 x the fresh one (it would allow the kernel more than the reference's own error justifies)."""
    m, c = measure(), go.measured()
    print(f'library ulps: measured {m["lib_ulps"]} (committed {c["lib_ulps"]}); bicubic, x 2^-23 max|x|: measured {m["bicubic_cases"]} '
          f'(committed {c["bicubic_cases"]})')
    L = go.lib_allowance(c['lib_ulps'])
    for f in go.LIB_FUNCTIONS:
        assert 0 < m['lib_ulps'][f] <= L[f] and c['lib_ulps'][f] <= 4 * m['lib_ulps'][f], f
        assert c['lib_ulps'][f] < 4, 'a libm function is good to an ulp or so; anything else is a mistake in the measurement'
    assert set(c['bicubic_cases']) == set(m['bicubic_cases'])
    for k, fresh in m['bicubic_cases'].items():
        assert 0 <= fresh <= go.BICUBIC_MARGIN * c['bicubic_cases'][k] and c['bicubic_cases'][k] <= 4 * fresh, k


def test_patterns_are_exhaustive():
    b, e = go.bf16_patterns(), go.e4m3_patterns()
    assert b.numel() == 65280 and e.numel() == 254 and bool(torch.isfinite(b).all()) and bool(torch.isfinite(e).all())
    assert torch.equal(go.encode('bf16', b).float(), b) and torch.equal(go.encode('fp8', e).float(), e)
    assert len(set(go.bits('bf16', go.encode('bf16', b)).tolist())) == 65280 and len(set(go.bits('fp8', go.encode('fp8', e)).tolist())) == 254
    w = go.widened_patterns()
    assert bool(torch.isfinite(w).all()) and torch.equal(w.view(torch.int32) >> 16, b.view(torch.int32) >> 16)
    for prec in ('bf16', 'fp32'):  # the knees are among the arguments
        x = go.act_inputs(prec)[1]
        for knee in (0., 3., -3., 20.):
            assert bool((x == knee).any())
    for x in act_arguments():
        assert float(x.max()) > 3 and float(x.min()) < -3 and bool((x == 0).any())
    assert max(float(x.max()) for x in act_arguments() if x.numel() == 256) > 20  # (fp8: the switch at 20 too)
    assert float(go.act_inputs('bf16')[1].abs().max()) > 3e38  # exp overflows at both ends


# ---- the plans of the GPU test: accepted, and sized as the cases expect ------------------------------------------------------------
def planned(plan, n, h, w):
    """-> [(byte offset, h, w, channels)] per tensor and the workspace size; host code only."""
    lib = _lib.load()
    handle = c_void_p()
    rc = lib.cpn_plan_create(handle, plan.tensors, len(plan.tensors), plan.ops, len(plan.ops), None, 0, None, 0, go.PRECISION_CODE[plan.prec])
    assert rc == 0, lib.cpn_last_error().decode()
    try:
        total = lib.cpn_plan_workspace_bytes(handle, n, h, w)
        assert total > 0, lib.cpn_last_error().decode()
        info = []
        for t in range(len(plan.tensors)):
            off, th, tw, ch = c_int64(), c_int32(), c_int32(), c_int32()
            rc = lib.cpn_plan_tensor_info(handle, n, h, w, t, byref(off), byref(th), byref(tw), byref(ch))
            info.append((off.value, th.value, tw.value, ch.value) if rc == 0 else None)
        return info, total
    finally:
        lib.cpn_plan_destroy(handle)


@pytest.mark.parametrize('prec', go.PRECISIONS)
def test_plans_are_accepted_and_sized(prec):
    scales = [2.0 ** -9] * 6
    # the five-op plan: input, 3/2/1 pool, 2/2/0 pool, resize, GELU -- the arena re-uses tensor 0 for tensor 2
    five = go.Plan(prec, go.C, go.pool_ops(go.POOLS) + [('resize', 0), ('act', 'gelu')], scales[:5])
    info, total = planned(five, 2, 75, 101)
    assert [i[1:3] for i in info] == [(75, 101), (38, 51), (19, 25), (75, 101), (75, 101)]
    assert info[2][0] == info[0][0], 'tensor 2 was expected on the dead tensor 0'
    for case in PLAN_RESIZE + [c for c in go.DYADIC_CASES if c[2]]:
        src, size, chain = case
        for mode in ((0,) if prec == 'fp8' else (0, 1)):
            plan = go.Plan(prec, go.C, go.pool_ops(chain) + [('resize', mode)], scales)
            info, total = planned(plan, 2, *size)
            elem = go.ELEM[prec]
            assert info[-2][1:3] == src and info[-1][1:3] == size and go.chain_size(size, chain) == src
            # the source and the destination of the op under test do not overlap, and the destination ends inside the workspace
            a, b = info[-2], info[-1]
            assert a[0] + 2 * a[1] * a[2] * a[3] * elem <= b[0] or b[0] + 2 * b[1] * b[2] * b[3] * elem <= a[0]
            assert b[0] + 2 * b[1] * b[2] * b[3] * elem <= total
    for kind in go.ACTS:
        info, total = planned(go.Plan(prec, go.C, [('act', kind)], (2.0 ** -4, 2.0 ** -5)), 2, 30, 34)
        assert info[0][0] != info[1][0] and info[1][1:] == (30, 34, go.C)
    for k, s, p in go.POOLS + ((1, 1, 0),):
        planned(go.Plan(prec, go.C, [('pool', k, s, p)], scales), 1, 9, 11)
    for c in (1, 3, 4):
        info, _ = planned(go.Plan(prec, c, [], scales), 2, 5, 7)
        assert info[0][1:] == (5, 7, 64 if prec == 'fp8' else 32)
    info, total = planned(go.Plan(prec, go.C, [('pool', 1, 1, 0), ('act', 'relu')], scales), *go.LAP_SHAPE[:1], *go.LAP_SHAPE[2:])
    assert info[1][0] != info[2][0] and total >= 2 * go.ELEM[prec] * torch.Size(go.LAP_SHAPE).numel()


def test_maxpool_rejects_padding_beyond_half_the_kernel():
    lib = _lib.load()
    for k, p, ok in ((3, 1, True), (2, 1, True), (3, 2, False), (2, 2, False), (1, 1, False)):
        plan = go.Plan('bf16', 3, [('pool', k, 2, p)])
        handle = c_void_p()
        rc = lib.cpn_plan_create(handle, plan.tensors, 2, plan.ops, 2, None, 0, None, 0, _lib.PRECISION_BF16)
        assert (rc == 0) == ok, (k, p, lib.cpn_last_error().decode())
        if ok:
            lib.cpn_plan_destroy(handle)


# ---- exact family ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', go.PRECISIONS)
def test_pool_cases_are_exact_in_fp32(prec):
    cases = go.pool_cases(prec) + [('identity', go.identity_values(prec), ((1, 1, 0),))]
    for name, x, pools in cases:
        assert bool(torch.isfinite(x).all()) and torch.equal(go.encode(prec, x).float(), x), name
        for k, s, p in pools:
            if name != 'identity':  # no window mixes +0 and -0 (the identity's windows hold one value)
                assert bool((x != 0).all()), name
            ref = go.pool_ref(x, k, s, p)
            go.judge_exact(f'{name} {k}/{s}/{p}', prec, go.encode(prec, F.max_pool2d(x, k, s, p)), go.encode(prec, ref))
            if name == 'all_negative':
                assert float(ref.max()) < 0
            if name == 'max_on_last_row_and_column' and (k, s, p) == (2, 2, 0):
                assert float(ref.max()) < 0 < float(go.pool_ref(x, 3, 2, 1).max()), 'the 2/2/0 pool drops the last row and column'
    assert go.identity_values(prec).unique().numel() >= (254 - 1 if prec == 'fp8' else 65280 - 1)


@pytest.mark.parametrize('prec', go.PRECISIONS)
def test_input_reference(prec):
    for scale in (go.FP8_INPUT_SCALES if prec == 'fp8' else (None,)):
        for c in (1, 3, 4):
            f32, u8 = go.input_sources(c, scale)
            assert float(f32.min()) >= 0 and float(f32.max()) <= 1
            ref = go.input_ref(prec, f32, scale)
            if prec == 'bf16':  # the ties are ties: both neighbours are equally far, RNE takes the even one
                v = f32[0, 0].reshape(-1)[3:27].double()
                r = ref[0, 0].reshape(-1)[3:27].double()
                assert bool(((r - v).abs() == torch.exp2(torch.floor(torch.log2(v))) * 2.0 ** -8).all())
                assert bool(((go.bits('bf16', ref[0, 0].reshape(-1)[3:27]) & 1) == 0).all())
            if prec == 'fp8':
                code = ref[1, 0].reshape(-1)[:8].float().double() * scale
                assert bool((code != f32[1, 0].reshape(-1)[:8].double()).all())
            go.judge_exact('u8', prec, go.input_ref(prec, u8, scale), go.input_ref(prec, u8.float() / 255., scale))
    for name, src, flag in go.range_flag_sources():
        v = src.float() / 255 if src.dtype == torch.uint8 else src
        assert int(not bool(((v >= 0) & (v <= 1)).all())) == flag, name
    assert tuple(go.stem_ref(go.input_sources(3)[0]).shape) == (2, 11, 15, 4)


@pytest.mark.parametrize('prec', go.PRECISIONS)
def test_dyadic_bilinear_is_exact_in_fp32(prec):
    ties = 0
    for case in go.DYADIC_CASES:
        src, size, chain = case
        assert go.is_dyadic(src[0], size[0]) and go.is_dyadic(src[1], size[1])
        for direct in ((True, False) if chain else (True,)):
            x, s = go.resize_source(prec, case, direct, 'grid')
            assert torch.equal(go.encode(prec, s).float(), s) and (direct or torch.equal(go.chain_ref(x, chain), s))
            ref, _ = go.bilinear_ref(s, size)
            got = F.interpolate(s, size, mode='bilinear', align_corners=False)
            assert torch.equal(got.double(), ref), 'every fp32 operation of the blend is exact on grid values'
            stored = go.encode(prec, ref)
            lo, hi = go.interval(prec, ref, 1e-12)
            ties += int((lo != hi).sum())
    assert prec == 'fp32' or ties > 0, 'values that the output format has to round are among the cases'


# ---- interval family ---------------------------------------------------------------------------------------------------------------
def resize_variants(prec):
    for case in go.RESIZE_CASES:
        if case[2] is not None:
            yield case, False
        if prec == 'bf16':
            yield case, True


@pytest.mark.parametrize('prec', go.PRECISIONS)
def test_f32_bilinear_is_within_the_interval_and_the_cap_holds(prec):
    for case, direct in resize_variants(prec):
        x, s = go.resize_source(prec, case, direct, 'interval')
        assert float(s.min()) >= .5 and float(s.max()) <= 2 and s.unique().numel() >= 16
        assert direct or (torch.equal(go.chain_ref(x, case[2]), s) and tuple(x.shape[2:]) == case[1])
        ref, e = go.bilinear_ref(s, case[1])
        lo, hi = go.interval(prec, ref, e)
        got = go.encode(prec, F.interpolate(s, case[1], mode='bilinear', align_corners=False))
        r = go.judge_interval(go.resize_name(case), got.float(), lo, hi, ref, prec, e)
        raw = float(((F.interpolate(s, case[1], mode='bilinear', align_corners=False).double() - ref).abs() / e).max())
        line = f'{prec} bilinear {go.resize_name(case)}{" direct" if direct else ""}: worst error / bound {r:.3f}, before the store {raw:.3f}'
        if prec != 'fp32':
            share, more = go.interval_widths(prec, lo, hi)
            line += f', two-valued {100 * share:.2f} %, wider {more}'
            assert share <= go.TWO_VALUED_CAP and more == 0, line
        print(line)
        assert raw <= 1
        if case[0][0] > 1 and case[0][1] > 1 and not go.is_dyadic(case[0][0], case[1][0]):
            wrong = go.encode(prec, F.interpolate(s, case[1], mode='bilinear', align_corners=True)).double()
            rejected = float(((wrong < lo) | (wrong > hi)).double().mean())
            assert rejected > .1, f'an align_corners=True resize passes on {100 * (1 - rejected):.0f} % of {line}'


@pytest.mark.parametrize('prec,case', BICUBIC, ids=[f'{p}_{go.resize_name(c)}' for p, c in BICUBIC])
def test_f32_bicubic_is_within_the_bound(prec, case):
    x = go.resize_source(prec, case, False, 'bicubic')[1]
    ref, (lo, hi) = go.bicubic_interval(prec, case, x)
    got = go.encode(prec, F.interpolate(x, case[1], mode='bicubic', align_corners=False))
    e = go.bicubic_bound(prec, case) * 2 * go.U * float(x.abs().max())
    print(f'{prec} bicubic {go.resize_name(case)}: worst error / bound {go.judge_interval("bicubic", got.float(), lo, hi, ref, prec, e):.3f}')


@pytest.mark.parametrize('kind', list(go.ACTS))
@pytest.mark.parametrize('prec', go.PRECISIONS)
def test_f32_activation_is_within_the_interval(prec, kind):
    for pair in (go.FP8_ACT_SCALES if prec == 'fp8' else (None,)):
        x = go.act_inputs(prec, pair)[1]
        ref, lo, hi, e = go.act_interval(prec, kind, x, pair)
        r = go.judge_interval(f'{prec} {kind} {pair}', go.act_standin(prec, kind, x, pair).float(), lo, hi, ref, prec, e)
        print(f'{prec} {kind} {pair or ""}: worst error / bound {r:.3f}')
        # the interval is no licence: a swapped scale or a truncating store leaves it
        if prec == 'fp8' and kind in ('relu', 'tanh'):
            swapped = go.encode(prec, go.act_f32(kind, x) * torch.tensor(go.inv_scale(pair[0]), dtype=torch.float32))
            with pytest.raises(cb.BoundError):
                go.judge_interval('swapped scales', swapped.float(), lo, hi, ref)
        if prec == 'bf16' and kind in ('leaky_relu', 'gelu'):
            trunc = (go.act_f32(kind, x).view(torch.int32) & -65536).view(torch.float32)
            with pytest.raises(cb.BoundError):
                go.judge_interval('truncated', trunc, lo, hi, ref)


def test_lap_cases_have_a_ragged_second_lap():
    items = torch.Size(go.LAP_SHAPE).numel() // 8
    assert go.LAP_ITEMS < items < 2 * go.LAP_ITEMS
    for prec in ('bf16', 'fp8'):
        v = go.lap_values(prec)
        assert torch.equal(go.encode(prec, v).float(), v) and float(v.min()) > 0
        assert float(v.max()) <= (448 if prec == 'fp8' else 1)
    # bf16 bilinear 65 x 65 -> 260 x 260: dyadic x4, the exact judge applies
    assert go.is_dyadic(65, 260)


if __name__ == '__main__':
    with open(go.MEASURED, 'w') as f:
        json.dump(measure(), f, indent=1, sort_keys=True)
        f.write('\n')
    print(open(go.MEASURED).read())
