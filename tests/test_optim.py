"""CPU tests of the optimizer step (celldetection_amd/optim.py, csrc/optim.hip, csrc/optim_chunks.h): the two restatements of
tests/optim_oracle.py against each other at the derived bounds and against torch's own float64 AdamW, the state_dict interchange
with torch.optim.AdamW, what is refused, the partition on the host (through the library and, under sanitizers, as a program of its
own) and the header.  Nothing here needs a GPU."""
import copy
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import celldetection_amd as cda
import optim_oracle as oracle
from celldetection_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('cpn_optim_info', 'cpn_optim_chunk_map', 'cpn_optim_upload', 'cpn_optim_sumsq', 'cpn_optim_norm', 'cpn_optim_adamw',
               'cpn_optim_scale')
HYPER = dict(lr=1e-3, betas=(.9, .999), eps=1e-8, weight_decay=1e-2)


def _state(n, seed, tiny_v=False):
    r = np.random.default_rng(seed)
    p = r.standard_normal(n).astype(np.float32)
    g = (r.standard_normal(n) * 10. ** r.uniform(-6, 1, n)).astype(np.float32)
    m = (r.standard_normal(n) * 10. ** r.uniform(-6, 1, n)).astype(np.float32)
    v = (10. ** (r.uniform(-30, -22, n) if tiny_v else r.uniform(-12, 2, n))).astype(np.float32)
    return p, g, m, v


CASES = [('defaults', dict(HYPER), 7, False, None), ('step 1', dict(HYPER), 1, False, None),
         ('large step', dict(HYPER), 250000, False, None), ('no decay', dict(HYPER, weight_decay=0.), 3, False, None),
         ('tiny v: eps dominates', dict(HYPER), 2, True, None), ('tiny v, step 1, no decay', dict(HYPER, weight_decay=0.), 1, True, None),
         ('large lr and decay', dict(HYPER, lr=.5, weight_decay=.3), 12, False, None),
         ('other betas, large eps', dict(HYPER, betas=(.5, .9), eps=1e-3), 4, False, None),
         ('clipped', dict(HYPER), 5, False, np.float32(.37)), ('clipped, tiny v', dict(HYPER), 1, True, np.float32(1e-3))]


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0])
def test_step_f32_is_within_the_derived_bounds_of_step_f64(case):
    _, hyper, step, tiny_v, coef = case
    p, g, m, v = _state(20000, step, tiny_v)
    if tiny_v:  # gradients so small that sqrt(v') stays far below eps, and zeros
        g = (g * np.float32(1e-9)).astype(np.float32)
        g[::7] = 0.
        m[::5] = 0.
    g[:4], m[:4] = m[:4], g[:4].copy()  # and g == m for a few: the difference cancels to zero
    got, want = oracle.step_f32(p, g, m, v, step=step, coef=coef, **hyper), oracle.step_f64(p, g, m, v, step=step, coef=coef, **hyper)
    for name, a, b, e in zip('pmv', got, want, oracle.bounds(p, g, m, v, step=step, coef=coef, **hyper)):
        err = np.abs(a.astype(np.float64) - b)
        assert np.all(np.isfinite(b)) and np.all(err <= e), (name, float((err / np.maximum(e, 1e-300)).max()))
        assert float((err / np.maximum(e, 1e-300)).max()) > .02, name  # (the bound is not vacuous: some element comes near it)
    if tiny_v:
        assert float(np.median(np.sqrt(want[2]))) < 1e-2 * hyper['eps']


@pytest.mark.parametrize('max_grad_norm', [None, .5, 1e6], ids=lambda v: f'clip {v}')
def test_step_f64_agrees_with_torch_float64_adamw_over_three_steps(max_grad_norm):
    shapes = [(7,), (3, 5), (2, 3, 4)]
    hyper = dict(HYPER, lr=2e-3)
    g_ = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(s, generator=g_, dtype=torch.float64)) for s in shapes]
    opt = torch.optim.AdamW(params, foreach=False, **hyper)
    ours = [(p.detach().numpy().copy(), np.zeros(p.shape), np.zeros(p.shape)) for p in params]
    for step in (1, 2, 3):
        grads = [torch.randn(s, generator=g_, dtype=torch.float64) * 3 for s in shapes]
        coef = None
        if max_grad_norm is not None:
            coef = min(1., max_grad_norm / (oracle.norm_f64([g.numpy() for g in grads]) + 1e-6))
        for p, g in zip(params, grads):
            p.grad = g.clone()
        if max_grad_norm is not None:
            total = torch.nn.utils.clip_grad_norm_(params, max_grad_norm, foreach=False)
            assert abs(float(total) - oracle.norm_f64([g.numpy() for g in grads])) <= 1e-12 * float(total)
        opt.step()
        for i, (p, g) in enumerate(zip(params, grads)):
            before = ours[i]
            ours[i] = oracle.step_f64(before[0], g.numpy(), before[1], before[2], step=step, coef=coef, **hyper)
            e = oracle.bounds(before[0], g.numpy(), before[1], before[2], step=step, coef=coef, **hyper)
            state = opt.state[p]
            for name, a, b, bound in zip('pmv', ours[i], (p.detach(), state['exp_avg'], state['exp_avg_sq']), e):
                assert np.all(np.abs(a - b.numpy()) <= bound), (step, i, name)
                assert np.all(np.abs(a - b.numpy()) <= 1e-6 * bound + 1e-300), (step, i, name)  # (fp64: far inside)
    if max_grad_norm == .5:
        assert coef < 1.
    if max_grad_norm == 1e6:
        assert coef == 1.


def _stepped_torch_adamw(dtype=torch.float32, steps=2):
    g_ = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(s, generator=g_).to(dtype)) for s in ((4, 3), (5,))]
    opt = torch.optim.AdamW([dict(params=params[:1], lr=3e-3), dict(params=params[1:], weight_decay=.1)], lr=1e-3, foreach=False)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g_).to(dtype)
        opt.step()
    return params, opt


def test_state_dict_of_torch_adamw_loads_here_and_back():
    params, opt = _stepped_torch_adamw()
    sd = copy.deepcopy(opt.state_dict())
    mine = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ours = cda.optim.AdamW([dict(params=mine[:1]), dict(params=mine[1:])])
    ours.load_state_dict(sd)
    assert [g['lr'] for g in ours.param_groups] == [3e-3, 1e-3] and ours.param_groups[1]['weight_decay'] == .1
    for p, q in zip(params, mine):
        s, t = opt.state[p], ours.state[q]
        assert set(t) == {'step', 'exp_avg', 'exp_avg_sq'}
        assert t['step'].dtype == torch.float32 and t['step'].device.type == 'cpu' and t['step'].dim() == 0 and float(t['step']) == 2.
        for name in ('exp_avg', 'exp_avg_sq'):
            assert t[name].dtype == torch.float32 and torch.equal(t[name], s[name]) and t[name].data_ptr() != s[name].data_ptr()
    # ... and back: a fresh torch.optim.AdamW loaded from this optimizer continues exactly like the original
    back = [torch.nn.Parameter(p.detach().clone()) for p in params]
    fresh = torch.optim.AdamW([dict(params=back[:1]), dict(params=back[1:])], foreach=False)
    fresh.load_state_dict(ours.state_dict())
    g_ = torch.Generator().manual_seed(5)
    for p, q in zip(params, back):
        p.grad = torch.randn(p.shape, generator=g_)
        q.grad = p.grad.clone()
    opt.step()
    fresh.step()
    for p, q in zip(params, back):
        assert torch.equal(p, q) and torch.equal(opt.state[p]['exp_avg_sq'], fresh.state[q]['exp_avg_sq'])
        assert float(fresh.state[q]['step']) == 3.


def test_loaded_moments_stay_float32_for_a_bfloat16_parameter():
    params, opt = _stepped_torch_adamw()
    mine = [torch.nn.Parameter(p.detach().to(torch.bfloat16)) for p in params]
    ours = cda.optim.AdamW([dict(params=mine[:1]), dict(params=mine[1:])])
    ours.load_state_dict(opt.state_dict())
    for p, q in zip(params, mine):
        assert ours.state[q]['exp_avg'].dtype == torch.float32 and torch.equal(ours.state[q]['exp_avg_sq'], opt.state[p]['exp_avg_sq'])
    params, opt = _stepped_torch_adamw()
    sd = opt.state_dict()
    sd['param_groups'][0]['amsgrad'] = True
    with pytest.raises(NotImplementedError, match='amsgrad'):
        ours.load_state_dict(sd)


def test_the_optimizer_is_a_torch_optimizer_with_groups_and_schedulers():
    p, q = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))
    opt = cda.optim.AdamW([p], lr=.1, max_grad_norm=2)
    assert isinstance(opt, torch.optim.Optimizer) and opt.max_grad_norm == 2. and opt.last_grad_norm is None
    opt.add_param_group(dict(params=[q], lr=.01, weight_decay=0.))
    assert [g['lr'] for g in opt.param_groups] == [.1, .01] and opt.param_groups[1]['betas'] == (.9, .999)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda epoch: .5 ** epoch)
    opt.step()  # (no parameter has a gradient: nothing to do, nowhere to fail, no state)
    sched.step()
    assert [g['lr'] for g in opt.param_groups] == [.05, .005] and len(opt.state) == 0
    # the scheduler classes the reference's WarmUp and SequentialLR derive from (celldetection/optim/lr_scheduler.py)
    lrs = torch.optim.lr_scheduler
    seen = []
    for cls in (cda.optim.AdamW, torch.optim.AdamW):
        opt = cls([p], lr=1.)
        seq = lrs.SequentialLR(opt, [lrs.MultiplicativeLR(opt, lambda epoch: 2.), lrs.ConstantLR(opt, factor=.5, total_iters=1)], milestones=[2])
        seen.append([])
        for _ in range(4):
            opt.step()
            seq.step()
            seen[-1].append(opt.param_groups[0]['lr'])
    assert seen[0] == seen[1] and len(set(seen[0])) > 1  # the same schedule as on torch's own optimizer
    p.grad = torch.ones(3)
    opt.zero_grad()
    assert p.grad is None
    assert cda.AdamW is cda.optim.AdamW and cda.clip_grad_norm_ is cda.optim.clip_grad_norm_ and cda.grad_norm is cda.optim.grad_norm


def test_what_is_not_supported_raises_naming_the_argument():
    def param(dtype=torch.float32):
        return torch.nn.Parameter(torch.zeros(4, dtype=dtype))

    for key in ('amsgrad', 'maximize', 'capturable', 'differentiable', 'foreach', 'fused'):
        with pytest.raises(NotImplementedError, match=key):
            cda.optim.AdamW([param()], **{key: True})
        opt = cda.optim.AdamW([param()])
        with pytest.raises(NotImplementedError, match=key):
            opt.add_param_group({'params': [param()], key: True})
        opt = cda.optim.AdamW([param()])
        opt.param_groups[0][key] = True
        with pytest.raises(NotImplementedError, match=key):
            opt.step()
    with pytest.raises(NotImplementedError, match='lr'):
        cda.optim.AdamW([param()], lr=torch.tensor(1e-3))
    opt = cda.optim.AdamW([param()])
    opt.param_groups[0]['lr'] = torch.tensor(1e-3)
    with pytest.raises(NotImplementedError, match='lr'):
        opt.step()
    p = param()
    p.grad = torch.zeros(4).to_sparse()
    with pytest.raises(NotImplementedError, match='sparse'):
        cda.optim.AdamW([p]).step()
    with pytest.raises(NotImplementedError, match='sparse'):
        cda.optim.grad_norm([p])
    p = param(torch.complex64)
    p.grad = torch.zeros(4, dtype=torch.complex64)
    with pytest.raises(NotImplementedError, match='complex'):
        cda.optim.AdamW([p]).step()
    for bad in (1., 3, float('inf')):
        with pytest.raises(NotImplementedError, match='norm_type'):
            cda.optim.clip_grad_norm_([param()], 1., norm_type=bad)
    with pytest.raises(NotImplementedError, match='error_if_nonfinite'):
        cda.optim.clip_grad_norm_([param()], 1., error_if_nonfinite=True)
    for bad in (dict(lr=-1.), dict(eps=-1.), dict(betas=(1., .9)), dict(weight_decay=-1.), dict(max_grad_norm=-1.)):
        with pytest.raises(ValueError):
            cda.optim.AdamW([param()], **bad)


def test_a_cpu_parameter_is_refused_at_step_not_at_construction():
    p = torch.nn.Parameter(torch.zeros(4))
    opt = cda.optim.AdamW([p])  # (constructing is fine: a model is often moved later)
    p.grad = torch.ones(4)
    with pytest.raises(cda.objective.DeviceError, match='no CPU fallback'):
        opt.step()
    assert len(opt.state) == 0 and torch.equal(p.detach(), torch.zeros(4))
    for fn in (cda.optim.grad_norm, lambda ps: cda.optim.clip_grad_norm_(ps, 1.)):
        with pytest.raises(cda.objective.DeviceError, match='no CPU fallback'):
            fn([p])
    assert torch.equal(p.grad, torch.ones(4))


def test_step_info_at_the_chunk_edges():
    c = cda.optim.step_info([])['chunk_elements']
    assert c == _lib.OPTIM_CHUNK and cda.optim.step_info([]) == dict(chunk_elements=c, chunks=0, partials=0, tensors=[], vectors=None)
    sizes = [0, 1, c - 1, c, c + 1, 2 * c + 3]
    info = cda.optim.step_info(sizes, [torch.float32, torch.bfloat16] * 3)
    assert [t[1:] for t in info['tensors']] == [(0, 0), (1, 1), (1, c - 1), (1, c), (2, 1), (3, 3)]
    assert [t[0] for t in info['tensors']] == [0, 0, 1, 2, 3, 5] and info['chunks'] == info['partials'] == 8
    assert info['vectors'] == [4, 8] * 3
    for size, want in zip(sizes, info['tensors']):
        assert cda.optim.step_info([size])['tensors'] == [(0,) + want[1:]]
    assert cda.step_info is cda.optim.step_info
    with pytest.raises(NotImplementedError, match='dtypes'):
        cda.optim.step_info([1], [torch.float16])
    with pytest.raises(RuntimeError, match='negative'):
        cda.optim.step_info([4, -1])
    with pytest.raises(RuntimeError, match='2\\^31 - 1 chunks'):
        cda.optim.step_info([2 ** 62])


def test_the_chunks_of_a_list_are_disjoint_ordered_and_cover_every_element_once():
    lib = _lib.load()
    c = _lib.OPTIM_CHUNK
    r = np.random.default_rng(0)
    lists = [[1, 3, 4, 5, 8, 33, c - 1, c, c + 1, 2 * c + 3], [32] * 150 + [0] + [32] * 150, [0, 0], [5 * c]]
    lists += [[int(v) for v in r.integers(0, 3 * c, r.integers(1, 30))] for _ in range(20)]
    for sizes in lists:
        info = cda.optim.step_info(sizes)
        n, chunks = len(sizes), info['chunks']
        table = np.full((chunks + 1, 2), -7, dtype=np.int32)
        _lib.check(lib.cpn_optim_chunk_map((ctypes.c_int64 * n)(*sizes), n, table.ctypes.data, chunks), 'chunk_map')
        assert table[chunks].tolist() == [-7, -7]
        covered = [np.zeros(s, dtype=np.int32) for s in sizes]
        for i, (t, k) in enumerate(table[:chunks].tolist()):
            first, count, tail = info['tensors'][t]
            assert first + k == i and 0 <= k < count  # ordered: tensor after tensor, chunk after chunk
            covered[t][k * c:min((k + 1) * c, sizes[t])] += 1
            assert min((k + 1) * c, sizes[t]) - k * c == (tail if k == count - 1 else c)
        assert all(bool((a == 1).all()) for a in covered)
        assert lib.cpn_optim_chunk_map((ctypes.c_int64 * n)(*sizes), n, table.ctypes.data, chunks + 1) == _lib.E_INVALID
        assert b'cpn_optim_info' in lib.cpn_last_error()


def test_every_launch_refuses_bad_arguments_before_it_reads_a_pointer():
    lib = _lib.load()
    rec = np.zeros(2, dtype=cda.optim._RECORD)
    dev = ctypes.c_void_p(0x7f0000000000)  # (never read: every call below fails its checks first, or has nothing to do)
    for edit, what in ((dict(numel=-1), 'negative size'), (dict(dtype=2), 'dtype'), (dict(numel=4), 'null tensor pointer'),
                       (dict(numel=4, g=0x1002, dtype=0), 'not aligned to its element'), (dict(numel=4, g=0x1001, dtype=1), 'not aligned')):
        rec[:] = 0
        for key, value in edit.items():
            rec[key][1] = value
        assert lib.cpn_optim_upload(rec.ctypes.data_as(ctypes.POINTER(_lib.OptimTensor)), 2, 0, dev, None) == _lib.E_INVALID, what
        assert what.encode() in lib.cpn_last_error(), (what, lib.cpn_last_error())
    assert lib.cpn_optim_upload(None, 0, 1, None, None) == 0 and lib.cpn_optim_upload(None, 2, 1, dev, None) == _lib.E_INVALID
    for launch, tail in ((lib.cpn_optim_sumsq, (dev, None)), (lib.cpn_optim_adamw, (None, 0, None)), (lib.cpn_optim_scale, (dev, None))):
        assert launch(dev, -1, dev, 1, *tail) == _lib.E_INVALID and launch(dev, 1, dev, -1, *tail) == _lib.E_INVALID
        assert launch(None, 1, dev, 1, *tail) == _lib.E_INVALID and launch(dev, 1, None, 1, *tail) == _lib.E_INVALID
        assert launch(dev, 1, dev, 2 ** 31, *tail) == _lib.E_UNSUPPORTED
        assert launch(ctypes.c_void_p(0x7f0000000004), 1, dev, 1, *tail) == _lib.E_INVALID
        assert launch(dev, 1, dev, 0, *tail) == 0  # nothing to do: no launch
    assert lib.cpn_optim_adamw(dev, 1, dev, 1, None, 2, None) == _lib.E_INVALID and b'nontemporal' in lib.cpn_last_error()
    assert lib.cpn_optim_scale(dev, 1, dev, 1, None, None) == _lib.E_INVALID and lib.cpn_optim_sumsq(dev, 1, dev, 1, None, None) == _lib.E_INVALID
    for bad in (-1., float('nan')):
        assert lib.cpn_optim_norm(dev, 1, bad, dev, None) == _lib.E_INVALID and b'max_norm' in lib.cpn_last_error()
    assert lib.cpn_optim_norm(None, 1, 1., dev, None) == _lib.E_INVALID and lib.cpn_optim_norm(dev, 1, 1., None, None) == _lib.E_INVALID


def test_the_header_states_the_rule_and_the_library_exports_it():
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    section = hdr[hdr.index('/* ---- Optimizer step'):]
    for phrase in ('p = p * decay', 'm = m + (g - m) * w1', 'v = v * beta2 + (g * g) * w2', 'denom = sqrt(v) / bc2_sqrt + eps',
                   'p = p - step_size * (m / denom)', 'min(1, max_norm / ((double) norm + 1e-6))', 'No floating-point atomics',
                   'Additions to ABI 22', 'torch.nn.utils.clip_grad_norm_', 'lightning_base.py'):
        assert phrase in section, phrase
    code = re.sub(r'/\*.*?\*/', '', section, flags=re.S)
    assert set(re.findall(r'\b(cpn_[a-z0-9_]+)\s*\(', code)) == set(NEW_SYMBOLS)
    assert int(re.search(r'#define CPN_OPTIM_CHUNK (\d+)', code).group(1)) == _lib.OPTIM_CHUNK
    declared = set(re.findall(r'\b(cpn_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)))
    assert declared == set(_lib.EXPORTED_SYMBOLS) and set(NEW_SYMBOLS) <= declared
    lib = _lib.load()
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    assert cda.optim._RECORD.itemsize == _lib.OPTIM_TENSOR_BYTES == 80
    assert cda.optim._RECORD.names == ('p', 'g', 'm', 'v', 'numel', 'dtype', 'flags', 'lr', 'decay', 'w1', 'beta2', 'w2', 'eps', 'step_size',
                                       'bc2_sqrt')
    src = build.SOURCES['optim.hip']
    assert '-ffp-contract=off' in src and '-fhip-fp32-correctly-rounded-divide-sqrt' in src and 'optim_chunks.h' in build.HEADERS
    want = oracle.scalars(1e-3, (.9, .999), 1e-8, 1e-2, 3.)
    assert cda.optim.scalars(1e-3, (.9, .999), 1e-8, 1e-2, 3.)[1:] == want  # (the module and the oracle state the same scalars)


def test_the_oracles_roundings_to_bfloat16():
    x = np.array([1 + 2. ** -8, 1 + 3 * 2. ** -8, 1 + 2. ** -8 + 2. ** -30, -3.14159, 2. ** -130, 0.], dtype=np.float64)
    assert oracle.bf16_from_f64(x).tolist()[:3] == [1., 1 + 2. ** -6, 1 + 2. ** -7]
    f = x.astype(np.float32)
    assert np.array_equal(oracle.bf16_rne(f), torch.from_numpy(f).to(torch.bfloat16).float().numpy())
    # one rounding differs from two: 1 + 2^-8 + 2^-30 rounds up to 1 + 2^-7, but through float32 it first becomes the tie 1 + 2^-8
    assert float(oracle.bf16_rne(np.float32(x[2]))) == 1. and float(oracle.bf16_from_f64(x[2])) == 1 + 2. ** -7
    # the unit roundoff of bf16 is 2^-8 (8 significant bits): reached to within a factor 2, never exceeded
    r = np.random.default_rng(1).standard_normal(100000).astype(np.float32)
    rel = np.abs(oracle.bf16_rne(r).astype(np.float64) - r) / np.abs(r)
    assert 2. ** -9 < float(rel.max()) <= 2. ** -8
    assert float(oracle.clip_coef(np.float32(2.), 1.)) == float(np.float32(1. / (2. + 1e-6))) and float(oracle.clip_coef(.5, 1.)) == 1.


def test_host_build_of_the_chunk_arithmetic_agrees_with_brute_force(tmp_path):
    """``csrc/optim_chunks.h`` compiled for the host only, with AddressSanitizer and UBSan on the host code, by
    ``tests/optim_chunks_host.cpp`` (a program of its own, nothing preloaded)."""
    hipcc = build._hipcc()
    exe = str(tmp_path / 'optim_chunks_host')
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(ROOT, 'tests', 'optim_chunks_host.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r'ok \d+', run.stdout.strip()), run.stdout[-500:] + run.stderr[-2000:]
    assert int(run.stdout.split()[1]) > 100000
