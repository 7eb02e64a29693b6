"""GPU tests of the optimizer step (celldetection_amd/optim.py, csrc/optim.hip): AdamW bit for bit against the float32 restatement
of tests/optim_oracle.py at the chunk edges ``step_info`` names, in float32, bfloat16 and mixed; the bookkeeping over steps and
groups; misaligned views; many small tensors; the norm, the clip coefficient and both forms of clipping; torch's float64 AdamW at the
derived bounds; and real gradients of a conv + batch norm stack."""
import numpy as np
import pytest
import torch

import celldetection_amd as cda
import optim_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16 = torch.float32, torch.bfloat16
HYPER = dict(lr=1e-3, betas=(.9, .999), eps=1e-8, weight_decay=1e-2)
C = cda.optim.step_info([])['chunk_elements']
EDGES = [1, 3, 4, 5, 8, 33, C - 1, C, C + 1, 2 * C + 3]
LISTS = {'float32': [F32] * len(EDGES), 'bfloat16': [BF16] * len(EDGES), 'mixed': [F32, BF16] * (len(EDGES) // 2)}


def _host(sizes, dtypes, seed, state=True):
    """Per tensor float32 arrays p, g, m, v (p and g exact bf16 values where the dtype is bfloat16); magnitudes over several decades,
    all fp32-normal with normal squares."""
    r = np.random.default_rng(seed)
    out = []
    for n, dt in zip(sizes, dtypes):
        p = r.standard_normal(n).astype(np.float32)
        g = (r.standard_normal(n) * 10. ** r.uniform(-4, 1, n)).astype(np.float32)
        if dt == BF16:
            p, g = oracle.bf16_rne(p), oracle.bf16_rne(g)
        m = (r.standard_normal(n) * 10. ** r.uniform(-4, 1, n)).astype(np.float32) if state else np.zeros(n, np.float32)
        v = (10. ** r.uniform(-10, 2, n)).astype(np.float32) if state else np.zeros(n, np.float32)
        out.append(dict(p=p, g=g, m=m, v=v))
    return out


def _dev(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _params(host, dtypes):
    params = []
    for h, dt in zip(host, dtypes):
        p = torch.nn.Parameter(_dev(h['p'], dt))
        p.grad = _dev(h['g'], dt)
        params.append(p)
    return params


def _set_state(opt, params, host, step):
    for p, h in zip(params, host):
        opt.state[p] = dict(step=torch.tensor(float(step), dtype=F32), exp_avg=_dev(h['m']), exp_avg_sq=_dev(h['v']))


_np, _same = oracle.np_of, oracle.same  # (the checks of one step live in tests/optim_oracle.py: the training-step tests share them)


def _expect(h, dt, step, hyper=HYPER, coef=None):
    return oracle.expect(h, dt == BF16, step, hyper, coef)


def _assert_step(opt, params, host, dtypes, step, hyper=HYPER, coef=None):
    oracle.assert_step(opt, params, host, [dt == BF16 for dt in dtypes], step, hyper, coef)


@pytest.mark.parametrize('kind', list(LISTS))
def test_one_step_is_the_float32_rule_bit_for_bit_at_the_chunk_edges(kind):
    dtypes = LISTS[kind]
    info = cda.optim.step_info(EDGES, dtypes)
    assert [t[1] for t in info['tensors']] == [1] * 8 + [2, 3] and info['tensors'][-1][2] == 3 and info['tensors'][6][2] == C - 1
    host = _host(EDGES, dtypes, seed=1)
    params = _params(host, dtypes)
    opt = cda.optim.AdamW(params, **HYPER)
    _set_state(opt, params, host, 6)
    opt.step()
    _assert_step(opt, params, host, dtypes, 7)
    assert opt.last_grad_norm is None


@pytest.mark.parametrize('nontemporal', [0, 1])
def test_both_store_policies_of_the_moments_give_the_rule(nontemporal, monkeypatch):
    monkeypatch.setattr(cda.optim, 'NONTEMPORAL', nontemporal)
    sizes, dtypes = [5, C + 1, 2 * C + 3, 33], [F32, BF16, F32, BF16]
    host = _host(sizes, dtypes, seed=9)
    params = _params(host, dtypes)
    opt = cda.optim.AdamW(params, **HYPER)
    _set_state(opt, params, host, 1)
    opt.step()
    _assert_step(opt, params, host, dtypes, 2)


def test_three_steps_over_two_groups_with_an_lr_change():
    sizes, dtypes = [5, C + 1, 33, 2 * C + 3], [F32, BF16, BF16, F32]
    host = _host(sizes, dtypes, seed=2, state=False)
    params = _params(host, dtypes)
    hypers = [dict(HYPER, lr=2e-3, weight_decay=0.), dict(HYPER, lr=5e-4, weight_decay=.1, betas=(.8, .99))]
    opt = cda.optim.AdamW([dict(params=params[:2], **hypers[0]), dict(params=params[2:], **hypers[1])])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=.5)
    r = np.random.default_rng(20)
    for step in (1, 2, 3):
        for p, h, dt in zip(params, host, dtypes):
            g = r.standard_normal(h['g'].shape).astype(np.float32)
            h['g'] = oracle.bf16_rne(g) if dt == BF16 else g
            p.grad = _dev(h['g'], dt)  # a new tensor every step, as after zero_grad(set_to_none=True)
        lrs = [g['lr'] for g in opt.param_groups]
        assert lrs == [hypers[0]['lr'] * .5 ** (step - 1), hypers[1]['lr'] * .5 ** (step - 1)]
        opt.step()
        for lo, hi, hyper, lr in ((0, 2, hypers[0], lrs[0]), (2, 4, hypers[1], lrs[1])):
            _assert_step(opt, params[lo:hi], host[lo:hi], dtypes[lo:hi], step, dict(hyper, lr=lr))
        for i, (h, dt) in enumerate(zip(host, dtypes)):
            h['p'], h['m'], h['v'] = _expect(h, dt, step, dict(hypers[i // 2], lr=lrs[i // 2]))
        sched.step()
        opt.zero_grad()


@pytest.mark.parametrize('dtype', [F32, BF16], ids=str)
@pytest.mark.parametrize('which', ['parameter', 'gradient'])
def test_a_view_at_storage_offset_one_takes_the_scalar_path_with_the_same_bits(which, dtype):
    sizes, dtypes = [33, C + 5], [dtype, dtype]
    host = _host(sizes, dtypes, seed=3)
    params = []
    for h in host:
        n = h['p'].size
        if which == 'parameter':
            buf = torch.zeros(n + 1, dtype=dtype, device=DEV)
            buf[1:].copy_(_dev(h['p'], dtype))
            p = torch.nn.Parameter(buf[1:])
            p.grad = _dev(h['g'], dtype)
        else:
            p = torch.nn.Parameter(_dev(h['p'], dtype))
            buf = torch.zeros(n + 1, dtype=dtype, device=DEV)
            buf[1:].copy_(_dev(h['g'], dtype))
            p.grad = buf[1:]
        moved = p if which == 'parameter' else p.grad
        assert moved.storage_offset() == 1 and moved.data_ptr() % 16 != 0 and moved.is_contiguous()
        params.append(p)
    opt = cda.optim.AdamW(params, max_grad_norm=1e-2, **HYPER)
    _set_state(opt, params, host, 2)
    opt.step()
    # the aligned run on the same values: the same bits in p, m, v and in the norm
    aligned = _params(host, dtypes)
    ref = cda.optim.AdamW(aligned, max_grad_norm=1e-2, **HYPER)
    _set_state(ref, aligned, host, 2)
    ref.step()
    assert all(t.data_ptr() % 16 == 0 for p in aligned for t in (p, p.grad))
    assert _same(opt.last_grad_norm, _np(ref.last_grad_norm)) and _same(opt.last_clip_coef, _np(ref.last_clip_coef))
    for p, q in zip(params, aligned):
        assert _same(p, _np(q)) and _same(opt.state[p]['exp_avg'], _np(ref.state[q]['exp_avg']))
        assert _same(opt.state[p]['exp_avg_sq'], _np(ref.state[q]['exp_avg_sq']))
    _assert_step(opt, params, host, dtypes, 3, coef=_np(opt.last_clip_coef))


def test_many_small_tensors_some_without_a_gradient_one_empty():
    sizes = [32] * 150 + [0] + [32] * 150
    dtypes = [F32 if i % 3 else BF16 for i in range(len(sizes))]
    host = _host(sizes, dtypes, seed=4, state=False)
    params = _params(host, dtypes)
    absent = set(range(0, len(sizes), 7))
    for i in absent:
        params[i].grad = None
    opt = cda.optim.AdamW(params, **HYPER)
    opt.step()
    for i, (p, h, dt) in enumerate(zip(params, host, dtypes)):
        if i in absent:
            assert _same(p, h['p']) and p not in opt.state
        else:
            _assert_step(opt, [p], [h], [dt], 1)
    assert 150 not in absent and opt.state[params[150]]['exp_avg'].numel() == 0


def test_more_chunks_than_workgroups():
    """2500 tensors of 3 elements: 2500 chunks walked by the 2048 workgroups of a launch, in the norm as in the update."""
    n = 2500
    assert cda.optim.step_info([3] * n)['chunks'] == n > 2048
    host = _host([3] * n, [F32] * n, seed=5)
    flat = {k: np.zeros(4 * n, np.float32) for k in 'pgmv'}
    for i, h in enumerate(host):
        for k in 'pgmv':
            flat[k][4 * i:4 * i + 3] = h[k]
    dev = {k: _dev(a) for k, a in flat.items()}
    params = []
    for i in range(n):
        p = torch.nn.Parameter(dev['p'][4 * i:4 * i + 3])
        p.grad = dev['g'][4 * i:4 * i + 3]
        params.append(p)
    opt = cda.optim.AdamW(params, max_grad_norm=1., **HYPER)
    for i, p in enumerate(params):
        opt.state[p] = dict(step=torch.tensor(1., dtype=F32), exp_avg=dev['m'][4 * i:4 * i + 3], exp_avg_sq=dev['v'][4 * i:4 * i + 3])
    opt.step()
    want = oracle.norm_f64([h['g'] for h in host])
    norm = float(opt.last_grad_norm)
    assert abs(norm - want) <= oracle.norm_bound([h['g'] for h in host]) * want
    coef = _np(opt.last_clip_coef)
    assert coef == oracle.clip_coef(norm, 1.) and coef < 1.
    got = {k: _np(dev[k]).reshape(n, 4) for k in 'pmv'}
    for i in (0, 1, 2047, 2048, 2049, n - 1):
        for k, w in zip('pmv', _expect(host[i], F32, 2, coef=coef)):
            assert np.array_equal(got[k][i, :3], w), (i, k)
    assert all(bool((got[k][:, 3] == 0).all()) for k in 'pmv')  # the gaps between the views are untouched
    p, m, v = oracle.step_f32(flat['p'], flat['g'], flat['m'], flat['v'], step=2, coef=coef, **HYPER)
    keep = np.arange(4 * n) % 4 != 3
    assert np.array_equal(got['p'].ravel()[keep], p[keep]) and np.array_equal(got['v'].ravel()[keep], v[keep])


def test_the_norm_is_within_its_bound_repeats_and_does_not_depend_on_the_storage():
    dtypes = LISTS['mixed']
    host = _host(EDGES, dtypes, seed=6)
    params = _params(host, dtypes)
    want = oracle.norm_f64([h['g'] for h in host])
    first = cda.optim.grad_norm(params)
    assert first.dtype == F32 and first.dim() == 0 and first.is_cuda
    assert abs(float(first) - want) <= oracle.norm_bound([h['g'] for h in host]) * want
    assert _same(cda.optim.grad_norm(params), _np(first))
    assert all(_same(p.grad, h['g']) for p, h in zip(params, host))
    # the partition is per tensor, so "the same order and chunking" holds for any storage of the same list: here every gradient is
    # a view into one flat buffer of each dtype, back to back (most views start at an address that is no multiple of 16)
    flats = {dt: torch.cat([p.grad for p, d in zip(params, dtypes) if d == dt]) for dt in (F32, BF16)}
    offsets, views, odd = {F32: 0, BF16: 0}, [], 0
    for p, dt in zip(params, dtypes):
        q = torch.nn.Parameter(p.detach().clone())
        q.grad = flats[dt][offsets[dt]:offsets[dt] + p.numel()]
        odd += q.grad.data_ptr() % 16 != 0
        offsets[dt] += p.numel()
        views.append(q)
    assert odd >= 4 and _same(cda.optim.grad_norm(views), _np(first))
    # a single tensor, a parameter without a gradient among others, and non-finite values
    assert float(cda.optim.grad_norm(params[3])) == float(np.float32(oracle.norm_f64([host[3]['g']])))
    params[0].grad = None
    rest = oracle.norm_f64([h['g'] for h in host[1:]])
    assert abs(float(cda.optim.grad_norm(params)) - rest) <= oracle.norm_bound([h['g'] for h in host[1:]]) * rest
    params[2].grad[1] = float('inf')
    assert float(cda.optim.grad_norm(params)) == float('inf')
    params[2].grad[1] = float('nan')
    assert np.isnan(float(cda.optim.grad_norm(params)))


@pytest.mark.parametrize('kind', ['float32', 'mixed'])
def test_clipping_inside_the_step_and_on_its_own(kind):
    dtypes = LISTS[kind]
    host = _host(EDGES, dtypes, seed=7)
    norm = _np(cda.optim.grad_norm(_params(host, dtypes)))
    assert norm > 1.
    for max_norm in (.5 * float(norm), float(norm), 2. * float(norm)):
        coef = oracle.clip_coef(norm, max_norm)
        assert coef < 1. if max_norm < float(norm) else (coef == 1. if max_norm > float(norm) else coef <= 1.)
        params = _params(host, dtypes)
        opt = cda.optim.AdamW(params, max_grad_norm=max_norm, **HYPER)
        _set_state(opt, params, host, 9)
        opt.step()
        assert _same(opt.last_grad_norm, norm) and opt.last_grad_norm.dtype == F32 and opt.last_grad_norm.dim() == 0
        assert _same(opt.last_clip_coef, coef)  # the float32-rounded float64 expression, from the float32 norm
        _assert_step(opt, params, host, dtypes, 10, coef=coef)  # (asserts that .grad is unchanged, too)
        params = _params(host, dtypes)
        total = cda.optim.clip_grad_norm_(params, max_norm)
        assert _same(total, norm) and total.dim() == 0 and total.is_cuda
        for p, h, dt in zip(params, host, dtypes):
            want = oracle.bf16_from_f64(h['g'].astype(np.float64) * float(coef)) if dt == BF16 else h['g'] * coef
            assert _same(p.grad, want), (p.numel(), dt)


@pytest.mark.parametrize('max_grad_norm', [None, 3.], ids=lambda v: f'clip {v}')
@pytest.mark.parametrize('dtype', [F32, BF16], ids=str)
def test_one_step_against_torch_float64_adamw_at_the_derived_bounds(dtype, max_grad_norm):
    sizes, dtypes = [33, C + 1], [dtype, dtype]
    host = _host(sizes, dtypes, seed=8)
    params = _params(host, dtypes)
    opt = cda.optim.AdamW(params, max_grad_norm=max_grad_norm, **HYPER)
    _set_state(opt, params, host, 4)
    opt.step()
    cpu = [torch.nn.Parameter(torch.from_numpy(h['p'].astype(np.float64))) for h in host]
    for q, h in zip(cpu, host):
        q.grad = torch.from_numpy(h['g'].astype(np.float64))
    ref = torch.optim.AdamW(cpu, foreach=False, **HYPER)
    for q, h in zip(cpu, host):
        ref.state[q] = dict(step=torch.tensor(4.), exp_avg=torch.from_numpy(h['m'].astype(np.float64)),
                            exp_avg_sq=torch.from_numpy(h['v'].astype(np.float64)))
    coef = None
    if max_grad_norm is not None:
        total = float(torch.nn.utils.clip_grad_norm_(cpu, max_grad_norm, foreach=False))
        coef = min(1., max_grad_norm / (total + 1e-6))
        assert coef < 1. and abs(float(opt.last_grad_norm) - total) <= oracle.norm_bound([h['g'] for h in host]) * total
    ref.step()
    for p, q, h in zip(params, cpu, host):
        e = oracle.bounds(h['p'], h['g'], h['m'], h['v'], step=5, coef=coef, bf16=dtype == BF16, **HYPER)
        for name, got, want, bound in zip('pmv', (p, opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq']),
                                          (q.detach(), ref.state[q]['exp_avg'], ref.state[q]['exp_avg_sq']), e):
            err = np.abs(_np(got).astype(np.float64) - want.numpy())
            assert np.all(err <= bound), (name, float((err / np.maximum(bound, 1e-300)).max()))


def test_real_gradients_of_a_conv_and_batch_norm_stack():
    torch.manual_seed(0)
    net = torch.nn.Sequential(cda.nn.Conv2d(32, 32, 3), cda.nn.BatchNorm2d(32)).to(DEV).train()
    x = torch.randn(1, 32, 8, 8, device=DEV)
    net(x).float().square().mean().backward()
    params = [p for p in net.parameters()]
    assert len(params) == 4 and all(p.grad is not None and p.grad.is_cuda for p in params)
    host = [dict(p=_np(p).copy(), g=_np(p.grad).copy(), m=np.zeros(p.numel(), np.float32).reshape(p.shape),
                 v=np.zeros(p.numel(), np.float32).reshape(p.shape)) for p in params]
    dtypes = [p.dtype for p in params]
    assert float(np.abs(host[0]['g']).max()) > 0.
    opt = cda.optim.AdamW(net.parameters(), max_grad_norm=1., **HYPER)
    opt.step()
    want = oracle.norm_f64([h['g'] for h in host])
    norm = _np(opt.last_grad_norm)
    assert abs(float(norm) - want) <= oracle.norm_bound([h['g'] for h in host]) * want
    _assert_step(opt, params, host, dtypes, 1, coef=oracle.clip_coef(norm, 1.))
    assert _same(opt.last_clip_coef, oracle.clip_coef(norm, 1.))


def test_a_non_contiguous_parameter_or_gradient_is_refused():
    p = torch.nn.Parameter(torch.zeros(4, 6, device=DEV).t())
    p.grad = torch.ones(6, 4, device=DEV)
    with pytest.raises(NotImplementedError, match='non-contiguous parameter'):
        cda.optim.AdamW([p]).step()
    q = torch.nn.Parameter(torch.zeros(6, 4, device=DEV))
    q.grad = torch.ones(4, 6, device=DEV).t()
    with pytest.raises(NotImplementedError, match='non-contiguous gradient'):
        cda.optim.AdamW([q]).step()
    with pytest.raises(NotImplementedError, match='non-contiguous gradient'):
        cda.optim.clip_grad_norm_([q], 1.)
    h = torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float16))
    h.grad = torch.ones(4, device=DEV, dtype=torch.float16)
    with pytest.raises(NotImplementedError, match='float16'):
        cda.optim.AdamW([h]).step()
    assert float(q.detach().abs().sum()) == 0. and float(q.grad.sum()) == 24.
