"""CPU tests of the trainable batch normalisation (celldetection_amd/nn/batch_norm.py, csrc/batch_norm.hip, csrc/bn_slabs.h): the fp64
statements of tests/batch_norm_oracle.py against torch's own autograd, the wrong rules the cases tell apart, the judge of the GPU
tests on a CPU emulation of the stated arithmetic (and on three wrong ones), the lane mapping on the host under sanitizers, the
host-side entry points and the Python surface.  Nothing here needs a GPU."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest
import torch

import celldetection_amd as cda
from celldetection_amd import _lib, build
import batch_norm_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('cpn_bn_info', 'cpn_bn_workspace_bytes', 'cpn_bn_train_stats', 'cpn_bn_eval_coeffs', 'cpn_bn_apply',
         'cpn_bn_backward_reduce', 'cpn_bn_backward_input')


def _operands(n, c, h, w, seed=0, affine=True, offset=0.):
    g = torch.Generator().manual_seed(seed + 100 * c + h)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * (1 + torch.arange(c, dtype=torch.float64).reshape(1, c, 1, 1) / c) \
        + offset + torch.randn(1, c, 1, 1, generator=g, dtype=torch.float64)
    dy = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(c, generator=g, dtype=torch.float64) if affine else None
    b = torch.randn(c, generator=g, dtype=torch.float64) if affine else None
    rm = torch.randn(c, generator=g, dtype=torch.float64)
    rv = torch.rand(c, generator=g, dtype=torch.float64) + .5
    return x, dy, wt, b, rm, rv


# (n, c, h, w): M = 2 (the smallest batch torch trains on), odd sizes, more than one image
SHAPES = [(2, 8, 1, 1), (1, 8, 1, 2), (2, 16, 5, 7), (3, 8, 4, 3)]


@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('affine', [True, False], ids=['affine', 'plain'])
@pytest.mark.parametrize('momentum', [0.1, 1.0, 'cumulative'], ids=str)
def test_statements_equal_torch_autograd(shape, training, affine, momentum):
    x, dy, wt, b, rm, rv = _operands(*shape, affine=affine)
    eps = 1e-5
    close = dict(rtol=1e-12, atol=1e-12)
    steps = 3 if momentum == 'cumulative' else 1  # torch's cumulative average: momentum = 1 / num_batches_tracked, step by step
    for step in range(1, steps + 1):
        mom = 1. / step if momentum == 'cumulative' else momentum
        for relu in (False, True):
            y, dx, dg, db, new_rm, new_rv = oracle.autograd64(x, dy, wt, b, rm, rv, training, mom, eps, relu)
            f = oracle.forward(x, wt, b, rm, rv, training, mom, eps, relu)
            torch.testing.assert_close(f['y'], y, **close)
            torch.testing.assert_close(f['running_mean'], new_rm, **close)
            torch.testing.assert_close(f['running_var'], new_rv, **close)
            back = oracle.backward(x, dy, wt, f['mean'], f['invstd'], oracle.mask(f['t']) if relu else None, training)
            torch.testing.assert_close(back['dx'], dx, **close)
            if affine:
                torch.testing.assert_close(back['dgamma'], dg, **close)
                torch.testing.assert_close(back['dbeta'], db, **close)
            assert bool((back['S_dx'] >= back['dx'].abs() - 1e-9).all()) and bool((back['S_dgamma'] >= back['dgamma'].abs() - 1e-9).all())
        rm, rv = new_rm, new_rv
    # without running buffers the statement normalises with the batch statistics in eval mode too, as torch's module does (it
    # then calls its functional with training = True)
    y, dx, *_ = oracle.autograd64(x, dy, wt, b, None, None, True, 0.1, eps, True)
    f = oracle.forward(x, wt, b, None, None, training, 0.1, eps, True)
    torch.testing.assert_close(f['y'], y, **close)
    torch.testing.assert_close(oracle.backward(x, dy, wt, f['mean'], f['invstd'], oracle.mask(f['t']), True)['dx'], dx, **close)


def test_wrong_rules_are_told_apart():
    """Each rule of batch_norm_oracle.WRONG_RULES moves some result of a case by at least a tenth of that result's mean magnitude:
    far more than any bound the GPU tests accept.  (M / (M - 1) is 2 at M = 2 and 1.014 at M = 70: the two variance rules are told
    apart on the small case, every other rule on both.)"""
    assert len(oracle.WRONG_RULES) >= 8
    told = set()
    for shape in [(2, 8, 1, 1), (2, 16, 5, 7)]:
        x, dy, wt, b, rm, rv = _operands(*shape)
        x[0, :, 0, 0] = rm  # eval: t is exactly beta here; with beta = 0 the mask's edge
        zero_b = torch.zeros_like(b)

        def differs(got, ref):
            return float((got - ref).abs().max()) > .1 * float(ref.abs().mean())

        f = oracle.forward(x, wt, b, rm, rv, True, 0.1, 1e-5, True)
        for rule, key in (('unbiased_variance_normalises', 'y'), ('eps_outside_root', 'y'), ('biased_running_var', 'running_var'),
                          ('momentum_swapped', 'running_mean')):
            eps = 1. if rule == 'eps_outside_root' else 1e-5  # (an eps the result can see)
            ref = oracle.forward(x, wt, b, rm, rv, True, 0.1, eps, True)
            apart = differs(oracle.forward(x, wt, b, rm, rv, True, 0.1, eps, True, rule)[key], ref[key])
            assert apart or (shape[2] > 1 and rule in ('unbiased_variance_normalises', 'biased_running_var')), (rule, shape)
            if apart:
                told.add(rule)
        ev = oracle.forward(x, wt, b, rm, rv, False, 0.1, 1e-5, True)
        assert differs(oracle.forward(x, wt, b, rm, rv, False, 0.1, 1e-5, True, 'eval_uses_batch_statistics')['y'], ev['y']), shape
        told.add('eval_uses_batch_statistics')
        back = oracle.backward(x, dy, wt, f['mean'], f['invstd'], oracle.mask(f['t']), True)
        for rule in ('dx_without_mean_term', 'dx_without_projection_term'):
            wrong = oracle.backward(x, dy, wt, f['mean'], f['invstd'], oracle.mask(f['t']), True, rule)
            assert differs(wrong['dx'], back['dx']), (rule, shape)
            told.add(rule)
        e0 = oracle.forward(x, wt, zero_b, rm, rv, False, 0.1, 1e-5, True)
        assert bool((e0['t'][0, :, 0, 0] == 0).all())
        right = oracle.backward(x, dy, wt, e0['mean'], e0['invstd'], oracle.mask(e0['t']), False)
        wrong = oracle.backward(x, dy, wt, e0['mean'], e0['invstd'], oracle.mask(e0['t'], 'mask_includes_zero'), False)
        assert bool((right['dx'][0, :, 0, 0] == 0).all()) and differs(wrong['dx'], right['dx']), shape
        told.add('mask_includes_zero')
    assert told == set(oracle.WRONG_RULES)


# ---- the judge of the GPU tests, on the CPU

def _judge_all(name, x, dy, out, chain, wt, b, rm, rv, training, relu):
    oracle.judge_stats(name, x, out, chain, wt, b, rm, rv, training, 0.1, 1e-5)
    oracle.judge_y(name, x, out['y'], out['scale'], out['shift'], relu)
    oracle.judge_grads(name, x, dy, out, chain, wt, out['save_mean'], out['save_invstd'], out['scale'], out['shift'], relu,
                       training or rm is None)


def _typed(shape, dtype, offset=0., seed=0):
    x, dy, wt, b, rm, rv = _operands(*shape, seed=seed, offset=offset)
    return x.to(dtype), dy.to(dtype), wt.float(), b.float(), rm.float(), rv.float()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('relu', [False, True], ids=['none', 'relu'])
def test_judge_accepts_the_stated_arithmetic(dtype, training, relu):
    for shape in [(2, 8, 1, 1), (2, 24, 5, 7), (2, 8, 17, 33)]:
        x, dy, wt, b, rm, rv = _typed(shape, dtype)
        m = x.numel() // shape[1]
        out = oracle.emulate(x, dy, wt, b, rm, rv, training, 0.1, 1e-5, relu)
        _judge_all(f'{shape}', x, dy, out, cda.nn.batch_norm_info(m, shape[1])['chain'], wt, b, rm, rv, training, relu)
    x, dy, wt, b, rm, rv = _typed((2, 8, 17, 33), dtype, offset=300.)
    out = oracle.emulate(x, dy, wt, b, rm, rv, training, 0.1, 1e-5, relu)
    _judge_all('x = 300 + randn', x, dy, out, cda.nn.batch_norm_info(2 * 17 * 33, 8)['chain'], wt, b, rm, rv, training, relu)


def test_judge_rejects_fp32_sum_of_squares():
    x, dy, wt, b, rm, rv = _typed((2, 8, 17, 33), torch.float32, offset=300.)
    chain = cda.nn.batch_norm_info(2 * 17 * 33, 8)['chain']
    out = oracle.emulate(x, dy, wt, b, rm, rv, True, 0.1, 1e-5, False, sumsq_dtype=torch.float32)
    with pytest.raises(AssertionError, match='save_invstd'):
        oracle.judge_stats('fp32 sums', x, out, chain, wt, b, rm, rv, True, 0.1, 1e-5)


def test_judge_rejects_one_bf16_step():
    x, dy, wt, b, rm, rv = _typed((2, 8, 5, 7), torch.bfloat16)
    out = oracle.emulate(x, dy, wt, b, rm, rv, True, 0.1, 1e-5, True)
    oracle.judge_y('as stated', x, out['y'], out['scale'], out['shift'], True)
    y = out['y'].clone()
    bits = y.view(torch.int16)
    where = int(torch.argmax(y.float().reshape(-1)))  # one positive element, one bf16 step up
    bits.view(-1)[where] += 1
    with pytest.raises(AssertionError):
        oracle.judge_y('one step', x, y, out['scale'], out['shift'], True)
    for key in ('dx',):
        dx = out[key].clone()
        dx.view(torch.int16).view(-1)[int(torch.argmax(dx.float().abs().reshape(-1)))] += 1
        with pytest.raises(AssertionError):
            oracle.judge_grads('one step', x, dy, dict(dx=dx), 100, wt, out['save_mean'], out['save_invstd'], out['scale'],
                               out['shift'], True)


def test_judge_rejects_a_mask_from_the_unrounded_coefficients():
    """x == running_mean in eval mode with beta = 0: t is exactly 0 with the fp64 coefficients (mask off), and whatever sign
    x * fl32(scale) + fl32(-mean * scale) has with the fp32 coefficients the kernel uses -- the judge goes by the latter."""
    c = 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, c, 3, 3, generator=g)
    dy = torch.randn(2, c, 3, 3, generator=g) + 3.
    rm = x[0, :, 0, 0].clone()
    rv = torch.rand(c, generator=g) + .5
    wt, b = torch.rand(c, generator=g) + .5, torch.zeros(c)
    right = oracle.emulate(x, dy, wt, b, rm, rv, False, 0.1, 1e-5, True)
    wrong = oracle.emulate(x, dy, wt, b, rm, rv, False, 0.1, 1e-5, True, mask_from_fp64=True)
    decided = oracle.exact_t(x, right['scale'], right['shift'])[0, :, 0, 0] > 0
    assert 4 <= int(decided.sum()) <= c - 4  # the fp32 coefficients say "positive" for some channels, "not" for others
    args = (100, wt, right['save_mean'], right['save_invstd'], right['scale'], right['shift'], True, False)
    oracle.judge_grads('fp32 mask', x, dy, right, *args)
    with pytest.raises(AssertionError):
        oracle.judge_grads('fp64 mask', x, dy, wrong, *args)


# ---- the lane mapping on the host

def test_host_build_of_the_lane_mapping_agrees_with_brute_force(tmp_path):
    """``csrc/bn_slabs.h`` compiled for the host only, with AddressSanitizer and UBSan on the host code, by
    ``tests/bn_slabs_host.cpp`` (a program of its own, nothing preloaded): every (pixel, vector) owned exactly once and the chain
    lengths, for all M <= 4096, V in 1 ... 256, C in {2056, 4096} and slab_pixels in {0, 1, 3, 64}, against brute force inside the
    program."""
    hipcc = build._hipcc()
    exe = str(tmp_path / 'bn_slabs_host')
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(ROOT, 'tests', 'bn_slabs_host.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r'ok \d+', run.stdout.strip()), run.stdout[-500:] + run.stderr[-2000:]
    assert int(run.stdout.split()[1]) >= 4096 * 258 * 6


# ---- host-side entry points

def test_bn_info_answers_without_a_gpu():
    info = cda.nn.batch_norm_info
    lib = _lib.load()
    for m, c in itertools.product((1, 2, 70, 2 * 33 * 70, 1 << 20, (1 << 31) - 1), (8, 24, 64, 2048, 2056, 4096)):
        for sp in (0, 1, 3, 64):
            if sp and -(-m // min(sp, m)) > (1 << 24) - 1:  # more slabs than one launch takes workgroups: refused, never launched
                with pytest.raises(RuntimeError, match=r'2\^24 - 1 slabs'):
                    info(m, c, sp)
                assert lib.cpn_bn_workspace_bytes(m, c, sp) == 0
                continue
            i = info(m, c, sp)
            v = c // 8
            assert i['slabs'] == -(-m // i['slab_pixels']) and i['channel_blocks'] == -(-v // 256)
            assert sp == 0 or i['slab_pixels'] == min(sp, m)
            assert sp != 0 or i['slab_pixels'] == m or i['slab_pixels'] >= 64
            assert i['rows'] == 256 // min(v, 256)
            chains = []
            for vb in {min(v, 256), v - (i['channel_blocks'] - 1) * 256}:
                r = 256 // vb
                chains.append(-(-i['slab_pixels'] // r) + min(r, i['slab_pixels']) + i['slabs'] + 6)
            assert i['chain'] == max(chains) <= m + i['slabs'] + 8
            assert lib.cpn_bn_workspace_bytes(m, c, sp) == i['slabs'] * c * 16
    assert info(1 << 20, 64)['slabs'] == 2048  # the auto partition: about eight workgroups per CU
    assert info((1 << 24) - 1, 8, 1)['slabs'] == (1 << 24) - 1  # the most slabs a forced slab_pixels may ask for
    assert info((1 << 31) - 1, 8)['slabs'] <= 2048


BAD = [((4, 12, 0), 'multiple of 8', _lib.E_INVALID), ((0, 8, 0), 'M must be', _lib.E_INVALID),
       ((1 << 31, 8, 0), '2^31 - 1', _lib.E_UNSUPPORTED), ((4, 8, -1), 'slab_pixels', _lib.E_INVALID),
       ((4, 0, 0), 'multiple of 8', _lib.E_INVALID), ((1 << 24, 8, 1), '2^24 - 1 slabs', _lib.E_UNSUPPORTED)]


def test_every_launch_refuses_bad_arguments_before_it_reads_a_pointer():
    """The pointers below are the address 1 (or a huge workspace size): a launch that read one would crash the test."""
    lib = _lib.load()
    out = (ctypes.c_int64 * 5)()
    p = 1
    for (m, c, sp), what, code in BAD:
        launches = {
            'cpn_bn_info': lambda: lib.cpn_bn_info(m, c, sp, out),
            'cpn_bn_train_stats': lambda: lib.cpn_bn_train_stats(p, 1, m, c, sp, p, 0, p, 0, p, p, 0, .1, 1e-5, p, p, p, p, p, 1 << 40, None),
            'cpn_bn_apply': lambda: lib.cpn_bn_apply(p, p, 1, m, c, sp, p, p, 1, None),
            'cpn_bn_backward_reduce': lambda: lib.cpn_bn_backward_reduce(p, p, 1, m, c, sp, p, p, 1, p, p, p, 0, p, 0, p, 0, p, p, 1 << 40,
                                                                         None),
            'cpn_bn_backward_input': lambda: lib.cpn_bn_backward_input(p, p, p, 1, m, c, sp, p, p, 1, p, p, p, None),
        }
        for name, call in launches.items():
            assert call() == code and what in lib.cpn_last_error().decode() and name in lib.cpn_last_error().decode(), \
                (name, (m, c, sp), lib.cpn_last_error())
        assert lib.cpn_bn_workspace_bytes(m, c, sp) == 0
    assert lib.cpn_bn_eval_coeffs(12, p, 0, p, 0, p, p, 0, 1e-5, p, p, p, p, None) == _lib.E_INVALID
    assert lib.cpn_bn_info(4, 8, 0, None) == _lib.E_INVALID
    # a short workspace
    need = lib.cpn_bn_workspace_bytes(70, 24, 3)
    assert need == 24 * 24 * 16
    assert lib.cpn_bn_train_stats(p, 1, 70, 24, 3, p, 0, p, 0, p, p, 0, .1, 1e-5, p, p, p, p, p, need - 1, None) == _lib.E_WORKSPACE
    assert 'workspace' in lib.cpn_last_error().decode()
    assert lib.cpn_bn_backward_reduce(p, p, 1, 70, 24, 3, p, p, 1, p, p, p, 0, p, 0, p, 0, p, p, need - 1, None) == _lib.E_WORKSPACE
    # dtypes, null pointers, the unbiased variance of a single value
    assert lib.cpn_bn_apply(p, p, 2, 4, 8, 0, p, p, 0, None) == _lib.E_INVALID
    assert lib.cpn_bn_apply(p, None, 1, 4, 8, 0, p, p, 0, None) == _lib.E_INVALID
    assert lib.cpn_bn_train_stats(p, 1, 1, 8, 0, p, 0, p, 0, p, p, 0, .1, 1e-5, p, p, p, p, p, 1 << 40, None) == _lib.E_INVALID
    assert lib.cpn_bn_backward_input(p, p, p, 1, 4, 8, 0, p, p, 0, p, p, None, None) == _lib.E_INVALID  # b without c
    # a tensor or workspace that does not start at a 16-byte aligned address (a = aligned, o = 8 bytes off; never read)
    a, o = 4096, 4096 + 8
    for x, ws in ((o, a), (a, o)):
        assert lib.cpn_bn_train_stats(x, 1, 70, 24, 3, a, 0, a, 0, a, a, 0, .1, 1e-5, a, a, a, a, ws, need, None) == _lib.E_INVALID
        assert '16-byte aligned' in lib.cpn_last_error().decode()
    for x, y in ((o, a), (a, o)):
        assert lib.cpn_bn_apply(x, y, 0, 70, 24, 3, a, a, 1, None) == _lib.E_INVALID
        assert '16-byte aligned' in lib.cpn_last_error().decode()
    for x, dy, ws in ((o, a, a), (a, o, a), (a, a, o)):
        assert lib.cpn_bn_backward_reduce(x, dy, 1, 70, 24, 3, a, a, 1, a, a, a, 0, a, 0, a, 0, a, ws, need, None) == _lib.E_INVALID
        assert '16-byte aligned' in lib.cpn_last_error().decode()
    for x, dy, dx in ((o, a, a), (a, o, a), (a, a, o)):
        assert lib.cpn_bn_backward_input(x, dy, dx, 1, 70, 24, 3, a, a, 1, a, a, a, None) == _lib.E_INVALID
        assert '16-byte aligned' in lib.cpn_last_error().decode()


def test_header_binding_and_exports_agree():
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    declared = set(re.findall(r'\b(cpn_bn_\w+)\s*\(', hdr))
    assert declared == set(NAMES) == {s for s in _lib.EXPORTED_SYMBOLS if s.startswith('cpn_bn_')}
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    flat_hdr = re.sub(r'\s*\n \*\s*', ' ', hdr)
    assert 'Trainable batch normalisation' in flat_hdr
    for phrase in ('t = fmaf(x, scale, shift)', 'dx = fmaf(a, g, fmaf(b, x, c))', 'No floating-point atomics', 'ascending slab order',
                   'var * M / (M - 1)', 'the gradient at t == 0 is 0', 'validates before it touches a pointer', '16-byte aligned address',
                   'more than 2^24 - 1 slabs'):
        assert phrase in flat_hdr, phrase
    assert build.SOURCES['batch_norm.hip'] == ['-ffp-contract=off'] and 'bn_slabs.h' in build.HEADERS
    assert {'batch_norm', 'batch_norm_forward', 'batch_norm_info', 'BatchNorm2d', 'convert_batchnorm2d_'} <= set(cda.nn.__all__)


def test_every_unsupported_argument_raises_naming_it():
    nn = cda.nn
    x = torch.zeros(2, 8, 3, 3)
    v = torch.ones(8)
    for args, kwargs, name in (((torch.zeros(2, 8, 3), None, None), {}, 'input of 3 dimensions'),
                               ((torch.zeros(2, 8, 3, 3, 3), None, None), {}, 'input of 5 dimensions'),
                               ((torch.zeros(2, 12, 3, 3), None, None), {}, 'num_features 12'),
                               ((x.half(), None, None), {}, 'input dtype'),
                               ((x.double(), None, None), {}, 'input dtype'),
                               ((x, None, None), dict(activation='gelu'), 'activation'),
                               ((x, None, None, v.double()), {}, 'weight'),
                               ((x, None, None, v, torch.ones(4)), {}, 'bias'),
                               ((x, v.double(), v.double()), {}, 'running_mean'),
                               ((x, v, None), {}, 'running_mean / running_var')):
        for fn in (nn.batch_norm, nn.batch_norm_forward):
            with pytest.raises(NotImplementedError, match=name):
                fn(*args, **kwargs)
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        nn.batch_norm(torch.zeros(1, 8, 1, 1), None, None, training=True)
    for fn in (nn.batch_norm, nn.batch_norm_forward):  # supported arguments on the CPU: the usual device error, no fallback
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x, v, v, v, v, True, 0.1, 1e-5, 'relu')
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.BatchNorm2d(8, activation='relu')(x)
    with pytest.raises(NotImplementedError, match='num_features'):
        nn.BatchNorm2d(12)
    with pytest.raises(NotImplementedError, match='activation'):
        nn.BatchNorm2d(8, activation='tanh')
    m = nn.BatchNorm2d(16, eps=1e-3, momentum=None, affine=False, track_running_stats=True, activation='relu')
    assert isinstance(m, torch.nn.BatchNorm2d) and m.weight is None and m.momentum is None and m.eps == 1e-3 and \
        list(m.state_dict()) == ['running_mean', 'running_var', 'num_batches_tracked'] and "activation='relu'" in repr(m)
    assert list(nn.BatchNorm2d(8).state_dict()) == list(torch.nn.BatchNorm2d(8).state_dict())


# ---- convert_batchnorm2d_

class _Net(torch.nn.Module):
    """The reference model's ReadOut.block and TwoConvNormRelu layouts, and everything the convert must leave alone."""

    def __init__(self):
        super().__init__()
        t = torch.nn
        self.block = t.Sequential(t.Conv2d(32, 32, 7, padding=3), t.BatchNorm2d(32), t.ReLU(), t.Dropout2d(.1), t.Conv2d(32, 2, 1))
        self.two = t.Sequential(t.Conv2d(32, 64, 3, padding=1), t.BatchNorm2d(64), t.ReLU(), t.Conv2d(64, 64, 3, padding=1),
                                t.BatchNorm2d(64), t.ReLU())
        shared = t.ReLU()
        self.twice = t.Sequential(t.Conv2d(32, 32, 3, padding=1), t.BatchNorm2d(32), shared, t.Conv2d(32, 32, 3, padding=1),
                                  t.BatchNorm2d(32, affine=False), shared)
        self.leaky = t.Sequential(t.BatchNorm2d(16), t.LeakyReLU())  # another activation: replaced, not fused
        self.lone = t.BatchNorm2d(8, track_running_stats=False)      # no Sequential parent: replaced, not fused
        self.lone_relu = t.ReLU()
        self.odd = t.Sequential(t.BatchNorm2d(12), t.ReLU())          # 12 channels: left
        again = t.Conv2d(8, 8, 1)                                     # the same conv before and after the norm: the slot behind
        self.between = t.Sequential(again, t.BatchNorm2d(8), again, t.ReLU())  # the norm holds the conv, not the ReLU: not fused
        both = t.BatchNorm2d(8)                                       # one norm in two slots: one replacement, not fused
        self.norm_twice = t.Sequential(both, t.ReLU(), t.Conv2d(8, 8, 1), both, t.ReLU())
        self.flat = t.BatchNorm1d(16)
        self.sync = t.SyncBatchNorm(16)


def test_convert_batchnorm2d_replaces_and_fuses_in_place():
    nn = cda.nn
    net = _Net()
    net.two.eval()
    hook = net.block[1].register_forward_hook(lambda *a: None)
    params = dict(net.named_parameters())
    buffers = dict(net.named_buffers())
    keys = list(net.state_dict().keys())
    replaced, fused, left = nn.convert_batchnorm2d_(net)
    assert replaced == ['lone', 'block.1', 'two.1', 'two.4', 'twice.1', 'twice.4', 'leaky.0', 'between.1', 'norm_twice.0',
                        'norm_twice.3']  # parents in named_modules order, slots in theirs
    assert fused == ['block.1', 'two.1', 'two.4']
    assert set(left) == {'odd.0', 'flat', 'sync'}
    assert 'num_features 12' in left['odd.0'] and 'BatchNorm1d' in left['flat'] and 'SyncBatchNorm' in left['sync']
    for name in replaced:
        m = net.get_submodule(name)
        assert type(m) is nn.BatchNorm2d and m.activation == ('relu' if name in fused else None), name
    for seq, i in ((net.block, 2), (net.two, 2), (net.two, 5)):
        assert type(seq[i]) is torch.nn.Identity
    assert type(net.twice[2]) is torch.nn.ReLU and net.twice[2] is net.twice[5] and type(net.odd[1]) is torch.nn.ReLU
    assert net.between[0] is net.between[2] and type(net.between[2]) is torch.nn.Conv2d and type(net.between[3]) is torch.nn.ReLU and \
        net.between[1].activation is None
    assert net.norm_twice[0] is net.norm_twice[3] and type(net.norm_twice[1]) is type(net.norm_twice[4]) is torch.nn.ReLU
    assert type(net.leaky[1]) is torch.nn.LeakyReLU and type(net.lone_relu) is torch.nn.ReLU
    assert type(net.odd[0]) is torch.nn.BatchNorm2d and type(net.flat) is torch.nn.BatchNorm1d and type(net.sync) is torch.nn.SyncBatchNorm
    # hooks, the training flag and the constructor attributes are kept
    assert net.block[1]._forward_hooks and net.block[1].training and not net.two[1].training and not net.two[4].training
    assert net.twice[4].weight is None and net.lone.running_mean is None and not net.lone.track_running_stats
    hook.remove()
    after_p, after_b = dict(net.named_parameters()), dict(net.named_buffers())
    assert after_p.keys() == params.keys() and all(after_p[k] is params[k] for k in params)  # the same Parameter objects
    assert after_b.keys() == buffers.keys() and all(after_b[k] is buffers[k] for k in buffers)  # ... and buffers
    assert list(net.state_dict().keys()) == keys
    fresh = _Net()
    fresh.load_state_dict(net.state_dict())  # state dicts interchange, both ways
    net.load_state_dict(fresh.state_dict())
    assert nn.convert_batchnorm2d_(net) == ([], [], left)  # a second call finds nothing to replace
    # without fusing: every ReLU stays
    plain = _Net()
    replaced2, fused2, left2 = nn.convert_batchnorm2d_(plain, fuse_relu=False)
    assert replaced2 == replaced and fused2 == [] and left2 == left and type(plain.block[2]) is torch.nn.ReLU and \
        plain.block[1].activation is None
    # convert_conv2d_ is untouched by all this and composes with it
    assert cda.nn.convert_conv2d_(net)[0] == ['block.0', 'two.0', 'two.3', 'twice.0', 'twice.3']  # (the 8-channel convs stay stock)
    lone = torch.nn.BatchNorm2d(8)
    assert nn.convert_batchnorm2d_(lone) == ([], [], {'': 'the root module cannot be replaced in place: convert its parent'})
