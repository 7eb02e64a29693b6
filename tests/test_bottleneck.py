"""CPU tests of the trainable bottleneck block (celldetection_amd/nn/blocks.py; csrc/batch_norm.hip,
csrc/grouped_conv_train.hip, csrc/grouped_conv.h): the fp64 statements of tests/bottleneck_oracle.py against torch's own autograd, the
wrong rules the cases tell apart, the judge of the GPU tests on a CPU emulation of the stated arithmetic (and on a wrong one), the
subsample's index arithmetic on the host under sanitizers, the host-side entry points, the Python surface and
``convert_bottleneck_``.  Nothing here needs a GPU."""
import itertools
import os
import re
import subprocess

import pytest
import torch

import celldetection_amd as cda
from celldetection_amd import _lib, build
import batch_norm_oracle as bo
import bottleneck_oracle as oracle
import conv_train_oracle
import grouped_conv_oracle
from test_grouped_conv import Bottleneck as LookAlike

nn = cda.nn
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('cpn_residual_bn_apply', 'cpn_residual_bn_backward_reduce', 'cpn_subsample2d')
CLOSE = dict(rtol=1e-12, atol=1e-12)


def _operands(n, c, h, w, seed=0, affine=True):
    g = torch.Generator().manual_seed(seed + 100 * c + 10 * h + w)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) + torch.randn(1, c, 1, 1, generator=g, dtype=torch.float64)
    r = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 1.5
    dy = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(c, generator=g, dtype=torch.float64) if affine else None
    b = torch.randn(c, generator=g, dtype=torch.float64) if affine else None
    rm = torch.randn(c, generator=g, dtype=torch.float64)
    rv = torch.rand(c, generator=g, dtype=torch.float64) + .5
    return x, r, dy, wt, b, rm, rv


# (n, c, h, w): M = 2 (the smallest batch torch trains on), non-square images, N = 3
TAIL_SHAPES = [(2, 8, 1, 1), (1, 8, 1, 2), (2, 16, 5, 7), (3, 8, 4, 3)]


@pytest.mark.parametrize('shape', TAIL_SHAPES, ids=str)
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('affine', [True, False], ids=['affine', 'plain'])
def test_tail_statement_equals_torch_autograd(shape, training, affine):
    x, r, dy, wt, b, rm, rv = _operands(*shape, affine=affine)
    for relu in (True, False):
        y, dx, dr, dg, db = oracle.tail_autograd64(x, r, dy, wt, b, rm, rv, training, 1e-5, relu)
        o = oracle.tail(x, r, dy, wt, b, rm, rv, training, 1e-5, relu)
        torch.testing.assert_close(o['y'], y, **CLOSE)
        torch.testing.assert_close(o['dx'], dx, **CLOSE)
        torch.testing.assert_close(o['dr'], dr, **CLOSE)
        if affine:
            torch.testing.assert_close(o['dgamma'], dg, **CLOSE)
            torch.testing.assert_close(o['dbeta'], db, **CLOSE)
        # the same through the batch norm's own backward statement on g: what the GPU judge uses
        back = bo.backward(x, o['g'], wt, o['mean'], o['invstd'], None, training)
        torch.testing.assert_close(back['dx'], dx, **CLOSE)


# (n, cin, cout, h, w): even and odd sizes down to 1 x 1 and 1 x 2
STRIDED_CASES = [(2, 4, 6, 1, 1), (2, 4, 6, 1, 2), (1, 3, 5, 2, 1), (2, 4, 6, 5, 7), (2, 4, 6, 6, 8), (1, 8, 4, 9, 11), (3, 4, 4, 6, 9)]


def _conv_operands(n, cin, cout, h, w, k=1, stride=2):
    g = torch.Generator().manual_seed(n + 3 * cin + 5 * cout + 7 * h + 11 * w + k)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    ho, wo = (oracle.out_size(h), oracle.out_size(w)) if stride == 2 else (h, w)
    dy = torch.randn(n, cout, ho, wo, generator=g, dtype=torch.float64)
    return x, wt, b, dy


@pytest.mark.parametrize('case', STRIDED_CASES, ids=str)
def test_strided_conv_statement_equals_torch_autograd(case):
    x, wt, b, dy = _conv_operands(*case)
    ref = oracle.strided_autograd64(x, wt, b, dy)
    o = oracle.strided(x, wt, b, dy)
    for key in ('y', 'dx', 'dw', 'db'):
        torch.testing.assert_close(o[key], ref[key], **CLOSE)
    assert o['y'].shape[2:] == (oracle.out_size(case[3]), oracle.out_size(case[4]))
    # dW(x, dy) = dW_dense(sub(x), dy) and dx = dilate(dgrad(dy)), with the dense weight gradient and the dilation already tested
    torch.testing.assert_close(conv_train_oracle.wgrad(oracle.sub(x), dy, 1)[0], ref['dw'], **CLOSE)
    torch.testing.assert_close(grouped_conv_oracle.dilate(oracle.dgrad1x1(dy, wt), x.shape[2:]), ref['dx'], **CLOSE)
    torch.testing.assert_close(torch.nn.functional.conv_transpose2d(dy, wt), oracle.dgrad1x1(dy, wt), **CLOSE)
    off_grid = ref['dx'].clone()
    off_grid[..., ::2, ::2] = 0
    assert bool((off_grid == 0).all())


@pytest.mark.parametrize('k', [1, 3])
def test_fork_statement_equals_torch_autograd(k):
    x, wt, _, dy = _conv_operands(2, 4, 6, 5, 7, k, stride=1)
    dskip = torch.randn(x.shape, generator=torch.Generator().manual_seed(k), dtype=torch.float64)
    torch.testing.assert_close(oracle.fork_dx(dy, wt, dskip), oracle.fork_autograd64(x, wt, dy, dskip), **CLOSE)
    torch.testing.assert_close(oracle.fork_dx(dy, wt, None), oracle.fork_autograd64(x, wt, dy, None), **CLOSE)


def _differs(got, ref):
    return got.shape != ref.shape or float((got - ref).abs().max()) > .1 * float(ref.abs().mean())


def test_wrong_rules_are_told_apart():
    """Each wrong rule moves some result of a case by at least a tenth of that result's mean magnitude (or changes its shape), and
    the statement itself equals torch's autograd on every one of these cases."""
    told = set()
    for shape in [(2, 8, 1, 1), (2, 16, 5, 7)]:
        for training in (True, False):
            x, r, dy, wt, b, rm, rv = _operands(*shape)
            b = torch.zeros_like(b)
            ref = oracle.tail_autograd64(x, r, dy, wt, b, rm, rv, training, 1e-5, True)
            right = oracle.tail(x, r, dy, wt, b, rm, rv, training, 1e-5, True)
            for key, want in zip(('y', 'dx', 'dr', 'dgamma', 'dbeta'), ref):
                torch.testing.assert_close(right[key], want, **CLOSE)
            # eval: t is exactly beta = 0 here and its sum with r exactly 0: the mask's edge.  (torch's own (x - mean) * invstd * w
            # is a few 1e-17 off zero there, so the statement is held against it on the operands above, before this pixel is set.)
            x[0, :, 0, 0], r[0, :, 0, 0], dy[0, :, 0, 0] = rm, 0., 3.
            right = oracle.tail(x, r, dy, wt, b, rm, rv, training, 1e-5, True)
            if not training:
                assert bool((right['s'][0, :, 0, 0] == 0).all()) and bool((right['dr'][0, :, 0, 0] == 0).all())
            for rule in oracle.TAIL_WRONG_RULES:
                wrong = oracle.tail(x, r, dy, wt, b, rm, rv, training, 1e-5, True, rule)
                keys = [k for k in ('y', 'dx', 'dr', 'dgamma', 'dbeta') if _differs(wrong[k], right[k])]
                if rule == 'mask_includes_zero':  # seen only where the sum is exactly zero: the designed pixel in eval mode
                    assert (keys != []) == (not training), (rule, shape, training)
                elif rule == 'residual_after_relu':
                    assert 'y' in keys, (rule, shape, training)
                elif rule in ('dr_unmasked', 'dr_times_a'):
                    assert 'dr' in keys, (rule, shape, training)
                elif rule == 'sum_g_unmasked':
                    assert 'dbeta' in keys, (rule, shape, training)
                if keys:
                    told.add(rule)
    assert {'mask_without_residual'} <= told  # (t > 0 and t + r > 0 differ on about a third of random elements)
    for case in [(2, 4, 6, 6, 8), (2, 4, 6, 4, 2)]:  # even sizes: both grids hold as many pixels
        x, wt, b, dy = _conv_operands(*case)
        ref = oracle.strided_autograd64(x, wt, b, dy)
        right = oracle.strided(x, wt, b, dy)
        assert not any(_differs(right[k], ref[k]) for k in ref)
        wrong = oracle.strided(x, wt, b, dy, 'subsample_odd_grid')
        assert _differs(wrong['y'], ref['y']) and _differs(wrong['dw'], ref['dw']) and not _differs(wrong['dx'], ref['dx'])
        wrong = oracle.strided(x, wt, b, dy, 'dilate_odd_grid')
        assert _differs(wrong['dx'], ref['dx']) and not _differs(wrong['y'], ref['y'])
        told.update(('subsample_odd_grid', 'dilate_odd_grid'))
    for k in (1, 3):
        x, wt, _, dy = _conv_operands(2, 4, 6, 5, 7, k, stride=1)
        dskip = torch.randn(x.shape, generator=torch.Generator().manual_seed(k), dtype=torch.float64)
        ref = oracle.fork_autograd64(x, wt, dy, dskip)
        assert not _differs(oracle.fork_dx(dy, wt, dskip), ref)
        for rule in ('skip_dropped', 'skip_twice'):
            assert _differs(oracle.fork_dx(dy, wt, dskip, rule), ref), rule
            told.add(rule)
    assert told == set(oracle.TAIL_WRONG_RULES) | set(oracle.CONV_WRONG_RULES)


# ---- the judge of the GPU tests, on the CPU

def _typed(shape, dtype, seed=0):
    x, r, dy, wt, b, rm, rv = _operands(*shape, seed=seed)
    return x.to(dtype), r.to(dtype), dy.to(dtype), wt.float(), b.float(), rm.float(), rv.float()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('relu', [False, True], ids=['none', 'relu'])
def test_judge_accepts_the_stated_arithmetic(dtype, training, relu):
    for shape in [(2, 8, 1, 1), (2, 24, 5, 7), (2, 8, 17, 33)]:
        x, r, dy, wt, b, rm, rv = _typed(shape, dtype)
        m = x.numel() // shape[1]
        chain = nn.batch_norm_info(m, shape[1])['chain']
        stats = bo.emulate(x, dy, wt, b, rm, rv, training, 0.1, 1e-5, False)  # the statistics pass is the batch norm's own
        y = oracle.emulate_tail(x, r, stats['scale'], stats['shift'], relu)
        assert y.dtype == dtype
        oracle.judge_tail_y(f'{shape}', x, r, y, stats['scale'], stats['shift'], relu)
        g = oracle.masked(dy, y, relu)
        back = bo.emulate(x, g, wt, b, rm, rv, training, 0.1, 1e-5, False)  # the sums and the input kernel on g, relu = 0
        got = dict(dr=g, dx=back['dx'], dgamma=back['dgamma'], dbeta=back['dbeta'])
        oracle.judge_tail_grads(f'{shape}', x, dy, y, got, chain, wt, stats['save_mean'], stats['save_invstd'], relu, training)
        with pytest.raises(AssertionError, match='bit for bit'):  # ... and an unmasked dr is refused
            oracle.judge_tail_grads(f'{shape}', x, dy, y, dict(dr=dy if relu else dy * 2), chain, wt, stats['save_mean'],
                                    stats['save_invstd'], relu, training)


@pytest.mark.parametrize('relu', [False, True], ids=['none', 'relu'])
def test_judge_rejects_t_rounded_to_bf16_before_the_add(relu):
    """scale = 1 + 2^-9, shift = 0, x = 1: t = 1 + 2^-9 is an fp32 value and no bf16 value (bf16 steps by 2^-7 there).  With r = -1
    the stated arithmetic returns 2^-9 exactly; a tail that rounds t to bf16 first returns 0: 2^-9 against a bound of 2^-23."""
    c = 8
    x = torch.ones(2, c, 3, 5, dtype=torch.bfloat16)
    r = -torch.ones(2, c, 3, 5, dtype=torch.bfloat16)
    scale, shift = torch.full((c,), 1. + 2. ** -9), torch.zeros(c)
    right = oracle.emulate_tail(x, r, scale, shift, relu)
    assert bool((right.float() == 2. ** -9).all())
    oracle.judge_tail_y('as stated', x, r, right, scale, shift, relu)
    wrong = oracle.emulate_tail(x, r, scale, shift, relu, round_t=True)
    assert bool((wrong.float() == 0).all())
    with pytest.raises(AssertionError):
        oracle.judge_tail_y('t rounded first', x, r, wrong, scale, shift, relu)
    # on random operands too: the rounding of t is 2^-9 of it, the bound 2^-23
    x, r, dy, wt, b, rm, rv = _typed((2, 24, 5, 7), torch.bfloat16)
    stats = bo.emulate(x, dy, wt, b, rm, rv, True, 0.1, 1e-5, False)
    oracle.judge_tail_y('as stated', x, r, oracle.emulate_tail(x, r, stats['scale'], stats['shift'], relu), stats['scale'], stats['shift'], relu)
    with pytest.raises(AssertionError):
        oracle.judge_tail_y('t rounded first', x, r, oracle.emulate_tail(x, r, stats['scale'], stats['shift'], relu, round_t=True),
                            stats['scale'], stats['shift'], relu)


def test_judge_rejects_one_bf16_step_and_a_non_zero_below_zero():
    x, r, dy, wt, b, rm, rv = _typed((2, 8, 5, 7), torch.bfloat16)
    stats = bo.emulate(x, dy, wt, b, rm, rv, True, 0.1, 1e-5, False)
    y = oracle.emulate_tail(x, r, stats['scale'], stats['shift'], True)
    up = y.clone()
    up.view(torch.int16).view(-1)[int(torch.argmax(y.float().reshape(-1)))] += 1
    with pytest.raises(AssertionError):
        oracle.judge_tail_y('one step', x, r, up, stats['scale'], stats['shift'], True)
    t, d = oracle.tail_noise(x, r, stats['scale'], stats['shift'])
    below = y.clone()
    below.view(-1)[int(torch.argmin(t.reshape(-1)))] = 2. ** -100
    with pytest.raises(AssertionError, match='non-zero output'):
        oracle.judge_tail_y('below zero', x, r, below, stats['scale'], stats['shift'], True)


# ---- the subsample's index arithmetic on the host

def test_host_build_of_the_subsample_agrees_with_brute_force(tmp_path):
    """``gc_subsample_source`` of ``csrc/grouped_conv.h`` compiled for the host only, with AddressSanitizer and UBSan on the host
    code, by ``tests/subsample_host.cpp`` (a program of its own, nothing preloaded)."""
    hipcc = build._hipcc()
    exe = str(tmp_path / 'subsample_host')
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(ROOT, 'tests', 'subsample_host.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r'ok \d+', run.stdout.strip()), run.stdout[-500:] + run.stderr[-2000:]
    assert int(run.stdout.split()[1]) >= 10000


# ---- host-side entry points

def test_every_new_launch_refuses_bad_arguments_before_it_reads_a_pointer():
    """The pointers below are the address 1, 4096 or 4104 (or a huge workspace size): a launch that read one would crash the test."""
    lib = _lib.load()
    p = 1
    bad = [((4, 12, 0), 'multiple of 8', _lib.E_INVALID), ((0, 8, 0), 'M must be', _lib.E_INVALID),
           ((1 << 31, 8, 0), '2^31 - 1', _lib.E_UNSUPPORTED), ((4, 8, -1), 'slab_pixels', _lib.E_INVALID),
           ((4, 0, 0), 'multiple of 8', _lib.E_INVALID), ((1 << 24, 8, 1), '2^24 - 1 slabs', _lib.E_UNSUPPORTED)]
    for (m, c, sp), what, code in bad:
        launches = {
            'cpn_residual_bn_apply': lambda: lib.cpn_residual_bn_apply(p, p, p, 1, m, c, sp, p, p, 1, None),
            'cpn_residual_bn_backward_reduce': lambda: lib.cpn_residual_bn_backward_reduce(p, p, p, p, 1, m, c, sp, p, p, 1, p, p, p, 0, p,
                                                                                           0, p, 0, p, p, 1 << 40, None),
        }
        for name, call in launches.items():
            assert call() == code and what in lib.cpn_last_error().decode() and name in lib.cpn_last_error().decode(), \
                (name, (m, c, sp), lib.cpn_last_error())
    a, o = 4096, 4096 + 8
    # NULLs and dtypes
    for args in ((None, a, a), (a, None, a), (a, a, None)):
        assert lib.cpn_residual_bn_apply(*args, 1, 70, 24, 3, a, a, 1, None) == _lib.E_INVALID
        assert 'null pointer' in lib.cpn_last_error().decode()
    assert lib.cpn_residual_bn_apply(a, a, a, 1, 70, 24, 3, None, a, 1, None) == _lib.E_INVALID
    assert lib.cpn_residual_bn_apply(a, a, a, 2, 70, 24, 3, a, a, 1, None) == _lib.E_INVALID
    need = lib.cpn_bn_workspace_bytes(70, 24, 3)

    def reduce(x=a, dy=a, y=a, g=a, ws=a, nbytes=need, dtype=1, relu=1, mean=a):
        return lib.cpn_residual_bn_backward_reduce(x, dy, y, g, dtype, 70, 24, 3, None, None, relu, mean, a, a, 0, a, 0, a, 0, a, ws,
                                                   nbytes, None)

    for kw in (dict(x=None), dict(dy=None), dict(y=None), dict(g=None), dict(ws=None), dict(mean=None)):
        assert reduce(**kw) == _lib.E_INVALID and 'null pointer' in lib.cpn_last_error().decode(), kw
    assert reduce(dtype=3) == _lib.E_INVALID
    assert reduce(nbytes=need - 1) == _lib.E_WORKSPACE and 'workspace' in lib.cpn_last_error().decode()
    assert reduce(nbytes=need - 1, relu=0, y=None, g=None) == _lib.E_WORKSPACE  # without ReLU: the batch norm's own call and checks
    # misaligned addresses (never read)
    for args in ((o, a, a), (a, o, a), (a, a, o)):
        assert lib.cpn_residual_bn_apply(*args, 0, 70, 24, 3, a, a, 1, None) == _lib.E_INVALID
        assert '16-byte aligned' in lib.cpn_last_error().decode()
    for kw in (dict(x=o), dict(dy=o), dict(y=o), dict(g=o), dict(ws=o)):
        assert reduce(**kw) == _lib.E_INVALID and '16-byte aligned' in lib.cpn_last_error().decode(), kw
    # the subsample: sizes, channels, stride, limits, NULLs, alignment
    sub = lib.cpn_subsample2d
    for args, what, code in (((a, 0, 5, 7, 8, 2, a), 'at least 1', _lib.E_INVALID), ((a, 2, 0, 7, 8, 2, a), 'at least 1', _lib.E_INVALID),
                             ((a, 2, 5, -1, 8, 2, a), 'at least 1', _lib.E_INVALID), ((a, 2, 5, 7, 12, 2, a), 'multiple of 8', _lib.E_INVALID),
                             ((a, 2, 5, 7, 0, 2, a), 'multiple of 8', _lib.E_INVALID), ((a, 2, 5, 7, 8, 1, a), 'stride', _lib.E_INVALID),
                             ((a, 2, 5, 7, 8, 3, a), 'stride', _lib.E_INVALID),
                             ((p, 1 << 15, 1 << 15, 4, 8, 2, p), '2^31 - 1 pixels', _lib.E_UNSUPPORTED),
                             ((p, 1, 1 << 13, 1 << 13, 16, 2, p), '2^30', _lib.E_UNSUPPORTED),
                             ((None, 2, 5, 7, 8, 2, a), 'null pointer', _lib.E_INVALID), ((a, 2, 5, 7, 8, 2, None), 'null pointer', _lib.E_INVALID),
                             ((o, 2, 5, 7, 8, 2, a), '16-byte aligned', _lib.E_INVALID), ((a, 2, 5, 7, 8, 2, o), '16-byte aligned', _lib.E_INVALID)):
        assert sub(*args, None) == code and what in lib.cpn_last_error().decode() and 'cpn_subsample2d' in lib.cpn_last_error().decode(), \
            (args, lib.cpn_last_error())


def test_header_binding_and_exports_agree():
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    flat_hdr = re.sub(r'\s*\n \*\s*', ' ', hdr)
    section = flat_hdr[flat_hdr.index('Trainable bottleneck block'):]
    for phrase in ('Additions to ABI 22', 's = t + r, an fp32 add', 'two roundings in fp32', 'g = dy where y > 0', 'g IS the residual',
                   'Three passes over the tensor', '4 + 3 = 7', 'xs[n][i][j] = x[n][stride i][stride j]', 'every unit of xs written once',
                   'validates before it touches a pointer', 'res = dskip, res_stride = cin', 'one rounding'):
        assert phrase in section, phrase
    assert 'grouped_conv.h' in build.HEADERS and 'bn_slabs.h' in build.HEADERS
    assert {'conv2d_fork', 'strided_conv1x1', 'StridedConv1x1', 'subsample2d', 'Bottleneck', 'convert_bottleneck_'} <= set(nn.__all__)
    assert all(hasattr(nn, name) for name in nn.__all__)
    import inspect
    for fn in (nn.batch_norm, nn.batch_norm_forward):
        assert inspect.signature(fn).parameters['residual'].default is None
    assert list(inspect.signature(nn.BatchNorm2d.forward).parameters)[:3] == ['self', 'x', 'residual']
    assert inspect.signature(nn.Conv2d.forward).parameters['fork'].default is False
    doc = nn.__doc__
    assert 'the strided 1x1 shortcuts and the residual add of the encoder' not in doc and 'convert_bottleneck_' in doc


def test_every_unsupported_argument_raises_naming_it():
    x = torch.zeros(2, 8, 3, 3)
    for residual, name in ((torch.zeros(2, 8, 3, 4), 'residual of shape'), (torch.zeros(2, 8, 3, 3).half(), 'residual dtype'),
                           (torch.zeros(2, 8, 3), 'residual of shape'), (1., 'residual of shape')):
        for fn in (nn.batch_norm, nn.batch_norm_forward):
            with pytest.raises(NotImplementedError, match=name):
                fn(x, None, None, residual=residual)
    with pytest.raises(NotImplementedError, match='activation'):
        nn.BatchNorm2d(8)(x, residual=x, activation='gelu')
    for fn in (nn.batch_norm, nn.batch_norm_forward):  # supported arguments on the CPU: the usual device error, no fallback
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x, None, None, training=True, activation='relu', residual=x)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.BatchNorm2d(8)(x, residual=x, activation='relu')
    w = torch.zeros(64, 32, 1, 1)
    x32 = torch.zeros(2, 32, 5, 7)
    for args, kwargs, name in (((x32, torch.zeros(64, 32, 3, 3)), {}, 'kernel_size 3'), ((x32, w), dict(stride=1), 'stride 1'),
                               ((x32, w), dict(stride=(2, 1)), 'stride'), ((x32, torch.zeros(64, 48, 1, 1)), {}, 'in_channels 48'),
                               ((x32, torch.zeros(40, 32, 1, 1)), {}, 'out_channels 40'), ((x32[0], w), {}, 'input of 3 dimensions'),
                               ((x32.half(), w), {}, 'input dtype'), ((x32, w.double()), {}, 'weight dtype'),
                               ((x32, w, torch.zeros(32)), {}, 'bias')):
        with pytest.raises(NotImplementedError, match=name):
            nn.strided_conv1x1(*args, **kwargs)
    with pytest.raises(ValueError, match='channels'):
        nn.strided_conv1x1(torch.zeros(2, 64, 5, 7), w)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.strided_conv1x1(x32, w)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.conv2d_fork(x32, torch.zeros(64, 32, 3, 3))
    with pytest.raises(NotImplementedError, match='in_channels 48'):
        nn.conv2d_fork(torch.zeros(2, 48, 5, 7), torch.zeros(64, 48, 3, 3))
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.Conv2d(32, 64, 1)(x32, fork=True)
    for x_, name in ((torch.zeros(2, 12, 5, 7), '12 channels'), (torch.zeros(8, 5, 7), 'input of 3 dimensions')):
        with pytest.raises(NotImplementedError, match=name):
            nn.subsample2d(x_)
    with pytest.raises(NotImplementedError, match='stride 3'):
        nn.subsample2d(torch.zeros(2, 8, 5, 7), 3)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.subsample2d(torch.zeros(2, 8, 5, 7))
    for kwargs, name in ((dict(kernel_size=3), 'kernel_size'), (dict(stride=1), 'stride'), (dict(groups=2), 'groups'),
                         (dict(dilation=2), 'dilation'), (dict(padding=1), 'padding'), (dict(padding_mode='reflect'), 'padding_mode'),
                         (dict(in_channels=48), 'in_channels'), (dict(out_channels=40), 'out_channels')):
        kw = dict(in_channels=32, out_channels=64)
        kw.update(kwargs)
        with pytest.raises(NotImplementedError, match=name):
            nn.StridedConv1x1(**kw)
    m = nn.StridedConv1x1(32, 64, bias=False)
    stock = torch.nn.Conv2d(32, 64, 1, 2, bias=False)
    assert isinstance(m, torch.nn.Conv2d) and list(m.state_dict()) == list(stock.state_dict()) and m.stride == (2, 2)
    m.load_state_dict(stock.state_dict())
    stock.load_state_dict(m.state_dict())


# ---- convert_bottleneck_

def _tv_forward(self, x):
    identity = x
    out = self.relu(self.bn1(self.conv1(x)))
    out = self.relu(self.bn2(self.conv2(out)))
    out = self.bn3(self.conv3(out))
    if self.downsample is not None:
        identity = self.downsample(x)
    out += identity
    return self.relu(out)


# what marks torchvision's function (torchvision itself is not needed, and not imported, by the library)
_tv_forward.__module__, _tv_forward.__qualname__ = 'torchvision.models.resnet', 'Bottleneck.forward'


class Block(torch.nn.Module):
    """A bottleneck block that assigns torchvision's ``Bottleneck.forward`` (here: a function that carries its names)."""

    def __init__(self, inplanes=64, width=128, groups=32, stride=1, out=256, downsample='conv', dilation=1):
        super().__init__()
        t = torch.nn
        self.conv1 = t.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = t.BatchNorm2d(width)
        self.conv2 = t.Conv2d(width, width, 3, stride, dilation, dilation, groups, bias=False)
        self.bn2 = t.BatchNorm2d(width)
        self.conv3 = t.Conv2d(width, out, 1, bias=False)
        self.bn3 = t.BatchNorm2d(out)
        self.relu = t.ReLU(inplace=True)
        self.stride = stride
        if downsample == 'conv':
            self.downsample = t.Sequential(t.Conv2d(inplanes, out, 1, stride, bias=False), t.BatchNorm2d(out))
        elif downsample == 'avg':
            self.downsample = t.Sequential(t.AvgPool2d(2, stride, ceil_mode=True, count_include_pad=False),
                                           t.Conv2d(inplanes, out, 1, bias=False), t.BatchNorm2d(out))
        else:
            self.downsample = None

    forward = _tv_forward


class SameNames(Block):
    """The same attribute names, a forward of its own: not torchvision's block."""

    def forward(self, x):
        return _tv_forward(self, x) * 2


def _signature(net):
    return [(name, type(m)) for name, m in net.named_modules()]


def _net():
    return torch.nn.Sequential(Block(64, 128, 32, 2, 256), Block(256, 128, 32, 1, 256, None), Block(256, 64, 1, 1, 256, 'conv'))


def _expect_converted(net):
    b0, b1, b2 = net
    assert type(b0) is type(b1) is type(b2) is nn.Bottleneck
    for b in net:
        assert type(b.conv1) is type(b.conv3) is nn.Conv2d and type(b.bn1) is type(b.bn2) is type(b.bn3) is nn.BatchNorm2d
        assert type(b.relu) is torch.nn.ReLU and b.bn1.activation is b.bn2.activation is b.bn3.activation is None
    assert type(b0.conv2) is type(b1.conv2) is nn.GroupedConv2d and type(b2.conv2) is nn.Conv2d
    assert b0.conv2.stride == (2, 2) and b0.stride == 2 and b1.downsample is None
    assert type(b0.downsample) is torch.nn.Sequential and type(b0.downsample[0]) is nn.StridedConv1x1 and \
        type(b0.downsample[1]) is nn.BatchNorm2d and type(b2.downsample[0]) is nn.Conv2d and type(b2.downsample[1]) is nn.BatchNorm2d


def test_convert_bottleneck_on_torchvision_style_blocks():
    """with and without downsample, stride 1 and 2, groups 32 and 1"""
    net = _net()
    net[1].eval()
    hook = net[0].register_forward_hook(lambda *a: None)
    child_hook = net[0].conv1.register_forward_hook(lambda *a: None)
    params, buffers, keys = dict(net.named_parameters()), dict(net.named_buffers()), list(net.state_dict().keys())
    down = net[0].downsample
    replaced, left = nn.convert_bottleneck_(net)
    assert (replaced, left) == (['0', '1', '2'], {})
    _expect_converted(net)
    assert net[0].downsample is down and net[0]._forward_hooks and net[0].conv1._forward_hooks
    assert net[0].training and not net[1].training and not net[1].bn2.training and net[0].bn1.training
    after_p, after_b = dict(net.named_parameters()), dict(net.named_buffers())
    assert after_p.keys() == params.keys() and all(after_p[k] is params[k] for k in params)  # the same Parameter objects
    assert after_b.keys() == buffers.keys() and all(after_b[k] is buffers[k] for k in buffers)  # ... and buffers
    assert list(net.state_dict().keys()) == keys
    fresh = _net()
    fresh.load_state_dict(net.state_dict())  # state dicts interchange, both ways
    net.load_state_dict(fresh.state_dict())
    assert nn.convert_bottleneck_(net) == ([], {})  # a second call finds nothing
    # the four other converts leave a converted block alone and report nothing about it
    assert nn.convert_conv2d_(net) == ([], {}) and nn.convert_batchnorm2d_(net) == ([], [], {})
    assert nn.convert_readout_tail_(net) == ([], {}) and nn.convert_grouped_conv2d_(net) == ([], {})
    _expect_converted(net)
    hook.remove()
    child_hook.remove()
    with pytest.raises(RuntimeError, match='MI355X'):  # no GPU here: the block runs this library's ops, nothing else
        net[2](torch.zeros(2, 256, 4, 4))


_CONVERTS = dict(conv=nn.convert_conv2d_, bn=nn.convert_batchnorm2d_, tail=nn.convert_readout_tail_, grouped=nn.convert_grouped_conv2d_,
                 block=nn.convert_bottleneck_)


def test_convert_bottleneck_with_the_four_other_converts_in_all_120_orders():
    reference = _net()
    nn.convert_bottleneck_(reference)
    want = _signature(reference)
    orders = list(itertools.permutations(_CONVERTS))
    assert len(orders) == 120
    for order in orders:
        net = _net()
        params, buffers, keys = dict(net.named_parameters()), dict(net.named_buffers()), list(net.state_dict().keys())
        results = {name: _CONVERTS[name](net) for name in order}
        assert results['block'] == (['0', '1', '2'], {}), order
        assert _signature(net) == want, order
        _expect_converted(net)
        after_p, after_b = dict(net.named_parameters()), dict(net.named_buffers())
        assert after_p.keys() == params.keys() and all(after_p[k] is params[k] for k in params), order
        assert after_b.keys() == buffers.keys() and all(after_b[k] is buffers[k] for k in buffers), order
        assert list(net.state_dict().keys()) == keys, order
        for name in order[order.index('block') + 1:]:  # whatever runs after it reports nothing
            assert all(not part for part in results[name]), (order, name, results[name])


def test_convert_bottleneck_leaves_everything_else_with_a_reason_naming_the_attribute():
    t = torch.nn
    twice = Block(256, 128, 32, 1, 256, None)
    leaky = Block(256, 128, 32, 1, 256, None)
    leaky.relu = t.LeakyReLU()
    group_norm = Block(256, 128, 32, 1, 256, None)
    group_norm.bn3 = t.GroupNorm(8, 256)
    no_attr = Block(256, 128, 32, 1, 256, None)
    del no_attr.bn2
    padded = Block(64, 128, 32, 1, 256)
    padded.downsample[0] = t.Conv2d(64, 256, 1, 1, 1, bias=False)
    identity_strided = Block(256, 128, 32, 2, 256, None)
    net = t.ModuleDict(dict(
        avg=Block(64, 128, 32, 2, 256, 'avg'), dilated=Block(256, 128, 32, 1, 256, None, dilation=2),
        dense_strided=Block(64, 64, 1, 2, 256), narrow=Block(64, 48, 1, 1, 256), odd_out=Block(64, 128, 32, 1, 200),
        a=twice, b=twice, leaky=leaky, group_norm=group_norm, no_attr=no_attr, padded=padded, identity_strided=identity_strided,
        same_names=SameNames(), look_alike=LookAlike(), fine=Block(64, 128, 32, 2, 256)))
    before = _signature(net)
    replaced, left = nn.convert_bottleneck_(net)
    assert replaced == ['fine']
    assert set(left) == {'avg', 'dilated', 'dense_strided', 'narrow', 'odd_out', 'a', 'b', 'leaky', 'group_norm', 'no_attr', 'padded',
                         'identity_strided'}  # the two classes with forwards of their own are not candidates: not even named
    for name, words in (('avg', ('downsample', 'AvgPool2d')), ('dilated', ('conv2', 'dilation')), ('dense_strided', ('conv2', 'stride')),
                        ('narrow', ('conv1', 'out_channels 48')), ('odd_out', ('conv3', 'out_channels 200')), ('a', ('2 slots',)),
                        ('b', ('2 slots',)), ('leaky', ('relu', 'LeakyReLU')), ('group_norm', ('bn3', 'GroupNorm')),
                        ('no_attr', ('bn2', 'no such attribute')), ('padded', ('downsample.0', 'padding')),
                        ('identity_strided', ('downsample', 'stride'))):
        assert all(w in left[name] for w in words), (name, left[name])
    after = _signature(net)
    assert [s for s in after if not s[0].startswith('fine')] == [s for s in before if not s[0].startswith('fine')]  # all stock still
    assert type(net['same_names']) is SameNames and type(net['look_alike']) is LookAlike and type(net['look_alike'].conv1) is t.Conv2d
    assert type(net['fine']) is nn.Bottleneck
    # a listed class is converted; an unlisted look-alike stays
    net2 = t.Sequential(LookAlike(64, 128, 32, 2, 256), SameNames())
    assert nn.convert_bottleneck_(net2) == ([], {})
    assert nn.convert_bottleneck_(net2, block_types=(LookAlike,)) == (['0'], {})
    assert type(net2[0]) is nn.Bottleneck and type(net2[0].downsample[0]) is nn.StridedConv1x1 and type(net2[1]) is SameNames
    # the root module is not replaced: reported as left, like the other converts do
    assert nn.convert_bottleneck_(Block()) == ([], {'': 'the root module cannot be replaced in place: convert its parent'})
    assert 'downsample' in nn.convert_bottleneck_(Block(64, 128, 32, 2, 256, 'avg'))[1]['']
    assert nn.convert_bottleneck_(t.Conv2d(32, 32, 1)) == ([], {})


def test_bottleneck_constructor_takes_this_librarys_modules_only():
    def parts(stride=1, cin=64, width=64, out=256):
        return [nn.Conv2d(cin, width, 1, bias=False), nn.BatchNorm2d(width),
                nn.GroupedConv2d(width, width, stride=stride, groups=16, bias=False), nn.BatchNorm2d(width),
                nn.Conv2d(width, out, 1, bias=False), nn.BatchNorm2d(out)]

    block = nn.Bottleneck(*parts(2), downsample=torch.nn.Sequential(nn.StridedConv1x1(64, 256, bias=False), nn.BatchNorm2d(256)))
    stock = Block(64, 64, 16, 2, 256)
    assert list(block.state_dict()) == list(stock.state_dict())
    block.load_state_dict(stock.state_dict())
    assert [n for n, _ in block.named_children()] == ['conv1', 'bn1', 'conv2', 'bn2', 'conv3', 'bn3', 'relu', 'downsample']
    nn.Bottleneck(*parts(1, 256))
    p = parts()
    p[0] = torch.nn.Conv2d(64, 64, 1, bias=False)
    with pytest.raises(NotImplementedError, match='conv1'):
        nn.Bottleneck(*p)
    with pytest.raises(NotImplementedError, match='downsample'):
        nn.Bottleneck(*parts(2))
    with pytest.raises(NotImplementedError, match='downsample.0'):
        nn.Bottleneck(*parts(2), downsample=torch.nn.Sequential(torch.nn.Conv2d(64, 256, 1, 2), nn.BatchNorm2d(256)))
