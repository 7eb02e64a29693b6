"""CPU tests of the trainable stem and max-pool (celldetection_amd/nn/stem.py, nn/pool.py, csrc/stem_train.hip, csrc/pool_train.hip, csrc/pool_adjoint.h): the fp64
statements of tests/stem_oracle.py against torch's own float64 results, the wrong rules the cases tell apart, the pool's index
arithmetic and the stem's staging on the host under sanitizers, the host-side entry points, the Python surface and the two converts
on stand-ins with the reference's layout.  Nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import celldetection_amd as cda
import stem_oracle as oracle
from celldetection_amd import _lib, build
from test_bottleneck import Block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nn = cda.nn
GEOMETRIES = [(3, 2, 1), (2, 2, 0)]
NEW_SYMBOLS = ('cpn_stem_train_pack', 'cpn_stem_train_forward', 'cpn_stem_wgrad_info', 'cpn_stem_wgrad_workspace_bytes', 'cpn_stem_wgrad',
               'cpn_maxpool2d_indexed', 'cpn_maxpool2d_backward')


def _stem_operands(h, w, c, cout=8, n=3):
    g = torch.Generator().manual_seed(100 * h + 10 * w + c)
    ho, wo = oracle.out_size(h, w)
    return (torch.randn(n, c, h, w, generator=g, dtype=torch.float64), torch.randn(cout, c, 7, 7, generator=g, dtype=torch.float64),
            torch.randn(cout, generator=g, dtype=torch.float64), torch.randn(n, cout, ho, wo, generator=g, dtype=torch.float64))


def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('c', [1, 3, 4])
@pytest.mark.parametrize('size', [(5, 7), (9, 13), (1, 1), (2, 2), (3, 66)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_stem_statements_equal_torch_autograd(size, c):
    x, w, b, dy = _stem_operands(*size, c)
    y, dw, db = oracle.autograd64(x, w, b, dy)
    assert y.shape[2:] == oracle.out_size(*size)
    _close(oracle.forward(x, w, b), y)
    got, S = oracle.wgrad(x, dy)
    _close(got, dw)
    assert bool((S >= got.abs() - 1e-9).all())
    _close(oracle.bgrad(dy)[0], db)
    _close(oracle.forward(x, w), F.conv2d(x, w, None, 2, 3))


def test_the_pack_statement_is_the_record_layout_of_the_header():
    w = torch.arange(64 * 3 * 49, dtype=torch.float32).reshape(64, 3, 7, 7)
    p = oracle.pack(w)
    assert p.shape == (7, 64, 32) and p.dtype == torch.bfloat16
    rec = p.reshape(7, 64, 8, 4)
    assert bool((rec[:, :, 7] == 0).all()) and bool((rec[..., 3] == 0).all())
    assert float(rec[2, 5, 4, 1]) == float(w[5, 1, 2, 4].to(torch.bfloat16))
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2.0 ** -133]).reshape(1, 1, 1, 3)  # to even: down, up; a subnormal
    assert ties.to(torch.bfloat16).flatten().tolist()[:2] == [1.0, 1 + 2.0 ** -6]


def _pool_inputs(h, w, c=8, n=2):
    g = torch.Generator().manual_seed(31 * h + w)
    relu = torch.randn(n, c, h, w, generator=g, dtype=torch.float64).sub(.4).clamp_min(0.)  # more than half exact zeros
    return dict(relu=relu, constant=torch.full((n, c, h, w), 1.5, dtype=torch.float64),
                increasing=torch.arange(n * c * h * w, dtype=torch.float64).reshape(n, c, h, w))


@pytest.mark.parametrize('geometry', GEOMETRIES, ids=str)
def test_pool_statements_equal_torch_bit_for_bit(geometry):
    k, s, pad = geometry
    ran = 0
    for h in range(1, 8):
        for w in range(1, 10):
            if h + 2 * pad < k or w + 2 * pad < k:
                continue
            for name, x in _pool_inputs(h, w).items():
                y, index = oracle.pool_forward(x, k, s, pad)
                g = torch.Generator().manual_seed(h * w)
                dy = torch.randint(-64, 64, y.shape, generator=g).double() / 8  # (sums of such terms are exact in any order)
                want_y, want_dx = oracle.pool_autograd64(x, dy, k, s, pad)
                assert torch.equal(y, want_y), (name, h, w)
                dx, S, count = oracle.pool_backward(dy, index, (h, w), k, s, pad)
                assert torch.equal(dx, want_dx), (name, h, w)
                assert int(count.sum()) == y.numel() and int(count.max()) <= 4 and torch.equal(oracle.pool_gradient(x, dy, k, s, pad), dx)
                if name == 'relu' and h * w >= 12:
                    assert float((x == 0).double().mean()) > .5
                if name == 'constant':  # the whole gradient of a window lands on its first in-image pixel
                    first = torch.zeros_like(dx)
                    for oy in range(y.shape[2]):
                        for ox in range(y.shape[3]):
                            first[:, :, max(oy * s - pad, 0), max(ox * s - pad, 0)] += dy[:, :, oy, ox]
                    assert torch.equal(dx, first)
                if name == 'increasing':  # ... and on its last
                    last = torch.zeros_like(dx)
                    for oy in range(y.shape[2]):
                        for ox in range(y.shape[3]):
                            last[:, :, min(oy * s - pad + k, h) - 1, min(ox * s - pad + k, w) - 1] += dy[:, :, oy, ox]
                    assert torch.equal(dx, last)
                if k == 2:  # an odd last row or column lies in no window: exactly 0
                    assert bool((dx[:, :, 2 * y.shape[2]:] == 0).all()) and bool((dx[:, :, :, 2 * y.shape[3]:] == 0).all())
                ran += 1
    assert ran >= 3 * 48


def test_wrong_rules_are_told_apart():
    """Each rule of stem_oracle.WRONG_RULES moves a result of the case named beside it by an amount of the order of the values
    themselves; the GPU tests accept rounding noise only."""
    told = set()

    def differs(a, b):
        return a.shape != b.shape or float((a - b).abs().max()) > .1 * float(b.abs().mean())

    x, w, b, dy = _stem_operands(5, 7, 3)
    y, dw, db = oracle.autograd64(x, w, b, dy)
    for rule in ('taps_not_offset', 'stride_1', 'kx_ky_swapped'):
        assert differs(oracle.forward(x, w, b, rule), y) and differs(oracle.wgrad(x, dy, rule)[0], dw), rule
        told.add(rule)
    assert differs(oracle.wgrad(x, dy, 'kx7_leaks')[0], dw)
    told.add('kx7_leaks')
    for c in (1, 3):  # (with 4 real channels there is nothing to leak)
        xc, wc, bc, dyc = _stem_operands(5, 7, c)
        assert differs(oracle.wgrad(xc, dyc, 'channel_leaks')[0], oracle.wgrad(xc, dyc)[0]), c
    x4, _, _, dy4 = _stem_operands(5, 7, 4)
    assert torch.equal(oracle.wgrad(x4, dy4, 'channel_leaks')[0], oracle.wgrad(x4, dy4)[0])
    told.add('channel_leaks')
    for slab_rows in (1, 3):  # 3 images x 3 output rows: the last slab is one or three rows
        assert differs(oracle.wgrad(x, dy, 'last_slab_dropped', slab_rows)[0], dw), slab_rows
    told.add('last_slab_dropped')

    inputs = _pool_inputs(5, 7)
    for k, s, pad in GEOMETRIES:
        x = inputs['relu']
        y, index = oracle.pool_forward(x, k, s, pad)
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(k), dtype=torch.float64)
        right = oracle.pool_gradient(x, dy, k, s, pad)
        assert not torch.equal(oracle.pool_forward(x, k, s, pad, 'last_maximum')[1], index)
        for rule in ('last_maximum', 'ties_split', 'every_maximum'):
            assert differs(oracle.pool_gradient(x, dy, k, s, pad, rule), right), (rule, k)
    told.update(('last_maximum', 'ties_split', 'every_maximum'))
    x = inputs['relu'] + 1.
    dy = torch.ones(2, 8, 2, 3, dtype=torch.float64)
    right = oracle.pool_gradient(x, dy, 2, 2, 0)
    wrong = oracle.pool_gradient(x, dy, 2, 2, 0, 'odd_last_row_gets_gradient')
    assert bool((right[:, :, 4] == 0).all()) and bool((right[:, :, :, 6] == 0).all()) and bool((wrong[:, :, 4] != 0).any())
    assert oracle.pool_forward(x, 2, 2, 0, 'odd_last_row_gets_gradient')[0].shape[2:] == (3, 4)
    told.add('odd_last_row_gets_gradient')
    x = inputs['constant']
    y, index = oracle.pool_forward(x, 3, 2, 1)
    dy = torch.ones_like(y)
    assert int(index[0, 0, 0, 0]) == 4 and int(oracle.pool_forward(x, 3, 2, 1, 'window_clamped')[1][0, 0, 0, 0]) == 0
    assert differs(oracle.pool_gradient(x, dy, 3, 2, 1, 'window_clamped'), oracle.pool_gradient(x, dy, 3, 2, 1))
    told.add('window_clamped')
    assert told == set(oracle.WRONG_RULES) and len(told) >= 8


def test_host_build_of_the_pool_arithmetic_agrees_with_brute_force(tmp_path):
    """``csrc/pool_adjoint.h`` and the stem's staging over ``csrc/wgrad_slabs.h`` compiled for the host only, with AddressSanitizer
    and UBSan on the host code, by ``tests/pool_adjoint_host.cpp`` (a program of its own, nothing preloaded)."""
    hipcc = build._hipcc()
    exe = str(tmp_path / 'pool_adjoint_host')
    include = ['-I' + os.path.join(os.path.dirname(os.path.dirname(hipcc)), 'include')] if os.path.isabs(hipcc) else []
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__'] + include +
                          [os.path.join(ROOT, 'tests', 'pool_adjoint_host.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.fullmatch(r'ok \d+', run.stdout.strip()), run.stdout[-500:] + run.stderr[-2000:]
    assert int(run.stdout.split()[1]) > 100000


def test_wgrad_info_and_every_launch_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    for n, h, w in ((2, 1, 1), (2, 2, 2), (2, 5, 7), (2, 3, 66), (2, 4, 259), (2, 33, 70), (8, 512, 512)):
        ho, wo = oracle.out_size(h, w)
        for slab_rows in (0, 1, 3):
            for cout in (32, 64):
                i = nn.stem_weight_grad_info(n, h, w, cout, slab_rows)
                rows = n * ho
                assert i['slabs'] == -(-rows // i['slab_rows']) and i['reduce_chain'] == i['slabs'] and i['slabs'] <= max(256, rows if slab_rows else 0)
                assert slab_rows == 0 or i['slab_rows'] == min(slab_rows, rows)
                assert i['steps'] == -(-i['slab_rows'] * wo // 16)
                assert i['steps'] + 2 + i['reduce_chain'] <= -(-n * ho * wo // 16) + 2 + i['slabs'] + 3
                assert i['bias_chain'] == -(-i['slab_rows'] * wo // 8) + 8 + i['slabs']
                assert lib.cpn_stem_wgrad_workspace_bytes(n, h, w, cout, slab_rows) == i['slabs'] * (7 * cout * 32 + cout) * 4
    assert nn.stem_weight_grad_info(8, 512, 512, 64) == dict(slabs=256, slab_rows=8, steps=128, reduce_chain=256, bias_chain=256 + 8 + 256)
    out = (ctypes.c_int32 * 5)()
    # (N, H, W, cout, slab_rows)
    for bad, what in (((0, 4, 4, 64, 0), 'N, H and W'), ((2, 0, 4, 64, 0), 'N, H and W'), ((2, 4, 4, 48, 0), 'cout'), ((2, 4, 4, 128, 0), 'cout'),
                      ((2, 4, 4, 64, -1), 'slab_rows'), ((65536, 65536, 1, 64, 0), '2^31 - 1'), ((2, 2 ** 30, 2 ** 30, 64, 0), '2^31 - 1')):
        rc = lib.cpn_stem_wgrad_info(*bad, out)
        assert rc in (_lib.E_INVALID, _lib.E_UNSUPPORTED) and what in lib.cpn_last_error().decode(), (bad, lib.cpn_last_error())
        assert lib.cpn_stem_wgrad_workspace_bytes(*bad) == 0
        # the launches reject the same call before they touch a buffer (the pointers are never read)
        assert lib.cpn_stem_wgrad(16, 16, *bad[:3], 3, *bad[3:], 16, 0, 16, 0, 16, 1 << 40, None) == rc
        if bad[4] == 0:
            assert lib.cpn_stem_train_forward(16, 16, None, *bad[:4], 16, None) == rc
    ok = (2, 4, 4)
    assert lib.cpn_stem_wgrad_info(*ok, 64, 0, None) == _lib.E_INVALID
    launch = lib.cpn_stem_wgrad
    assert launch(16, 16, *ok, 3, 64, 0, 16, 0, 16, 0, 16, 16, None) == _lib.E_WORKSPACE
    for cin in (0, 5):
        assert launch(16, 16, *ok, cin, 64, 0, 16, 0, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID and 'cin' in lib.cpn_last_error().decode()
    assert launch(None, 16, *ok, 3, 64, 0, 16, 0, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID
    assert launch(16, 8, *ok, 3, 64, 0, 16, 0, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID and 'aligned' in lib.cpn_last_error().decode()
    assert launch(16, 16, *ok, 3, 64, 0, 16, 2, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID  # dtype code
    assert launch(16, 16, *ok, 3, 64, 0, None, 0, None, 0, 16, 1 << 40, None) == _lib.E_INVALID  # nothing to compute
    assert lib.cpn_stem_train_forward(None, 16, None, *ok, 64, 16, None) == _lib.E_INVALID
    assert lib.cpn_stem_train_forward(16, 24, None, *ok, 64, 16, None) == _lib.E_INVALID and 'aligned' in lib.cpn_last_error().decode()
    # (weight, dtype, cout, cin, packed)
    for bad in ((16, 0, 48, 3, 16), (16, 0, 64, 0, 16), (16, 0, 64, 5, 16), (16, 2, 64, 3, 16), (None, 0, 64, 3, 16), (16, 0, 64, 3, None)):
        assert lib.cpn_stem_train_pack(*bad, None) == _lib.E_INVALID and 'cpn_stem_train_pack' in lib.cpn_last_error().decode(), bad
    # the pool: (dtype, N, H, W, C, k, stride, pad)
    for bad, code in (((1, 0, 4, 4, 8, 3, 2, 1), _lib.E_INVALID), ((1, 2, 4, 4, 12, 3, 2, 1), _lib.E_INVALID), ((1, 2, 4, 4, 0, 3, 2, 1), _lib.E_INVALID),
                      ((2, 2, 4, 4, 8, 3, 2, 1), _lib.E_INVALID), ((1, 2, 4, 4, 8, 3, 1, 1), _lib.E_INVALID), ((1, 2, 4, 4, 8, 2, 2, 1), _lib.E_INVALID),
                      ((1, 2, 4, 4, 8, 3, 2, 0), _lib.E_INVALID), ((1, 2, 1, 4, 8, 2, 2, 0), _lib.E_INVALID), ((1, 2, 4, 1, 8, 2, 2, 0), _lib.E_INVALID),
                      ((1, 65536, 65536, 1, 8, 3, 2, 1), _lib.E_UNSUPPORTED)):
        assert lib.cpn_maxpool2d_indexed(16, *bad, 16, 16, None) == code and 'cpn_maxpool2d_indexed' in lib.cpn_last_error().decode(), bad
        assert lib.cpn_maxpool2d_backward(16, 16, *bad, 16, None) == code and 'cpn_maxpool2d_backward' in lib.cpn_last_error().decode(), bad
    good = (1, 2, 4, 4, 8, 3, 2, 1)
    assert lib.cpn_maxpool2d_indexed(None, *good, 16, 16, None) == _lib.E_INVALID
    assert lib.cpn_maxpool2d_indexed(16, *good, 16, 8, None) == _lib.E_INVALID and 'aligned' in lib.cpn_last_error().decode()
    assert lib.cpn_maxpool2d_backward(16, None, *good, 16, None) == _lib.E_INVALID
    assert lib.cpn_maxpool2d_backward(24, 16, *good, 16, None) == _lib.E_INVALID and 'aligned' in lib.cpn_last_error().decode()


def test_header_binding_and_exports_agree():
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
        assert not name.startswith(('cpn_bn_', 'cpn_tail_'))
    assert lib.cpn_abi_version() == _lib.ABI_VERSION
    flat_hdr = re.sub(r'\s*\n \*\s*', ' ', hdr)
    assert 'Trainable stem and max-pool' in flat_hdr
    for phrase in ('Additions to ABI 22', 'zeros at kx = 7 and c >= cin', '14 v_mfma_f32_32x32x16_bf16 steps', 'ascending slab order',
                   'never reach dw', 'no cross-wave sum', 'strictly greater', 'the first maximum wins', 'cut at the border, not clamped',
                   'raster order of (oy, ox)', 'gets an exact 0', 'No floating-point atomics', 'NaN is outside the contract',
                   'There is no input gradient'):
        assert phrase in flat_hdr, phrase
    assert 'stem_train.hip' in build.SOURCES and 'pool_adjoint.h' in build.HEADERS and 'image_train.h' in build.HEADERS
    assert build.SOURCES['pool_train.hip'] == build.SOURCES['stem_train.hip'] == []
    assert {'stem_conv2d', 'StemConv2d', 'convert_stem_conv2d_', 'stem_pack_weight', 'stem_weight_grad', 'stem_weight_grad_info',
            'max_pool2d', 'MaxPool2d', 'convert_maxpool2d_'} <= set(nn.__all__)
    # the stem's unit, what it shares with the image conv (csrc/image_train.h, the bias launch of csrc/wgrad_bias.h) and the pool's unit
    src, family, bias, pool = (open(os.path.join(ROOT, 'celldetection_amd', 'csrc', name)).read()
                               for name in ('stem_train.hip', 'image_train.h', 'wgrad_bias.h', 'pool_train.hip'))
    for text in (src, family, bias, pool):
        assert 'atomic' not in text.replace('No floating-point atomics', '') and 'fmaxf' not in text
    assert '#include "image_train.h"' in src and '#include "wgrad_bias.h"' in family and '#include "pool_adjoint.h"' in pool
    assert 'cpn_maxpool2d_indexed(' in pool and 'cpn_maxpool2d_backward(' in pool and 'maxpool' not in src
    # the forward loop and its swap-and-store are csrc/stem_mfma.h (shared with csrc/stem.hip), the transposed read csrc/mfma_frag.h
    loop, frag = (open(os.path.join(ROOT, 'celldetection_amd', 'csrc', name)).read() for name in ('stem_mfma.h', 'mfma_frag.h'))
    assert '#include "stem_mfma.h"' in src and '#include "mfma_frag.h"' in src and {'stem_mfma.h', 'mfma_frag.h'} <= set(build.HEADERS)
    assert 'atomic' not in loop + frag and 'fmaxf' not in loop + frag
    assert 'ds_read_tr16_b64' in frag and 'mf_operand(' in src and 'mfma_f32_32x32x16_bf16' in src
    assert 'mfma_f32_32x32x16_bf16' in loop and 'permlane32_swap' in loop and 'stem_mfma_loop<NF>(' in src
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'stem_conv2d' in text and 'max_pool2d' in text, doc
    assert 'the stem, the max-pool and' not in open(os.path.join(ROOT, 'README.md')).read()
    assert 'stay stock torch operations' not in nn.__doc__ and 'the stem, the max-pool' not in nn.__doc__


def test_every_unsupported_argument_raises_naming_it():
    x, w = torch.zeros(2, 3, 9, 11), torch.zeros(64, 3, 7, 7)
    for args, name in (((x[0], w), 'input of 3 dimensions'), ((x, w[0]), 'weight of 3 dimensions'), ((x, torch.zeros(64, 3, 3, 3)), 'kernel_size'),
                       ((x, torch.zeros(64, 3, 7, 5)), 'kernel_size'), ((torch.zeros(2, 5, 9, 11), torch.zeros(64, 5, 7, 7)), '5 channels'),
                       ((x, torch.zeros(64, 5, 7, 7)), 'in_channels 5'), ((x, torch.zeros(48, 3, 7, 7)), 'out_channels 48'),
                       ((x, torch.zeros(128, 3, 7, 7)), 'out_channels 128'), ((x.double(), w), 'input dtype'), ((x, w.half()), 'weight dtype'),
                       ((x, w, torch.zeros(32)), 'bias'), ((x, w, torch.zeros(64).double()), 'bias'), ((torch.zeros(2, 3, 0, 11), w), 'at least one pixel'),
                       ((x.clone().requires_grad_(True), w), 'x requires a gradient')):
        with pytest.raises(NotImplementedError, match=name):
            nn.stem_conv2d(*args)
    with pytest.raises(ValueError, match='channels'):
        nn.stem_conv2d(x, torch.zeros(64, 4, 7, 7))
    with pytest.raises(RuntimeError, match='MI355X'):  # supported arguments on the CPU: the usual device error, no fallback
        nn.stem_conv2d(x, w)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.StemConv2d(3, 64)(x)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.stem_pack_weight(w)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.stem_weight_grad(x, torch.zeros(2, 64, 5, 6))
    for bad, name in ((dict(x=torch.zeros(2, 5, 9, 11)), '5 channels'), (dict(grad_output=torch.zeros(2, 48, 5, 6)), 'out_channels 48'),
                      (dict(dtype=torch.float64), 'dtype')):
        kw = dict(x=x, grad_output=torch.zeros(2, 64, 5, 6))
        kw.update(bad)
        with pytest.raises(NotImplementedError, match=name):
            nn.stem_weight_grad(**kw)
    with pytest.raises(NotImplementedError, match='kernel_size'):
        nn.stem_pack_weight(torch.zeros(64, 3, 3, 3))
    for kwargs, name in ((dict(kernel_size=3), 'kernel_size'), (dict(stride=1), 'stride'), (dict(padding=0), 'padding'), (dict(padding='same'), 'padding'),
                         (dict(dilation=2), 'dilation'), (dict(groups=3), 'groups'), (dict(padding_mode='reflect'), 'padding_mode'),
                         (dict(in_channels=5), 'in_channels'), (dict(out_channels=16), 'out_channels')):
        kw = dict(in_channels=3, out_channels=64)
        kw.update(kwargs)
        with pytest.raises(NotImplementedError, match=name):
            nn.StemConv2d(**kw)
    m, stock = nn.StemConv2d(3, 64, bias=False), torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    assert isinstance(m, torch.nn.Conv2d) and list(m.state_dict()) == list(stock.state_dict()) and (m.stride, m.padding) == ((2, 2), (3, 3))
    m.load_state_dict(stock.state_dict())
    stock.load_state_dict(m.state_dict())
    # the pool
    p = torch.zeros(2, 8, 9, 11)
    for kwargs, name in ((dict(dilation=2), 'dilation'), (dict(ceil_mode=True), 'ceil_mode'), (dict(return_indices=True), 'return_indices'),
                         (dict(kernel_size=3, stride=1, padding=1), 'stride 1'), (dict(kernel_size=3, stride=2, padding=0), 'padding 0'),
                         (dict(kernel_size=2, stride=2, padding=1), 'padding 1'), (dict(kernel_size=5, stride=2, padding=2), 'kernel_size 5'),
                         (dict(kernel_size=(3, 2), stride=2, padding=1), 'kernel_size'), (dict(x=torch.zeros(2, 12, 9, 11)), 'C % 8'),
                         (dict(x=torch.zeros(2, 4, 9, 11)), 'C % 8'), (dict(x=p[0]), 'input of 3 dimensions'), (dict(x=p.double()), 'input dtype')):
        kw = dict(x=p, kernel_size=3, stride=2, padding=1)
        kw.update(kwargs)
        with pytest.raises(NotImplementedError, match=name):
            nn.max_pool2d(**kw)
        ctor = {k_: v for k_, v in kw.items() if k_ != 'x'}
        if 'x' not in kwargs:
            with pytest.raises(NotImplementedError, match=name):
                nn.MaxPool2d(**ctor)
    for size in ((1, 1), (1, 2), (2, 1)):  # as in torch: a 2x2 window does not fit
        with pytest.raises(ValueError, match='empty'):
            nn.max_pool2d(torch.zeros(2, 8, *size), 2)
        with pytest.raises(RuntimeError):
            F.max_pool2d(torch.zeros(2, 8, *size), 2)
    for args in ((3, 2, 1), (2,), (2, 2), (2, None, 0)):
        with pytest.raises(RuntimeError, match='MI355X'):
            nn.max_pool2d(p, *args)
        with pytest.raises(RuntimeError, match='MI355X'):
            nn.MaxPool2d(*args)(p)
    assert nn.MaxPool2d(2).stride == 2 and isinstance(nn.MaxPool2d(3, 2, 1), torch.nn.MaxPool2d)


# ---- the converts

class _Encoder(torch.nn.Sequential):
    """The reference's ResNet (models/resnet.py:274-284) in both layouts, with one stage of two blocks."""

    def __init__(self, in_channels=3, fused_initial=True, base=64):
        t = torch.nn
        initial = [t.Conv2d(in_channels, base, 7, padding=3, bias=False, stride=2), t.BatchNorm2d(base), t.ReLU(inplace=True)]
        pool = t.MaxPool2d(kernel_size=3, stride=2, padding=1)
        layer1 = t.Sequential(Block(base, 128, 32, 1, 256, 'conv'), Block(256, 128, 32, 1, 256, None))
        if fused_initial:
            super().__init__(t.Sequential(*initial, pool, layer1))
        else:
            super().__init__(t.Sequential(*initial), t.Sequential(pool, layer1))


def _signature(net):
    return [(name, type(m), getattr(m, 'activation', None)) for name, m in net.named_modules()]


@pytest.mark.parametrize('fused_initial', [True, False])
def test_the_two_converts_on_the_reference_layout(fused_initial):
    net = _Encoder(3, fused_initial)
    net[0][0].register_forward_hook(lambda *a: None)
    params, buffers, keys = dict(net.named_parameters()), dict(net.named_buffers()), list(net.state_dict().keys())
    conv_name, pool_name = '0.0', '0.3' if fused_initial else '1.0'
    assert nn.convert_stem_conv2d_(net) == ([conv_name], {})
    assert nn.convert_maxpool2d_(net) == ([pool_name], {})
    stem, pool = net.get_submodule(conv_name), net.get_submodule(pool_name)
    assert type(stem) is nn.StemConv2d and type(pool) is nn.MaxPool2d and stem._forward_hooks
    assert (pool.kernel_size, pool.stride, pool.padding, pool.ceil_mode) == (3, 2, 1, False) and stem.training and pool.training
    after_p, after_b = dict(net.named_parameters()), dict(net.named_buffers())
    assert after_p.keys() == params.keys() and all(after_p[k] is params[k] for k in params)  # the same Parameter objects
    assert after_b.keys() == buffers.keys() and all(after_b[k] is buffers[k] for k in buffers)
    assert list(net.state_dict().keys()) == keys
    fresh = _Encoder(3, fused_initial)
    fresh.load_state_dict(net.state_dict())
    net.load_state_dict(fresh.state_dict())
    assert nn.convert_stem_conv2d_(net) == ([], {}) and nn.convert_maxpool2d_(net) == ([], {})  # a second call finds nothing
    left = nn.convert_conv2d_(net)[1]
    assert conv_name not in left  # not reported as "a subclass of torch.nn.Conv2d"
    with pytest.raises(RuntimeError, match='MI355X'):  # the converted modules run this library's kernels: no CPU fallback
        stem(torch.zeros(2, 3, 16, 16))
    with pytest.raises(RuntimeError, match='MI355X'):
        pool(torch.zeros(2, 64, 8, 8))


def test_roots_shared_slots_and_what_is_left():
    t = torch.nn
    assert nn.convert_stem_conv2d_(t.Conv2d(3, 64, 7, 2, 3)) == ([], {'': 'the root module cannot be replaced in place: convert its parent'})
    assert nn.convert_maxpool2d_(t.MaxPool2d(3, 2, 1)) == ([], {'': 'the root module cannot be replaced in place: convert its parent'})
    assert nn.convert_conv2d_(nn.StemConv2d(3, 64)) == ([], {})
    conv, pool = t.Conv2d(1, 32, 7, 2, 3), t.MaxPool2d(2)
    both = t.ModuleList([conv, t.Sequential(conv, pool), pool])  # a module that sits in two slots stays one object
    assert nn.convert_stem_conv2d_(both) == (['0', '1.0'], {}) and nn.convert_maxpool2d_(both) == (['2', '1.1'], {})  # (parents first)
    assert both[0] is both[1][0] and type(both[0]) is nn.StemConv2d and both[2] is both[1][1] and type(both[2]) is nn.MaxPool2d
    assert both[0].weight is conv.weight and both[0].bias is conv.bias
    # a U-Net encoder's 2x2 pool is taken (graph.py: UNetEncoder)
    unet = t.Sequential(t.Conv2d(32, 32, 3, padding=1), t.MaxPool2d(2), t.Conv2d(32, 64, 3, padding=1), t.MaxPool2d(2, 2))
    assert nn.convert_maxpool2d_(unet) == (['1', '3'], {}) and nn.convert_stem_conv2d_(unet) == ([], {})

    class Own(t.MaxPool2d):
        pass

    odd = t.ModuleDict(dict(ceil=t.MaxPool2d(3, 2, 1, ceil_mode=True), dil=t.MaxPool2d(3, 2, 1, dilation=2), idx=t.MaxPool2d(2, return_indices=True),
                            geo=t.MaxPool2d(3, 1, 1), own=Own(2), five=t.Conv2d(5, 64, 7, 2, 3), out=t.Conv2d(3, 16, 7, 2, 3), k3=t.Conv2d(3, 32, 3, 1, 1),
                            pad=t.Conv2d(3, 64, 7, 2, 2), grp=t.Conv2d(4, 64, 7, 2, 3, groups=2), refl=t.Conv2d(3, 64, 7, 2, 3, padding_mode='reflect'),
                            dense=t.Conv2d(64, 64, 7, padding=3), f16=t.Conv2d(3, 64, 7, 2, 3).half()))
    sig = _signature(odd)
    replaced, left = nn.convert_maxpool2d_(odd)
    assert replaced == [] and set(left) == {'ceil', 'dil', 'idx', 'geo', 'own'}
    assert left['ceil'].startswith('ceil_mode True') and left['dil'].startswith('dilation 2') and left['idx'].startswith('return_indices') and \
        left['geo'].startswith('kernel_size 3, stride 1, padding 1') and left['own'].startswith('a subclass of torch.nn.MaxPool2d (Own)')
    replaced, left = nn.convert_stem_conv2d_(odd)
    assert replaced == [] and set(left) == {'five', 'out', 'k3', 'pad', 'grp', 'refl', 'f16'}  # (the dense 7x7 stride-1 conv is convert_conv2d_'s)
    assert left['five'].startswith('in_channels 5') and left['out'].startswith('out_channels 16') and left['k3'].startswith('kernel_size (3, 3)') and \
        left['pad'].startswith('padding (2, 2)') and left['grp'].startswith('groups 2') and left['refl'].startswith("padding_mode 'reflect'") and \
        left['f16'].startswith('weight dtype torch.float16')
    assert _signature(odd) == sig


CONVERTS = {'conv': nn.convert_conv2d_, 'bn': nn.convert_batchnorm2d_, 'grouped': nn.convert_grouped_conv2d_, 'bottleneck': nn.convert_bottleneck_,
            'stem': nn.convert_stem_conv2d_, 'pool': nn.convert_maxpool2d_}
ORDERS = (('conv', 'bn', 'grouped', 'bottleneck', 'stem', 'pool'), ('pool', 'stem', 'bottleneck', 'grouped', 'bn', 'conv'),
          ('stem', 'bn', 'pool', 'conv', 'bottleneck', 'grouped'))


def converted(net, order):
    for name in order:
        CONVERTS[name](net)
    return net


@pytest.mark.parametrize('fused_initial', [True, False])
def test_all_six_converts_in_any_order_give_the_same_modules(fused_initial):
    want = None
    for order in ORDERS:
        net = _Encoder(3, fused_initial)
        params, keys = dict(net.named_parameters()), list(net.state_dict().keys())
        converted(net, order)
        sig = _signature(net)
        want = want or sig
        assert sig == want, order
        after = dict(net.named_parameters())
        assert after.keys() == params.keys() and all(after[k] is params[k] for k in params) and list(net.state_dict().keys()) == keys
    first = net[0]
    assert type(first[0]) is nn.StemConv2d and type(first[1]) is nn.BatchNorm2d and first[1].activation == 'relu' and type(first[2]) is torch.nn.Identity
    pool, layer1 = (first[3], first[4]) if fused_initial else (net[1][0], net[1][1])
    assert type(pool) is nn.MaxPool2d and all(type(b) is nn.Bottleneck for b in layer1)
    stock = (torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.MaxPool2d, torch.nn.ReLU)
    for name, m in net.named_modules():  # no stock operation is left (a block's `relu` is kept for its name only)
        assert type(m) not in stock or name.endswith('.relu'), name
