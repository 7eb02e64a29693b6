"""CPU tests of the trainable image conv (celldetection_amd/nn/image_conv.py, csrc/image_conv_train.hip): the fp64 statements of
tests/image_conv_oracle.py against torch's own float64 autograd, the wrong rules the cases tell apart, the host-side entry points, the
Python surface and ``convert_image_conv2d_`` on a stand-in with the layout of the reference's ``UNetEncoder``
(tests/unet_encoder_standin.py).  Nothing here needs a GPU."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import celldetection_amd as cda
import cpn_core_standin
import image_conv_oracle as oracle
import unet_encoder_standin as standin
from celldetection_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nn = cda.nn
NEW_SYMBOLS = ('cpn_image_conv_pad', 'cpn_image_conv_pack', 'cpn_image_conv_forward', 'cpn_image_conv_wgrad_info',
               'cpn_image_conv_wgrad_workspace_bytes', 'cpn_image_conv_wgrad')
SIZES = [(5, 7), (9, 4), (1, 1), (2, 3), (3, 34)]


def _operands(h, w, c, cout=32, n=3, rule=None):
    g = torch.Generator().manual_seed(100 * h + 10 * w + c + cout)
    ho, wo = oracle.out_size(h, w, rule)
    return (torch.randn(n, c, h, w, generator=g, dtype=torch.float64), torch.randn(cout, c, 3, 3, generator=g, dtype=torch.float64),
            torch.randn(cout, generator=g, dtype=torch.float64), torch.randn(n, cout, ho, wo, generator=g, dtype=torch.float64))


def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('cout', [32, 64, 128])
@pytest.mark.parametrize('c', [1, 3, 4])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_statements_equal_torch_autograd(size, c, cout):
    x, w, b, dy = _operands(*size, c, cout)
    y, dw, db = oracle.autograd64(x, w, b, dy)
    assert y.shape[2:] == size
    _close(oracle.forward(x, w, b), y)
    got, S = oracle.wgrad(x, dy)
    _close(got, dw)
    assert bool((S >= got.abs() - 1e-9).all())
    _close(oracle.bgrad(dy)[0], db)
    _close(oracle.forward(x, w), F.conv2d(x, w, None, 1, 1))
    for slab_rows in (1, 3, 1000):  # the slab partition adds up to the whole
        parts, slabs = oracle.wgrad_slabs(x, dy, slab_rows)
        _close(parts, dw)
        assert slabs == -(-3 * size[0] // min(slab_rows, 3 * size[0]))


def test_the_pad_and_pack_statements_are_the_layouts_of_the_header():
    w = torch.arange(64 * 3 * 9, dtype=torch.float32).reshape(64, 3, 3, 3)
    p = oracle.pack(w)
    assert p.shape == (3, 64, 16) and p.dtype == torch.bfloat16
    rec = p.reshape(3, 64, 4, 4)
    assert bool((rec[:, :, 3] == 0).all()) and bool((rec[..., 3] == 0).all())
    assert float(rec[2, 5, 1, 1]) == float(w[5, 1, 2, 1].to(torch.bfloat16))
    x = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5) + 1
    q = oracle.pad(x)
    assert q.shape == (2, 6, 8, 4) and q.dtype == torch.bfloat16
    assert bool((q[:, 0] == 0).all()) and bool((q[:, 5] == 0).all()) and bool((q[:, :, 0] == 0).all()) and bool((q[:, :, 6:] == 0).all())
    assert bool((q[..., 3] == 0).all()) and float(q[1, 1 + 2, 1 + 3, 2]) == float(x[1, 2, 2, 3].to(torch.bfloat16))
    # the 16 values output pixel (y, x) meets in filter row ky are contiguous at Xq[n][y + ky][x], and the conv over them is the stock one
    wt = torch.randn(32, 3, 3, 3, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    xs = torch.randn(2, 3, 4, 5, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    q, rec = oracle.pad(xs).double(), oracle.pack(wt).double()
    flat = q.reshape(2, -1)
    y = torch.zeros(2, 32, 4, 5, dtype=torch.float64)
    for yy in range(4):
        for xx in range(5):
            for ky in range(3):
                at = ((yy + ky) * 8 + xx) * 4
                assert at + 16 <= flat.shape[1]  # every read lies inside Xq
                y[:, :, yy, xx] += flat[:, at:at + 16] @ rec[ky].T
    assert ((3 + 2) * 8 + 4) * 4 + 16 == flat.shape[1]  # the last read ends at Xq's last byte
    _close(y, F.conv2d(xs.double(), wt.double(), None, 1, 1))


def test_wrong_rules_are_told_apart():
    """Each rule of image_conv_oracle.WRONG_RULES moves a result of every case by an amount of the order of the values themselves;
    the GPU tests accept rounding noise only."""
    told = set()

    def differs(a, b):
        return a.shape != b.shape or float((a - b).abs().max()) > .1 * float(b.abs().mean())

    for size in SIZES:
        if size == (1, 1):  # (a single pixel meets the centre tap alone: the cases with more than one pixel tell the rules apart)
            continue
        for c in (1, 3, 4):
            for cout in (32, 64, 128):
                x, w, b, dy = _operands(*size, c, cout)
                y, dw, db = oracle.autograd64(x, w, b, dy)
                for rule in ('taps_not_offset', 'kx_ky_swapped'):
                    assert differs(oracle.forward(x, w, b, rule), y) and differs(oracle.wgrad(x, dy, rule)[0], dw), (rule, size, c, cout)
                    told.add(rule)
                for rule in ('stride_2', 'padding_0'):
                    assert differs(oracle.forward(x, w, b, rule), y), (rule, size, c, cout)
                    told.add(rule)
                assert differs(oracle.forward(x, w, b, 'bias_twice'), y) and torch.equal(oracle.forward(x, w, None, 'bias_twice'), oracle.forward(x, w))
                told.add('bias_twice')
                if size[1] >= 3:  # (column x + 3 of Xq holds a pixel only in rows of three or more)
                    assert differs(oracle.wgrad(x, dy, 'kx3_leaks')[0], dw), (size, c, cout)
                    told.add('kx3_leaks')
                if c < 4:
                    assert differs(oracle.wgrad(x, dy, 'channel_leaks')[0], dw), (size, c, cout)
                else:  # (with 4 real channels there is nothing to leak)
                    assert torch.equal(oracle.wgrad(x, dy, 'channel_leaks')[0], oracle.wgrad(x, dy)[0])
                told.add('channel_leaks')
                for slab_rows in (1, 3):
                    assert differs(oracle.wgrad(x, dy, 'last_slab_dropped', slab_rows)[0], dw), (slab_rows, size, c, cout)
                told.add('last_slab_dropped')
    # stride 2 and padding 0 against the stock expressions they are
    x, w, b, dy = _operands(5, 7, 3)
    _close(oracle.forward(x, w, b, 'stride_2'), F.conv2d(x, w, b, 2, 1))
    _close(oracle.forward(x, w, b, 'padding_0'), F.conv2d(x, w, b, 1, 0))
    assert told == set(oracle.WRONG_RULES) and len(told) >= 8


def test_wgrad_info_and_every_launch_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    for n, h, w in ((2, 1, 1), (2, 2, 2), (2, 5, 7), (2, 3, 33), (2, 4, 129), (2, 33, 70), (8, 512, 512)):
        for slab_rows in (0, 1, 3):
            for cout in (32, 64, 128):
                i = nn.image_weight_grad_info(n, h, w, cout, slab_rows)
                rows = n * h
                assert i['slabs'] == -(-rows // i['slab_rows']) and i['reduce_chain'] == i['slabs'] and i['slabs'] <= max(512, rows if slab_rows else 0)
                assert slab_rows == 0 or i['slab_rows'] == min(slab_rows, rows)
                assert i['steps'] == -(-i['slab_rows'] * w // 16)
                assert i['steps'] + 2 + i['reduce_chain'] <= -(-n * h * w // 16) + 2 + i['slabs'] + 3
                assert i['bias_chain'] == -(-i['slab_rows'] * w // 8) + 8 + i['slabs']
                assert lib.cpn_image_conv_wgrad_workspace_bytes(n, h, w, cout, slab_rows) == i['slabs'] * (3 * cout * 16 + cout) * 4
    assert nn.image_weight_grad_info(8, 512, 512, 64) == dict(slabs=512, slab_rows=8, steps=256, reduce_chain=512, bias_chain=512 + 8 + 512)
    out = (ctypes.c_int32 * 5)()
    # (N, H, W, cout, slab_rows)
    for bad, what in (((0, 4, 4, 64, 0), 'N, H and W'), ((2, 0, 4, 64, 0), 'N, H and W'), ((2, 4, 0, 64, 0), 'N, H and W'), ((2, 4, 4, 48, 0), 'cout'),
                      ((2, 4, 4, 256, 0), 'cout'), ((2, 4, 4, 64, -1), 'slab_rows'), ((65536, 65536, 1, 64, 0), '2^31 - 1'),
                      ((2, 2 ** 30, 2 ** 30, 64, 0), '2^31 - 1')):
        rc = lib.cpn_image_conv_wgrad_info(*bad, out)
        assert rc in (_lib.E_INVALID, _lib.E_UNSUPPORTED) and what in lib.cpn_last_error().decode(), (bad, lib.cpn_last_error())
        assert lib.cpn_image_conv_wgrad_workspace_bytes(*bad) == 0
        # the launches reject the same call before they touch a buffer (the pointers are never read)
        assert lib.cpn_image_conv_wgrad(16, 16, *bad[:3], 3, *bad[3:], 16, 0, 16, 0, 16, 1 << 40, None) == rc
        if bad[4] == 0:
            assert lib.cpn_image_conv_forward(16, 16, None, *bad[:4], 16, None) == rc
            if 'cout' not in what:
                assert lib.cpn_image_conv_pad(16, bad[0], 3, bad[1], bad[2], 16, None) == rc
    ok = (2, 4, 4)
    assert lib.cpn_image_conv_wgrad_info(*ok, 64, 0, None) == _lib.E_INVALID
    launch = lib.cpn_image_conv_wgrad
    assert launch(16, 16, *ok, 3, 64, 0, 16, 0, 16, 0, 16, 16, None) == _lib.E_WORKSPACE
    for cin in (0, 5):
        assert launch(16, 16, *ok, cin, 64, 0, 16, 0, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID and 'cin' in lib.cpn_last_error().decode()
    assert launch(None, 16, *ok, 3, 64, 0, 16, 0, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID
    assert launch(16, None, *ok, 3, 64, 0, 16, 0, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID
    assert launch(16, 16, *ok, 3, 64, 0, 16, 0, 16, 0, None, 1 << 40, None) == _lib.E_INVALID
    assert launch(16, 8, *ok, 3, 64, 0, 16, 0, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID and 'aligned' in lib.cpn_last_error().decode()
    assert launch(16, 16, *ok, 3, 64, 0, 16, 2, 16, 0, 16, 1 << 40, None) == _lib.E_INVALID  # dtype code
    assert launch(16, 16, *ok, 3, 64, 0, 16, 0, 16, -1, 16, 1 << 40, None) == _lib.E_INVALID  # dtype code of db
    assert launch(16, 16, *ok, 3, 64, 0, None, 0, None, 0, 16, 1 << 40, None) == _lib.E_INVALID  # nothing to compute
    assert lib.cpn_image_conv_forward(None, 16, None, *ok, 64, 16, None) == _lib.E_INVALID
    assert lib.cpn_image_conv_forward(16, 16, None, *ok, 64, None, None) == _lib.E_INVALID
    assert lib.cpn_image_conv_forward(16, 24, None, *ok, 64, 16, None) == _lib.E_INVALID and 'aligned' in lib.cpn_last_error().decode()
    # the pad: (src, N, C, H, W, xq)
    for bad in ((16, 2, 0, 4, 4, 16), (16, 2, 5, 4, 4, 16), (None, 2, 3, 4, 4, 16), (16, 2, 3, 4, 4, None), (16, 2, 3, 4, 4, 8), (18, 2, 3, 4, 4, 16)):
        assert lib.cpn_image_conv_pad(*bad, None) == _lib.E_INVALID and 'cpn_image_conv_pad' in lib.cpn_last_error().decode(), bad
    # the pack: (weight, dtype, cout, cin, packed)
    for bad in ((16, 0, 48, 3, 16), (16, 0, 64, 0, 16), (16, 0, 64, 5, 16), (16, 2, 64, 3, 16), (None, 0, 64, 3, 16), (16, 0, 64, 3, None)):
        assert lib.cpn_image_conv_pack(*bad, None) == _lib.E_INVALID and 'cpn_image_conv_pack' in lib.cpn_last_error().decode(), bad


def test_header_binding_and_build_list_agree():
    hdr = open(os.path.join(ROOT, 'include', 'cpn_hip.h')).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    assert lib.cpn_abi_version() == _lib.ABI_VERSION == 22
    flat_hdr = re.sub(r'\s*\n \*\s*', ' ', hdr)
    section = flat_hdr[flat_hdr.index('---- Trainable image conv'):]
    section = section[:section.index('int cpn_image_conv_pad(')]
    for phrase in ('Additions to ABI 22', 'This text is the contract', '[N][H + 2][Wq = W + 3][4]', 'zeros at kx = 3 and c >= cin',
                   '32 contiguous bytes at Xq[n][y + ky][x]', 'the last row of the last image included', 'Image values must be finite',
                   '3 steps per output in one fp32 accumulator', 'ascending slab order', 'never reach dw', 'no cross-wave sum',
                   'Wave w owns image w % 2', 'once for all three filter rows', 'No floating-point atomics', 'There is no input gradient',
                   'Both answer without a GPU', 'Every call validates before it reads a pointer', 'Known limits'):
        assert phrase in section, phrase
    assert 'image_conv_train.hip' in build.SOURCES and build.SOURCES['image_conv_train.hip'] == []
    assert {'wgrad_slabs.h', 'wgrad_bias.h', 'mfma_frag.h', 'stem_mfma.h'} <= set(build.HEADERS)
    assert {'image_conv2d', 'ImageConv2d', 'convert_image_conv2d_', 'image_pack_weight', 'image_weight_grad', 'image_weight_grad_info'} <= set(nn.__all__)
    # the unit and the shared headers its text moved to: csrc/image_train.h and the bias launch of csrc/wgrad_bias.h
    unit, family, bias = (open(os.path.join(ROOT, 'celldetection_amd', 'csrc', name)).read()
                          for name in ('image_conv_train.hip', 'image_train.h', 'wgrad_bias.h'))
    assert '#include "image_train.h"' in unit and '#include "wgrad_bias.h"' in family and 'image_train.h' in build.HEADERS
    src = unit + family + bias
    assert 'atomic' not in src.replace('No floating-point atomics', '') and 'fmaxf' not in src
    assert 'mfma_f32_32x32x16_bf16' in unit and 'mf_operand(' in unit and 'wgs_partition(' in src and 'ct_bias_slab_kernel' in src
    for doc in ('README.md',):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'image_conv2d' in text and 'convert_image_conv2d_' in text and 'Trainable image conv on the GPU' in text, doc
    assert 'image_conv2d' in nn.__doc__ and 'not the 3x3 first conv' not in nn.stem.__doc__ and 'image_conv2d' in nn.stem.__doc__


def test_every_unsupported_argument_raises_naming_it():
    x, w = torch.zeros(2, 3, 9, 11), torch.zeros(64, 3, 3, 3)
    for args, name in (((x[0], w), 'input of 3 dimensions'), ((x, w[0]), 'weight of 3 dimensions'), ((x, torch.zeros(64, 3, 7, 7)), 'kernel_size'),
                       ((x, torch.zeros(64, 3, 3, 1)), 'kernel_size'), ((torch.zeros(2, 5, 9, 11), torch.zeros(64, 5, 3, 3)), '5 channels'),
                       ((x, torch.zeros(64, 5, 3, 3)), 'in_channels 5'), ((x, torch.zeros(48, 3, 3, 3)), 'out_channels 48'),
                       ((x, torch.zeros(16, 3, 3, 3)), 'out_channels 16'), ((x, torch.zeros(256, 3, 3, 3)), 'out_channels 256'),
                       ((x.double(), w), 'input dtype'), ((x.half(), w), 'input dtype'), ((x, w.half()), 'weight dtype'),
                       ((x, w, torch.zeros(32)), 'bias'), ((x, w, torch.zeros(64).double()), 'bias'), ((torch.zeros(2, 3, 0, 11), w), 'at least one pixel'),
                       ((x.clone().requires_grad_(True), w), 'x requires a gradient')):
        with pytest.raises(NotImplementedError, match=name):
            nn.image_conv2d(*args)
    with pytest.raises(ValueError, match='channels'):
        nn.image_conv2d(x, torch.zeros(64, 4, 3, 3))
    with pytest.raises(RuntimeError, match='MI355X'):  # supported arguments on the CPU: the usual device error, no fallback
        nn.image_conv2d(x, w)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.ImageConv2d(3, 64)(x)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.image_pack_weight(w)
    with pytest.raises(RuntimeError, match='MI355X'):
        nn.image_weight_grad(x, torch.zeros(2, 64, 9, 11))
    for bad, name in ((dict(x=torch.zeros(2, 5, 9, 11)), '5 channels'), (dict(grad_output=torch.zeros(2, 48, 9, 11)), 'out_channels 48'),
                      (dict(dtype=torch.float64), 'dtype'), (dict(bias_dtype=torch.float16), 'dtype')):
        kw = dict(x=x, grad_output=torch.zeros(2, 64, 9, 11))
        kw.update(bad)
        with pytest.raises(NotImplementedError, match=name):
            nn.image_weight_grad(**kw)
    with pytest.raises(NotImplementedError, match='kernel_size'):
        nn.image_pack_weight(torch.zeros(64, 3, 7, 7))
    for kwargs, name in ((dict(kernel_size=7), 'kernel_size'), (dict(kernel_size=(3, 1)), 'kernel_size'), (dict(stride=2), 'stride'),
                         (dict(padding=0), 'padding'), (dict(padding='same'), 'padding'), (dict(dilation=2), 'dilation'), (dict(groups=3), 'groups'),
                         (dict(padding_mode='reflect'), 'padding_mode'), (dict(in_channels=5), 'in_channels'), (dict(out_channels=16), 'out_channels')):
        kw = dict(in_channels=3, out_channels=64)
        kw.update(kwargs)
        with pytest.raises(NotImplementedError, match=name):
            nn.ImageConv2d(**kw)
    for cout in (32, 64, 128):
        m, stock = nn.ImageConv2d(3, cout, bias=False), torch.nn.Conv2d(3, cout, 3, 1, 1, bias=False)
        assert isinstance(m, torch.nn.Conv2d) and list(m.state_dict()) == list(stock.state_dict())
        assert (m.kernel_size, m.stride, m.padding) == ((3, 3), (1, 1), (1, 1))
        m.load_state_dict(stock.state_dict())
        stock.load_state_dict(m.state_dict())
    assert list(nn.ImageConv2d(1, 32).state_dict()) == ['weight', 'bias']


# ---- the convert

def _signature(net):
    return [(name, type(m), getattr(m, 'activation', None)) for name, m in net.named_modules()]


def test_the_standin_has_the_layout_of_the_reference_encoder():
    enc = standin.UNetEncoder(3)
    assert isinstance(enc, torch.nn.Sequential) and len(enc) == 3 and enc.out_channels == [32, 64, 128]
    assert type(enc[0]) is standin.TwoConvNormRelu and type(enc[0]).forward is torch.nn.Sequential.forward
    for level in list(enc)[1:]:
        assert type(level) is torch.nn.Sequential and type(level[0]) is torch.nn.MaxPool2d and type(level[1]) is standin.TwoConvNormRelu
        assert (level[0].kernel_size, level[0].stride, level[0].padding) == (2, 2, 0)
    first = enc[0][0]
    assert (first.in_channels, first.out_channels, first.kernel_size, first.stride, first.padding) == (3, 32, (3, 3), (1, 1), (1, 1))
    x = torch.randn(2, 3, 22, 26)
    shapes = []
    for level in enc:
        x = level(x)
        shapes.append(tuple(x.shape[1:]))
    assert shapes == [(32, 22, 26), (64, 11, 13), (128, 5, 6)]


@pytest.mark.parametrize('channels', [1, 3, 4])
def test_the_convert_on_the_encoder_before_and_after_the_other_converts(channels):
    want = None
    for first in (True, False):
        enc = torch.nn.ModuleDict(dict(encoder=standin.UNetEncoder(channels)))
        enc['encoder'][0][0].register_forward_hook(lambda *a: None)
        params, buffers, keys = dict(enc.named_parameters()), dict(enc.named_buffers()), list(enc.state_dict().keys())
        others = (nn.convert_conv2d_, nn.convert_batchnorm2d_, nn.convert_maxpool2d_, nn.convert_stem_conv2d_)
        if first:
            assert nn.convert_image_conv2d_(enc) == (['encoder.0.0'], {})
        results = [convert(enc) for convert in others]
        # the existing converts keep their reasons for the conv they leave, and do not name a conv of this library
        if first:
            assert 'encoder.0.0' not in results[0][1] and results[3] == ([], {})
        else:
            assert 'encoder.0.0' in results[0][1] and results[3][1]['encoder.0.0'].startswith('kernel_size (3, 3)')
            assert nn.convert_image_conv2d_(enc) == (['encoder.0.0'], {})
        conv = enc['encoder'][0][0]
        assert type(conv) is nn.ImageConv2d and conv._forward_hooks and conv.training
        assert nn.convert_image_conv2d_(enc) == ([], {})  # a second call finds nothing
        after_p, after_b = dict(enc.named_parameters()), dict(enc.named_buffers())
        assert after_p.keys() == params.keys() and all(after_p[k] is params[k] for k in params)  # the same Parameter objects
        assert after_b.keys() == buffers.keys() and all(after_b[k] is buffers[k] for k in buffers)
        assert list(enc.state_dict().keys()) == keys
        fresh = torch.nn.ModuleDict(dict(encoder=standin.UNetEncoder(channels)))
        fresh.load_state_dict(enc.state_dict())
        enc.load_state_dict(fresh.state_dict())
        sig = _signature(enc)
        want = want or sig
        assert sig == want
        stock = (torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.MaxPool2d, torch.nn.ReLU)
        assert [name for name, m in enc.named_modules() if type(m) in stock] == []  # no stock operation is left
        with pytest.raises(RuntimeError, match='MI355X'):  # the converted module runs this library's kernels: no CPU fallback
            conv(torch.zeros(2, channels, 8, 8))


@pytest.mark.parametrize('order', standin.ORDERS, ids=lambda o: '-'.join(o[:3]))
def test_all_converts_take_the_whole_net_in_any_order(order):
    for case in standin.CASES.values():
        net = standin.build(case)
        params, keys = dict(net.named_parameters()), list(net.state_dict().keys())
        standin.convert_all_(net, nn, order)
        resized = 1 if case.full_res else 0
        want = {nn.ImageConv2d: 1, nn.MaxPool2d: 2, nn.CatConv2d: 2, nn.ResizedConv2d: resized, nn.Conv2d: 5 + 2 + 2 + 4 - resized,
                nn.BatchNorm2d: 6 + 4 + 4, nn.DropoutConv1x1: 4, cpn_core_standin.ScaledTanh: 1}
        assert standin.census(net) == {k: v for k, v in want.items() if v}
        assert type(net['core']) is nn.CPNCore and type(net['core'].backbone.unet) is nn.UNetDecoder
        after = dict(net.named_parameters())
        assert after.keys() == params.keys() and all(after[k] is params[k] for k in params) and list(net.state_dict().keys()) == keys


def test_roots_shared_slots_and_what_is_left():
    t = torch.nn
    assert nn.convert_image_conv2d_(t.Conv2d(3, 64, 3, 1, 1)) == ([], {'': 'the root module cannot be replaced in place: convert its parent'})
    assert nn.convert_conv2d_(nn.ImageConv2d(3, 64)) == ([], {}) and nn.convert_stem_conv2d_(nn.ImageConv2d(3, 64)) == ([], {})
    conv = t.Conv2d(1, 32, 3, 1, 1)
    both = t.ModuleList([conv, t.Sequential(conv, t.ReLU())])  # a module that sits in two slots stays one object
    assert nn.convert_image_conv2d_(both) == (['0', '1.0'], {})  # (parents first)
    assert both[0] is both[1][0] and type(both[0]) is nn.ImageConv2d and both[0].weight is conv.weight and both[0].bias is conv.bias

    class Own(t.Conv2d):
        pass

    odd = t.ModuleDict(dict(own=Own(3, 64, 3, 1, 1), five=t.Conv2d(5, 64, 3, 1, 1), out=t.Conv2d(3, 16, 3, 1, 1), s2=t.Conv2d(3, 64, 3, 2, 1),
                            pad=t.Conv2d(3, 64, 3, 1, 0), dil=t.Conv2d(3, 64, 3, 1, 1, dilation=2), grp=t.Conv2d(4, 64, 3, 1, 1, groups=2),
                            refl=t.Conv2d(3, 64, 3, 1, 1, padding_mode='reflect'), f16=t.Conv2d(3, 64, 3, 1, 1).half(), k7=t.Conv2d(3, 64, 7, 2, 3),
                            k1=t.Conv2d(3, 64, 1), dense=t.Conv2d(64, 64, 3, 1, 1), tr=t.ConvTranspose2d(3, 64, 3, 1, 1)))
    sig = _signature(odd)
    replaced, left = nn.convert_image_conv2d_(odd)
    # (five channels, another kernel size, a dense conv and a transposed conv are not its business)
    assert replaced == [] and set(left) == {'own', 'out', 's2', 'pad', 'dil', 'grp', 'refl', 'f16'}
    assert left['own'].startswith('a subclass of torch.nn.Conv2d (Own)') and left['out'].startswith('out_channels 16') and \
        left['s2'].startswith('stride (2, 2)') and left['pad'].startswith('padding (0, 0)') and left['dil'].startswith('dilation (2, 2)') and \
        left['grp'].startswith('groups 2') and left['refl'].startswith("padding_mode 'reflect'") and left['f16'].startswith('weight dtype torch.float16')
    assert _signature(odd) == sig
    # the existing converts keep their own reasons for the first conv of a U-Net encoder
    k3 = t.ModuleDict(dict(k3=t.Conv2d(3, 32, 3, 1, 1)))
    assert nn.convert_stem_conv2d_(k3)[1]['k3'].startswith('kernel_size (3, 3)') and 'k3' in nn.convert_conv2d_(k3)[1]
    assert type(k3['k3']) is t.Conv2d
