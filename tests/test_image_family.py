"""CPU tests of what the trainable stem and the trainable image conv share (celldetection_amd/nn/_image_family.py,
csrc/image_train.h) and of the max-pool's unit (csrc/pool_train.hip): every sentence the two families raise for an argument they do
not run, in Python and behind the C entry points, as a literal, and that both modules are bindings of one implementation.  Nothing
here needs a GPU."""
import ctypes
import inspect

import pytest
import torch

import celldetection_amd as cda
from celldetection_amd import _lib

nn = cda.nn


def _raised(kind, call, *args, **kwargs):
    with pytest.raises(kind) as e:
        call(*args, **kwargs)
    assert type(e.value) is kind
    return str(e.value)


class Own(torch.nn.Conv2d):
    pass


def _z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def _flagged_transposed(conv):
    conv.transposed = True  # (a stock ConvTranspose2d is not a Conv2d: the rule's first branch is met by the flag alone)
    return conv


# ---- the Python surface: (call, arguments, keywords, exception, the whole sentence)

def _stem_cases():
    x, w = _z(2, 3, 9, 11), _z(64, 3, 7, 7)
    ctor = lambda **kw: nn.StemConv2d(**{**dict(in_channels=3, out_channels=64), **kw})  # noqa: E731
    N, V = NotImplementedError, ValueError
    return [
        # _unsupported
        (nn.stem._stem_why_not, (_flagged_transposed(torch.nn.Conv2d(3, 64, 7, 2, 3)),), {}, None, 'transposed convs are not run'),
        (ctor, (), dict(kernel_size=3), N, 'kernel_size 3: 7x7 only'),
        (ctor, (), dict(kernel_size=(7, 5)), N, 'kernel_size (7, 5): 7x7 only'),
        (ctor, (), dict(stride=1), N, 'stride 1: stride 2 only'),
        (ctor, (), dict(padding=0), N, 'padding 0: 3 zeros only'),
        (ctor, (), dict(padding='same'), N, 'padding same: 3 zeros only'),
        (ctor, (), dict(dilation=2), N, 'dilation 2: dilation 1 only'),
        (ctor, (), dict(groups=3), N, 'groups 3: dense convs only'),
        (ctor, (), dict(padding_mode='reflect'), N, "padding_mode 'reflect': zeros only"),
        (ctor, (), dict(in_channels=5), N, 'in_channels 5: 1 ... 4 only'),
        (ctor, (), dict(in_channels=0), N, 'in_channels 0: 1 ... 4 only'),
        (ctor, (), dict(out_channels=16), N, 'out_channels 16: (32, 64) only'),
        (ctor, (), dict(out_channels=128), N, 'out_channels 128: (32, 64) only'),
        # _check_input
        (nn.stem_conv2d, (x[0], w), {}, N, 'input of 3 dimensions: the trainable stem takes a 4-D [N, C, H, W] input'),
        (nn.stem_conv2d, (x.double(), w), {}, N, 'input dtype torch.float64: the trainable stem takes float32 or bfloat16 images'),
        (nn.stem_conv2d, (_z(2, 5, 9, 11), _z(64, 5, 7, 7)), {}, N, 'input of 5 channels: the trainable stem takes 1 ... 4'),
        (nn.stem_conv2d, (_z(2, 3, 0, 11), w), {}, N, 'input of size (2, 3, 0, 11): the trainable stem needs at least one pixel'),
        # _check_weight
        (nn.stem_conv2d, (x, w[0]), {}, N, 'weight of 3 dimensions: the trainable stem needs [Cout, C, 7, 7]'),
        (nn.stem_conv2d, (x, _z(64, 3, 7, 5)), {}, N, 'kernel_size (7, 5): the trainable stem runs 7x7 kernels only'),
        (nn.stem_conv2d, (x, w.half()), {}, N, 'weight dtype torch.float16: the trainable stem takes float32 or bfloat16 parameters'),
        (nn.stem_conv2d, (x, _z(64, 5, 7, 7)), {}, N, 'in_channels 5: the trainable stem takes 1 ... 4'),
        (nn.stem_conv2d, (x, _z(48, 3, 7, 7)), {}, N, 'out_channels 48: the trainable stem writes (32, 64) only'),
        (nn.stem_pack_weight, (_z(64, 3, 3, 3),), {}, N, 'kernel_size (3, 3): the trainable stem runs 7x7 kernels only'),
        # bias, channel mismatch, requires_grad
        (nn.stem_conv2d, (x, w, _z(32)), {}, N, 'bias (32,) torch.float32: the trainable stem takes a float32 or bfloat16 [Cout] bias'),
        (nn.stem_conv2d, (x, w, _z(64).double()), {}, N,
         'bias (64,) torch.float64: the trainable stem takes a float32 or bfloat16 [Cout] bias'),
        (nn.stem_conv2d, (x, w, _z(1, 64)), {}, N, 'bias (1, 64) torch.float32: the trainable stem takes a float32 or bfloat16 [Cout] bias'),
        (nn.stem_conv2d, (x, _z(64, 4, 7, 7)), {}, V, 'input has 3 channels, weight expects 4'),
        (nn.stem_conv2d, (x.clone().requires_grad_(True), w), {}, N,
         'x requires a gradient: the trainable stem has no input gradient (the image needs none; detach x)'),
        # the weight gradient's own
        (nn.stem_weight_grad, (_z(2, 5, 9, 11), _z(2, 64, 5, 6)), {}, N, 'input of 5 channels: the trainable stem takes 1 ... 4'),
        (nn.stem_weight_grad, (x, _z(2, 48, 5, 6)), {}, N, 'out_channels 48: the trainable stem writes (32, 64) only'),
        (nn.stem_weight_grad, (x, _z(2, 64, 5, 6)), dict(dtype=torch.float64), N,
         'dtype torch.float64 / torch.float64: gradients are float32 or bfloat16'),
        # the convert's rule
        (nn.stem._stem_why_not, (Own(3, 64, 7, 2, 3),), {}, None, 'a subclass of torch.nn.Conv2d (Own): its forward may differ'),
        (nn.stem._stem_why_not, (torch.nn.Conv2d(3, 64, 7, 2, 3).half(),), {}, None, 'weight dtype torch.float16: float32 or bfloat16 only'),
        (nn.stem._stem_why_not, (torch.nn.Conv2d(3, 64, 7, 2, 2),), {}, None, 'padding (2, 2): 3 zeros only'),
        (nn.stem._stem_why_not, (torch.nn.Conv2d(3, 64, 7, 2, 3),), {}, None, None),
    ]


def _image_cases():
    x, w = _z(2, 3, 9, 11), _z(64, 3, 3, 3)
    ctor = lambda **kw: nn.ImageConv2d(**{**dict(in_channels=3, out_channels=64), **kw})  # noqa: E731
    N, V = NotImplementedError, ValueError
    return [
        # _unsupported
        (nn.image_conv._image_why_not, (_flagged_transposed(torch.nn.Conv2d(3, 64, 3, 1, 1)),), {}, None, 'transposed convs are not run'),
        (ctor, (), dict(kernel_size=7), N, 'kernel_size 7: 3x3 only'),
        (ctor, (), dict(kernel_size=(3, 1)), N, 'kernel_size (3, 1): 3x3 only'),
        (ctor, (), dict(stride=2), N, 'stride 2: stride 1 only'),
        (ctor, (), dict(padding=0), N, 'padding 0: 1 zero only'),
        (ctor, (), dict(padding='same'), N, 'padding same: 1 zero only'),
        (ctor, (), dict(dilation=2), N, 'dilation 2: dilation 1 only'),
        (ctor, (), dict(groups=3), N, 'groups 3: dense convs only'),
        (ctor, (), dict(padding_mode='reflect'), N, "padding_mode 'reflect': zeros only"),
        (ctor, (), dict(in_channels=5), N, 'in_channels 5: 1 ... 4 only'),
        (ctor, (), dict(in_channels=0), N, 'in_channels 0: 1 ... 4 only'),
        (ctor, (), dict(out_channels=16), N, 'out_channels 16: (32, 64, 128) only'),
        (ctor, (), dict(out_channels=256), N, 'out_channels 256: (32, 64, 128) only'),
        # _check_input
        (nn.image_conv2d, (x[0], w), {}, N, 'input of 3 dimensions: the trainable image conv takes a 4-D [N, C, H, W] input'),
        (nn.image_conv2d, (x.double(), w), {}, N, 'input dtype torch.float64: the trainable image conv takes float32 or bfloat16 images'),
        (nn.image_conv2d, (x.half(), w), {}, N, 'input dtype torch.float16: the trainable image conv takes float32 or bfloat16 images'),
        (nn.image_conv2d, (_z(2, 5, 9, 11), _z(64, 5, 3, 3)), {}, N, 'input of 5 channels: the trainable image conv takes 1 ... 4'),
        (nn.image_conv2d, (_z(2, 3, 0, 11), w), {}, N, 'input of size (2, 3, 0, 11): the trainable image conv needs at least one pixel'),
        # _check_weight
        (nn.image_conv2d, (x, w[0]), {}, N, 'weight of 3 dimensions: the trainable image conv needs [Cout, C, 3, 3]'),
        (nn.image_conv2d, (x, _z(64, 3, 3, 1)), {}, N, 'kernel_size (3, 1): the trainable image conv runs 3x3 kernels only'),
        (nn.image_conv2d, (x, w.half()), {}, N, 'weight dtype torch.float16: the trainable image conv takes float32 or bfloat16 parameters'),
        (nn.image_conv2d, (x, _z(64, 5, 3, 3)), {}, N, 'in_channels 5: the trainable image conv takes 1 ... 4'),
        (nn.image_conv2d, (x, _z(48, 3, 3, 3)), {}, N, 'out_channels 48: the trainable image conv writes (32, 64, 128) only'),
        (nn.image_pack_weight, (_z(64, 3, 7, 7),), {}, N, 'kernel_size (7, 7): the trainable image conv runs 3x3 kernels only'),
        # bias, channel mismatch, requires_grad
        (nn.image_conv2d, (x, w, _z(32)), {}, N, 'bias (32,) torch.float32: the trainable image conv takes a float32 or bfloat16 [Cout] bias'),
        (nn.image_conv2d, (x, w, _z(64).double()), {}, N,
         'bias (64,) torch.float64: the trainable image conv takes a float32 or bfloat16 [Cout] bias'),
        (nn.image_conv2d, (x, w, _z(1, 64)), {}, N,
         'bias (1, 64) torch.float32: the trainable image conv takes a float32 or bfloat16 [Cout] bias'),
        (nn.image_conv2d, (x, _z(64, 4, 3, 3)), {}, V, 'input has 3 channels, weight expects 4'),
        (nn.image_conv2d, (x.clone().requires_grad_(True), w), {}, N,
         'x requires a gradient: the trainable image conv has no input gradient (the image needs none; detach x)'),
        # the weight gradient's own
        (nn.image_weight_grad, (_z(2, 5, 9, 11), _z(2, 64, 9, 11)), {}, N, 'input of 5 channels: the trainable image conv takes 1 ... 4'),
        (nn.image_weight_grad, (x, _z(2, 48, 9, 11)), {}, N, 'out_channels 48: the trainable image conv writes (32, 64, 128) only'),
        (nn.image_weight_grad, (x, _z(2, 64, 9, 11)), dict(bias_dtype=torch.float16), N,
         'dtype torch.float32 / torch.float16: gradients are float32 or bfloat16'),
        # the convert's rule
        (nn.image_conv._image_why_not, (Own(3, 64, 3, 1, 1),), {}, None, 'a subclass of torch.nn.Conv2d (Own): its forward may differ'),
        (nn.image_conv._image_why_not, (torch.nn.Conv2d(3, 64, 3, 1, 1).half(),), {}, None,
         'weight dtype torch.float16: float32 or bfloat16 only'),
        (nn.image_conv._image_why_not, (torch.nn.Conv2d(3, 64, 3, 1, 0),), {}, None, 'padding (0, 0): 1 zero only'),
        (nn.image_conv._image_why_not, (torch.nn.Conv2d(3, 64, 3, 1, 1),), {}, None, None),
    ]


@pytest.mark.parametrize('cases', [_stem_cases, _image_cases], ids=['stem', 'image_conv'])
def test_every_python_sentence_is_the_one_it_was(cases):
    table = cases()
    assert len(table) >= 35
    for call, args, kwargs, kind, sentence in table:
        got = call(*args, **kwargs) if kind is None else _raised(kind, call, *args, **kwargs)
        assert got == sentence, (args, kwargs)


# ---- the C entry points: the code and cpn_last_error() of every call the families' own tests make

P, Q = 16, 1 << 40  # an aligned "pointer" that is never read; a workspace size that is always enough
GEOMETRY = {  # (N, H, W, cout, slab_rows) -> (code, what)
    'stem': [((0, 4, 4, 64, 0), 'E_INVALID', 'N, H and W must be at least 1'), ((2, 0, 4, 64, 0), 'E_INVALID', 'N, H and W must be at least 1'),
             ((2, 4, 0, 64, 0), 'E_INVALID', 'N, H and W must be at least 1'), ((2, 4, 4, 48, 0), 'E_INVALID', 'cout must be 32 or 64'),
             ((2, 4, 4, 128, 0), 'E_INVALID', 'cout must be 32 or 64'), ((2, 4, 4, 64, -1), 'E_INVALID', 'slab_rows must be 0 (auto) or positive'),
             ((65536, 65536, 1, 64, 0), 'E_UNSUPPORTED', 'more than 2^31 - 1 pixels in the padded input'),
             ((2, 2 ** 30, 2 ** 30, 64, 0), 'E_UNSUPPORTED', 'more than 2^31 - 1 pixels in the padded input')],
    'image_conv': [((0, 4, 4, 64, 0), 'E_INVALID', 'N, H and W must be at least 1'), ((2, 0, 4, 64, 0), 'E_INVALID', 'N, H and W must be at least 1'),
                   ((2, 4, 0, 64, 0), 'E_INVALID', 'N, H and W must be at least 1'), ((2, 4, 4, 48, 0), 'E_INVALID', 'cout must be 32, 64 or 128'),
                   ((2, 4, 4, 256, 0), 'E_INVALID', 'cout must be 32, 64 or 128'),
                   ((2, 4, 4, 64, -1), 'E_INVALID', 'slab_rows must be 0 (auto) or positive'),
                   ((65536, 65536, 1, 64, 0), 'E_UNSUPPORTED', 'more than 2^31 - 1 pixels in the padded input'),
                   ((2, 2 ** 30, 2 ** 30, 64, 0), 'E_UNSUPPORTED', 'more than 2^31 - 1 pixels in the padded input')],
}
ENTRY = {'stem': dict(forward='cpn_stem_train_forward', pack='cpn_stem_train_pack', pad=None, x='xp'),
         'image_conv': dict(forward='cpn_image_conv_forward', pack='cpn_image_conv_pack', pad='cpn_image_conv_pad', x='xq')}


def _refused(lib, name, *args):
    """-> (the code's name, cpn_last_error()) of a call that must fail."""
    rc = getattr(lib, name)(*args)
    codes = {getattr(_lib, c): c for c in ('E_INVALID', 'E_UNSUPPORTED', 'E_WORKSPACE')}
    assert rc in codes, (name, args, rc)
    return codes[rc], lib.cpn_last_error().decode()


@pytest.mark.parametrize('family', ['stem', 'image_conv'])
def test_every_c_sentence_of_a_family_is_the_one_it_was(family):
    lib, e = _lib.load(), ENTRY[family]
    info, bytes_, launch, forward = (f'cpn_{family}_wgrad_info', f'cpn_{family}_wgrad_workspace_bytes', f'cpn_{family}_wgrad', e['forward'])
    out = (ctypes.c_int32 * 5)()
    for bad, code, what in GEOMETRY[family]:
        assert _refused(lib, info, *bad, out) == (code, f'{info}: {what}'), bad
        assert getattr(lib, bytes_)(*bad) == 0 and lib.cpn_last_error().decode() == f'{bytes_}: {what}', bad
        assert _refused(lib, launch, P, P, *bad[:3], 3, *bad[3:], P, 0, P, 0, P, Q, None) == (code, f'{launch}: {what}'), bad
        if bad[4] == 0:
            assert _refused(lib, forward, P, P, None, *bad[:4], P, None) == (code, f'{forward}: {what}'), bad
            if e['pad'] and 'cout' not in what:
                assert _refused(lib, e['pad'], P, bad[0], 3, bad[1], bad[2], P, None) == (code, f"{e['pad']}: {what}"), bad
    ok, x = (2, 4, 4), e['x']
    singles = [
        ((info, *ok, 64, 0, None), 'E_INVALID', f'{info}: null pointer'),
        ((launch, P, P, *ok, 3, 64, 0, P, 0, P, 0, P, 16, None), 'E_WORKSPACE', f'{launch}: workspace smaller than {bytes_}'),
        ((launch, P, P, *ok, 0, 64, 0, P, 0, P, 0, P, Q, None), 'E_INVALID', f'{launch}: cin must lie in 1 ... 4'),
        ((launch, P, P, *ok, 5, 64, 0, P, 0, P, 0, P, Q, None), 'E_INVALID', f'{launch}: cin must lie in 1 ... 4'),
        ((launch, None, P, *ok, 3, 64, 0, P, 0, P, 0, P, Q, None), 'E_INVALID', f'{launch}: null pointer'),
        ((launch, P, None, *ok, 3, 64, 0, P, 0, P, 0, P, Q, None), 'E_INVALID', f'{launch}: null pointer'),
        ((launch, P, P, *ok, 3, 64, 0, P, 0, P, 0, None, Q, None), 'E_INVALID', f'{launch}: null pointer'),
        ((launch, P, P, *ok, 3, 64, 0, None, 0, None, 0, P, Q, None), 'E_INVALID', f'{launch}: null pointer'),  # nothing to compute
        ((launch, P, 8, *ok, 3, 64, 0, P, 0, P, 0, P, Q, None), 'E_INVALID',
         f'{launch}: {x}, dy and workspace must start at 16-byte aligned addresses'),
        ((launch, P, P, *ok, 3, 64, 0, P, 2, P, 0, P, Q, None), 'E_INVALID', f'{launch}: an output dtype must be 0 (fp32) or 1 (bf16)'),
        ((launch, P, P, *ok, 3, 64, 0, P, 0, P, -1, P, Q, None), 'E_INVALID', f'{launch}: an output dtype must be 0 (fp32) or 1 (bf16)'),
        ((forward, None, P, None, *ok, 64, P, None), 'E_INVALID', f'{forward}: null pointer'),
        ((forward, P, P, None, *ok, 64, None, None), 'E_INVALID', f'{forward}: null pointer'),
        ((forward, P, 24, None, *ok, 64, P, None), 'E_INVALID', f'{forward}: {x}, packed and y must start at 16-byte aligned addresses'),
        # the pack: (weight, dtype, cout, cin, packed)
        ((e['pack'], P, 0, 48, 3, P, None), 'E_INVALID', f"{e['pack']}: {GEOMETRY[family][3][2]}"),
        ((e['pack'], P, 0, 64, 0, P, None), 'E_INVALID', f"{e['pack']}: cin must lie in 1 ... 4"),
        ((e['pack'], P, 0, 64, 5, P, None), 'E_INVALID', f"{e['pack']}: cin must lie in 1 ... 4"),
        ((e['pack'], P, 2, 64, 3, P, None), 'E_INVALID', f"{e['pack']}: weight_dtype must be 0 (fp32) or 1 (bf16)"),
        ((e['pack'], None, 0, 64, 3, P, None), 'E_INVALID', f"{e['pack']}: null pointer"),
        ((e['pack'], P, 0, 64, 3, None, None), 'E_INVALID', f"{e['pack']}: null pointer"),
    ]
    if e['pad']:  # (src, N, C, H, W, xq)
        pad = e['pad']
        singles += [((pad, P, 2, 0, 4, 4, P, None), 'E_INVALID', f'{pad}: C must lie in 1 ... 4'),
                    ((pad, P, 2, 5, 4, 4, P, None), 'E_INVALID', f'{pad}: C must lie in 1 ... 4'),
                    ((pad, None, 2, 3, 4, 4, P, None), 'E_INVALID', f'{pad}: null pointer'),
                    ((pad, P, 2, 3, 4, 4, None, None), 'E_INVALID', f'{pad}: null pointer'),
                    ((pad, P, 2, 3, 4, 4, 8, None), 'E_INVALID', f'{pad}: src must start at a 4-byte, xq at a 16-byte aligned address'),
                    ((pad, 18, 2, 3, 4, 4, P, None), 'E_INVALID', f'{pad}: src must start at a 4-byte, xq at a 16-byte aligned address')]
    for call, code, sentence in singles:
        assert _refused(lib, *call) == (code, sentence), call


def test_every_c_sentence_of_the_pool_is_the_one_it_was():
    lib = _lib.load()
    # (dtype, N, H, W, C, k, stride, pad)
    table = [((1, 0, 4, 4, 8, 3, 2, 1), 'E_INVALID', 'N, H and W must be at least 1'),
             ((1, 2, 4, 4, 12, 3, 2, 1), 'E_INVALID', 'C must be a positive multiple of 8'),
             ((0, 2, 4, 4, 12, 2, 2, 0), 'E_INVALID', 'C must be a positive multiple of 8'),
             ((1, 2, 4, 4, 0, 3, 2, 1), 'E_INVALID', 'C must be a positive multiple of 8'),
             ((2, 2, 4, 4, 8, 3, 2, 1), 'E_INVALID', 'dtype must be 0 (fp32) or 1 (bf16)'),
             ((2, 2, 4, 4, 8, 2, 2, 0), 'E_INVALID', 'dtype must be 0 (fp32) or 1 (bf16)'),
             ((1, 2, 4, 4, 8, 3, 1, 1), 'E_INVALID', '(k, stride, pad) must be (3, 2, 1) or (2, 2, 0)'),
             ((1, 2, 4, 4, 8, 2, 2, 1), 'E_INVALID', '(k, stride, pad) must be (3, 2, 1) or (2, 2, 0)'),
             ((1, 2, 4, 4, 8, 3, 2, 0), 'E_INVALID', '(k, stride, pad) must be (3, 2, 1) or (2, 2, 0)'),
             ((1, 2, 1, 4, 8, 2, 2, 0), 'E_INVALID', 'H and W must hold at least one window'),
             ((1, 2, 4, 1, 8, 2, 2, 0), 'E_INVALID', 'H and W must hold at least one window'),
             ((1, 2, 1, 1, 8, 2, 2, 0), 'E_INVALID', 'H and W must hold at least one window'),
             ((0, 2, 1, 1, 8, 2, 2, 0), 'E_INVALID', 'H and W must hold at least one window'),
             ((1, 65536, 65536, 1, 8, 3, 2, 1), 'E_UNSUPPORTED', 'more than 2^31 - 1 pixels or workgroups')]
    fwd, bwd = 'cpn_maxpool2d_indexed', 'cpn_maxpool2d_backward'
    for bad, code, what in table:
        assert _refused(lib, fwd, P, *bad, P, P, None) == (code, f'{fwd}: {what}'), bad
        assert _refused(lib, bwd, P, P, *bad, P, None) == (code, f'{bwd}: {what}'), bad
    good = (1, 2, 4, 4, 8, 3, 2, 1)
    for call, sentence in (((fwd, None, *good, P, P, None), f'{fwd}: null pointer'), ((fwd, P, *good, None, P, None), f'{fwd}: null pointer'),
                           ((fwd, P, *good, P, 8, None), f'{fwd}: x, y and index must start at 16-byte aligned addresses'),
                           ((bwd, P, None, *good, P, None), f'{bwd}: null pointer'), ((bwd, P, P, *good, None, None), f'{bwd}: null pointer'),
                           ((bwd, 24, P, *good, P, None), f'{bwd}: dy, index and dx must start at 16-byte aligned addresses')):
        assert _refused(lib, *call) == ('E_INVALID', sentence), call


# ---- one implementation

def test_both_modules_bind_one_implementation():
    from celldetection_amd.nn import _image_family as family
    stem, image = nn.stem, nn.image_conv
    assert stem._StemConv2dFunction is image._ImageConv2dFunction is family.ImageConv2dFunction
    assert stem.STEM != image.IMAGE and type(stem.STEM) is type(image.IMAGE) is family.ImageFamily
    for a, b, shared in ((stem._stem_pad, image._image_pad, family.pad), (stem._stem_forward, image._image_forward, family.run_forward),
                         (stem._stem_wgrad, image._image_wgrad, family.wgrad), (stem._stem_why_not, image._image_why_not, family.why_not)):
        assert a.func is b.func is shared and a.args == (stem.STEM,) and b.args == (image.IMAGE,)
    assert nn.StemConv2d.forward is nn.ImageConv2d.forward is family.ImageFamilyConv2d.forward
    assert nn.StemConv2d.family is stem.STEM and nn.ImageConv2d.family is image.IMAGE
    # neither module holds a rule, a check or a launch of its own: apart from the bindings above, its functions and its module's
    # __init__ call the shared module and nothing else of this package
    for module in (stem, image):
        own = [f for f in vars(module).values() if inspect.isfunction(f) and f.__module__ == module.__name__]
        own += [module.StemConv2d.__init__ if module is stem else module.ImageConv2d.__init__]
        assert len(own) == 6
        for f in own:
            assert not {'_lib', '_need_cuda', '_weight_grad', '_weight_grad_info', '_DTYPES', 'NotImplementedError'} & set(f.__code__.co_names), f
    assert (stem.STEM.kernel, stem.STEM.stride, stem.STEM.padding, stem.STEM.out_channels, stem.STEM.pad_rows, stem.STEM.pad_cols,
            stem.STEM.record, stem.STEM.max_in_channels) == (7, 2, 3, nn.STEM_OUT_CHANNELS, 6, 8, 32, nn.STEM_MAX_IN_CHANNELS)
    assert (image.IMAGE.kernel, image.IMAGE.stride, image.IMAGE.padding, image.IMAGE.out_channels, image.IMAGE.pad_rows, image.IMAGE.pad_cols,
            image.IMAGE.record, image.IMAGE.max_in_channels) == (3, 1, 1, nn.IMAGE_OUT_CHANNELS, 2, 3, 16, nn.IMAGE_MAX_IN_CHANNELS)
