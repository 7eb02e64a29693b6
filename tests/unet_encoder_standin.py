"""A stand-in for the reference's ``UNetEncoder`` (``models/unet.py:29-58``), written from torch ops, and a small whole net on top of
it (test helper, not a conftest).  The reference itself is neither needed nor imported.

The encoder is an ``nn.Sequential`` of levels: level 0 is ``TwoConvNormRelu(in_channels, base)`` -- conv3x3 - BatchNorm - ReLU -
conv3x3 - BatchNorm - ReLU, the first conv on the image itself --, every further level ``Sequential(MaxPool2d(2, 2),
TwoConvNormRelu(c, 2 c))``.  With depth 3 and base 32 it writes 32 / 64 / 128 channels at strides 1 / 2 / 4.

The whole net (``build``) is that encoder, a two-level decoder made of ``unet_standin.Decoder`` (no bridge level: both levels have a
lateral) and the core of tests/cpn_core_standin.py, whose score, location and fourier heads read the decoder's '0' (32 channels at
the image's size) and whose refinement head reads '1' (64 channels at half the size)::

    level 1: lateral f1 (64), top = inner_blocks[1] = Conv 1x1 128 -> 64 of f2 resized;   block 128 -> 64
    level 0: lateral f0 (32), top = inner_blocks[0] = Conv 1x1 64 -> 32 of level 1 resized; block 64 -> 32

The two cases keep every pool odd.  A: N = 2, 3x22x26: 11x13, 5x6, so both pools drop a row or a column and the nearest resizes are
not x2.  B: N = 1, one input channel, 19x25: 9x12, 4x6.
"""
import collections

import torch

import cpn_core_standin
import unet_standin

ORDER = 3
Case = collections.namedtuple('Case', 'name n channels h w full_res')
CASES = {'A': Case('A', 2, 3, 22, 26, True), 'B': Case('B', 1, 1, 19, 25, False)}


class TwoConvNormRelu(torch.nn.Sequential):
    """The reference's level block: a SUBCLASS of ``nn.Sequential`` with a constructor of its own and no ``forward`` of its own."""

    def __init__(self, cin, cout, stride=1):
        t = torch.nn
        super().__init__(t.Conv2d(cin, cout, 3, padding=1, stride=stride), t.BatchNorm2d(cout), t.ReLU(inplace=True),
                         t.Conv2d(cout, cout, 3, padding=1), t.BatchNorm2d(cout), t.ReLU(inplace=True))


class UNetEncoder(torch.nn.Sequential):
    def __init__(self, in_channels, depth=3, base_channels=32, factor=2):
        layers, self.out_channels = [], []
        for i in range(depth):
            cin = in_channels if i == 0 else base_channels * factor ** (i - 1)
            cout = base_channels * factor ** i
            self.out_channels.append(cout)
            block = TwoConvNormRelu(cin, cout)
            layers.append(block if i == 0 else torch.nn.Sequential(torch.nn.MaxPool2d(2, stride=2), block))
        super().__init__(*layers)


def decoder():
    """``unet_standin.Decoder`` with two levels, both with a lateral, for encoder features of 32 / 64 / 128 channels."""
    t = torch.nn
    dec = unet_standin.Decoder()
    dec.inner_blocks = t.ModuleList([t.Conv2d(64, 32, 1), t.Conv2d(128, 64, 1)])
    dec.layer_blocks = t.ModuleList([unet_standin.block(64, 32), unet_standin.block(128, 64)])
    dec.has_lat, dec.bridges, dec.depth = {0: True, 1: True}, 0, 2
    return dec


class Backbone(torch.nn.Module):
    """The encoder's levels one by one, their outputs as the decoder's laterals -> the decoder's dict."""

    def __init__(self, in_channels=3):
        super().__init__()
        self.encoder = UNetEncoder(in_channels)
        self.unet = decoder()

    def forward(self, x):
        features = {}
        for i, level in enumerate(self.encoder):
            x = level(x)
            features[str(i)] = x
        return self.unet(features)


def build(case, p=0., seed=1):
    """The stock net of a case in float32 on the CPU, in training mode, as ``ModuleDict(core=...)`` (a convert cannot replace the
    root), with randomised norms and out-of-place ReLUs (every leaf's operand survives its call).  ``p``: the heads' dropout."""
    torch.manual_seed(seed)
    core = cpn_core_standin.Core(order=ORDER, score_channels=1, refinement_full_res=case.full_res)
    core.backbone = Backbone(case.channels)
    read = cpn_core_standin.ReadOut
    core.score_head, core.location_head = read(32, 1, 7, dropout=p), read(32, 2, 7, dropout=p)
    core.fourier_head = read(32, ORDER * 4, 7, dropout=p)
    core.refinement_head = read(64, 2, 7, cpn_core_standin.ScaledTanh(3.), dropout=p)
    core.score_features = core.location_features = core.contour_features = '0'
    core.refinement_features = '1'
    net = torch.nn.ModuleDict(dict(core=core))
    for m in net.modules():
        if isinstance(m, torch.nn.ReLU):
            m.inplace = False
    return cpn_core_standin.randomise_(net, seed + 1).train()


def converts(nn):
    """name -> convert, the eight this net needs."""
    return dict(image=nn.convert_image_conv2d_, conv=nn.convert_conv2d_, bn=nn.convert_batchnorm2d_, tail=nn.convert_readout_tail_,
                pool=nn.convert_maxpool2d_, unet=nn.convert_unet_decoder_, core=nn.convert_cpn_core_, stem=nn.convert_stem_conv2d_)


ORDERS = (('image', 'pool', 'unet', 'core', 'bn', 'conv', 'tail', 'stem'), ('tail', 'conv', 'bn', 'core', 'unet', 'pool', 'stem', 'image'),
          ('stem', 'conv', 'image', 'bn', 'tail', 'unet', 'pool', 'core'))


def convert_all_(net, nn, order=ORDERS[0]):
    table = converts(nn)
    assert sorted(order) == sorted(table)
    return {name: table[name](net) for name in order}


def census(net):
    """{type: count} of every childless module of the net but ``Identity``."""
    found = collections.Counter(type(m) for m in net.modules() if next(m.children(), None) is None and type(m) is not torch.nn.Identity)
    return dict(found)


def bf16_exact(*shape, seed, scale=1.):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).float()


def image(case):
    return bf16_exact(case.n, case.channels, case.h, case.w, seed=9)


def cotangents(case):
    """Fixed bf16-exact gradients of the four maps (scores, locations, refinement, fourier), all at the image's size."""
    return [bf16_exact(case.n, c, case.h, case.w, seed=20 + i) for i, c in enumerate((1, 2, 2, ORDER * 4))]


def run(net, x, cots=None):
    """Forward and, with ``cots``, backward -> (the four maps, detached; {parameter name: gradient})."""
    for p in net.parameters():
        p.grad = None
    scores, locations, refinement, fourier, uncertainty = net['core'](x)
    assert uncertainty is None
    maps = [scores, locations, refinement, fourier]
    if cots is not None:
        torch.autograd.backward(maps, [c.to(m.dtype) for c, m in zip(cots, maps)])
    return [m.detach() for m in maps], {name: p.grad for name, p in net.named_parameters()}
