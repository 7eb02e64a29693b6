"""A whole stand-in network for the training-step tests, assembled from the existing stand-ins (test helper, not a conftest): the
ResNeXt-style encoder of ``test_bottleneck.Block``s, the decoder of tests/unet_standin.py and the core of tests/cpn_core_standin.py::

    stem    Conv 7x7 s2 C->64 (no bias) - BN - ReLU                     -> '0' (64, stride 2)
    pool    MaxPool2d(3, 2, 1)
    layer1  Block(64,128,32,1,64,'conv'), Block(64,128,32,1,64,None)    -> '1' (64, stride 4)
    layer2  Block(64,128,32,2,128,'conv'), Block(128,128,32,1,128,None) -> '2' (128, stride 8)
    unet    unet_standin.Decoder() on {'0', '1', '2'}
    core    cpn_core_standin.Core(order=3, score_channels=1); the score, location and fourier heads read the decoder's '0' (32
            channels at the image's size), the refinement head the decoder's '1' (64 channels at half the size)

Every ReLU is made out of place: the values are the same, and every leaf module's operand survives its call, so that a recorded call
can be run again on what it saw.  All nine converts take the net completely (``convert_all_``); ``census`` is what they leave.  The topology -- which tensor has
which consumers -- is written out by hand at the end of this file, for the converted net and for the stock one.

The two cases keep every edge at the smallest size.  A: N = 2, 3x44x52, ``refinement_full_res``: the strides give 22x26, 11x13 and
6x7, so the strided convs take the ceil, the nearest resize 6x7 -> 11x13 is not x2, and the ``ResizedConv2d`` enlarges 22x26 ->
44x52.  B: N = 1, one input channel, 38x50, no full-resolution refinement: 19x25, 10x13, 5x7, and the head map goes through
``bilinear_resize`` on fp32 planes.
"""
import collections
import functools

import numpy as np
import torch

import cpn_core_standin
import unet_standin
from test_bottleneck import Block

ORDER, SAMPLES = 3, 8
Case = collections.namedtuple('Case', 'name n channels h w full_res')
CASES = {'A': Case('A', 2, 3, 44, 52, True), 'B': Case('B', 1, 1, 38, 50, False)}


class Encoder(torch.nn.Module):
    """The backbone: stem, pool, two stages of two blocks, the decoder -> the decoder's dict."""

    def __init__(self, in_channels=3):
        super().__init__()
        t = torch.nn
        self.stem = t.Sequential(t.Conv2d(in_channels, 64, 7, stride=2, padding=3, bias=False), t.BatchNorm2d(64), t.ReLU())
        self.pool = t.MaxPool2d(3, 2, 1)
        self.layer1 = t.Sequential(Block(64, 128, 32, 1, 64, 'conv'), Block(64, 128, 32, 1, 64, None))
        self.layer2 = t.Sequential(Block(64, 128, 32, 2, 128, 'conv'), Block(128, 128, 32, 1, 128, None))
        self.unet = unet_standin.Decoder()

    def forward(self, x):
        f0 = self.stem(x)
        f1 = self.layer1(self.pool(f0))
        f2 = self.layer2(f1)
        return self.unet({'0': f0, '1': f1, '2': f2})


def build(case, p=0., seed=1):
    """The stock net of a case in float32 on the CPU, in training mode, as ``ModuleDict(core=...)`` (a convert cannot replace the
    root), with randomised norms.  ``p``: the heads' dropout."""
    torch.manual_seed(seed)
    core = cpn_core_standin.Core(order=ORDER, score_channels=1, refinement_full_res=case.full_res)
    core.backbone = Encoder(case.channels)
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
    """name -> convert, the nine of them."""
    return dict(conv=nn.convert_conv2d_, bn=nn.convert_batchnorm2d_, tail=nn.convert_readout_tail_, grouped=nn.convert_grouped_conv2d_,
                stem=nn.convert_stem_conv2d_, pool=nn.convert_maxpool2d_, block=nn.convert_bottleneck_, unet=nn.convert_unet_decoder_,
                core=nn.convert_cpn_core_)


TAILS = ['core.%s_head.block.4' % h for h in ('score', 'location', 'fourier', 'refinement')]


ORDER_OF_CONVERTS = ('stem', 'pool', 'grouped', 'block', 'unet', 'core', 'bn', 'conv', 'tail')


def convert_all_(net, nn, order=ORDER_OF_CONVERTS):
    """Runs the nine converts in ``order`` -> {name: what the convert returned}.  In the default order every convert reports nothing
    left, except that ``convert_conv2d_`` names the four ReadOut tails, which ``convert_readout_tail_`` then takes.  In any other
    order ``convert_conv2d_`` and ``convert_readout_tail_`` also name the convs a family that has not run yet will take: whatever
    a convert names as left must be a module of this library in the end."""
    table = converts(nn)
    assert sorted(order) == sorted(table)
    results = {name: table[name](net) for name in order}
    ours = tuple(census(CASES['A'], nn))
    for name in order:
        left = results[name][-1]
        if tuple(order) == ORDER_OF_CONVERTS:
            assert sorted(left) == (sorted(TAILS) if name == 'conv' else []), (name, left)
        assert name in ('conv', 'tail') or left == {}, (name, left)
        assert all(isinstance(net.get_submodule(n), ours) for n in left), (name, left)
    return results


def census(case, nn):
    """type -> how many modules of exactly that type the converted net of a case holds."""
    resized = 1 if case.full_res else 0  # (without full-resolution refinement slot 0 of that head stays a plain Conv2d)
    return {nn.CPNCore: 1, nn.UNetDecoder: 1, nn.Bottleneck: 4, nn.StemConv2d: 1, nn.MaxPool2d: 1, nn.GroupedConv2d: 4,
            nn.StridedConv1x1: 1, nn.CatConv2d: 3, nn.ResizedConv2d: resized, nn.Conv2d: 18 - resized, nn.BatchNorm2d: 25,
            nn.DropoutConv1x1: 4}


def bf16_exact(*shape, seed, scale=1.):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).float()


def image(case):
    return bf16_exact(case.n, case.channels, case.h, case.w, seed=9)


def map_shapes(case):
    """(scores, locations, refinement, fourier): all at the image's size, the decoder's level 0."""
    return [(case.n, c, case.h, case.w) for c in (1, 2, 2, ORDER * 4)]


def cotangents(case):
    """Fixed bf16-exact gradients of the four maps."""
    return [bf16_exact(*shape, seed=20 + i) for i, shape in enumerate(map_shapes(case))]


def label_images(case):
    """One label image per batch entry with a few discs, int32 [H, W]."""
    yy, xx = np.mgrid[:case.h, :case.w]
    discs = (((10, 11, 7), (26, 36, 8), (29, 10, 6)), ((13, 15, 8), (26, 35, 9)))  # inside 38 x 50, the smaller image
    out = []
    for i in range(case.n):
        lab = np.zeros((case.h, case.w), np.int32)
        for j, (cy, cx, r) in enumerate(discs[i % 2]):
            lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = j + 1
        out.append(lab)
    return out


@functools.lru_cache(maxsize=None)
def stock_results(name, kind):
    """(maps, parameter gradients) of the stock net of a case with p = 0 on the CPU: 'fp64', 'fp32' or 'bf16' (CPU autocast), once."""
    case = CASES[name]
    net, x, cots = build(case), image(case), cotangents(case)
    if kind == 'fp64':
        return run(net.double(), x.double(), cots)
    if kind == 'fp32':
        return run(net, x, cots)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        return run(net, x, cots)


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


# ---- the topology, stated by hand: what the recorder finds is held against it

B = 'core.backbone.'
HEADS = ('score', 'location', 'fourier', 'refinement')


def head(name, slot):
    return f'core.{name}_head.block.{slot}'


def fan_out_converted():
    """{(producer, call, output): [(consumer, call, operand key)]} of every tensor with more than one consumer in the converted
    net, the consumers in the order they run.  (Inside a block the input has ONE consumer, conv1, whose second output is the skip.)"""
    return {
        (B + 'stem.1', 0, 0): [(B + 'pool', 0, 0), (B + 'unet.layer_blocks.1.0', 0, 0)],  # the pool and the lateral of level 1
        (B + 'layer1.1.bn3', 0, 0): [(B + 'layer2.0.conv1', 0, 0), (B + 'unet.layer_blocks.2.0', 0, 0)],  # next stage, lateral of 2
        (B + 'unet.layer_blocks.1.4', 0, 0): [(B + 'unet.inner_blocks.0', 0, 0), (head('refinement', 0), 0, 0)],
        (B + 'unet.layer_blocks.0.4', 0, 0): [(head(h, 0), 0, 0) for h in HEADS[:3]],
    }


def routes_converted():
    """[(producer, consumer)] of every handoff between two families that the decoder, the blocks and the core make: the fan-outs
    above, the tops of the three levels, the skips of the four blocks, the pool and the stage boundaries."""
    routes = [(p, c) for p, consumers in fan_out_converted().items() for c in consumers]
    u = B + 'unet.'
    routes += [((u + 'inner_blocks.2', 0, 0), (u + 'layer_blocks.2.0', 0, 1)), ((u + 'layer_blocks.2.4', 0, 0), (u + 'layer_blocks.1.0', 0, 1)),
               ((u + 'inner_blocks.0', 0, 0), (u + 'layer_blocks.0.0', 0, 1)), ((B + 'layer2.1.bn3', 0, 0), (u + 'inner_blocks.2', 0, 0)),
               ((B + 'pool', 0, 0), (B + 'layer1.0.conv1', 0, 0)), ((B + 'layer1.0.bn3', 0, 0), (B + 'layer1.1.conv1', 0, 0)),
               ((B + 'layer2.0.bn3', 0, 0), (B + 'layer2.1.conv1', 0, 0))]
    for block, down in (('layer1.0', True), ('layer1.1', False), ('layer2.0', True), ('layer2.1', False)):
        skip = (B + block + '.conv1', 0, 1)
        if down:
            routes += [(skip, (B + block + '.downsample.0', 0, 0)), ((B + block + '.downsample.1', 0, 0), (B + block + '.bn3', 0, 'residual'))]
        else:
            routes.append((skip, (B + block + '.bn3', 0, 'residual')))
    return routes


def _adjoint(fn, shape, g):
    leaf = torch.zeros(shape, dtype=g.dtype, requires_grad=True)
    return torch.autograd.grad(fn(leaf), leaf, g)[0]


def fan_out_stock(rec, case):
    """[(name, the gradient the producer received, [the shares of its consumers])] of the stock net.  Where a consumer reads the
    tensor through a stock function (the concat, a resize, the block's in-place add), its share is that function's fp64 adjoint of
    what the next recorded module sent back."""
    import torch.nn.functional as F

    def sent(name, index=0, key=0):
        return rec.get(name, index).grad_in[key]

    def received(name, index=0):
        return rec.get(name, index).grad_out[0]

    u = B + 'unet.'
    level1 = rec[u + 'layer_blocks.1.5'].outputs[0].shape
    to_refinement = sent(head('refinement', 0))
    if case.full_res:
        to_refinement = _adjoint(lambda t: F.interpolate(t, size=(case.h, case.w), mode='bilinear', align_corners=False), level1, to_refinement)
    return [
        ('stem', received(B + 'stem.2'), [sent(B + 'pool'), sent(u + 'layer_blocks.1.0')[:, :64]]),
        ('pool', received(B + 'pool'), [sent(B + 'layer1.0.conv1'), sent(B + 'layer1.0.downsample.0')]),
        ('layer1.0', received(B + 'layer1.0.relu', 2), [sent(B + 'layer1.1.conv1'), received(B + 'layer1.1.bn3')]),
        ('layer1.1', received(B + 'layer1.1.relu', 2), [sent(B + 'layer2.0.conv1'), sent(B + 'layer2.0.downsample.0'),
                                                        sent(u + 'layer_blocks.2.0')[:, :64]]),
        ('layer2.0', received(B + 'layer2.0.relu', 2), [sent(B + 'layer2.1.conv1'), received(B + 'layer2.1.bn3')]),
        ('decoder level 1', received(u + 'layer_blocks.1.5'),
         [_adjoint(lambda t: F.interpolate(t, scale_factor=2, mode='nearest'), level1, sent(u + 'inner_blocks.0')), to_refinement]),
        ('decoder level 0', received(u + 'layer_blocks.0.5'), [sent(head(h, 0)) for h in HEADS[:3]]),
    ]


def laterals_stock(rec):
    """[(name, what the level's first conv saw of the lateral, what the encoder wrote)] of the stock net."""
    u = B + 'unet.'
    return [('lateral of level 1', rec[u + 'layer_blocks.1.0'].operands[0][:, :64], rec[B + 'stem.2'].outputs[0]),
            ('lateral of level 2', rec[u + 'layer_blocks.2.0'].operands[0][:, :64], rec.get(B + 'layer1.1.relu', 2).outputs[0])]
