"""A stand-in for the reference's U-Net decoder, written from torch ops (test helper, not a conftest).  Its ``forward`` carries the
names of ``celldetection.models.unet.GeneralizedUNet.forward`` -- what ``cda.nn.convert_unet_decoder_`` recognises a candidate by;
the reference itself is neither needed nor imported.  tests/test_cat_conv.py pins it in float64 to
``oracle.cpn_oracle._generalized_unet`` on its own ``state_dict`` before anything is converted.

Default geometry: three encoder features of (64, 64, 128) channels at strides (2, 4, 8), hence one bridge level::

    level 2: lateral x[1] (64), top = inner_blocks[2] = Conv 1x1 128 -> 64 of x[2]; block 128 -> 64
    level 1: lateral x[0] (64), top = inner_blocks[1] = Identity;                   block 128 -> 64
    level 0: no lateral (bridge, x2),  top = inner_blocks[0] = Conv 1x1 64 -> 32;    block  32 -> 32

A block is conv3x3 - BatchNorm - ReLU - conv3x3 - BatchNorm - ReLU (slots 0 ... 5), the first conv without bias, held by
``TwoConvNormRelu``, a subclass of ``nn.Sequential`` without a forward of its own, as in the reference.
"""
import torch
import torch.nn.functional as F

FEATURES = ((64, 2), (64, 4), (128, 8))  # (channels, stride) of the encoder features


class TwoConvNormRelu(torch.nn.Sequential):
    """The shape of the reference's level block: a SUBCLASS of ``nn.Sequential`` with a constructor of its own and no ``forward`` of
    its own (commons.py:120 of the reference)."""

    def __init__(self, cin, cout, k=3):
        t = torch.nn
        super().__init__(t.Conv2d(cin, cout, k, padding=k // 2, bias=False), t.BatchNorm2d(cout), t.ReLU(inplace=True),
                         t.Conv2d(cout, cout, 3, padding=1), t.BatchNorm2d(cout), t.ReLU(inplace=True))


class OwnForward(TwoConvNormRelu):
    """A Sequential subclass WITH a forward of its own: calling its slots one by one would not be what it computes."""

    def forward(self, x):
        return super().forward(x) * 2


block = TwoConvNormRelu


def _forward(self, x, size=None):
    features, names, x = x, list(x.keys()), list(x.values())
    last = x[-1]
    results = [last]
    for i in reversed(range(self.depth)):
        lateral = x[i - self.bridges] if self.has_lat[i] else None
        kw = dict(scale_factor=2) if lateral is None else dict(size=lateral.shape[2:])
        top = self.inner_blocks[i](F.interpolate(last, mode=self.interpolate, **kw))  # resize first, then the inner conv
        if lateral is None:
            inp = top
        else:
            inp = torch.cat((lateral, top) if self.cat_order == 0 else (top, lateral), 1)
        last = self.layer_blocks[i](inp)
        results.insert(0, last)
    final = results[0] if size is None else F.interpolate(last, size=size, mode=self.final_interpolate, align_corners=False)
    if self.out_layer is not None:
        final = self.out_layer(final)
    if self.final_activation is not None:
        final = self.final_activation(final)
    if self.out_layer is not None:
        return final
    out = dict(zip(['out'] + names, [final] + results))
    if self.keep_features:
        out.update({f'{self.features_prefix}.{k}': v for k, v in features.items()})
    return out


# what marks the reference's function
_forward.__module__, _forward.__qualname__ = 'celldetection.models.unet', 'GeneralizedUNet.forward'


class Decoder(torch.nn.Module):
    def __init__(self, k=3, out_channels=0, **flags):
        super().__init__()
        t = torch.nn
        self.inner_blocks = t.ModuleList([t.Conv2d(64, 32, 1), t.Identity(), t.Conv2d(128, 64, 1)])
        self.layer_blocks = t.ModuleList([block(32, 32, k), block(128, 64, k), block(128, 64, k)])
        self.has_lat, self.bridges, self.depth = {0: False, 1: True, 2: True}, 1, 3
        self.interpolate, self.cat_order = 'nearest', 0
        self.block_cat = self.block_interpolate = self.bridge_block_interpolate = False
        self.extra_blocks = None
        self.out_layer = t.Conv2d(32, out_channels, 1) if out_channels else None
        self.final_interpolate, self.final_activation = 'bilinear', None
        self.keep_features, self.features_prefix = True, 'encoder'
        for name, v in flags.items():
            setattr(self, name, v)

    forward = _forward


class SameNames(Decoder):
    """The same attributes, a forward of its own: not the reference's decoder."""

    def forward(self, x, size=None):
        return _forward(self, x, size)


def features(n, h, w, dtype=torch.float32, seed=0, device='cpu'):
    """Encoder features for an image of h x w: strides 2, 4, 8 by the rule of a stride-2 conv with padding (ceil halves)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for i, (c, s) in enumerate(FEATURES):
        fh, fw = h, w
        for _ in range(s.bit_length() - 1):
            fh, fw = (fh + 1) // 2, (fw + 1) // 2
        out[str(i)] = torch.randn(n, c, fh, fw, generator=g).to(torch.bfloat16).to(dtype).to(device)
    return out


def randomise_(module, seed=0):
    """Running statistics and affine parameters away from their initial 0 / 1, so that the norms matter."""
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.modules.batchnorm._NormBase):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * .1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + .5)
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.num_features, generator=g) + .5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * .1)
    return module
