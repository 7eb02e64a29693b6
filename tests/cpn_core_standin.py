"""A stand-in for the reference's ``CPNCore``, written from torch ops (test helper, not a conftest).  Its ``forward`` carries the names
of ``celldetection.models.cpn.CPNCore.forward`` -- what ``cda.nn.convert_cpn_core_`` recognises a candidate by; the reference itself
is neither needed nor imported.  tests/test_bilinear_resize.py pins it in float64 to the stock expression written out there.

Geometry: the backbone turns an image ``[N, 3, H, W]`` into two features of 32 channels at half the size (a 7x7 stride-2 stem with
norm and ReLU: ``'0'``; one more 3x3 conv with norm and ReLU: ``'1'``).  The score, location, fourier and uncertainty heads read
``'1'``, the refinement head reads ``'0'``, enlarged to the image's size when ``refinement_full_res``.  A head is the reference's
``ReadOut``: ``block`` = conv k x k - BatchNorm - ReLU - Dropout2d - conv 1x1, then ``activation``.
"""
import torch
import torch.nn.functional as F

CHANNELS = 32


class ScaledTanh(torch.nn.Module):
    def __init__(self, factor):
        super().__init__()
        self.factor = factor

    def forward(self, x):
        return torch.tanh(x) * self.factor


class ReadOut(torch.nn.Module):
    def __init__(self, channels_in, channels_out, kernel_size=7, final_activation=None, dropout=.1, channels_mid=None):
        super().__init__()
        t = torch.nn
        mid = channels_in if channels_mid is None else channels_mid
        self.channels_out = channels_out
        self.attention = None
        self.block = t.Sequential(t.Conv2d(channels_in, mid, kernel_size, padding=kernel_size // 2), t.BatchNorm2d(mid), t.ReLU(),
                                  t.Dropout2d(p=dropout) if dropout else t.Identity(), t.Conv2d(mid, channels_out, 1))
        self.activation = t.Identity() if final_activation is None else final_activation

    def forward(self, x):
        attended = x if self.attention is None else self.attention(x)
        return self.activation(self.block(attended))


class Backbone(torch.nn.Module):
    def __init__(self):
        super().__init__()
        t = torch.nn
        self.stem = t.Sequential(t.Conv2d(3, CHANNELS, 7, stride=2, padding=3, bias=False), t.BatchNorm2d(CHANNELS), t.ReLU())
        self.body = t.Sequential(t.Conv2d(CHANNELS, CHANNELS, 3, padding=1, bias=False), t.BatchNorm2d(CHANNELS), t.ReLU())

    def forward(self, x):
        a = self.stem(x)
        return {'0': a, '1': self.body(a)}


# head -> the attribute that holds the key(s) of the features it reads, in the order the heads run
FEATURE_KEYS = {'score': 'score_features', 'location': 'location_features', 'fourier': 'contour_features',
                'uncertainty': 'uncertainty_features', 'refinement': 'refinement_features'}


def _to_input_size(t, image, mode):
    """Stock resize of ``t`` to the image's height and width, skipped when it has them already."""
    want = tuple(image.shape[-2:])
    return t if tuple(t.shape[-2:]) == want else F.interpolate(t, size=want, mode=mode, align_corners=False)


def _forward(self, inputs):
    """The behaviour of the reference's core, written as a walk over FEATURE_KEYS: every head that exists reads its feature(s) of the
    backbone's result (a lone tensor serves all heads), through its fuse module if it has one; the refinement head reads them
    enlarged to the image's size when ``refinement_full_res``, and its map is enlarged to that size if it is still smaller."""
    produced = self.backbone(inputs)
    maps = dict.fromkeys(FEATURE_KEYS)
    for head_name, key_attribute in FEATURE_KEYS.items():
        head = getattr(self, head_name + '_head')
        if head is None:
            continue
        if torch.is_tensor(produced):
            source = produced
        else:
            keys = getattr(self, key_attribute)
            source = [produced[k] for k in keys] if isinstance(keys, (list, tuple)) else produced[keys]
        fuse = getattr(self, head_name + '_fuse')
        if fuse is not None:
            source = fuse(source)
        if head_name != 'refinement':
            maps[head_name] = head(source)
            continue
        mode = self.refinement_interpolation
        if self.refinement_full_res:
            source = _to_input_size(source, inputs, mode)
        maps[head_name] = _to_input_size(head(source), inputs, mode)
    return maps['score'], maps['location'], maps['refinement'], maps['fourier'], maps['uncertainty']


# what marks the reference's function
_forward.__module__, _forward.__qualname__ = 'celldetection.models.cpn', 'CPNCore.forward'


class Core(torch.nn.Module):
    def __init__(self, order=3, score_channels=2, kernel_size=7, refinement_buckets=1, uncertainty_head=False, **flags):
        super().__init__()
        self.order = order
        self.backbone = Backbone()
        self.refinement_interpolation, self.refinement_buckets, self.refinement_full_res = 'bilinear', refinement_buckets, True
        self.contour_features = self.location_features = self.score_features = self.uncertainty_features = '1'
        self.refinement_features = '0'
        self.score_fuse = self.location_fuse = self.fourier_fuse = self.uncertainty_fuse = self.refinement_fuse = None
        self.score_head = ReadOut(CHANNELS, score_channels, kernel_size)
        self.location_head = ReadOut(CHANNELS, 2, kernel_size)
        self.fourier_head = ReadOut(CHANNELS, order * 4, kernel_size)
        self.uncertainty_head = ReadOut(CHANNELS, 4, kernel_size, final_activation=torch.nn.Sigmoid()) if uncertainty_head else None
        self.refinement_head = ReadOut(CHANNELS, 2 * refinement_buckets, kernel_size, final_activation=ScaledTanh(3.))
        for name, v in flags.items():
            setattr(self, name, v)

    forward = _forward


class SameNames(Core):
    """The same attributes, a forward of its own: not the reference's core."""

    def forward(self, inputs):
        return _forward(self, inputs)


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
