"""CPU tests of what the families of celldetection_amd/nn/ share (convert.py, _common.py): the one tree walk behind the nine
converts keeps an object that sits in several slots one object, the converts commute, and ``_nhwc`` hands the kernels a 16-byte
aligned operand.  Module surgery needs no GPU."""
import copy

import pytest
import torch

import celldetection_amd as cda
import cpn_core_standin
import unet_standin
from test_bottleneck import Block

nn = cda.nn
t = torch.nn

# (convert, an eligible stock module, the class it becomes)
SHARED = {'conv': (nn.convert_conv2d_, lambda: t.Conv2d(32, 32, 3, padding=1), nn.Conv2d),
          'batch_norm': (nn.convert_batchnorm2d_, lambda: t.BatchNorm2d(32), nn.BatchNorm2d),
          'readout_tail': (nn.convert_readout_tail_, lambda: t.Conv2d(32, 2, 1), nn.DropoutConv1x1),
          'grouped': (nn.convert_grouped_conv2d_, lambda: t.Conv2d(64, 64, 3, padding=1, groups=16), nn.GroupedConv2d),
          'stem': (nn.convert_stem_conv2d_, lambda: t.Conv2d(3, 64, 7, stride=2, padding=3), nn.StemConv2d),
          'max_pool': (nn.convert_maxpool2d_, lambda: t.MaxPool2d(3, 2, 1), nn.MaxPool2d)}


@pytest.mark.parametrize('family', list(SHARED))
def test_an_object_in_three_slots_is_replaced_by_one_object_in_all_of_them(family):
    convert, make, cls = SHARED[family]
    shared = make()
    params, buffers = list(shared.parameters()), list(shared.buffers())
    root = t.Sequential()  # (a Sequential: the ReadOut tail is replaced inside one only)
    root.add_module('a', t.Sequential(shared))
    root.add_module('b', t.Sequential(shared))
    root.add_module('c', shared)
    keys = list(root.state_dict().keys())
    result = convert(root)
    replaced, left = result[0], result[-1]
    assert sorted(replaced) == ['a.0', 'b.0', 'c'] and left == {}
    assert type(root.c) is cls and root.a[0] is root.c and root.b[0] is root.c
    after_p, after_b = list(root.c.parameters()), list(root.c.buffers())
    assert len(after_p) == len(params) and all(p is q for p, q in zip(after_p, params))  # the original Parameter objects
    assert len(after_b) == len(buffers) and all(p is q for p, q in zip(after_b, buffers))
    assert list(root.state_dict().keys()) == keys
    assert all(not part for part in convert(root))  # a second call finds nothing


class Model(torch.nn.Module):
    """Everything the nine converts take, from the stand-ins of the other tests: the CPN core (stem, norms with ReLU, ReadOut tails,
    the refinement head behind a resize), a max-pool, a torchvision-style bottleneck block at a stage entry and a U-Net decoder."""

    def __init__(self):
        super().__init__()
        self.core = cpn_core_standin.Core(uncertainty_head=True)
        self.pool = t.MaxPool2d(3, 2, 1)
        self.block = Block(64, 128, 32, 2, 256)
        self.decoder = unet_standin.Decoder()


CONVERTS = (nn.convert_conv2d_, nn.convert_batchnorm2d_, nn.convert_readout_tail_, nn.convert_grouped_conv2d_, nn.convert_stem_conv2d_,
            nn.convert_maxpool2d_, nn.convert_bottleneck_, nn.convert_unet_decoder_, nn.convert_cpn_core_)


def test_the_nine_converts_commute():
    first = Model()
    second = copy.deepcopy(first)
    params = dict(first.named_parameters())
    for convert in CONVERTS:
        convert(first)
    for convert in reversed(CONVERTS):
        convert(second)
    types = [(name, type(m)) for name, m in first.named_modules()]
    assert types == [(name, type(m)) for name, m in second.named_modules()]
    assert list(first.state_dict().keys()) == list(second.state_dict().keys()) == list(Model().state_dict().keys())
    after = dict(first.named_parameters())
    assert after.keys() == params.keys() and all(after[k] is params[k] for k in params)
    # every family and every block took part, and nothing of stock torch that a convert takes is left
    found = {cls for _, cls in types}
    assert {nn.Conv2d, nn.BatchNorm2d, nn.DropoutConv1x1, nn.GroupedConv2d, nn.StridedConv1x1, nn.StemConv2d, nn.MaxPool2d, nn.CatConv2d,
            nn.ResizedConv2d, nn.Bottleneck, nn.UNetDecoder, nn.CPNCore} <= found
    assert not found & {t.Conv2d, t.BatchNorm2d, t.MaxPool2d, t.Dropout2d, Block, unet_standin.Decoder, cpn_core_standin.Core}
    for convert in CONVERTS:  # a second round finds nothing
        assert all(not part for part in convert(first)), convert.__name__


def test_nhwc_clones_a_view_that_does_not_start_at_a_16_byte_address():
    n, c, h, w = 1, 32, 4, 5
    buf = torch.arange(n * h * w * c + 1, dtype=torch.float32).to(torch.bfloat16)
    view = buf[1:].view(n, h, w, c).permute(0, 3, 1, 2)  # channels-last bf16, one element into the buffer
    assert view.is_contiguous(memory_format=torch.channels_last) and view.data_ptr() % 16 == 2
    for dtype in (None, torch.bfloat16):
        got = nn._common._nhwc(view, dtype)
        assert got.data_ptr() % 16 == 0 and got.is_contiguous(memory_format=torch.channels_last) and torch.equal(got, view)
        aligned = view.clone(memory_format=torch.channels_last)
        assert aligned.data_ptr() % 16 == 0
        same = nn._common._nhwc(aligned.requires_grad_(True), dtype)
        assert same.data_ptr() == aligned.data_ptr() and not same.requires_grad  # the tensor's own storage, detached: no copy
