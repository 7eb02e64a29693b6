"""GPU test of a whole training step of a U-Net-encoder model: image -> encoder -> decoder -> heads -> maps -> gradients -> AdamW, on
the stand-in network of tests/unet_encoder_standin.py after all converts, in training mode.  The encoder family's first module, the
3x3 conv on the image itself (``ImageConv2d``), is the one piece the other step test (tests/test_gpu_train_step.py) does not meet:
here it is recorded in the chain, replayed alone bit for bit and judged by its family's bounds on the operands it saw."""
import functools

import pytest
import torch

import celldetection_amd as cda
import conv_bounds as cb
import image_conv_oracle
import train_step_oracle as oracle
import unet_encoder_standin as standin
from test_gpu_conv_train import check_sum
from test_gpu_image_conv import FWD_CHAIN
from train_step_oracle import same_bits

pytestmark = pytest.mark.gpu
nn = cda.nn
CASES = standin.CASES
FIRST = 'core.backbone.encoder.0.0'
HYPER = dict(lr=1e-3, betas=(.9, .999), eps=1e-8)
case_ids = pytest.mark.parametrize('case', CASES.values(), ids=list(CASES))


def converted(case, order=standin.ORDERS[0]):
    net = standin.build(case)
    standin.convert_all_(net, nn, order)
    return net.cuda()


def leaf(m):
    """The leaves of tests/train_step_oracle.py and the image conv."""
    return oracle.library_leaf(nn)(m) or isinstance(m, nn.ImageConv2d)


@functools.lru_cache(maxsize=None)
def chain(name):
    """The converted net of a case on the GPU: the recorded run first, then two plain runs -> dict(net, rec, hooked, first, second),
    each run as (maps, gradients)."""
    case = CASES[name]
    net = converted(case)
    x, cots = standin.image(case).cuda(), [c.cuda() for c in standin.cotangents(case)]

    def run():
        maps, grads = standin.run(net, x, cots)
        return maps, {k: g.clone() for k, g in grads.items()}

    functions = {} if case.full_res else {'bilinear_resize': (cda.nn.blocks, 'bilinear_resize')}
    with oracle.Recorder(net, leaf, functions, norm_types=(nn.BatchNorm2d,)) as rec:
        hooked = run()
        rec.finish()
    return dict(net=net, rec=rec, hooked=hooked, first=run(), second=run())


@case_ids
def test_no_stock_module_is_left_in_any_order_of_the_converts(case):
    stock = (torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.ReLU, torch.nn.MaxPool2d, torch.nn.Dropout2d)
    want = None
    for order in standin.ORDERS:
        net = standin.build(case)
        standin.convert_all_(net, nn, order)
        found = standin.census(net)
        assert [t for t in found if t in stock] == [], (order, found)
        assert found[nn.ImageConv2d] == 1 and found[nn.MaxPool2d] == 2 and found[nn.BatchNorm2d] == 14 and found[nn.CatConv2d] == 2
        assert type(net.get_submodule(FIRST)) is nn.ImageConv2d
        want = want or found
        assert found == want, order


@case_ids
def test_two_runs_and_the_hooked_run_give_the_same_bits(case):
    c = chain(case.name)
    maps, grads = c['first']
    assert [tuple(m.shape) for m in maps] == [(case.n, k, case.h, case.w) for k in (1, 2, 2, standin.ORDER * 4)]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values()) and FIRST + '.weight' in grads and FIRST + '.bias' in grads
    assert bool((grads[FIRST + '.weight'] != 0).any())
    for other in ('second', 'hooked'):
        maps2, grads2 = c[other]
        assert all(same_bits(a, b) for a, b in zip(maps, maps2)), other
        assert [k for k in grads if not same_bits(grads[k], grads2[k])] == [], other
    rec = c['rec']
    assert len(rec.by_name[FIRST]) == 1 and {call.name + '.' + k for call in rec.calls for k in call.param_grads} == set(grads)
    for call in rec.calls:  # what the recorder kept for a parameter IS the gradient of the run
        assert all(same_bits(g, grads[call.name + '.' + k]) for k, g in call.param_grads.items())


@case_ids
def test_the_image_conv_replays_alone_bit_for_bit_and_lies_within_its_bounds(case):
    rec = chain(case.name)['rec']
    call = rec[FIRST]
    m = call.module
    assert type(m) is nn.ImageConv2d and m.in_channels == case.channels and m.out_channels == 32 and call.grad_in == {}
    # through the module itself (tests/train_step_oracle.py's functional table does not know this family)
    oracle.compare_calls(call, oracle.replay(call), oracle.assert_same_bits)
    # the operands it saw: the image, the gradient the norm behind it sent back
    x, y, dy = call.operands[0].detach().cpu().float(), call.outputs[0], call.grad_out[0]
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last) and dy.dtype == torch.bfloat16
    assert tuple(x.shape) == (case.n, case.channels, case.h, case.w) and tuple(y.shape) == (case.n, 32, case.h, case.w)
    dy = dy.detach().cpu().float()
    wq = m.weight.detach().cpu().to(torch.bfloat16).double()
    ref, S, d = cb.conv_with_noise(x, wq, m.bias.detach().cpu().double(), 1, 1, n=FWD_CHAIN)
    cb.check(f'{FIRST} forward', y.detach().cpu().float(), *cb.bf16_bounds(ref, d), ref, S)
    info = nn.image_weight_grad_info(case.n, case.h, case.w, 32)
    check_sum(f'{FIRST} dW', call.param_grads['weight'], *image_conv_oracle.wgrad(x, dy), info['steps'] + 2 + info['reduce_chain'])
    # (the conv sits in front of a training-mode norm, so the exact db is 0: the bound is relative to the sum of |dy|, as everywhere)
    check_sum(f'{FIRST} db', call.param_grads['bias'], *image_conv_oracle.bgrad(dy), info['bias_chain'])
    # the norm behind it read what the conv wrote
    oracle.judge_routes(rec, [((FIRST, 0, 0), (FIRST[:-1] + '1', 0, 0))])


@case_ids
def test_one_adamw_step_runs(case):
    net = converted(case, standin.ORDERS[1])
    x, cots = standin.image(case).cuda(), [c.cuda() for c in standin.cotangents(case)]
    named = dict(net.named_parameters())
    decayed = [k for k, p in named.items() if p.dim() == 4]
    plain = [k for k, p in named.items() if p.dim() == 1]
    groups = [dict(params=[named[k] for k in decayed], weight_decay=1e-2), dict(params=[named[k] for k in plain], weight_decay=0.)]
    opt = cda.optim.AdamW(groups, max_grad_norm=1., **HYPER)
    before = {k: p.detach().clone() for k, p in named.items()}
    maps, grads = standin.run(net, x, cots)
    assert all(g is not None and g.dtype == named[k].dtype and bool(torch.isfinite(g).all()) for k, g in grads.items())
    opt.step()
    assert bool(torch.isfinite(opt.last_grad_norm).all()) and float(opt.last_grad_norm) > 0
    for k, p in named.items():
        assert bool(torch.isfinite(p).all()) and float(opt.state[p]['step']) == 1, k
    assert not torch.equal(named[FIRST + '.weight'], before[FIRST + '.weight'])
    moved = [k for k, p in named.items() if not torch.equal(p, before[k])]
    assert set(decayed) <= set(moved)
    # the same step from the same start gives the same parameters, bit for bit
    again = converted(case, standin.ORDERS[1])
    named2 = dict(again.named_parameters())
    opt2 = cda.optim.AdamW([dict(params=[named2[k] for k in decayed], weight_decay=1e-2), dict(params=[named2[k] for k in plain], weight_decay=0.)],
                           max_grad_norm=1., **HYPER)
    standin.run(again, x, cots)
    opt2.step()
    assert [k for k in named if not same_bits(named[k].detach(), named2[k].detach())] == []
    # a second step runs
    opt.zero_grad()
    standin.run(net, x, cots)
    opt.step()
    assert all(bool(torch.isfinite(p).all()) and float(opt.state[p]['step']) == 2 for p in named.values())
