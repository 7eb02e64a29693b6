"""CPU tests of the training-step test gear (tests/train_step_standin.py, tests/train_step_oracle.py): the nine converts on the
whole stand-in network, the recorder held against torch's own fp64 autograd, the judges told apart from planted faults, and the
conditioning measurement that decides how tests/test_gpu_train_step.py judges: every module on the operands it saw, not the whole
net against fp64.  Nothing here needs a GPU."""
import collections
import functools
import random

import pytest
import torch
import torch.nn.functional as F

import celldetection_amd as cda
import train_step_oracle as oracle
import train_step_standin as standin
from test_bottleneck import Block

nn = cda.nn
CASES = standin.CASES
B = standin.B


# ---- the converts

def _signature(net):
    return [(name, type(m)) for name, m in net.named_modules()]


def _orders():
    names = list(standin.ORDER_OF_CONVERTS)
    rnd = random.Random(5)
    return [tuple(names), tuple(reversed(names)), tuple(standin.converts(nn))] + [tuple(rnd.sample(names, len(names))) for _ in range(5)]


@pytest.mark.parametrize('case', CASES.values(), ids=list(CASES))
def test_the_nine_converts_take_the_whole_net_in_any_order(case):
    want = None
    for order in _orders():
        net = standin.build(case, p=.1)
        params, buffers, keys = dict(net.named_parameters()), dict(net.named_buffers()), list(net.state_dict().keys())
        assert len(params) == 94
        standin.convert_all_(net, nn, order)
        want = want or _signature(net)
        assert _signature(net) == want, order
        after_p, after_b = dict(net.named_parameters()), dict(net.named_buffers())
        assert list(after_p) == list(params) and all(after_p[k] is params[k] for k in params), order  # the same Parameter objects
        assert list(after_b) == list(buffers) and all(after_b[k] is buffers[k] for k in buffers), order
        assert list(net.state_dict().keys()) == keys, order
        count = collections.Counter(type(m) for m in net.modules())
        assert {t: count[t] for t in standin.census(case, nn)} == standin.census(case, nn), order
        stock = (torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.MaxPool2d, torch.nn.Dropout2d, Block, standin.unet_standin.Decoder,
                 standin.cpn_core_standin.Core)
        assert [name for name, m in net.named_modules() if type(m) in stock] == [], order
        assert all(net.get_submodule(standin.head(h, 4)).p == .1 for h in standin.HEADS)
        assert all(m.activation == ('relu' if name.split('.')[-2] in ('stem', 'block') or 'layer_blocks' in name else None)
                   for name, m in net.named_modules() if type(m) is nn.BatchNorm2d), order
        for convert in standin.converts(nn).values():  # a second round finds nothing
            assert all(not part for part in convert(net)), order
    with pytest.raises(RuntimeError, match='MI355X'):  # no GPU here: the net runs this library's ops, nothing else
        net['core'](standin.image(case))


def test_the_hand_written_topology_names_modules_of_the_converted_net():
    net = standin.build(CASES['A'])
    standin.convert_all_(net, nn)
    leaf = oracle.library_leaf(nn)
    for producer, consumer in standin.routes_converted():
        assert leaf(net.get_submodule(producer[0])) and leaf(net.get_submodule(consumer[0])), (producer, consumer)
    assert sum(leaf(m) for m in net.modules()) == sum(v for t, v in standin.census(CASES['A'], nn).items()
                                                      if t not in (nn.CPNCore, nn.UNetDecoder, nn.Bottleneck))


# ---- the recorder tells the truth

@functools.lru_cache(maxsize=None)
def recorded64(name):
    """The stock net of a case in fp64 under the recorder, once."""
    case = CASES[name]
    net = standin.build(case).double()
    with oracle.Recorder(net, oracle.stock_leaf) as rec:
        maps, grads = standin.run(net, standin.image(case).double(), [c.double() for c in standin.cotangents(case)])
    rec.finish()
    plain = standin.build(case).double()  # the hooks change nothing: the same net without them
    maps_plain, grads_plain = standin.run(plain, standin.image(case).double(), [c.double() for c in standin.cotangents(case)])
    assert all(torch.equal(a, b) for a, b in zip(maps, maps_plain)) and all(torch.equal(grads[k], grads_plain[k]) for k in grads)
    return rec


def _within64(name, got, want, scale):
    assert bool(((got - want).abs() <= 1e-12 * (1 + scale)).all()), name


def judge_all(rec, case):
    """The judges that need no arithmetic model, on fp64 records -> the names of those that object."""
    flagged = []

    def attempt(name, fn):
        try:
            fn()
        except AssertionError:
            flagged.append(name)

    def replays():
        for call in rec.calls:
            oracle.compare_calls(call, oracle.replay(call), oracle.assert_close64)

    def fan_outs():
        for name, got, shares in standin.fan_out_stock(rec, case):
            oracle.judge_fan_out(name, got, shares)

    def routes():
        for name, saw, wrote in standin.laterals_stock(rec):
            oracle.assert_close64(name, saw, wrote)

    def buffers():
        for call in rec.calls:
            if isinstance(call.module, torch.nn.BatchNorm2d):
                oracle.judge_buffers(call, _within64)

    for name, fn in (('replay', replays), ('fan-out', fan_outs), ('routes', routes), ('buffers', buffers)):
        attempt(name, fn)
    return flagged


@pytest.mark.parametrize('case', CASES.values(), ids=list(CASES))
def test_the_recorder_agrees_with_a_replay_of_every_call_and_the_shares_add_up(case):
    """Every recorded call of the stock fp64 net, run again through a deep copy of its module on the recorded operands, gives the
    recorded outputs, input gradients, parameter gradients and buffers to 1e-12; for every tensor with several consumers the
    recorded shares add up to the gradient its producer received.  This is what licenses the local judgement on the GPU."""
    rec = recorded64(case.name)
    assert len(rec.calls) == 81 and all(len(c.outputs) == 1 for c in rec.calls)
    norms = [c for c in rec.calls if isinstance(c.module, torch.nn.BatchNorm2d)]
    assert len(norms) == 25 and all(int(c.buffers_after['num_batches_tracked']) == 1 for c in norms)
    with_params = {c.name + '.' + k for c in rec.calls for k in c.param_grads}
    assert with_params == {k for k, _ in standin.build(case).named_parameters()}  # all 94 were seen
    assert all(c.grad_out and (c.grad_in or c.name == B + 'stem.0') for c in rec.calls), [c for c in rec.calls if not c.grad_out]
    assert judge_all(rec, case) == []
    assert len(standin.fan_out_stock(rec, case)) == 7


# ---- the judges are told apart from planted faults

def _swap(holder, key, value):
    old = holder[key]
    holder[key] = value
    return lambda: holder.__setitem__(key, old)


def plant_dropped_share(rec, case):
    """A fan-out that forgets one consumer: the pool's share of the stem's gradient."""
    call = rec[B + 'pool']
    return _swap(call.grad_in, 0, torch.zeros_like(call.grad_in[0]))


def plant_neighbouring_lateral(rec, case):
    """Level 1 of the decoder reads the lateral of level 2 (brought to its size) instead of its own."""
    call = rec[B + 'unet.layer_blocks.1.0']
    x = call.operands[0].clone()
    wrong = rec.get(B + 'layer1.1.relu', 2).outputs[0]
    x[:, :64] = F.interpolate(wrong, size=x.shape[2:], mode='nearest')
    return _swap(call.operands, 0, x)


def plant_second_update(rec, case):
    """A norm that runs its update twice in one forward."""
    call = rec[B + 'layer2.0.downsample.1']
    mean, _ = oracle.batch_statistics64(call.operands[0])
    f = call.module.momentum
    return _swap(call.buffers_after, 'running_mean', (1 - f) * call.buffers_after['running_mean'] + f * mean)


def plant_missing_skip(rec, case):
    """A block input whose gradient lacks the skip's share."""
    call = rec.get(B + 'layer1.0.relu', 2)
    return _swap(call.grad_out, 0, call.grad_out[0] - rec[B + 'layer1.1.bn3'].grad_out[0])


def plant_transposed_wgrad(rec, case):
    """The weight gradient of a square 1x1 conv with the channel roles swapped."""
    call = rec[B + 'layer2.1.conv1']
    assert call.param_grads['weight'].shape == (128, 128, 1, 1)
    return _swap(call.param_grads, 'weight', call.param_grads['weight'].transpose(0, 1).contiguous())


# fault -> the judge that must object (others may, too: a replay sees most things)
FAULTS = {plant_dropped_share: 'fan-out', plant_neighbouring_lateral: 'routes', plant_second_update: 'buffers',
          plant_missing_skip: 'fan-out', plant_transposed_wgrad: 'replay'}


@pytest.mark.parametrize('case', CASES.values(), ids=list(CASES))
def test_planted_faults_are_told_apart(case):
    rec = recorded64(case.name)
    assert judge_all(rec, case) == []
    for plant, judge in FAULTS.items():
        restore = plant(rec, case)
        try:
            flagged = judge_all(rec, case)
        finally:
            restore()
        assert judge in flagged, (plant.__name__, flagged)
    assert judge_all(rec, case) == []


def test_the_fan_out_judge_counts_roundings():
    """k - 1 roundings of the sum of the absolute shares: a bf16 sum of three shares may be two roundings off, not three; a share
    of another dtype or shape is refused."""
    g = torch.Generator().manual_seed(3)
    shares = [torch.randn(2, 8, 5, 7, generator=g).to(torch.bfloat16) for _ in range(3)]
    right = (shares[0] + shares[1]) + shares[2]
    assert oracle.judge_fan_out('bf16', right, shares) <= 1
    assert oracle.judge_fan_out('other order', (shares[2] + shares[1]) + shares[0], shares) <= 1
    assert oracle.judge_fan_out('one consumer', shares[0], shares[:1]) == 0
    S = sum(s.double().abs() for s in shares)
    off = (sum(s.double() for s in shares) + 3 * 2. ** -8 * S).to(torch.bfloat16)
    with pytest.raises(AssertionError, match='not the sum'):
        oracle.judge_fan_out('three roundings off', off, shares)
    with pytest.raises(AssertionError, match='not the sum'):
        oracle.judge_fan_out('dropped', shares[0] + shares[1], shares)
    with pytest.raises(AssertionError, match='not the sum'):
        oracle.judge_fan_out('one share passed on', shares[0], shares[:2])
    with pytest.raises(AssertionError):
        oracle.judge_fan_out('dtype', right, [shares[0].float()] + shares[1:])


# ---- the conditioning measurement

stock_results = standin.stock_results


def test_whole_net_errors_of_stock_fp32_and_bf16_against_stock_fp64():
    """The measurement that decides the design, on case A: relative L2 errors of the maps and of the parameter gradients of stock
    fp32 and of stock CPU-autocast bf16 against stock fp64.  Printed; asserted only as far as the gate of the GPU tests needs them:
    finite and non-zero."""
    maps64, grads64 = stock_results('A', 'fp64')
    for kind in ('fp32', 'bf16'):
        maps, grads = stock_results('A', kind)
        e_maps = [oracle.rel_l2(m, r) for m, r in zip(maps, maps64)]
        e_grads = sorted(oracle.rel_l2(grads[k], grads64[k]) for k in grads64)
        print(f'{kind}: maps {", ".join(f"{e:.2e}" for e in e_maps)}; parameter gradients: median {e_grads[len(e_grads) // 2]:.2e}, '
              f'largest {e_grads[-1]:.2e}, smallest {e_grads[0]:.2e}')
        assert all(0 < e < float('inf') for e in e_maps + e_grads), kind


def test_a_conv_bias_in_front_of_a_training_norm_has_gradient_zero_in_exact_arithmetic():
    """... so its relative error means nothing, and the GPU tests bound it absolutely: in fp64 it is rounding noise of the weight
    gradient's scale."""
    maps64, grads64 = stock_results('A', 'fp64')
    names = [standin.head(h, 0) for h in standin.HEADS] + [B + f'unet.layer_blocks.{i}.3' for i in range(3)]
    for name in names:
        assert float(grads64[name + '.bias'].abs().max()) <= 1e-12 * float(grads64[name + '.weight'].abs().max()), name
    assert all(float(g.abs().max()) > 0 for k, g in grads64.items() if k not in {n + '.bias' for n in names})  # every other one is non-zero
