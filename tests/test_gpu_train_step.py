"""GPU tests of a whole training step: stem -> max-pool -> ResNeXt stages -> U-Net decoder -> CPN core -> objective -> ``backward()``
-> AdamW, on the stand-in network of tests/train_step_standin.py after all nine converts, in training mode.

A whole-net gradient comparison against fp64 cannot tell a right bf16 implementation from a wrong one (tests/test_train_step.py
measures it), so every leaf module is judged on the operands IT saw, recorded by ``train_step_oracle.Recorder``:

A  two runs and a hooked run give the same bits in the maps and in all 94 parameter gradients;
B  every recorded call, run again alone through its family's functional entry point, gives the same bits everywhere -- no family
   is compared within a bound here: every reduction of this library has a fixed order;
C  the tensors with several consumers are the ones listed by hand, and what their producer received is the sum of the shares;
D  every call lies within its family's derived bounds of the fp64 statement of the operation on the operands it saw, with the
   module's own parameters rounded as the family rounds them (the same-named stock module holds the same values: the converts share
   the ``Parameter`` objects).  No tolerance is new: the oracles, chain lengths and judges are those of the family's own test file;
E  the step itself from label images, with dropout: the objective's gradients, the global norm, one AdamW step, a second step;
F  every norm updated its buffers exactly once; an eval forward leaves them alone;
G  the maps against the stock fp64 net, at most twice the error of stock CPU bf16 autocast (the rule of
   tests/test_gpu_bottleneck.py); the gradient errors are printed beside the yardstick's, not asserted.

In A - D and G the cotangents of the four maps are fixed bf16-exact tensors and p = 0: no objective, whose clamps would add
discontinuities.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import batch_norm_oracle as bo
import bilinear_oracle
import bottleneck_oracle
import cat_conv_oracle
import celldetection_amd as cda
import conv_bounds as cb
import conv_train_oracle as dense
import grouped_conv_oracle
import optim_oracle
import readout_tail_oracle
import stem_oracle
import train_step_oracle as oracle
import train_step_standin as standin
from test_gpu_cat_conv import check_sum, dtop_bounds
from test_gpu_stem import FWD_CHAIN as STEM_CHAIN, judge_pool_gradient
from train_step_oracle import same_bits

pytestmark = pytest.mark.gpu
nn = cda.nn
CASES = standin.CASES
B = standin.B
BF16 = torch.bfloat16
case_ids = pytest.mark.parametrize('case', CASES.values(), ids=list(CASES))


def converted(case, p=0.):
    net = standin.build(case, p)
    standin.convert_all_(net, nn)
    return net.cuda()


def functions(case):
    """The one function the converted core calls that is no module: the resize of the head map (case B)."""
    return {} if case.full_res else {'bilinear_resize': (cda.nn.blocks, 'bilinear_resize')}


def cpu(t):
    return None if t is None else t.detach().cpu()


@functools.lru_cache(maxsize=None)
def chain(name):
    """The converted net of a case on the GPU with p = 0: the recorded run first (so the records hold the first update of every
    buffer), then two plain runs -> dict(net, rec, hooked, first, second), each run as (maps, gradients)."""
    case = CASES[name]
    net = converted(case)
    x, cots = standin.image(case).cuda(), [c.cuda() for c in standin.cotangents(case)]

    def run():
        maps, grads = standin.run(net, x, cots)
        return maps, {k: g.clone() for k, g in grads.items()}

    with oracle.Recorder(net, oracle.library_leaf(nn), functions(case), norm_types=(nn.BatchNorm2d,)) as rec:
        hooked = run()
        rec.finish()
    assert cda.nn.blocks.bilinear_resize is nn.bilinear_resize  # the recorder put the function back
    return dict(net=net, rec=rec, hooked=hooked, first=run(), second=run())


# ---- A: repeatability and hook neutrality

@case_ids
def test_two_runs_and_the_hooked_run_give_the_same_bits(case):
    c = chain(case.name)
    maps, grads = c['first']
    assert [tuple(m.shape) for m in maps] == standin.map_shapes(case) and all(m.dtype == torch.float32 and m.is_contiguous() for m in maps)
    assert len(grads) == 94 and all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    zero_in_exact_arithmetic = {name + '.bias' for name in IN_FRONT_OF_A_NORM}  # (bounded absolutely in part D)
    assert [k for k, g in grads.items() if k not in zero_in_exact_arithmetic and not bool((g != 0).any())] == []
    for other in ('second', 'hooked'):
        maps2, grads2 = c[other]
        assert all(same_bits(a, b) for a, b in zip(maps, maps2)), other
        assert [k for k in grads if not same_bits(grads[k], grads2[k])] == [], other
    rec = c['rec']
    leaves = sum(v for t, v in standin.census(case, nn).items() if t not in (nn.CPNCore, nn.UNetDecoder, nn.Bottleneck))
    assert len(rec.calls) == leaves + len(functions(case)) and all(len(v) == 1 for v in rec.by_name.values())
    assert {call.name + '.' + k for call in rec.calls for k in call.param_grads} == set(grads)
    for call in rec.calls:  # what the recorder kept for a parameter IS the gradient of the run
        assert all(same_bits(g, grads[call.name + '.' + k]) for k, g in call.param_grads.items())


# ---- B: every call alone, bit for bit

@case_ids
def test_every_recorded_call_replays_alone_bit_for_bit(case):
    """A difference means the module behaves differently inside the chain than in its own test file: a view, an alignment, an alias,
    a stale saved tensor."""
    rec = chain(case.name)['rec']
    for call in rec.calls:
        oracle.compare_calls(call, oracle.replay(call, nn), oracle.assert_same_bits)
    norms = [call for call in rec.calls if type(call.module) is nn.BatchNorm2d]
    assert len(norms) == 25 and all(len(call.saved) == 4 and all(v.dtype == torch.float32 for v in call.saved) for call in norms)
    forks = [call for call in rec.calls if call.extras.get('fork')]
    assert len(forks) == 4 and all(len(call.outputs) == 2 and sorted(call.grad_out) == [0, 1] for call in forks)


# ---- C: fan-out sums

@case_ids
def test_fan_outs_are_the_listed_ones_and_their_shares_add_up(case):
    rec = chain(case.name)['rec']
    found = oracle.fan_out(rec)
    want = standin.fan_out_converted()
    assert {k: v for k, v in found.items() if len(v) > 1} == want
    edges = {(p, c) for p, consumers in found.items() for c in consumers}
    assert set(standin.routes_converted()) <= edges
    oracle.judge_routes(rec, sorted(edges, key=str))  # what every consumer saw is what its producer wrote: nothing overwrote it
    for (name, index, out), consumers in found.items():
        got = rec.get(name, index).grad_out[out]
        shares = [rec.get(c, i).grad_in[key] for c, i, key in consumers]
        assert got.dtype == BF16, name
        r = oracle.judge_fan_out(f'{name} -> {[c for c, _, _ in consumers]}', got, shares)
        if len(consumers) > 1:
            print(f'{name}: {len(consumers)} consumers, {got.dtype}, largest error / bound {r:.3f}')
        else:
            assert same_bits(got, shares[0]), name


@case_ids
def test_the_fork_adds_the_skip_gradient_inside_every_block(case):
    """dx = dgrad(dy) + dskip, judged as tests/test_gpu_bottleneck.py judges it: the conv rule with the skip gradient as the residual
    operand; the skip IS the input (one storage), and what the shortcut sent back is what arrived at the skip."""
    rec = chain(case.name)['rec']
    for block, down in (('layer1.0', True), ('layer1.1', False), ('layer2.0', True), ('layer2.1', False)):
        call = rec[B + block + '.conv1']
        assert call.extras == dict(fork=True) and same_bits(call.outputs[1], call.operands[0])
        assert call.out_refs[1].data_ptr() == call.inputs[0].data_ptr()
        sender = rec[B + block + '.downsample.0'].grad_in[0] if down else rec[B + block + '.bn3'].grad_in['residual']
        assert same_bits(call.grad_out[1], sender)
        judge_conv(call, {})


# ---- D: each call against the fp64 statement on the operands it saw

def f32(t):
    return cpu(t).float()


def bf16_operand(t):
    """An activation as the kernels read it: already bf16 in this net (asserted), widened exactly."""
    assert t.dtype == BF16, t.dtype
    return f32(t)


def note(ratios, key, r):
    ratios[key] = max(ratios.get(key, 0.), float(r))


def judge_conv(call, ratios, norm=None):
    """The dense conv (``Conv2d``; a ``ResizedConv2d`` without a size), with or without the fork: tests/test_gpu_conv_train.py."""
    m, name = call.module, call.name
    x, y, dy = bf16_operand(call.operands[0]), call.outputs[0], bf16_operand(call.grad_out[0])
    n, cin, h, w = x.shape
    cout, k = m.out_channels, m.kernel_size[0]
    wq = cpu(m.weight).to(BF16).double()
    b64 = None if m.bias is None else cpu(m.bias).double()
    ref, S, d = cb.conv_with_noise(x, wq, b64, 1, k // 2, n=cb.chain_length(k, k, cin))
    assert y.dtype == BF16 and y.is_contiguous(memory_format=torch.channels_last)
    note(ratios, 'forward', cb.check(f'{name} forward', f32(y), *cb.bf16_bounds(ref, d), ref, S))
    dskip = bf16_operand(call.grad_out[1]) if call.extras.get('fork') else None
    wd = dense.unpack(dense.pack_dgrad(wq), cout, k)
    ref, S, d = cb.conv_with_noise(dy, wd, None, 1, k // 2, n=cb.chain_length(k, k, cout), res=dskip)
    note(ratios, 'dx', cb.check(f'{name} dx', f32(call.grad_in[0]), *cb.bf16_bounds(ref, d), ref, S))
    info = nn.weight_grad_info(n, h, w, cin, cout, k)
    note(ratios, 'dW', check_sum(f'{name} dW', call.param_grads['weight'], *dense.wgrad(x, dy, k), info['steps'] + 2 + info['reduce_chain']))
    if m.bias is not None:
        judge_bias(call, ratios, dy, dense.bgrad(dy), info['bias_chain'], norm)


def judge_bias(call, ratios, dy, ref_and_S, bias_chain, norm=None):
    """The bias gradient by the family's bound, gamma(bias_chain) sum |dy| and one fp32 rounding, around the fp64 sum of the dy it saw.

    ``norm``: the recorded call of the training-mode norm this conv sits directly in front of.  Then the exact value is 0 -- the
    norm's input gradient sums to zero over every channel -- and a relative error means nothing, so |db| itself is bounded: the dy
    this conv read is the dx the norm stored, which ``batch_norm_oracle.judge_grads`` accepts in [lo, hi] around a reference that
    sums to zero, hence |db| <= the family's bound on sum |dy| + the sum of the accepted half-widths.  Against the family's bound
    alone |db| is printed: it need not hold, because each stored dx was rounded to bf16 once and the rounded values do not sum to zero
    (measured on an MI355X: 15 to 574 times gamma(bias_chain) sum |dy| over the two cases, while db is within 0.006 of that bound
    around the fp64 sum of the dy it read, and |db| within 0.48 of the bound asserted here)."""
    db = call.param_grads['bias']
    ref, S = ref_and_S
    note(ratios, 'db', check_sum(f'{call.name} db', db, ref, S, bias_chain))
    if norm is None:
        assert bool((db != 0).any()), call.name
        return
    m = norm.module
    assert type(m) is nn.BatchNorm2d and m.activation == 'relu' and 'residual' not in norm.operands and same_bits(norm.grad_in[0], call.grad_out[0])
    x = cpu(norm.operands[0])
    mean, invstd, scale, shift = (cpu(v) for v in norm.saved)
    o = bo.backward(x, cpu(norm.grad_out[0]), cpu(m.weight), mean, invstd, bo.mask(bo.exact_t(x, scale, shift)), True)
    lo, hi = cb.bf16_bounds(o['dx'], (cb.gamma(3) + 2.0 ** -40) * o['S_dx'])
    slack = torch.maximum(hi - o['dx'], o['dx'] - lo).sum((0, 2, 3)) + o['dx'].sum((0, 2, 3)).abs()
    own = cb.gamma(bias_chain) * S
    bound = slack + own + cb.U * (slack + own)
    r = float((db.double().cpu().abs() / bound).max())
    print(f'{call.name}: |db| / bound {r:.3f} (exact value 0); |db| / (gamma({bias_chain}) sum |dy|) {float((db.double().cpu().abs() / own).max()):.3f}; '
          f'largest |db| {float(db.abs().max()):.3e} beside a largest |dW| of {float(call.param_grads["weight"].abs().max()):.3e}')
    note(ratios, '|db| of an exact zero', r)
    assert r <= 1, (call.name, r)


IN_FRONT_OF_A_NORM = {standin.head(h, 0) for h in standin.HEADS} | {B + f'unet.layer_blocks.{i}.3' for i in range(3)}  # convs with a bias


def following_norm(name):
    """The next slot of the same ``Sequential``."""
    stem, slot = name.rsplit('.', 1)
    return f'{stem}.{int(slot) + 1}'


def family_conv(rec, case, ratios):
    calls = [c for c in rec.calls if type(c.module) is nn.Conv2d or (type(c.module) is nn.ResizedConv2d and 1 not in c.extras)]
    assert len(calls) == standin.census(case, nn)[nn.Conv2d]
    biased = {c.name for c in calls if c.module.bias is not None}
    assert IN_FRONT_OF_A_NORM - {standin.head('refinement', 0)} <= biased and len(biased - IN_FRONT_OF_A_NORM) == 2  # (the inner convs)
    for call in calls:
        judge_conv(call, ratios, rec[following_norm(call.name)] if call.name in IN_FRONT_OF_A_NORM else None)


def family_resized(rec, case, ratios):
    """The refinement head's conv behind the bilinear resize: tests/test_gpu_bilinear_resize.py."""
    calls = [c for c in rec.calls if type(c.module) is nn.ResizedConv2d and 1 in c.extras]
    assert len(calls) == (1 if case.full_res else 0)
    for call in calls:
        m, name = call.module, call.name
        size = tuple(call.extras[1])
        x, y, dy = bf16_operand(call.operands[0]), call.outputs[0], call.grad_out[0]
        n, c, h, w = x.shape
        cout, k = m.out_channels, m.kernel_size[0]
        assert size == (case.h, case.w) and (h, w) == (22, 26) and dy.dtype == BF16
        wq = cpu(m.weight).to(BF16).double()
        ref, S, d = bilinear_oracle.forward_bounds(x, wq, cpu(m.bias).double(), size)
        note(ratios, 'forward', cb.check(f'{name} forward', f32(y), *cb.bf16_bounds(ref, d), ref, S))
        info = nn.resized_weight_grad_info(n, size[0], size[1], c, (h, w), cout, k)
        bilinear_oracle.check_wgrad(f'{name} dW', call.param_grads['weight'], x, f32(dy), k, info['steps'] + 2 + info['reduce_chain'])
        judge_bias(call, ratios, f32(dy), bilinear_oracle.bgrad(f32(dy)), info['bias_chain'], rec[following_norm(name)])
        # T, the gradient at size, as the backward computed it (the same deterministic call), by the conv rule; dx on that T
        t = nn._common._run_conv(nn._common._nhwc(dy, BF16), nn.pack_weight(m.weight.detach(), 'dgrad'), None, cout, c, k)
        ref, S, d = cb.conv_with_noise(f32(dy), dense.unpack(dense.pack_dgrad(wq), cout, k), None, 1, k // 2, n=cb.chain_length(k, k, cout))
        note(ratios, 'T', cb.check(f'{name} T', f32(t), *cb.bf16_bounds(ref, d), ref, S))
        assert same_bits(call.grad_in[0], nn.bilinear_resize_backward(t, (h, w)))
        note(ratios, 'dx', bilinear_oracle.check_adjoint(f'{name} dx', f32(call.grad_in[0]), f32(t), (h, w)) or 0.)


def family_strided(rec, case, ratios):
    """The stride-2 shortcut: tests/test_gpu_bottleneck.py."""
    calls = [c for c in rec.calls if type(c.module) is nn.StridedConv1x1]
    assert len(calls) == 1
    for call in calls:
        m, name = call.module, call.name
        x, y, dy = bf16_operand(call.operands[0]), call.outputs[0], bf16_operand(call.grad_out[0])
        n, cin, h, w = x.shape
        cout = m.out_channels
        ho, wo = bottleneck_oracle.out_size(h), bottleneck_oracle.out_size(w)
        assert tuple(y.shape) == (n, cout, ho, wo) and (h % 2 or w % 2)  # the ceil is taken
        wq = cpu(m.weight).to(BF16).double()
        ref, S, d = cb.conv_with_noise(x, wq, None, 2, 0, n=cb.chain_length(1, 1, cin))
        note(ratios, 'forward', cb.check(f'{name} forward', f32(y), *cb.bf16_bounds(ref, d), ref, S))
        ref, S, d = cb.conv_with_noise(dy, dense.unpack(dense.pack_dgrad(wq), cout, 1), None, 1, 0, n=cb.chain_length(1, 1, cout))
        dx = f32(call.grad_in[0])
        note(ratios, 'dx', cb.check(f'{name} dx', dx[..., ::2, ::2], *cb.bf16_bounds(ref, d), ref, S))
        off_grid = dx.clone()
        off_grid[..., ::2, ::2] = 0
        assert bool((off_grid == 0).all())
        info = nn.weight_grad_info(n, ho, wo, cin, cout, 1)
        note(ratios, 'dW', check_sum(f'{name} dW', call.param_grads['weight'], *dense.wgrad(bottleneck_oracle.sub(x), dy, 1),
                                     info['steps'] + 2 + info['reduce_chain']))
        assert m.bias is None


def family_grouped(rec, case, ratios):
    """The grouped 3x3 conv2 of every block, stride 1 and 2: tests/test_gpu_grouped_conv.py."""
    calls = [c for c in rec.calls if type(c.module) is nn.GroupedConv2d]
    assert sorted(c.module.stride[0] for c in calls) == [1, 1, 1, 2]
    for call in calls:
        m, name = call.module, call.name
        x, y, dy = bf16_operand(call.operands[0]), call.outputs[0], bf16_operand(call.grad_out[0])
        n, c, h, w = x.shape
        stride, groups = m.stride[0], m.groups
        cig = c // groups
        wq = cpu(m.weight).to(BF16).double()
        bw, bundles = grouped_conv_oracle.geometry(c, cig)[:2]
        wd = grouped_conv_oracle.unpack(grouped_conv_oracle.pack_dgrad(wq)).reshape(c, bw, 3, 3)
        n_chain = cb.chain_length(3, 3, bw)
        ref, S, d = cb.conv_with_noise(x, wq, None, stride, 1, groups, n=n_chain)
        assert tuple(y.shape) == tuple(ref.shape)
        note(ratios, 'forward', cb.check(f'{name} forward', f32(y), *cb.bf16_bounds(ref, d), ref, S))
        dz = dy.double() if stride == 1 else grouped_conv_oracle.dilate(dy.double(), (h, w))
        ref, S, d = cb.conv_with_noise(dz, wd, None, 1, 1, bundles, n=n_chain)
        note(ratios, 'dx', cb.check(f'{name} dx', f32(call.grad_in[0]), *cb.bf16_bounds(ref, d), ref, S))
        info = nn.grouped_weight_grad_info(n, h, w, c, groups, stride)
        note(ratios, 'dW', check_sum(f'{name} dW', call.param_grads['weight'], *grouped_conv_oracle.wgrad(x, dy, cig, stride),
                                     info['steps'] + 2 + info['reduce_chain']))
        assert m.bias is None


def family_stem(rec, case, ratios):
    """The 7x7 stride-2 conv on the image (no input gradient: the image needs none): tests/test_gpu_stem.py."""
    call = rec[B + 'stem.0']
    m = call.module
    x, y, dy = f32(call.operands[0]), call.outputs[0], bf16_operand(call.grad_out[0])
    n, c, h, w = x.shape
    assert type(m) is nn.StemConv2d and c == case.channels and call.grad_in == {} and m.bias is None
    wq = cpu(m.weight).to(BF16).double()
    ref, S, d = cb.conv_with_noise(x, wq, None, 2, 3, n=STEM_CHAIN)
    note(ratios, 'forward', cb.check('stem forward', f32(y), *cb.bf16_bounds(ref, d), ref, S))
    info = nn.stem_weight_grad_info(n, h, w, m.out_channels)
    note(ratios, 'dW', check_sum('stem dW', call.param_grads['weight'], *stem_oracle.wgrad(x, dy), info['steps'] + 2 + info['reduce_chain']))


def family_pool(rec, case, ratios):
    """The max-pool: the forward is exact, the gradient goes to the first maximum of every window: tests/test_gpu_stem.py."""
    call = rec[B + 'pool']
    x, y, dy = bf16_operand(call.operands[0]), call.outputs[0], bf16_operand(call.grad_out[0])
    want, index = stem_oracle.pool_forward(x, 3, 2, 1)
    assert same_bits(cpu(y).contiguous(), want.to(BF16).contiguous())
    ref, S, count = stem_oracle.pool_backward(dy, index, tuple(x.shape[2:]), 3, 2, 1)
    judge_pool_gradient('pool dx', cpu(call.grad_in[0]), ref, S, count, BF16)
    assert int((x == 0).sum()) > x.numel() // 4  # post-ReLU: ties in many windows
    note(ratios, 'forward', 0.)


def judge_cat(call, ratios):
    """The decoder's resize + concat + conv: tests/test_gpu_cat_conv.py."""
    m, name = call.module, call.name
    lateral = bf16_operand(call.operands[0]) if 0 in call.operands else None
    top, y, dy = bf16_operand(call.operands[1]), call.outputs[0], bf16_operand(call.grad_out[0])
    assert (lateral is None) == name.endswith('layer_blocks.0.0') and call.extras == ({} if lateral is not None else {0: None})
    n, c1, h, w = top.shape
    c0 = 0 if lateral is None else lateral.shape[1]
    H, W = y.shape[2:]
    cout, k = m.out_channels, m.kernel_size[0]
    wq = cpu(m.weight).to(BF16).double()
    ref, S, d = cb.conv_with_noise(cat_conv_oracle.concat(lateral, top), wq, None, 1, k // 2, n=cb.chain_length(k, k, c0 + c1))
    note(ratios, 'forward', cb.check(f'{name} forward', f32(y), *cb.bf16_bounds(ref, d), ref, S))
    if c0:
        ref, S, d = cb.conv_with_noise(dy, dense.unpack(dense.pack_dgrad(wq[:, :c0]), cout, k), None, 1, k // 2, n=cb.chain_length(k, k, cout))
        note(ratios, 'd_lateral', cb.check(f'{name} d_lateral', f32(call.grad_in[0]), *cb.bf16_bounds(ref, d), ref, S))
    t = dtop_bounds(dy, wq[:, c0:], (h, w))
    note(ratios, 'd_top', cb.check(f'{name} d_top', f32(call.grad_in[1]), t['lo'], t['hi'], t['ref'], t['S']))
    info = nn.cat_weight_grad_info(n, H, W, c0, c1, (h, w), cout, k)
    note(ratios, 'dW', check_sum(f'{name} dW', call.param_grads['weight'], *cat_conv_oracle.wgrad(lateral, top, dy, k),
                                 info['steps'] + 2 + info['reduce_chain']))
    assert m.bias is None


def family_cat(rec, case, ratios):
    """The three levels of the decoder, the bridge level included."""
    calls = [c for c in rec.calls if type(c.module) is nn.CatConv2d]
    assert len(calls) == 3
    for call in calls:
        judge_cat(call, ratios)
    sizes = {c.name[-3]: (tuple(c.operands[1].shape[2:]), tuple(c.outputs[0].shape[2:])) for c in calls}
    assert sizes['2'][1][0] != 2 * sizes['2'][0][0] or sizes['2'][1][1] != 2 * sizes['2'][0][1]  # a nearest resize that is not x2


def judge_norm(call, ratios):
    """A norm, with or without the residual tail: tests/test_gpu_batch_norm.py and tests/test_gpu_bottleneck.py."""
    m, name = call.module, call.name
    x, y, dy = cpu(call.operands[0]), cpu(call.outputs[0]), cpu(call.grad_out[0])
    assert x.dtype == y.dtype == dy.dtype == BF16
    c = x.shape[1]
    chain_length = nn.batch_norm_info(x.numel() // c, c)['chain']
    mean, invstd, scale, shift = (cpu(v) for v in call.saved)
    weight, bias = cpu(m.weight), cpu(m.bias)
    got = dict(save_mean=mean, save_invstd=invstd, scale=scale, shift=shift, running_mean=cpu(call.buffers_after['running_mean']),
               running_var=cpu(call.buffers_after['running_var']))
    bo.judge_stats(name, x, got, chain_length, weight, bias, cpu(call.buffers_before['running_mean']),
                   cpu(call.buffers_before['running_var']), True, m.momentum, m.eps)
    relu = call.extras.get('activation', m.activation) == 'relu'
    grads = dict(dx=cpu(call.grad_in[0]), dgamma=cpu(call.param_grads['weight']), dbeta=cpu(call.param_grads['bias']))
    if 'residual' in call.operands:
        r = cpu(call.operands['residual'])
        assert relu and r.dtype == BF16
        bottleneck_oracle.judge_tail_y(name, x, r, y, scale, shift, relu)
        grads['dr'] = cpu(call.grad_in['residual'])
        bottleneck_oracle.judge_tail_grads(name, x, dy, y, grads, chain_length, weight, mean, invstd, relu, True)
    else:
        bo.judge_y(name, x, y, scale, shift, relu)
        bo.judge_grads(name, x, dy, grads, chain_length, weight, mean, invstd, scale, shift, relu, True)
    assert bool((grads['dgamma'] != 0).any()) and bool((grads['dbeta'] != 0).any()), name


def family_norm(rec, case, ratios):
    """All 25 norms, the four residual tails among them."""
    calls = [c for c in rec.calls if type(c.module) is nn.BatchNorm2d]
    assert len(calls) == 25 and sum('residual' in c.operands for c in calls) == 4
    for call in calls:
        judge_norm(call, ratios)


def family_tail(rec, case, ratios):
    """The four ReadOut tails with p = 0: tests/test_gpu_readout_tail.py."""
    calls = [c for c in rec.calls if type(c.module) is nn.DropoutConv1x1]
    assert len(calls) == 4
    for call in calls:
        m, name = call.module, call.name
        x, y, dy = bf16_operand(call.operands[0]), call.outputs[0], cpu(call.grad_out[0])
        n, cin, h, w = x.shape
        cout = m.out_channels
        assert y.dtype == dy.dtype == torch.float32 and y.is_contiguous() and m.p == 0.
        wq = cpu(m.weight).to(BF16).double().reshape(cout, cin)
        keep, s = torch.ones(n, cin, dtype=torch.float64), 1.
        gq = dy.to(BF16).double()
        info = nn.readout_tail_info(n, h * w, cin, cout)
        ref, S = readout_tail_oracle.forward(x, wq, cpu(m.bias), keep, s)
        d = cb.gamma(info['forward_chain']) * s * S
        d = d + cb.U * (ref.abs() + d)  # the rounding of the fma
        note(ratios, 'forward', cb.check(f'{name} forward', cpu(y), ref - d, ref + d, ref, S))
        ref, S = readout_tail_oracle.input_grad(gq, wq, keep, s)
        d = cb.gamma(info['dx_steps'] + 2) * s * S
        d = d + cb.U * (ref.abs() + d)  # the multiplication by s
        note(ratios, 'dx', cb.check(f'{name} dx', f32(call.grad_in[0]), *cb.bf16_bounds(ref, d), ref, S))
        ref, S = readout_tail_oracle.weight_grad(x, gq, keep, s)
        note(ratios, 'dW', check_sum(f'{name} dW', call.param_grads['weight'].reshape(cout, cin), ref, S, info['steps'] + 2 + info['reduce_chain']))
        ref, S = readout_tail_oracle.bias_grad(gq)
        note(ratios, 'db', check_sum(f'{name} db', call.param_grads['bias'], ref, S, info['bias_chain']))
        assert bool((call.param_grads['weight'] != 0).any()) and bool((call.param_grads['bias'] != 0).any()), name


def family_resize(rec, case, ratios):
    """The resize of the refinement map on fp32 planes (case B): tests/test_gpu_bilinear_resize.py."""
    calls = [c for c in rec.calls if c.name == 'bilinear_resize']
    assert len(calls) == (0 if case.full_res else 1)
    for call in calls:
        planes, out = call.operands[0], call.outputs[0]
        size, low = tuple(call.extras[1]), tuple(planes.shape[2:])
        assert planes.dtype == out.dtype == torch.float32 and size == (case.h, case.w) and low == (19, 25)
        bilinear_oracle.check_blend('head map', cpu(out), cpu(planes), size, stored='fp32')
        bilinear_oracle.check_adjoint('head map gradient', cpu(call.grad_in[0]), cpu(call.grad_out[0]), low, stored='fp32')


FAMILIES = dict(conv=family_conv, resized=family_resized, strided=family_strided, grouped=family_grouped, stem=family_stem, pool=family_pool,
                cat=family_cat, norm=family_norm, tail=family_tail, resize=family_resize)


@pytest.mark.parametrize('family', list(FAMILIES))
@case_ids
def test_every_call_lies_within_its_familys_bounds_on_the_operands_it_saw(case, family, monkeypatch):
    rec = chain(case.name)['rec']
    ratios, inner = {}, []
    check, within = cb.check, bo._within
    # the judges of the norm and of the resize do not hand their ratios back: listen to the two functions that all of them end in
    monkeypatch.setattr(cb, 'check', lambda *a, **kw: inner.append(check(*a, **kw)) or inner[-1])
    monkeypatch.setattr(bo, '_within', lambda *a, **kw: inner.append(within(*a, **kw)) or inner[-1])
    FAMILIES[family](rec, case, ratios)
    used = max(list(ratios.values()) + inner + [0.])
    print(f'case {case.name}, {family}: largest fraction of a bound used {used:.3f}; {ratios}')
    assert used <= 1


def altered(call, **fields):
    """A shallow copy of a record with some of its dicts replaced by altered copies: {field: {key: value}}."""
    new = copy.copy(call)
    for field, changes in fields.items():
        merged = dict(getattr(call, field))
        merged.update(changes)
        setattr(new, field, merged)
    return new


@case_ids
def test_faults_planted_in_the_gpu_records_are_flagged(case):
    """The bounds the GPU records pass are narrow enough to tell the faults this file exists for: each judge accepts the record as it
    is (parts C and D) and refuses it with one fault planted, as tests/test_train_step.py shows for the fp64 records."""
    rec = chain(case.name)['rec']
    # a share dropped at a fan-out
    (name, index, out), consumers = next(iter(standin.fan_out_converted().items()))
    shares = [rec.get(c, i).grad_in[key] for c, i, key in consumers]
    oracle.judge_fan_out(name, rec.get(name, index).grad_out[out], shares)
    with pytest.raises(AssertionError, match='not the sum'):
        oracle.judge_fan_out(name, rec.get(name, index).grad_out[out], shares[:-1])
    # the lateral of the neighbouring level (brought to the size)
    call = rec[B + 'unet.layer_blocks.1.0']
    wrong = torch.nn.functional.interpolate(rec[B + 'layer1.1.bn3'].outputs[0].float(), size=call.operands[0].shape[2:]).to(BF16)
    assert wrong.shape == call.operands[0].shape
    with pytest.raises(cb.BoundError, match='forward'):
        judge_cat(altered(call, operands={0: wrong}), {})
    # running statistics updated twice
    call = rec[B + 'layer2.0.downsample.1']
    mean, _ = oracle.batch_statistics64(call.operands[0])
    f = call.module.momentum
    twice = ((1 - f) * call.buffers_after['running_mean'].double().cpu() + f * mean).float().cuda()
    with pytest.raises(AssertionError, match='running_mean'):
        judge_norm(altered(call, buffers_after=dict(running_mean=twice)), {})
    # a skip gradient missing from a block input
    call = rec[B + 'layer1.1.conv1']
    without = (call.grad_in[0].float() - call.grad_out[1].float()).to(BF16)
    with pytest.raises(cb.BoundError, match='dx'):
        judge_conv(altered(call, grad_in={0: without}), {})
    # a transposed 1x1 weight gradient
    call = rec[B + 'layer2.1.conv1']
    assert call.param_grads['weight'].shape == (128, 128, 1, 1)
    with pytest.raises(AssertionError, match='dW'):
        judge_conv(altered(call, param_grads=dict(weight=call.param_grads['weight'].transpose(0, 1).contiguous())), {})


# ---- E: the step itself

HYPER = dict(lr=1e-3, betas=(.9, .999), eps=1e-8)
DECAY = 1e-2


@case_ids
def test_the_step_from_label_images_to_adamw(case):
    np.random.seed(3)
    gens = []
    for lab in standin.label_images(case):
        gen = cda.CPNTargetGenerator(samples=standin.SAMPLES, order=standin.ORDER)
        gen.feed(torch.as_tensor(lab[..., None]).cuda())
        gens.append(gen)
    targets = cda.collate_cpn_targets(gens)
    net = converted(case, p=.1)
    assert all(net.get_submodule(standin.head(h, 4)).p == .1 for h in standin.HEADS)
    objective = cda.CPNObjective(standin.ORDER, standin.SAMPLES, refinement_iterations=2)
    x, size = standin.image(case).cuda(), (case.h, case.w)
    named = dict(net.named_parameters())
    decayed = [k for k, p in named.items() if p.dim() == 4]
    plain = [k for k, p in named.items() if p.dim() == 1]  # norms and biases
    assert len(decayed) == 31 and len(plain) == 63
    groups = [dict(params=[named[k] for k in decayed], weight_decay=DECAY), dict(params=[named[k] for k in plain], weight_decay=0.)]
    opt = cda.optim.AdamW(groups, max_grad_norm=1., **HYPER)
    torch.manual_seed(21)
    with oracle.Recorder(net, lambda m: type(m) is nn.DropoutConv1x1) as tails:  # the four calls that draw from the generator
        maps = list(net['core'](x)[:4])
        arrived = {}
        for i, m in enumerate(maps):
            m.register_hook(lambda g, i=i: arrived.__setitem__(i, g.detach().clone()))
        loss, losses = objective(*maps, targets, size=size)
        loss.backward()
        tails.finish()
    assert bool(torch.isfinite(loss))
    # every tail alone, from the generator state it met: the same mask, hence the same bits; some channel of some image was dropped
    assert len(tails.calls) == 4 and len({bytes(call.rng.numpy()) for call in tails.calls}) == 4
    for call in tails.calls:
        oracle.compare_calls(call, oracle.replay(call, nn), oracle.assert_same_bits)
    assert any(bool((call.grad_in[0].float().abs().amax((2, 3)) == 0).any()) for call in tails.calls)
    # the objective alone on detached copies of the maps: the same gradients, bit for bit
    alone = [m.detach().clone().requires_grad_(True) for m in maps]
    loss_alone, _ = objective(*alone, targets, size=size)
    loss_alone.backward()
    assert same_bits(loss.detach(), loss_alone.detach())
    assert all(same_bits(arrived[i], a.grad) for i, a in enumerate(alone)) and all(bool((a.grad != 0).any()) for a in alone)
    # every gradient is there, contiguous, finite
    for k, p in named.items():
        assert p.grad is not None and p.grad.is_contiguous() and p.grad.shape == p.shape and p.grad.dtype == p.dtype, k
        assert bool(torch.isfinite(p.grad).all()), k
    order = decayed + plain
    params = [named[k] for k in order]
    host = [dict(p=optim_oracle.np_of(p).copy(), g=optim_oracle.np_of(p.grad).copy(), m=np.zeros(tuple(p.shape), np.float32),
                 v=np.zeros(tuple(p.shape), np.float32)) for p in params]
    sizes = sorted(p.numel() for p in params)
    assert len(sizes) == 94 and sizes[0] == 1 and sizes[-1] == 64 * 64 * 49 and len(set(sizes)) >= 10  # about a hundred tensors of mixed sizes
    opt.step()
    want = optim_oracle.norm_f64([h['g'] for h in host])
    norm = optim_oracle.np_of(opt.last_grad_norm)
    print(f'case {case.name}: loss {float(loss.detach()):.4f}, gradient norm {float(norm):.6f} (fp64 {want:.6f}), '
          f'|norm - fp64| / bound {abs(float(norm) - want) / (optim_oracle.norm_bound([h["g"] for h in host]) * want):.3f}')
    assert abs(float(norm) - want) <= optim_oracle.norm_bound([h['g'] for h in host]) * want
    coef = optim_oracle.clip_coef(norm, 1.)
    assert optim_oracle.same(opt.last_clip_coef, coef)
    for keys, decay in ((decayed, DECAY), (plain, 0.)):
        hyper = dict(HYPER, weight_decay=decay)
        lo = order.index(keys[0])
        part = slice(lo, lo + len(keys))
        # the float32 rule bit for bit, as tests/test_gpu_optim.py checks a step ...
        optim_oracle.assert_step(opt, params[part], host[part], [False] * len(keys), 1, hyper, coef)
        # ... and within the derived bounds of the fp64 rule
        for k, p, h in zip(keys, params[part], host[part]):
            ref = optim_oracle.step_f64(h['p'], h['g'], h['m'], h['v'], step=1, coef=float(coef), **hyper)
            bounds = optim_oracle.bounds(h['p'], h['g'], h['m'], h['v'], step=1, coef=float(coef), **hyper)
            state = opt.state[p]
            for what, got, r, e in zip('pmv', (p, state['exp_avg'], state['exp_avg_sq']), ref, bounds):
                err = np.abs(optim_oracle.np_of(got).astype(np.float64) - r)
                assert np.all(err <= e), (k, what, float((err / np.maximum(e, 1e-300)).max()))
    # a second step runs
    opt.zero_grad()
    maps = list(net['core'](x)[:4])
    loss2, _ = objective(*maps, targets, size=size)
    loss2.backward()
    opt.step()
    assert bool(torch.isfinite(loss2)) and all(float(opt.state[p]['step']) == 2 for p in params)
    assert all(bool(torch.isfinite(p).all()) for p in params)


# ---- F: buffers

@case_ids
def test_every_norm_updates_its_buffers_once_and_eval_leaves_them_alone(case):
    """After the first training forward every one of the 25 norms counts one batch and its running statistics lie within
    ``judge_stats`` of one update from the statistics of the input it saw; an eval forward under ``no_grad`` writes no buffer."""
    c = chain(case.name)
    rec = c['rec']
    norms = [call for call in rec.calls if type(call.module) is nn.BatchNorm2d]
    assert len(norms) == 25
    for call in norms:
        assert int(call.buffers_before['num_batches_tracked']) == 0 and int(call.buffers_after['num_batches_tracked']) == 1, call.name
        assert not same_bits(call.buffers_before['running_mean'], call.buffers_after['running_mean'])
        x = cpu(call.operands[0])
        chain_length = nn.batch_norm_info(x.numel() // x.shape[1], x.shape[1])['chain']
        mean, invstd, scale, shift = (cpu(v) for v in call.saved)
        got = dict(save_mean=mean, save_invstd=invstd, scale=scale, shift=shift, running_mean=cpu(call.buffers_after['running_mean']),
                   running_var=cpu(call.buffers_after['running_var']))
        bo.judge_stats(call.name, x, got, chain_length, cpu(call.module.weight), cpu(call.module.bias),
                       cpu(call.buffers_before['running_mean']), cpu(call.buffers_before['running_var']), True, call.module.momentum,
                       call.module.eps)
    net = copy.deepcopy(c['net']).eval()  # (after the three training forwards of ``chain``)
    assert all(int(m.num_batches_tracked) == 3 for m in net.modules() if type(m) is nn.BatchNorm2d)
    before = {k: b.clone() for k, b in net.named_buffers()}
    assert len(before) == 75
    with torch.no_grad():
        maps = net['core'](standin.image(case).cuda())[:4]
    assert all(bool(torch.isfinite(m).all()) and tuple(m.shape) == s for m, s in zip(maps, standin.map_shapes(case)))
    assert [k for k, b in net.named_buffers() if not same_bits(b, before[k])] == []
    assert not any(same_bits(a, b) for a, b in zip(maps, c['first'][0]))  # eval uses the running statistics: other maps


# ---- G: one global gate with a measured yardstick

@case_ids
def test_the_maps_against_stock_fp64_with_stock_bf16_autocast_as_the_yardstick(case):
    """Both are bf16 chains with the same operand roundings: at most twice the yardstick's error on every map.  A wrong route, a
    missing lateral or a mask error is of order 1.  The yardstick is stock torch, computed here, never the code under test."""
    maps64, grads64 = standin.stock_results(case.name, 'fp64')
    maps16, grads16 = standin.stock_results(case.name, 'bf16')
    maps, grads = chain(case.name)['first']
    for name, got, yard, ref in zip(('scores', 'locations', 'refinement', 'fourier'), maps, maps16, maps64):
        e, e16 = oracle.rel_l2(got, ref), oracle.rel_l2(yard, ref)
        print(f'case {case.name} {name}: relative L2 error {e:.3e}, stock bf16 autocast {e16:.3e}, ratio {e / e16:.3f}')
        assert 0 < e16 < float('inf') and e <= 2 * e16, name
    ours = sorted(oracle.rel_l2(grads[k], grads64[k]) for k in grads64)
    theirs = sorted(oracle.rel_l2(grads16[k], grads64[k]) for k in grads64)
    for what, e in (('this library', ours), ('stock bf16 autocast', theirs)):  # printed, not asserted: see the module docstring
        print(f'case {case.name} parameter gradients, {what}: median {e[len(e) // 2]:.3e}, smallest {e[0]:.3e}, largest {e[-1]:.3e}')
