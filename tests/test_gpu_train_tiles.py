"""GPU tests of every weight-gradient slab kernel instantiation at its tile and chunk edges: the case table of tests/train_tiles.py
(what each entry shows is held without a GPU by tests/test_train_tiles.py), every entry at every slab_rows of it, twice.

Bound test.  Random bf16-exact operands; dW and db of the route's public ``*_weight_grad`` in fp32 against the fp64 statements of
the existing oracles, by the existing rule, imported: |got - ref| <= gamma(chain) * S + one fp32 rounding, chain = MFMA steps per
slab + 2 + reduce chain as the route's info call reports them (``check_sum`` of tests/test_gpu_conv_train.py); the resized route
with the allowance its own test makes for the bf16 blend of the staged row (``bilinear_oracle.check_wgrad``).  Where S = 0 -- the
taps an image narrower or shorter than the padding never reaches -- the bound is 0.  No allowance counts, no share left out.

Exact test.  The same entries with integers in [-4, 4]: every product and partial sum is an integer below 2^24 (asserted), so the
fp32 result is the fp64 statement bit for bit whatever the order of the sum, and a dropped, doubled or misplaced pixel, tile or
tap is a wrong integer at a named place.  Resized entries take part where their blend weights are multiples of 1 / 16
(``train_tiles.dyadic``; the others are named in ``train_tiles.INEXACT``): there the staged bf16 blend of integers is exact, too.

Every failure message starts with ``train_tiles.locate``: instantiation, tile, fragment and tap of the worst element.
"""
import pytest
import torch

import bilinear_oracle
import conv_bounds as cb
import train_tiles as tt
from test_gpu_conv_train import check_sum

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def chain_of(key, slab_rows):
    cfg = tt.TABLE[key]
    info = tt.info(key, slab_rows)
    chain = info['steps'] + 2 + info['reduce_chain']
    assert chain <= -(-cfg['n'] * cfg['h'] * cfg['w'] // 16) + 2 + info['slabs'], info
    assert slab_rows == 0 or info['slab_rows'] == min(slab_rows, cfg['n'] * cfg['h'])
    return info, chain


def shapes_of(key):
    route, k, _ = tt.parse_key(key)
    cfg = tt.TABLE[key]
    return (cfg['cout'], cfg['cin'], k, k), (cfg['cout'],)


@pytest.mark.parametrize('case', tt.cases(), ids=tt.case_id)
def test_weight_and_bias_gradient_within_the_chain_bound(case):
    key, slab_rows = case
    route, k, _ = tt.parse_key(key)
    info, chain = chain_of(key, slab_rows)
    o = tt.operands(key, 'normal')
    dw, db = tt.weight_grad(key, o, slab_rows)
    assert dw.dtype == db.dtype == torch.float32 and (tuple(dw.shape), tuple(db.shape)) == shapes_of(key)
    if route == 'resized':
        ref, tol = bilinear_oracle.wgrad_tolerance(o['x'], o['dy'], k, chain)
    else:
        ref, S = o['wgrad']
        d = cb.gamma(chain) * S
        tol = d + cb.U * (ref.abs() + d)
    where = tt.locate(key, tt.worst_index((dw.double().cpu() - ref).abs(), tol))  # (tol names the element; the judges below assert)
    name = f'{where}; dW slab_rows {slab_rows} ({info["slabs"]} slabs of {info["slab_rows"]} rows)'
    if route == 'resized':
        worst = bilinear_oracle.check_wgrad(name, dw, o['x'], o['dy'], k, chain)
    else:
        worst = check_sum(name, dw, ref, S, chain)
    print(f'{key}@{slab_rows}: largest error / bound of dW to six places {worst:.6f}')
    ref_b, S_b = o['bgrad']
    worst_b = int(torch.argmax((db.double().cpu() - ref_b).abs()))
    check_sum(f'{tt.locate_bias(key, worst_b)}; db slab_rows {slab_rows}', db, ref_b, S_b, info['bias_chain'])


@pytest.mark.parametrize('case', [c for c in tt.cases() if tt.dyadic(c[0])], ids=tt.case_id)
def test_small_integers_are_bit_equal_to_the_statement(case):
    key, slab_rows = case
    o = tt.operands(key, 'integer')
    ref, S = o['wgrad']
    # the premise: every partial sum, in units of the blend weights' 1 / 16, is an integer below 2^24
    assert torch.equal(ref * 16, (ref * 16).round()) and float(S.max()) * 16 < 2 ** 24 and float(o['bgrad'][1].max()) < 2 ** 24
    dw, db = tt.weight_grad(key, o, slab_rows)
    assert dw.dtype == db.dtype == torch.float32 and (tuple(dw.shape), tuple(db.shape)) == shapes_of(key)
    got = dw.double().cpu()
    wrong = got != ref
    if bool(wrong.any()) or not bool(torch.isfinite(dw).all()):
        at = tt.worst_index((got - ref).abs(), torch.zeros_like(ref))
        taps = sorted({(int(i[2]), int(i[3])) for i in wrong.nonzero()[:2000]})
        raise AssertionError(f'{tt.locate(key, at)}; slab_rows {slab_rows}: got {float(got[at])}, the statement is {float(ref[at])}; '
                             f'{int(wrong.sum())} of {wrong.numel()} elements differ, in co {sorted(set(wrong.nonzero()[:, 0].tolist()))[:6]} ..., '
                             f'ci {sorted(set(wrong.nonzero()[:, 1].tolist()))[:6]} ..., taps {taps[:8]}')
    got_b, ref_b = db.double().cpu(), o['bgrad'][0]
    if not torch.equal(got_b, ref_b):
        at = int(torch.argmax((got_b - ref_b).abs()))
        raise AssertionError(f'{tt.locate_bias(key, at)}; slab_rows {slab_rows}: got {float(got_b[at])}, the statement is {float(ref_b[at])}')


@pytest.mark.parametrize('key', [f'{route}/k{k}/tiles' for route in tt.ROUTES for k in (3, 7)])
def test_bf16_gradients_are_the_fp32_ones_rounded_once_and_runs_agree(key):
    o = tt.operands(key, 'normal')
    slab_rows = tt.TABLE[key]['slab_rows'][0]
    dw, db = tt.weight_grad(key, o, slab_rows)
    dw2, db2 = tt.weight_grad(key, o, slab_rows)
    assert same_bits(dw, dw2) and same_bits(db, db2), f'{key}: two runs differ'
    dw16, db16 = tt.weight_grad(key, o, slab_rows, dtype=torch.bfloat16)
    assert dw16.dtype == db16.dtype == torch.bfloat16
    if not torch.equal(dw16, dw.to(torch.bfloat16)):
        at = tt.worst_index((dw16.double() - dw.to(torch.bfloat16).double()).abs().cpu(), torch.zeros(dw.shape, dtype=torch.float64))
        raise AssertionError(f'{tt.locate(key, at)}: the bf16 gradient is not the fp32 one rounded once')
    assert torch.equal(db16, db.to(torch.bfloat16)), f'{key}: the bf16 bias gradient is not the fp32 one rounded once'
