"""The one-job pieces of the weight packer (celldetection_amd/pack.py): layouts, blob accumulator, member-op weights.  No GPU."""
import itertools

import pytest
import torch

from celldetection_amd import _lib, graph, pack


def _random_state_dict(plan):
    g = torch.Generator().manual_seed(0)
    return {key: torch.zeros(shape, dtype=torch.long) if kind == 'long' else torch.rand(shape, generator=g) + .5
            for key, shape, kind in plan.entries}


@pytest.mark.parametrize('kc,k,bundles,chunks', list(itertools.product((32, 64), (1, 2, 3), (1, 4), (1, 2))))
def test_records_round_trip_and_zero_slab(kc, k, bundles, chunks):
    cout_b, cin_b = 8, chunks * kc
    dense = torch.randn(bundles, cout_b, cin_b, k, k, dtype=torch.float64, generator=torch.Generator().manual_seed(k))
    records = pack._records(dense, kc)
    items = chunks * k * k
    assert records.shape == (bundles, items, cout_b, kc)
    for chunk, ky, kx in itertools.product(range(chunks), range(k), range(k)):  # item = (chunk of kc input channels, tap)
        assert torch.equal(records[:, chunk * k * k + ky * k + kx], dense[:, :, chunk * kc:(chunk + 1) * kc, ky, kx])
    assert torch.equal(pack._records_inverse(records, cin_b, k), dense)
    # in the blob: a zero slab behind the items of every bundle exactly when their number is odd
    prec = pack._precision('fp8' if kc == 64 else 'bf16')
    assert prec.kc == kc
    stored = pack._quantise_e4m3(records)[0] if prec.fp8 else records.to(torch.bfloat16)
    blobs = pack._Blobs(prec)
    assert blobs.weights(stored if prec.fp8 else records) == 0 and blobs.bias(torch.zeros(cout_b)) == 0
    wblob = blobs.finish('cpu')[0]
    assert wblob.dtype == stored.dtype and wblob.numel() == bundles * (items + items % 2) * cout_b * kc
    wblob = wblob.reshape(bundles, items + items % 2, cout_b, kc)
    assert torch.equal(wblob[:, :items], stored)
    assert not wblob[:, items:].view(torch.uint8).any()  # (empty when the count is even)


def test_fp32_layout():
    dense = torch.randn(2, 3, 5, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    taps = pack._taps_f32(dense)
    assert taps.shape == (2, 9, 5, 3)
    for ky, kx in itertools.product(range(3), range(3)):
        assert torch.equal(taps[:, ky * 3 + kx], dense[:, :, :, ky, kx].transpose(1, 2))
    blobs = pack._Blobs(pack._precision('fp32'))
    blobs.bias(torch.zeros(3))
    blobs.weights(taps)  # an odd tap count gets no slab in this layout (270 + 2 floats to the 8-element alignment)
    assert torch.equal(blobs.finish('cpu')[0][:taps.numel()], taps.reshape(-1).float()) and blobs.woff == (taps.numel() + 2) * 4


@pytest.mark.parametrize('precision', ['bf16', 'fp32', 'fp8'])
def test_accumulator_offsets(precision):
    prec = pack._precision(precision)
    blobs = pack._Blobs(prec)
    g = torch.Generator().manual_seed(1)
    woffs, entries = [], []
    for n, (items, cout_b, kc) in enumerate([(1, 1, 3), (2, 3, 5), (3, 7, 1), (4, 8, 32), (9, 2, 7), (1, 5, 5)]):
        records = torch.randn(2, items, cout_b, kc, dtype=torch.float64, generator=g)  # sizes that need slab and padding
        woffs.append(blobs.weights(torch.randint(0, 256, records.shape, dtype=torch.uint8, generator=g) if prec.fp8 else records))
        bias, mult = torch.randn(2 * cout_b, dtype=torch.float64, generator=g), torch.rand(2, cout_b, generator=g) + 1.
        entries.append((blobs.bias(bias, mult if n % 2 else None), bias, mult.reshape(-1) if n % 2 else torch.ones(2 * cout_b)))
        if n % 3 == 0 and not prec.f32:  # raw bf16 weights of an aligned size, as the stem's and the ReadOut tail's are
            woffs.append(blobs.raw_bf16(torch.randn(32, 8 * (n + 1), dtype=torch.float64, generator=g)))
    assert all(off % 16 == 0 for off in woffs) and len(set(woffs)) == len(woffs) and blobs.woff % 16 == 0
    wblob, fblob, nb = blobs.finish('cpu')
    assert wblob.numel() * wblob.element_size() == blobs.woff
    assert (nb is None) == (not prec.fp8) and fblob.numel() == blobs.boff * (2 if prec.fp8 else 1)
    for off, bias, mult in entries:  # a bias entry and its multipliers share their relative offset
        assert torch.equal(fblob[off:off + bias.numel()], bias.float())
        if prec.fp8:
            assert torch.equal(fblob[nb + off:nb + off + mult.numel()], mult.float())
    with pytest.raises(AssertionError):
        blobs.raw_bf16(torch.zeros(3))  # 6 bytes: the next offset would not be aligned


def test_fp8_multiplier_offsets_of_a_packed_plan():
    plan = graph.build_plan('ResNet18FPN', 3, subpixel='triples', bilinear_phases=True, fuse_bilinear=False,
                            backbone_kwargs=dict(fpn_channels=32, backbone_kwargs=dict(base_channel=8)))
    scales = [.01 + .001 * i for i in range(len(plan.tensors))]
    tens, ops, wblob, fblob, mblob, op_scales = pack.pack(plan, _random_state_dict(plan), 'cpu', precision='fp8', act_scales=scales)
    convs = [d for d in ops if d.op == _lib.OP_CONV]
    assert convs and {d.mult_offset - d.bias_offset for d in convs} == {fblob.numel() - mblob.numel()}
    assert mblob.numel() * 2 == fblob.numel() and all(d.weight_offset % 16 == 0 for d in ops if d.op == _lib.OP_CONV)
    assert all(d.mult_offset == -1 for d in ops if d.op != _lib.OP_CONV)


def test_share_parts_add_up_to_the_stated_conv():
    """Fuse2d over four features at cout = 8: the head input is built from partial 1x1 convs (``share`` ops), the last of them over
    [running sum | feature] with an identity block.  Side by side the parts are the stated conv; one of them carries its bias."""
    plan = graph.build_plan('U22', 3, features=dict(score=['0', '1', '2', '3']),
                            backbone_kwargs=dict(backbone_kwargs=dict(base_channels=8)))
    sd = _random_state_dict(plan)
    parts = sorted((op for op in plan.ops if op.get('share') is not None), key=lambda op: op['share'][0])
    assert len(parts) == 3 and [len(op['share']) for op in parts] == [3, 3, 4] and all(op['cout'] == 8 for op in parts)
    assert len({op['w'] for op in parts}) == 1
    w, b = pack._fold(sd, parts[0])
    assert w.shape == (8, 8 + 16 + 32 + 64, 1, 1) and bool((b != 0).all())
    ws, bs = zip(*(pack._member_weights(op, *pack._fold(sd, op)) for op in parts))
    assert torch.equal(ws[2][:, :8], torch.eye(8, dtype=torch.float64)[:, :, None, None])  # the running sum passes unchanged
    assert torch.equal(torch.cat((ws[0], ws[1], ws[2][:, 8:]), 1), w)
    assert [bool(b_.any()) for b_ in bs] == [False, False, True] and torch.equal(bs[2], b)
    # fp8: the sources' scales are folded in per source
    w8, _ = pack._member_weights(parts[2], *pack._fold(sd, parts[2]), c0=8, in_scales=(.5, .25))
    assert torch.equal(w8[:, :8], ws[2][:, :8] * .5) and torch.equal(w8[:, 8:], ws[2][:, 8:] * .25)


def test_graph_re_exports_the_packer():
    for name in ('pack', '_fold', '_bundle_geometry'):
        assert getattr(graph, name) is getattr(pack, name)
    for name in ('reference_flops', 'head_activation_name', 'Plan', 'build_plan', 'BACKBONES', '_two_conv_norm_relu', 'FUSE_READOUT'):
        assert hasattr(graph, name)
    assert 'graph' not in vars(pack)  # (graph imports pack, never the other way round)
