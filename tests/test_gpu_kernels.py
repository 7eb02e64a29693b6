"""GPU parity tests of the individual HIP kernels, called through the C ABI (ctypes).

* conv (test_conv and its mode variants, e4m3): every output within the rounding bound of the fp64 conv of exactly the
  operands the kernel reads (tests/conv_bounds.py), outputs written between guard bands, padded channels zero.
* pool / resize / input conversion and the remaining conv-family tests: a plain PyTorch fp32 CPU reference of the same op
  on the same bf16-rounded operands.
* compaction / decode / refinement / NMS / border filter: compared bit-exactly with the CPU oracle and with the
  golden vectors generated from the reference.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_bounds as cb
import read_guards as rg

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _pad32(c):
    return (c + 31) // 32 * 32


def to_nhwc_bf16(x, cpad=None):
    """NCHW fp32 -> NHWC bf16 with zero-padded channels."""
    n, c, h, w = x.shape
    cpad = cpad or _pad32(c)
    out = torch.zeros(n, h, w, cpad, dtype=torch.bfloat16, device=x.device)
    out[..., :c] = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    return out.contiguous()


def from_nhwc(y, c):
    return y[..., :c].permute(0, 3, 1, 2).float()


guarded, assert_guards, BF16_GUARD, F32_GUARD = cb.guarded, cb.assert_guards, cb.BF16_GUARD, cb.F32_GUARD


def conv_plan(*, cin, cout, k, stride=1, groups=1, bias=True, bn=True, act='relu', cin1=0, up0=False, up1=False, res=False,
              res_up=False, out_f32=False, act_scale=3., seed=0, fuse_cout=0, fuse_act='none', bilinear=False, **_):
    """The one-conv plan of run_conv and its seeded parameters -> (plan, state dict, generator); needs no GPU
    (tests/conv_tiles.py asks the library which kernel the same plan runs)."""
    from celldetection_amd import _lib, graph
    g = torch.Generator().manual_seed(seed)
    P = graph.Plan()
    s0 = P.tensor(cin, 2 if (up0 or bilinear) else 1)
    if bilinear:  # source stored at half resolution, read through the fused bilinear resize (MODE_BL)
        up0 = 'bilinear'
    s1 = P.tensor(cin1, 2 if up1 else 1) if cin1 else None
    r = P.tensor(cout, (2 if res_up else 1) * stride) if res else None
    P.conv(s0, cout, k, w='c.', bn='b.' if bn else None, bias=bias, stride=stride, groups=groups, act=act,
           act_scale=act_scale, src1=s1, up0=up0, up1=up1, res=r, res_up=res_up,
           out_index=_lib.OUT_SCORES if (out_f32 or fuse_cout) else None,
           fuse=dict(w='f.', cout=fuse_cout, act=fuse_act, act_scale=act_scale) if fuse_cout else None)
    return P, random_state_dict(P, g), g


def random_state_dict(P, g):
    sd = {}
    for key, shape, kind in P.entries:
        if key.endswith('running_var'):
            sd[key] = torch.rand(shape, generator=g) + .5
        elif key.endswith('num_batches_tracked'):
            sd[key] = torch.zeros((), dtype=torch.long)
        elif len(shape) == 4:
            sd[key] = torch.randn(shape, generator=g) / np.sqrt(np.prod(shape[1:]))
        else:
            sd[key] = torch.randn(shape, generator=g) * .5 + (1. if key.endswith('b.weight') else 0.)
    return sd


def run_conv(dev, *, n, h, w, cin, cout, k, stride=1, groups=1, bias=True, bn=True, act='relu', cin1=0, up0=False,
             up1=False, res=False, res_up=False, out_f32=False, act_scale=3., seed=0, fuse_cout=0, fuse_act='none',
             bilinear=False, reference=True, embed=None):
    """Builds a one-conv plan, runs cpn_conv2d -> (got as fp32 NCHW CPU tensor, bound check or None, out_f32).
    ``embed``: a byte pattern of tests/read_guards.py; the two sources and the residual then lie between bands of that pattern,
    which must come back intact around unchanged operands, and the library must have received exactly those pointers.

    The output lies in a buffer with guard bands (a whole output row before and after bf16 NHWC outputs, a whole plane
    around fp32 NCHW ones) that must come back untouched; the padded channels cout..cpad of a bf16 output must be zeros
    (the next conv reduces over them: NaN x 0 = NaN).  The check (tests/conv_bounds.py) holds the fp64 conv of exactly the
    operands the kernel reads; check(name, got) asserts every element and returns the largest |got - ref| / bound.
    Resized sources are stored at (Hin >> 1, Win >> 1) and read through the nearest rule floor(dst * Hs / Hin) of
    F.interpolate(size=...): odd Hin / Win included."""
    from celldetection_amd import _lib, graph
    P, sd, g = conv_plan(cin=cin, cout=cout, k=k, stride=stride, groups=groups, bias=bias, bn=bn, act=act, cin1=cin1, up0=up0,
                         up1=up1, res=res, res_up=res_up, out_f32=out_f32, act_scale=act_scale, seed=seed, fuse_cout=fuse_cout,
                         fuse_act=fuse_act, bilinear=bilinear)
    hin, win = h, w
    up0 = up0 or bilinear
    out_f32 = out_f32 or bool(fuse_cout)
    tens, ops, wblob, bblob = graph.pack(P, sd, dev)
    op = ops[0]

    def mk(c, hh, ww):
        return (torch.randn(n, c, hh, ww, generator=g)).to(torch.bfloat16).float()

    x0 = mk(cin, hin >> 1 if up0 else hin, win >> 1 if up0 else win)
    x1 = mk(cin1, hin >> 1 if up1 else hin, win >> 1 if up1 else win) if cin1 else None
    ho, wo = (hin + 2 * (k // 2) - k) // stride + 1, (win + 2 * (k // 2) - k) // stride + 1
    xr = mk(cout, ho >> 1 if res_up else ho, wo >> 1 if res_up else wo) if res else None
    d0 = to_nhwc_bf16(x0.to(dev))
    d1 = to_nhwc_bf16(x1.to(dev)) if cin1 else None
    dr = to_nhwc_bf16(xr.to(dev)) if res else None
    lib = _lib.load()
    e = rg.Embedding(embed)
    d0, d1, dr = e('src0', d0), e('src1', d1), e('res', dr)
    cout_out = fuse_cout or cout
    if out_f32:
        guard, sentinel = ho * wo, F32_GUARD
        dst, buf = guarded((n, cout_out, ho, wo), torch.float32, guard, sentinel, dev)
        dstride = 0
    else:
        guard, sentinel = wo * _pad32(cout), BF16_GUARD
        dst, buf = guarded((n, ho, wo, _pad32(cout)), torch.bfloat16, guard, sentinel, dev)
        dstride = _pad32(cout)
    with e.watch(lib, 'cpn_conv2d'):
        _lib.check(lib.cpn_conv2d(op, _lib.ptr(d0), d0.shape[-1], _lib.ptr(d1), 0 if d1 is None else d1.shape[-1],
                                  _lib.ptr(dr), 0 if dr is None else dr.shape[-1], _lib.ptr(dst), dstride, n, hin, win,
                                  _lib.ptr(wblob), _lib.ptr(bblob), _lib.stream_ptr()), 'conv2d')
    torch.cuda.synchronize()
    assert_guards('conv2d', buf, guard, sentinel)
    e.check()
    if out_f32:
        got = dst.cpu()
    else:
        pad = dst.cpu()[..., cout:].float()
        assert bool((pad == 0).all()), f'padded output channels {cout}..{_pad32(cout)} are not zero ' \
                                       f'({int((pad != 0).sum())} elements, e.g. {pad[pad != 0][:4].tolist()})'
        got = from_nhwc(dst.cpu(), cout)
    if not reference:
        return got, None, out_f32
    # ---- reference: fp64 conv on exactly the operands the kernel reads (folded weights rounded as graph.pack rounds them)
    wf, bf = graph._fold(sd, P.ops[0])
    wq = wf.to(torch.bfloat16).double()
    bq = bf.to(torch.float32).double()
    half = None
    if bilinear:  # blended in fp32 and rounded to bf16 inside the kernel: an interval operand
        xin, half = cb.bilinear_bf16_operand(x0, (hin, win))
    else:
        xin = F.interpolate(x0.double(), size=(hin, win), mode='nearest') if up0 else x0.double()
    if cin1:
        xin = torch.cat((xin, F.interpolate(x1.double(), size=(hin, win), mode='nearest') if up1 else x1.double()), 1)
    xres = None
    if res:
        xres = F.interpolate(xr.double(), size=(ho, wo), mode='nearest') if res_up else xr.double()
    nchain = cb.chain_length(k, k, cb.cin_read(cin + (_pad32(cin) - cin if cin1 else 0) + cin1, cout, groups))
    ref, S, d = cb.conv_with_noise(xin, wq, bq, stride, k // 2, groups, n=nchain, x_half=half, res=xres)
    if fuse_cout:  # fused ReadOut tail: the hidden activation is rounded to bf16 inside the kernel
        w2 = sd['f.weight'].double().to(torch.bfloat16).double().reshape(fuse_cout, cout)
        ref, S, d = cb.fused_tail(ref, d, w2, sd['f.bias'].to(torch.float32), act=act, act_scale=act_scale)
        act = fuse_act
    if out_f32:
        lo, hi = cb.f32_bounds(ref, d, act, act_scale)
    else:
        lo, hi = cb.bf16_bounds(ref, d, act, act_scale)
    return got, cb.Bounds(cb.apply_act(ref, act, act_scale), S, lo, hi), out_f32


CONV_CASES = {
    '1x1_64_64': dict(n=2, h=32, w=32, cin=64, cout=64, k=1),
    '1x1_flat_narrow': dict(n=4, h=16, w=16, cin=128, cout=256, k=1, act='none'),
    '1x1_res': dict(n=1, h=32, w=64, cin=96, cout=128, k=1, res=True),
    '1x1_s2': dict(n=2, h=32, w=32, cin=64, cout=128, k=1, stride=2, act='none'),
    '3x3_64_64': dict(n=2, h=32, w=32, cin=64, cout=64, k=3),
    '3x3_odd_channels': dict(n=1, h=32, w=64, cin=8, cout=24, k=3),
    '3x3_256_small_grid_4x64_tile': dict(n=1, h=64, w=64, cin=64, cout=256, k=3),  # 128 blocks at 4x256: the grid shrinks the tile
    '3x3_s2': dict(n=2, h=64, w=64, cin=32, cout=64, k=3, stride=2),
    '3x3_grouped_cpg8': dict(n=1, h=32, w=32, cin=256, cout=256, k=3, groups=32),
    '3x3_grouped_cpg64_s2': dict(n=1, h=32, w=32, cin=128, cout=128, k=3, groups=2, stride=2),
    '3x3_grouped_cpg1': dict(n=1, h=32, w=32, cin=32, cout=32, k=3, groups=32),
    '3x3_concat_up': dict(n=2, h=32, w=32, cin=64, cout=64, k=3, cin1=128, up1=True),
    '3x3_concat_up_pad': dict(n=1, h=32, w=32, cin=8, cout=16, k=3, cin1=16, up1=True),
    '3x3_bridge_up0': dict(n=1, h=64, w=64, cin=64, cout=64, k=3, up0=True, bias=False),
    '1x1_fpn_lateral': dict(n=2, h=32, w=32, cin=64, cout=256, k=1, res=True, res_up=True, bn=False, act='none'),
    '3x3_c64_th16_tile': dict(n=4, h=256, w=256, cin=64, cout=64, k=3),
    '7x7_c64_th16_tile': dict(n=4, h=256, w=256, cin=64, cout=64, k=7, seed=3),
    '7x7_head': dict(n=1, h=32, w=64, cin=64, cout=64, k=7),
    '7x7_head_256': dict(n=1, h=32, w=32, cin=256, cout=256, k=7),
    '7x7_stem_s2': dict(n=2, h=64, w=64, cin=3, cout=64, k=7, stride=2, bias=False),
    # more of the 64-output-channel tiles: a fused ReadOut head with 64 hidden units on <16,64,2,2>, a concat source with partial
    # tiles, three chunks of a 5x5
    'c64_fused_head_th16': dict(n=4, h=256, w=256, cin=64, cout=64, k=7, fuse_cout=2, fuse_act='tanh_scaled', seed=11),
    'c64_concat_up_partial': dict(n=3, h=40, w=72, cin=32, cout=64, k=3, cin1=64, up1=True, seed=12),
    'c64_k5_three_chunks': dict(n=2, h=64, w=64, cin=96, cout=64, k=5, seed=13),
    # 1024 blocks of 8 x 32 x 128: the plain 3x3 runs MODE_S1F <8,128,4,2>; the concat source and the fused head keep the flagship
    # <8,256,4,2> tile (tests/conv_tiles.py RECORDED holds what every case here runs; tests/test_conv_tiles.py asserts it)
    '3x3_256_flagship_tile': dict(n=8, h=128, w=128, cin=64, cout=256, k=3),
    '3x3_256_flagship_concat_up': dict(n=8, h=128, w=128, cin=32, cout=256, k=3, cin1=64, up1=True, seed=7),
    'fused_head_256_flagship_tile': dict(n=8, h=128, w=128, cin=96, cout=256, k=7, fuse_cout=20, fuse_act='none', seed=9),
    # outputs exactly 16 pixels wide: MODE_N (a pixel fragment = two rows x 16 columns)
    '3x3_narrow16_flagship': dict(n=16, h=16, w=16, cin=64, cout=512, k=3, seed=21),
    '3x3_narrow16_rows24_res': dict(n=2, h=24, w=16, cin=32, cout=64, k=3, res=True, seed=22),
    '3x3_narrow16_grouped': dict(n=4, h=16, w=16, cin=256, cout=256, k=3, groups=8, seed=23),
    '3x3_narrow16_concat_up': dict(n=8, h=16, w=16, cin=64, cout=256, k=3, cin1=96, up1=True, seed=24),
    '7x7_narrow16_fused_head': dict(n=4, h=32, w=16, cin=64, cout=128, k=7, fuse_cout=20, fuse_act='none', seed=25),
    '5x5_narrow16_f32_out': dict(n=2, h=16, w=16, cin=32, cout=3, k=5, bn=False, act='tanh_scaled', out_f32=True, seed=26),
    '1x1_flagship_tile': dict(n=16, h=32, w=32, cin=96, cout=1024, k=1, seed=11),
    '1x1_flagship_tile_res': dict(n=16, h=32, w=32, cin=64, cout=1024, k=1, res=True, seed=13),
    'fused_head_256': dict(n=1, h=32, w=64, cin=64, cout=256, k=7, fuse_cout=20, fuse_act='none'),
    'fused_head_128_sigmoid': dict(n=2, h=32, w=32, cin=32, cout=128, k=3, fuse_cout=1, fuse_act='sigmoid'),
    'fused_head_64_tanh_th16': dict(n=4, h=256, w=256, cin=64, cout=64, k=7, fuse_cout=2, fuse_act='tanh_scaled', seed=5),
    'fused_head_64_tanh': dict(n=1, h=32, w=32, cin=64, cout=64, k=7, fuse_cout=2, fuse_act='tanh_scaled'),
    'fused_head_small': dict(n=1, h=32, w=64, cin=8, cout=8, k=7, fuse_cout=20, fuse_act='none'),
    '7x7_bilinear_src_256': dict(n=1, h=64, w=64, cin=64, cout=256, k=7, bilinear=True),
    '3x3_bilinear_src_32': dict(n=2, h=32, w=64, cin=16, cout=24, k=3, bilinear=True),
    'fused_head_64_bilinear': dict(n=1, h=64, w=96, cin=64, cout=64, k=7, fuse_cout=2, fuse_act='tanh_scaled', bilinear=True),
    'fused_head_256_bilinear': dict(n=1, h=32, w=64, cin=256, cout=256, k=7, fuse_cout=2, fuse_act='tanh_scaled', bilinear=True),
    'final_sigmoid': dict(n=2, h=32, w=32, cin=64, cout=1, k=1, bn=False, act='sigmoid', out_f32=True),
    'final_tanh': dict(n=1, h=64, w=32, cin=64, cout=2, k=1, bn=False, act='tanh_scaled', out_f32=True),
    'final_fourier': dict(n=1, h=32, w=32, cin=128, cout=20, k=1, bn=False, act='none', out_f32=True),
}


@pytest.mark.parametrize('name', list(CONV_CASES))
def test_conv(dev, name):
    """Every output within the rounding bound of the fp64 conv of the same operands (tests/conv_bounds.py)."""
    got, chk, f32 = run_conv(dev, **CONV_CASES[name])
    ratio = chk(name, got)
    print(f'{name}: max |got - ref| / bound = {ratio:.3g}')


def test_conv_rejects_a_resized_source_of_no_pixels(dev):
    """A nearest-resized source is stored at (Hin >> 1, Win >> 1): at Hin = 1 it holds no pixels, and cpn_conv2d rejects
    the call with CPN_E_INVALID (-1) instead of launching."""
    with pytest.raises(RuntimeError, match=r'conv2d failed \(code -1\)'):
        run_conv(dev, n=1, h=1, w=40, cin=32, cout=32, k=1, up0=True)


S1F_CASES = {
    # MODE_S1F (two 4-wave workgroups per CU, flat pitch-36 halo tile): CPN_S1F=2 forces it wherever the kernel applies
    's1f_3x3_256': dict(n=8, h=128, w=128, cin=64, cout=256, k=3),                 # the decoder's 3x3 class
    's1f_3x3_one_chunk': dict(n=2, h=64, w=64, cin=32, cout=128, k=3, seed=31),   # a single chunk: one halo buffer
    's1f_3x3_partial_tiles': dict(n=3, h=44, w=72, cin=96, cout=256, k=3, seed=32),   # ragged rows / columns, 3 chunks
    's1f_3x3_res': dict(n=2, h=64, w=96, cin=64, cout=128, k=3, res=True, seed=33),
    's1f_5x5_falls_back': dict(n=2, h=64, w=64, cin=64, cout=128, k=5, seed=34),   # two halo tiles + slabs > 80 KiB: the plain tiles run
    's1f_2x2ish_k3_cin2048': dict(n=1, h=32, w=64, cin=2048, cout=128, k=3, seed=39),   # 64 chunks through the two-buffer ring
    's1f_3x3_512_two_blocks': dict(n=4, h=64, w=64, cin=128, cout=512, k=3, seed=36),   # four cout blocks folded into x
    's1f_3x3_odd_tile_count': dict(n=3, h=24, w=40, cin=64, cout=384, k=3, seed=37),    # tiles not a multiple of 8: padded grid
    's1f_3x3_no_bias_none': dict(n=1, h=32, w=32, cin=64, cout=128, k=3, bias=False, bn=False, act='none', seed=38),
}


@pytest.mark.parametrize('name', list(S1F_CASES))
def test_conv_two_workgroups_per_cu_mode(dev, name, monkeypatch):
    """MODE_S1F against the flagship path (CPN_S1F=0): same operands, K order and MFMA sequence per output element ->
    bit-identical; and within the rounding bound of the fp64 conv."""
    cfg = S1F_CASES[name]
    monkeypatch.setenv('CPN_S1F', '0')
    base, chk, _ = run_conv(dev, **cfg)
    monkeypatch.setenv('CPN_S1F', '2')
    got, _, _ = run_conv(dev, **cfg, reference=False)
    assert torch.isfinite(got).all()
    assert torch.equal(got, base), f'{name}: MODE_S1F differs from the one-workgroup-per-CU tiles ' \
                                   f'(max abs {(got - base).abs().max().item():.3e}, {(got != base).float().mean().item():.2e} of the outputs)'
    chk(name, base)


S1Q_CASES = {
    # MODE_S1Q (four K items per pipeline step, flat pitch-40 halo tiles) on the 64-output-channel 5x5 / 7x7 convs.  The mode needs
    # 448 tiles of 16 x 32: the first two cases run it, the last three (320, 288 and 256 tiles) run MODE_S1 <8,64,2,2> under either
    # switch value (tests/conv_tiles.py RECORDED); bf16/S1Q/16x64 and its +res entry there are the ragged / residual cases of the mode
    's1q_7x7_64_64': dict(n=4, h=256, w=256, cin=64, cout=64, k=7, seed=41),                      # 98 items -> 100 (two read zeros)
    's1q_7x7_fused_head': dict(n=4, h=256, w=256, cin=64, cout=64, k=7, fuse_cout=2, fuse_act='tanh_scaled', seed=42),
    's1q_7x7_one_chunk': dict(n=8, h=128, w=160, cin=32, cout=64, k=7, seed=43),                   # 49 items -> 52 (three read zeros)
    's1q_5x5_three_chunks_ragged': dict(n=6, h=120, w=176, cin=96, cout=64, k=5, seed=44),         # 75 items, partial tiles
    's1q_7x7_res': dict(n=4, h=128, w=256, cin=64, cout=64, k=7, res=True, seed=45),
}


@pytest.mark.parametrize('name', list(S1Q_CASES))
def test_conv_four_items_per_step_mode(dev, name, monkeypatch):
    """MODE_S1Q against the two-items-per-step loop (CPN_S1Q=0): same K order and MFMA sequence per output element -> bit-identical;
    and within the rounding bound of the fp64 conv."""
    cfg = S1Q_CASES[name]
    monkeypatch.setenv('CPN_S1Q', '0')
    base, chk, _ = run_conv(dev, **cfg)
    monkeypatch.setenv('CPN_S1Q', '1')
    got, _, _ = run_conv(dev, **cfg, reference=False)
    assert torch.isfinite(got).all()
    assert torch.equal(got, base), f'{name}: MODE_S1Q differs from the two-item loop (max abs {(got - base).abs().max().item():.3e}, ' \
                                   f'{(got != base).float().mean().item():.2e} of the outputs)'
    chk(name, base)


SUBPIXEL_CASES = {
    'sp_64_128_64': dict(n=2, h=32, w=32, c0=64, c1=128, cout=64),
    'sp_padded_channels': dict(n=1, h=64, w=64, c0=8, c1=16, cout=16),
    'sp_partial_tiles': dict(n=2, h=40, w=48, c0=32, c1=64, cout=96, seed=3),
    'sp_flagship_tile': dict(n=8, h=128, w=128, c0=32, c1=64, cout=256, seed=5),
    'sp_two_cout_blocks': dict(n=4, h=64, w=64, c0=64, c1=64, cout=512, seed=7),
    'sp_no_bias': dict(n=1, h=32, w=64, c0=32, c1=32, cout=32, bias=False, seed=9),
    'sp_narrow_lowres': dict(n=16, h=32, w=32, c0=64, c1=128, cout=256, seed=11),  # phase conv on 16 x 16 maps: MODE_N
}


def subpixel_plan(c):
    """The three-op plan (HEAD, PHASE, LATERAL) of test_subpixel_decoder_conv and its seeded parameters -> (plan, state dict,
    generator, id of the partial-sum tensor); needs no GPU."""
    from celldetection_amd import graph
    c = dict(dict(bias=True, seed=0), **c)
    c0, c1, cout = (c[k] for k in ('c0', 'c1', 'cout'))
    g = torch.Generator().manual_seed(c['seed'])
    P = graph.Plan()
    lat, top = P.tensor(c0, 1), P.tensor(c1, 2)
    kw = dict(w='c.', bn='b.', bias=c['bias'])
    x = P.conv(lat, cout, 3, act='relu', src1=top, up1=True, sub='head', **kw)
    ph = P.conv(top, cout, 2, pad=1, sub=('phase', c0), **kw)
    P.conv(lat, cout, 3, act='relu', res=ph, res_up='shuffle', sub=('lateral', c0), dst=x, **kw)
    return P, random_state_dict(P, g), g, ph


@pytest.mark.parametrize('name', list(SUBPIXEL_CASES))
def test_subpixel_decoder_conv(dev, name, embed=None):
    """Sub-pixel triple of a UNet decoder conv over cat(lateral, nearest-x2-upsampled top-down map)
    (models/unet.py:213-224): PHASE (four 2x2 convs on the low-resolution map) + LATERAL (3x3 on the lateral, pixel-
    shuffled partial sums as residual) against (a) an fp32 emulation of exactly that arithmetic on the same bf16-rounded
    operands -- tap sums rounded to bf16 ONCE, partial sums rounded to bf16 -- and (b) the HEAD conv = the reference's
    statement of the layer (both approximate the fp32 conv; they differ by the rounding of the tap sums and partials).
    ``embed`` (tests/test_gpu_read_guards.py; a byte pattern of tests/read_guards.py): both sources lie between bands of that
    pattern, checked as in run_conv, and the three stored results are returned after all of the above."""
    from celldetection_amd import _lib, graph
    from celldetection_amd.subpixel import collapse_upsampled_taps, phase_padding
    c = dict(bias=True, seed=0)
    c.update(SUBPIXEL_CASES[name])
    n, h, w, c0, c1, cout = (c[k] for k in ('n', 'h', 'w', 'c0', 'c1', 'cout'))
    P, sd, g, ph = subpixel_plan(c)
    tens, ops, wblob, bblob = graph.pack(P, sd, dev)
    assert [o.subpixel for o in ops] == [_lib.SUBPIXEL_HEAD, _lib.SUBPIXEL_PHASE, _lib.SUBPIXEL_LATERAL]
    assert tens[ph].channels == 4 * _pad32(cout)
    xl = torch.randn(n, c0, h, w, generator=g).to(torch.bfloat16).float()
    xt = torch.randn(n, c1, h // 2, w // 2, generator=g).to(torch.bfloat16).float()
    dl, dt = to_nhwc_bf16(xl.to(dev)), to_nhwc_bf16(xt.to(dev))
    e = rg.Embedding(embed)
    dl, dt = e('lateral', dl), e('top', dt)
    cp = _pad32(cout)
    lib = _lib.load()
    head, hbuf, hg = cb.guarded_nhwc_bf16(n, h, w, cp, dev)
    part, pbuf, pg = cb.guarded_nhwc_bf16(n, h // 2, w // 2, 4 * cp, dev)
    pair, qbuf, qg = cb.guarded_nhwc_bf16(n, h, w, cp, dev)
    args = (_lib.ptr(wblob), _lib.ptr(bblob), _lib.stream_ptr())
    with e.watch(lib, 'cpn_conv2d'):
        _lib.check(lib.cpn_conv2d(ops[0], _lib.ptr(dl), dl.shape[-1], _lib.ptr(dt), dt.shape[-1], _lib.ptr(None), 0,
                                  _lib.ptr(head), cp, n, h, w, *args), 'head')
        _lib.check(lib.cpn_conv2d(ops[1], _lib.ptr(dt), dt.shape[-1], _lib.ptr(None), 0, _lib.ptr(None), 0,
                                  _lib.ptr(part), 4 * cp, n, h // 2, w // 2, *args), 'phase')
        _lib.check(lib.cpn_conv2d(ops[2], _lib.ptr(dl), dl.shape[-1], _lib.ptr(None), 0, _lib.ptr(part), 4 * cp,
                                  _lib.ptr(pair), cp, n, h, w, *args), 'lateral')
    torch.cuda.synchronize()
    e.check()
    got_head = cb.assert_nhwc_bf16('head', hbuf, hg, head, cout)
    got = cb.assert_nhwc_bf16('lateral', qbuf, qg, pair, cout)
    cb.assert_guards('phase', pbuf, pg, cb.BF16_GUARD)
    part5 = part.cpu().float().reshape(n, h // 2, w // 2, 2, 2, cp)  # [n, Y, X, py, px, c]
    assert bool((part5[..., cout:] == 0).all()), 'phase: padded channels of the partial sums are not zero'
    got_part = part5[..., :cout].permute(0, 5, 1, 3, 2, 4).reshape(n, cout, h, w)
    wf, bf = graph._fold(sd, P.ops[0])
    bq = bf.to(torch.float32).double()
    # each launch against the fp64 conv of what it read: the head conv over cat(lateral, up(top)) ...
    up_t = F.interpolate(xt.double(), size=(h, w), mode='nearest')
    ref, S, d = cb.conv_with_noise(torch.cat((xl.double(), up_t), 1), wf.to(torch.bfloat16), bq, 1, 1,
                                   n=cb.chain_length(3, 3, _pad32(c0) + _pad32(c1)))
    r_head = cb.check(f'{name} head', got_head, *cb.bf16_bounds(ref, d, 'relu'), F.relu(ref), S)
    # ... the phase convs (collapsed 2x2 taps, rounded to bf16 by the packer; no bias, no activation) over the top map ...
    wc = collapse_upsampled_taps(wf[:, c0:]).to(torch.bfloat16).double()  # [py, px, cout, c1, 2, 2]
    psum, pS = torch.zeros(n, cout, h, w, dtype=torch.float64), torch.zeros(n, cout, h, w, dtype=torch.float64)
    for py in (0, 1):
        for px in (0, 1):
            pt, pl = phase_padding(py), phase_padding(px)
            psum[:, :, py::2, px::2], pS[:, :, py::2, px::2] = cb.conv64(F.pad(xt.double(), (pl, 1 - pl, pt, 1 - pt)), wc[py, px])
    pd = cb.gamma(cb.chain_length(2, 2, _pad32(c1), epilogue=1)) * pS
    r_phase = cb.check(f'{name} phase', got_part, *cb.bf16_bounds(psum, pd), psum, pS)
    # ... and the lateral conv with the partial sums the phase launch actually stored as its residual
    ref, S, d = cb.conv_with_noise(xl, wf[:, :c0].to(torch.bfloat16), bq, 1, 1, n=cb.chain_length(3, 3, _pad32(c0)),
                                   res=got_part)
    r_lat = cb.check(f'{name} lateral', got, *cb.bf16_bounds(ref, d, 'relu'), F.relu(ref), S)
    print(f'{name}: max |got - ref| / bound: head {r_head:.3g}, phase {r_phase:.3g}, lateral {r_lat:.3g}')
    # (b) the decomposition against the reference's statement of the layer: same function, different bf16 roundings
    full = F.relu(F.conv2d(torch.cat((xl, F.interpolate(xt, scale_factor=2, mode='nearest')), 1), wf.float(), bf.float(), 1, 1))
    rel_pair = ((got - full).norm() / full.norm()).item()
    rel_head = ((got_head - full).norm() / full.norm()).item()
    print(f'{name}: rel L2 vs the fp32 conv: sub-pixel pair {rel_pair:.2e}, head conv {rel_head:.2e}')
    assert rel_pair < 1e-2 and rel_pair < 2.5 * rel_head + 1e-3
    if e:
        return dict(head=got_head, partial_sums=got_part, lateral=got)


@pytest.mark.parametrize('n,h,w,cin,cout,bias', [(2, 32, 32, 64, 64, False), (1, 40, 72, 16, 24, True),
                                                  (4, 256, 256, 64, 64, False), (2, 64, 64, 32, 256, True)])
def test_subpixel_bridge_conv(dev, n, h, w, cin, cout, bias):
    """CPN_SUBPIXEL_SCATTER: the 3x3 conv of a GeneralizedUNet bridge level, whose only source is the x2-upsampled map
    (models/unet.py:100-107,213-217), as four 2x2 phase convs + bias + ReLU scattered to their output pixels; vs the fp32
    emulation of that arithmetic (tap sums rounded to bf16 once) and vs the fp32 conv over the upsampled map."""
    from celldetection_amd import _lib, graph
    from celldetection_amd.subpixel import collapse_upsampled_taps, phase_padding
    g = torch.Generator().manual_seed(n * 100 + cout)
    P = graph.Plan()
    top = P.tensor(cin, 2)
    dst = P.conv(top, cout, 2, w='c.', bn='b.', bias=bias, act='relu', pad=1, sub=('scatter', 0))
    assert P.tensors[dst]['down'] == 1 and [e[1] for e in P.entries if e[0] == 'c.weight'] == [(cout, cin, 3, 3)]
    sd = {}
    for key, shape, kind in P.entries:
        if key.endswith('running_var'):
            sd[key] = torch.rand(shape, generator=g) + .5
        elif key.endswith('num_batches_tracked'):
            sd[key] = torch.zeros((), dtype=torch.long)
        elif len(shape) == 4:
            sd[key] = torch.randn(shape, generator=g) / np.sqrt(np.prod(shape[1:]))
        else:
            sd[key] = torch.randn(shape, generator=g) * .5 + (1. if key.endswith('b.weight') else 0.)
    tens, ops, wblob, bblob = graph.pack(P, sd, dev)
    assert ops[0].subpixel == _lib.SUBPIXEL_SCATTER and ops[0].bundles == 4 and ops[0].kh == 2
    xt = torch.randn(n, cin, h // 2, w // 2, generator=g).to(torch.bfloat16).float()
    dt = to_nhwc_bf16(xt.to(dev))
    cp = _pad32(cout)
    out, obuf, og = cb.guarded_nhwc_bf16(n, h, w, cp, dev)
    _lib.check(_lib.load().cpn_conv2d(ops[0], _lib.ptr(dt), dt.shape[-1], _lib.ptr(None), 0, _lib.ptr(None), 0, _lib.ptr(out),
                                      cp, n, h // 2, w // 2, _lib.ptr(wblob), _lib.ptr(bblob), _lib.stream_ptr()), 'scatter')
    torch.cuda.synchronize()
    got = cb.assert_nhwc_bf16('scatter', obuf, og, out, cout)
    wf, bf = graph._fold(sd, P.ops[0])
    wc = collapse_upsampled_taps(wf).to(torch.bfloat16).double()
    ref, S = torch.zeros(n, cout, h, w, dtype=torch.float64), torch.zeros(n, cout, h, w, dtype=torch.float64)
    for py in (0, 1):
        for px in (0, 1):
            pt, pl = phase_padding(py), phase_padding(px)
            ref[:, :, py::2, px::2], S[:, :, py::2, px::2] = cb.conv64(F.pad(xt.double(), (pl, 1 - pl, pt, 1 - pt)), wc[py, px],
                                                                       bf.to(torch.float32))
    d = cb.gamma(cb.chain_length(2, 2, _pad32(cin))) * S
    print(f'max |got - ref| / bound {cb.check("scatter", got, *cb.bf16_bounds(ref, d, "relu"), F.relu(ref), S):.3g}')
    full = F.relu(F.conv2d(F.interpolate(xt, scale_factor=2, mode='nearest'), wf.float(), bf.float(), 1, 1))
    assert ((got - full).norm() / full.norm()).item() < 1e-2


@pytest.mark.parametrize('n,h,w,cin,cout,dtype', [(2, 64, 96, 3, 64, 0), (1, 75, 101, 3, 64, 0), (3, 33, 47, 1, 8, 1),
                                                   (2, 64, 64, 4, 32, 0), (16, 128, 128, 3, 64, 1), (1, 7, 9, 3, 64, 0)])
def test_stem_fast_path(dev, n, h, w, cin, cout, dtype, embed=None):
    """csrc/stem.hip: ResNet stem conv 7x7 stride 2 pad 3 + BN + ReLU (models/resnet.py:274-284) from the padded 4-channel
    input layout, against an fp32 conv on the same bf16-rounded operands; the input conversion itself must be exact.
    ``embed`` (tests/test_gpu_read_guards.py; a byte pattern of tests/read_guards.py): the image, the padded record (which the
    input conversion is documented to write) and the generic kernel's source lie between bands of that pattern, checked as in
    run_conv, and the stored results are returned after all of the above."""
    from celldetection_amd import _lib, graph
    g = torch.Generator().manual_seed(h * 1000 + w)
    P = graph.Plan()
    x = P.input(cin)
    P.conv(x, cout, 7, w='c.', bn='b.', stride=2, pad=3, act='relu')
    P.stem_fast_path(len(P.ops) - 1)
    assert [o['op'] for o in P.ops] == ['input', 'input_stem', 'conv', 'stem7'] and [o['alt'] for o in P.ops] == [1, 2, 1, 2]
    sd = {}
    for key, shape, kind in P.entries:
        if key.endswith('running_var'):
            sd[key] = torch.rand(shape, generator=g) + .5
        elif key.endswith('num_batches_tracked'):
            sd[key] = torch.zeros((), dtype=torch.long)
        elif len(shape) == 4:
            sd[key] = torch.randn(shape, generator=g) / np.sqrt(np.prod(shape[1:]))
        else:
            sd[key] = torch.randn(shape, generator=g) * .5 + (1. if key.endswith('b.weight') else 0.)
    tens, ops, wblob, bblob = graph.pack(P, sd, dev)
    lib = _lib.load()
    xin = torch.rand(n, cin, h, w, generator=g)
    e = rg.Embedding(embed)
    src = e('image', (xin.to(dev) if dtype == 0 else (xin * 255).to(torch.uint8).to(dev)).contiguous())
    xq = xin if dtype == 0 else (xin * 255).to(torch.uint8).float() / 255
    pad = e('stem record', torch.full((n, h + 6, w + 8, 4), 7., dtype=torch.bfloat16, device=dev), updated=True)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    with e.watch(lib, 'cpn_convert_input_stem'):
        _lib.check(lib.cpn_convert_input_stem(_lib.ptr(src.contiguous()), dtype, _lib.ptr(pad), n, cin, h, w, _lib.ptr(flag),
                                              _lib.stream_ptr()), 'input_stem')
    torch.cuda.synchronize()
    exp = torch.zeros(n, h + 6, w + 8, 4)
    exp[:, 3:3 + h, 3:3 + w, :cin] = xq.to(torch.bfloat16).float().permute(0, 2, 3, 1)
    assert torch.equal(pad.cpu().float(), exp) and flag.item() == 0
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    cp = _pad32(cout)
    out, obuf, og = cb.guarded_nhwc_bf16(n, ho, wo, cp, dev)
    # the generic kernel on the 32-channel input, same weights: both against the same bound
    gen_in = e('generic source', to_nhwc_bf16(xq.to(dev)))
    gen, gbuf, gg = cb.guarded_nhwc_bf16(n, ho, wo, cp, dev)
    with e.watch(lib, 'cpn_stem7', 'cpn_conv2d'):
        _lib.check(lib.cpn_stem7(ops[3], _lib.ptr(pad), _lib.ptr(out), cp, n, h, w, _lib.ptr(wblob), _lib.ptr(bblob), 0.,
                                 _lib.stream_ptr()), 'stem7')
        _lib.check(lib.cpn_conv2d(ops[2], _lib.ptr(gen_in), gen_in.shape[-1], _lib.ptr(None), 0, _lib.ptr(None), 0, _lib.ptr(gen),
                                  cp, n, h, w, _lib.ptr(wblob), _lib.ptr(bblob), _lib.stream_ptr()), 'generic stem')
    torch.cuda.synchronize()
    got = cb.assert_nhwc_bf16('stem7', obuf, og, out, cout)
    got_gen = cb.assert_nhwc_bf16('generic stem', gbuf, gg, gen, cout)
    wf, bf = graph._fold(sd, P.ops[2])
    ref, S, d = cb.conv_with_noise(xq.to(torch.bfloat16), wf.to(torch.bfloat16), bf.to(torch.float32), 2, 3,
                                   n=cb.chain_length(7, 7, 32))
    lo, hi = cb.bf16_bounds(ref, d, 'relu')
    r_stem = cb.check('stem7', got, lo, hi, F.relu(ref), S)
    r_gen = cb.check('generic stem', got_gen, lo, hi, F.relu(ref), S)
    # fp8 plans: the same bf16 stem with e4m3 output codes of value / scale (channel stride 64)
    scale = float(F.relu(ref).abs().max()) / 448. + 1e-12
    cp8 = (cout + 63) // 64 * 64
    tens8, ops8, wblob8, bblob8, _, _ = graph.pack(P, sd, dev, precision='fp8', act_scales=[1. / 448., scale])
    inv = float(np.float32(1. / scale))
    codes, cbuf = guarded((n, ho, wo, cp8), torch.uint8, wo * cp8, 0x7f, dev)
    _lib.check(lib.cpn_stem7(ops8[3], _lib.ptr(pad), _lib.ptr(codes), cp8, n, h, w, _lib.ptr(wblob8), _lib.ptr(bblob8),
                             1. / scale, _lib.stream_ptr()), 'stem7 fp8')
    torch.cuda.synchronize()
    e.check()
    assert_guards('stem7 fp8', cbuf, wo * cp8, 0x7f)
    c8 = codes.cpu()
    assert bool(((c8[..., cout:] == 0) | (c8[..., cout:] == 0x80)).all()), 'stem7 fp8: padded output codes not zero'
    got8 = c8[..., :cout].permute(0, 3, 1, 2).contiguous().view(torch.float8_e4m3fn).double()
    r8 = cb.check('stem7 fp8', got8, *cb.e4m3_bounds(ref, d, inv, 'relu'), F.relu(ref) * inv, S)
    print(f'max |got - ref| / bound: stem7 {r_stem:.3g}, generic {r_gen:.3g}, stem7 e4m3 {r8:.3g}')
    bad_in = xin.clone()
    bad_in[0, 0, 1, 1] = 1.5
    if dtype == 0:  # the range flag of the reference's Normalize assert (models/commons.py:694-697)
        _lib.check(lib.cpn_convert_input_stem(_lib.ptr(bad_in.to(dev)), 0, _lib.ptr(pad), n, cin, h, w, _lib.ptr(flag),
                                              _lib.stream_ptr()), 'input_stem')
        assert flag.item() == 1
    if e:
        return {'stem7': got, 'generic stem': got_gen, 'stem7 e4m3 codes': c8, 'stem record': pad.cpu()}


@pytest.mark.parametrize('name', ['1x1_flagship_tile', '1x1_flagship_tile_res'])
def test_conv_pointwise_register_weight_loop(dev, name):
    """Two launches of the flagship 1x1 tile on the same operands return the same bits (no atomics, no order-dependent
    reduction in the kernel), within the rounding bound of the fp64 conv."""
    first, chk, _ = run_conv(dev, **CONV_CASES[name])
    second, _, _ = run_conv(dev, **CONV_CASES[name], reference=False)
    assert torch.equal(second, first), f'max abs {(second - first).abs().max().item():.3e}'
    chk(name, first)


def test_maxpool_bilinear_input(dev):
    from celldetection_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 40, 32, 64, generator=g).to(torch.bfloat16).float()
    d = to_nhwc_bf16(x.to(dev), 64)
    for k, s, p in ((3, 2, 1), (2, 2, 0)):
        ho, wo = (32 + 2 * p - k) // s + 1, (64 + 2 * p - k) // s + 1
        out = torch.empty(2, ho, wo, 64, dtype=torch.bfloat16, device=dev)
        _lib.check(lib.cpn_maxpool2d(_lib.ptr(d), _lib.ptr(out), 2, 32, 64, 64, k, s, p, _lib.stream_ptr()))
        torch.cuda.synchronize()
        ref = F.max_pool2d(x, k, s, p)
        assert torch.equal(from_nhwc(out.cpu(), 40), ref), f'maxpool {k}/{s}/{p}'
    out = torch.empty(2, 64, 128, 64, dtype=torch.bfloat16, device=dev)
    _lib.check(lib.cpn_resize_bilinear(_lib.ptr(d), _lib.ptr(out), 2, 32, 64, 64, 128, 64, _lib.stream_ptr()))
    torch.cuda.synchronize()
    ref = F.interpolate(x, (64, 128), mode='bilinear', align_corners=False)
    import graph_ops_oracle as go  # the interval judge: fp64 reference, coordinate and arithmetic rounding, then the bf16 store
    ref64, e = go.bilinear_ref(x, (64, 128))
    assert float((ref64 - ref.double()).abs().max()) < 1e-6
    lo, hi = go.interval('bf16', ref64, e)
    print(f'bilinear worst error / bound {go.judge_interval("bilinear x2", from_nhwc(out.cpu(), 40), lo, hi, ref64, "bf16", e):.3f}')
    # input conversion + range flag
    xin = torch.rand(2, 3, 32, 64, generator=g)
    for dtype in (0, 1):
        src = xin.to(dev) if dtype == 0 else (xin * 255).to(torch.uint8).to(dev)
        out = torch.full((2, 32, 64, 32), 7., dtype=torch.bfloat16, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.cpn_convert_input(_lib.ptr(src.contiguous()), dtype, _lib.ptr(out), 2, 3, 32, 64, 32,
                                         _lib.ptr(flag), _lib.stream_ptr()))
        torch.cuda.synchronize()
        exp = xin if dtype == 0 else (xin * 255).to(torch.uint8).float() / 255
        assert torch.equal(from_nhwc(out.cpu(), 3), exp.to(torch.bfloat16).float())
        assert out[..., 3:].abs().max().item() == 0 and flag.item() == 0
    bad = xin.clone()
    bad[1, 2, 5, 5] = 1.5
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.cpn_convert_input(_lib.ptr(bad.to(dev)), 0, _lib.ptr(out), 2, 3, 32, 64, 32, _lib.ptr(flag),
                                     _lib.stream_ptr()))
    assert flag.item() == 1


# ------------------------------------------------------------------------------------------------------------
# decode / NMS: bit-exact vs oracle + golden
# ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gops():
    return np.load(os.path.join(G, 'ops.npz'))


@pytest.mark.parametrize('tag,samples', [('a', 32), ('b', 128), ('c', 7), ('d', 64)])
def test_fouriers2contours_golden(dev, gops, tag, samples):
    from celldetection_amd import ops
    out, _ = ops.fouriers2contours(torch.as_tensor(gops[f'f2c_{tag}_fourier']).to(dev),
                                   torch.as_tensor(gops[f'f2c_{tag}_loc']).to(dev), samples=samples)
    np.testing.assert_array_equal(out.cpu().numpy(), gops[f'f2c_{tag}_out'])


def test_fouriers2contours_custom_sampling_golden(dev, gops):
    """``sampling=`` of ops/cpn.py:44-95: one caller-supplied sampling vector shared by all contours (golden from the reference)."""
    from celldetection_amd import ops
    samp = torch.as_tensor(gops['f2c_s_sampling'])
    out, s_out = ops.fouriers2contours(torch.as_tensor(gops['f2c_s_fourier']).to(dev), torch.as_tensor(gops['f2c_s_loc']).to(dev),
                                       samples=5, sampling=samp.to(dev))
    np.testing.assert_array_equal(out.cpu().numpy(), gops['f2c_s_out'])
    assert torch.equal(s_out.cpu(), samp)
    with pytest.raises(NotImplementedError):
        ops.fouriers2contours(torch.zeros(9, 6, 4, device=dev), torch.zeros(9, 2, device=dev), sampling=torch.rand(9, 32))


def test_local_refinement_golden(dev, gops):
    from celldetection_amd import ops
    for iters in (1, 4):
        out = ops.local_refinement(torch.as_tensor(gops['refine_in']).to(dev), torch.as_tensor(gops['refine_map']).to(dev),
                                   iters, torch.as_tensor(gops['refine_b']).to(dev))
        np.testing.assert_array_equal(out.cpu().numpy(), gops[f'refine_out_{iters}'])


@pytest.mark.parametrize('thr', [.2, .5, 0.])
def test_nms_golden(dev, gops, thr):
    from celldetection_amd import ops
    keep = ops.nms(torch.as_tensor(gops['nms_boxes']).to(dev), torch.as_tensor(gops['nms_scores']).to(dev), thr)
    np.testing.assert_array_equal(keep.cpu().numpy(), gops[f'nms_keep_{thr}'])


def test_nmsi_golden(dev, gops):
    from celldetection_amd import ops
    b, s = torch.as_tensor(gops['nms_boxes']).to(dev), torch.as_tensor(gops['nms_scores']).to(dev)
    keep = ops.batched_box_nmsi([b], [s], .2, batch_size=128)[0]
    np.testing.assert_array_equal(keep.cpu().numpy(), gops['nmsi_chunked_keep'])
    keeps = ops.batched_box_nmsi([b, b[:50], b[:0]], [s, s[:50], s[:0]], .2)
    np.testing.assert_array_equal(keeps[0].cpu().numpy(), gops['nms_keep_0.2'])
    np.testing.assert_array_equal(keeps[1].cpu().numpy(), gops['nmsi_plain_keep'])
    assert keeps[2].numel() == 0


def test_border_golden(dev, gops):
    from celldetection_amd import ops
    con = torch.as_tensor(gops['border_in']).to(dev)
    flags = [(True, True, True, True), (False, True, False, True), (True, False, True, False)]
    for i, (top, right, bottom, left) in enumerate(flags):
        keep = ops.remove_border_contours(con, (48, 64), 4, top=top, right=right, bottom=bottom, left=left,
                                          offsets=torch.as_tensor(gops['border_offsets']))
        np.testing.assert_array_equal(keep.cpu().numpy(), gops[f'border_keep_{i}'])
    keep = ops.filter_contours_by_stitching_rule(con, (48, 64), torch.as_tensor(gops['stitch_overlaps']),
                                                 offsets=torch.as_tensor(gops['border_offsets']).to(dev))
    np.testing.assert_array_equal(keep.cpu().numpy(), gops['stitch_keep'])


@pytest.mark.parametrize('P,nseg', [(1, 1), (63, 1), (64, 1), (65, 2), (1000, 3), (5000, 4), (20000, 1)])
def test_nms_random_vs_oracle(dev, P, nseg):
    """Random boxes with many overlaps / ties / degenerate boxes; segmented NMS vs per-segment oracle."""
    import cpn_oracle as orc
    from celldetection_amd import ops
    rng = np.random.default_rng(P)
    xy = rng.uniform(0, 200 if P > 2000 else 60, (P, 2)).astype(np.float32)
    wh = rng.uniform(0, 20, (P, 2)).astype(np.float32)
    boxes = np.concatenate((xy, xy + wh), 1)
    boxes[::17, 2:] = boxes[::17, :2]  # zero-area
    scores = rng.random(P).astype(np.float32)
    scores[::5] = scores[0]  # ties
    cuts = sorted(rng.integers(0, P + 1, nseg - 1).tolist())
    offs = [0] + cuts + [P]
    bl = [torch.as_tensor(boxes[offs[i]:offs[i + 1]]).to(dev) for i in range(nseg)]
    sl = [torch.as_tensor(scores[offs[i]:offs[i + 1]]).to(dev) for i in range(nseg)]
    keeps = ops.batched_box_nmsi(bl, sl, .3)
    for i in range(nseg):
        exp = orc.nms(boxes[offs[i]:offs[i + 1]], scores[offs[i]:offs[i + 1]], .3)
        np.testing.assert_array_equal(keeps[i].cpu().numpy(), exp, err_msg=f'segment {i}')


@pytest.mark.parametrize('shape,density', [((2, 32, 48), .1), ((3, 17, 23), .5), ((1, 64, 64), 0.), ((2, 16, 16), 1.),
                                           ((16, 256, 256), .02)])
def test_compact_and_decode_vs_oracle(dev, shape, density):
    """Synthetic head maps -> HIP compaction + fused decode (+offsets) == oracle post-processing, bit-exact."""
    import cpn_oracle as orc
    from celldetection_amd import ops
    n, h, w = shape
    H, W = 2 * h, 2 * w
    g = torch.Generator().manual_seed(h * w)
    order, samples = 6, 33
    scores = torch.rand(n, 1, h, w, generator=g)
    thr = 1. - density if density > 0 else 2.
    if density >= 1.:
        thr = -1.
    loc = torch.randn(n, 2, h, w, generator=g)
    fourier = torch.randn(n, 4 * order, h, w, generator=g) * 4
    ref = (torch.rand(n, 2, H, W, generator=g) * 2 - 1) * 3
    offsets = torch.randint(-50, 5000, (n, 2), generator=g)
    idx, counts, _ = ops.compact_scores(scores.to(dev), thr)
    flat = ops.decode_proposals(idx, scores.to(dev), loc.to(dev), fourier.to(dev), ref.to(dev), size=(H, W),
                                order=order - 1, samples=samples, iterations=3, offsets=offsets)
    exp = orc.cpn_postprocess(scores, loc, ref, fourier, input_size=(H, W), order=order - 1, samples=samples,
                              score_thresh=thr, refinement_iterations=3, nms=False, offsets=offsets.numpy(),
                              scores_are_probabilities=True)
    assert counts == [len(e) for e in exp['scores']]
    for k in ('contours', 'boxes', 'scores', 'locations', 'fourier', 'contour_proposals'):
        np.testing.assert_array_equal(flat[k].cpu().numpy(), np.concatenate(exp[k]), err_msg=k)
    # no refinement: proposals alias clamped contours
    flat = ops.decode_proposals(idx, scores.to(dev), loc.to(dev), fourier.to(dev), None, size=(H, W), order=order,
                                samples=samples, iterations=0)
    exp = orc.cpn_postprocess(scores, loc, None, fourier, input_size=(H, W), order=order, samples=samples,
                              score_thresh=thr, refinement_iterations=0, nms=False, scores_are_probabilities=True)
    for k in ('contours', 'boxes', 'contour_proposals'):
        np.testing.assert_array_equal(flat[k].cpu().numpy(), np.concatenate(exp[k]), err_msg='norefine ' + k)


def test_box_voting_vs_oracle(dev):
    """filter_by_box_voting (ops/boxes.py:52-83) vs the numpy restatement: votes to 1e-5 relative, same keep set
    (boxes whose vote is within 1e-4 of the threshold are excluded from the set comparison)."""
    import cpn_oracle as orc
    from celldetection_amd import ops
    g = torch.Generator().manual_seed(5)
    xy = torch.rand(900, 2, generator=g) * 120
    wh = torch.rand(900, 2, generator=g) * 30 + 1
    boxes = torch.cat((xy, xy + wh), 1)
    boxes[7] = boxes[6]
    for thr, min_vote in ((.2, 2.), (.5, 1.5), (.1, 1.)):
        keep, votes = ops.filter_by_box_voting(boxes.to(dev), thr, min_vote, return_votes=True)
        ekeep, evotes = orc.filter_by_box_voting(boxes.numpy(), thr, min_vote)
        all_votes = orc.filter_by_box_voting(boxes.numpy(), thr, -1.)[1]
        sure = np.abs(all_votes - min_vote) > 1e-4
        got = np.zeros(len(boxes), bool)
        got[keep.cpu().numpy()] = True
        exp = np.zeros(len(boxes), bool)
        exp[ekeep] = True
        np.testing.assert_array_equal(got[sure], exp[sure])
        assert keep.dtype == torch.int32
        both = got & exp
        gv = np.zeros(len(boxes), np.float32)
        gv[keep.cpu().numpy()] = votes.cpu().numpy()
        np.testing.assert_allclose(gv[both], all_votes[both], rtol=1e-5, atol=1e-5)
    assert ops.filter_by_box_voting(boxes[:0].to(dev), .2, 1.).numel() == 0


# ---- fp8 (e4m3) conv kernel: v_mfma_scale_f32_32x32x64_f8f6f4 ---------------------------------------------------------
def _to_nhwc_fp8(x, scale, cpad):
    """NCHW fp32 -> (NHWC e4m3 codes as uint8 with zero-padded channels, dequantised NCHW fp32)."""
    n, c, h, w = x.shape
    q = (x / scale).clamp(-448, 448).to(torch.float8_e4m3fn)
    out = torch.zeros(n, h, w, cpad, dtype=torch.uint8, device=x.device)
    out[..., :c] = q.view(torch.uint8).permute(0, 2, 3, 1)
    return out.contiguous(), q.double() * scale  # (code x scale exactly: fp32 could round the product)


FP8_BLOCK_ERR = []  # max |got - ref| / S of every fp32-output e4m3 case run in this process (fuzz_conv reports it)

FP8_CASES = {
    '3x3_64_64': dict(n=2, h=32, w=32, cin=64, cout=64, k=3),
    '1x1_128_256': dict(n=2, h=32, w=32, cin=128, cout=256, k=1),
    '1x1_odd_chunks_res': dict(n=1, h=32, w=64, cin=192, cout=128, k=1, res=True),
    '3x3_odd_channels': dict(n=1, h=32, w=64, cin=24, cout=40, k=3),
    '3x3_s2': dict(n=2, h=64, w=64, cin=64, cout=128, k=3, stride=2),
    '7x7_256_small_grid_4x64_tile': dict(n=1, h=64, w=64, cin=128, cout=256, k=7),  # 128 blocks at 4x256: the grid shrinks the tile
    '3x3_concat_up': dict(n=2, h=32, w=32, cin=64, cout=64, k=3, cin1=128, up1=True),
    '3x3_grouped_cpg8': dict(n=1, h=32, w=32, cin=256, cout=256, k=3, groups=32),
    '7x7_stem_s2': dict(n=2, h=64, w=64, cin=3, cout=64, k=7, stride=2, bias=False),
    'final_f32': dict(n=1, h=32, w=32, cin=128, cout=20, k=1, bn=False, act='none', out_f32=True),
    'final_f32_one_block': dict(n=1, h=16, w=64, cin=3, cout=20, k=1, bn=False, act='none', out_f32=True),  # one MFMA per output
    'fused_head_64': dict(n=1, h=32, w=64, cin=64, cout=64, k=7, fuse_cout=20, fuse_act='none'),
}


def conv_fp8_plan(cfg):
    """The one-conv plan of run_conv_fp8 and its seeded parameters -> (plan, state dict, generator, (s0, s1, r) tensor ids);
    needs no GPU."""
    from celldetection_amd import _lib, graph
    cin, cout, k = (cfg[x] for x in ('cin', 'cout', 'k'))
    stride, groups, cin1, up1 = cfg.get('stride', 1), cfg.get('groups', 1), cfg.get('cin1', 0), cfg.get('up1', False)
    res, act, out_f32, fuse_cout = cfg.get('res', False), cfg.get('act', 'relu'), cfg.get('out_f32', False), \
        cfg.get('fuse_cout', 0)
    g = torch.Generator().manual_seed(cfg.get('seed', 11))
    P = graph.Plan()
    s0 = P.tensor(cin, 1)
    s1 = P.tensor(cin1, 2 if up1 else 1) if cin1 else None
    r = P.tensor(cout, stride) if res else None
    P.conv(s0, cout, k, w='c.', bn='b.' if cfg.get('bn', True) else None, bias=cfg.get('bias', True), stride=stride,
           groups=groups, act=act, src1=s1, up1=up1, res=r,
           out_index=_lib.OUT_SCORES if (out_f32 or fuse_cout) else None,
           fuse=dict(w='f.', cout=fuse_cout, act=cfg.get('fuse_act', 'none'), act_scale=3.) if fuse_cout else None)
    return P, random_state_dict(P, g), g, (s0, s1, r)


def run_conv_fp8(dev, name, **cfg):
    """fp8 conv kernel vs the fp64 conv of the SAME e4m3 operands (input codes x their scale, the packer's weight codes x
    their per-channel scale: graph.pack(effective_weights=...)): every output within the rounding bound of
    tests/conv_bounds.py -- e4m3 outputs one of the codes RNE can produce from the accumulation-noise window, at the
    output's code scale; fp32 outputs within the noise + 4 ulp.  No allowance.  Guard rows around the output come back
    untouched, and every padded output code is a zero (0x00 or 0x80).  -> max |got - ref| / bound; a BoundError carries
    .got / .lo / .hi / .ref (NCHW) for the caller's report.
    ``embed`` (a byte pattern of tests/read_guards.py): the sources and the residual lie between bands of that pattern, checked as
    in run_conv; ``reference=False`` then returns the stored output as it is instead of judging it."""
    from celldetection_amd import _lib, graph
    n, h, w, cin, cout, k = (cfg[x] for x in ('n', 'h', 'w', 'cin', 'cout', 'k'))
    stride, groups, cin1, up1 = cfg.get('stride', 1), cfg.get('groups', 1), cfg.get('cin1', 0), cfg.get('up1', False)
    res, act, out_f32, fuse_cout = cfg.get('res', False), cfg.get('act', 'relu'), cfg.get('out_f32', False), \
        cfg.get('fuse_cout', 0)
    P, sd, g, (s0, s1, r) = conv_fp8_plan(cfg)
    out_f32 = out_f32 or bool(fuse_cout)
    x0 = torch.randn(n, cin, h, w, generator=g)
    x1 = torch.randn(n, cin1, h // 2 if up1 else h, w // 2 if up1 else w, generator=g) * 2 if cin1 else None
    ho, wo = (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1
    xr = torch.randn(n, cout, ho, wo, generator=g) if res else None
    p64 = lambda c: (c + 63) // 64 * 64
    scales = {s0: float(x0.abs().max()) / 448}
    if cin1:
        scales[s1] = float(x1.abs().max()) / 448
    if res:
        scales[r] = float(xr.abs().max()) / 448
    d0, x0q = _to_nhwc_fp8(x0.to(dev), scales[s0], p64(cin))
    d1, x1q = _to_nhwc_fp8(x1.to(dev), scales[s1], p64(cin1)) if cin1 else (None, None)
    dr, xrq = _to_nhwc_fp8(xr.to(dev), scales[r], p64(cout)) if res else (None, None)
    e = rg.Embedding(cfg.get('embed'))
    d0, d1, dr = e('src0', d0), e('src1', d1), e('res', dr)
    # reference on the dequantised operands; the weight codes come from the packer (dequantised through mult)
    wf, bf = graph._fold(sd, P.ops[0])
    xin = x0q.cpu()
    if cin1:
        xin = torch.cat((xin, F.interpolate(x1q.cpu(), size=(h, w), mode='nearest') if up1 else x1q.cpu()), 1)
    # output scale from an fp32 dry run
    ref_full = F.conv2d(xin.float(), wf.float(), bf.float(), stride, k // 2, 1, groups)
    if res:
        ref_full = ref_full + xrq.cpu().float()
    if act == 'relu':
        ref_full = F.relu(ref_full)
    dst_id = P.ops[0]['dst']
    if dst_id is not None:
        scales[dst_id] = float(ref_full.abs().max()) / 448
    eff = []
    tens, ops, wblob, bblob, mblob, op_scales = graph.pack(P, sd, dev, precision='fp8', act_scales=scales, effective_weights=eff)
    op = ops[0]
    lib = _lib.load()
    if out_f32:
        guard, sentinel = ho * wo, F32_GUARD
        dst, buf = guarded((n, fuse_cout or cout, ho, wo), torch.float32, guard, sentinel, dev)
        dstride = 0
    else:
        guard, sentinel = wo * p64(cout), 0x7f
        dst, buf = guarded((n, ho, wo, p64(cout)), torch.uint8, guard, sentinel, dev)
        dstride = p64(cout)
    with e.watch(lib, 'cpn_conv2d_fp8'):
        _lib.check(lib.cpn_conv2d_fp8(op, _lib.ptr(d0), d0.shape[-1], _lib.ptr(d1), 0 if d1 is None else d1.shape[-1],
                                      _lib.ptr(dr), 0 if dr is None else dr.shape[-1], _lib.ptr(dst), dstride, n, h, w,
                                      _lib.ptr(wblob), _lib.ptr(bblob), _lib.ptr(mblob), op_scales[0][0], op_scales[0][1],
                                      _lib.stream_ptr()), 'conv2d_fp8')
    torch.cuda.synchronize()
    assert_guards(name, buf, guard, sentinel)
    e.check()
    if not cfg.get('reference', True):
        return dst.cpu()
    # the kernel: acc = sum of code products (exact in fp32), v = acc * mult + bias (+ code_r * res_scale), relu,
    # then RNE(sat(v * out_inv_scale)) -- mult, res_scale and out_inv_scale as the fp32 values it receives
    f32_ = lambda v: float(np.float32(v))
    weff, beff = eff[0]['w'], eff[0]['b'].to(torch.float32).double()
    # the packer's quantisation rule, restated: per output channel scale = row max / 448 of w x input scale (the row of a
    # grouped conv's bundle holds only that channel's group), codes = RNE_e4m3 in fp32, dequantised through the same scales
    wq = torch.empty_like(wf)
    for co in range(cout):
        row = wf[co].clone()
        if cin1:
            row[:cin] *= scales[s0]
            row[cin:] *= scales[s1]
        else:
            row *= scales[s0]
        sw = max(float(row.abs().max()) / 448., 1e-30)
        rq = (row / sw).float().to(torch.float8_e4m3fn).double() * sw
        if cin1:
            rq[:cin] /= scales[s0]
            rq[cin:] /= scales[s1]
        else:
            rq /= scales[s0]
        wq[co] = rq
    torch.testing.assert_close(weff, wq, rtol=1e-12, atol=0, msg=f'{name}: the packer\'s e4m3 weights differ from the rule')
    xres = dr.cpu()[..., :cout].view(torch.float8_e4m3fn).double().permute(0, 3, 1, 2) * f32_(op_scales[0][0]) if res else None
    nchain = cb.chain_length(k, k, cb.cin_read(p64(cin) + cin1 if cin1 else cin, cout, groups, 64), mfma_k=64, epilogue=5)
    ref, S, d = cb.conv_with_noise(xin.double(), weff, beff, stride, k // 2, groups, n=nchain, res=xres,
                                   block_u=cb.E4M3_BLOCK_U)
    if fuse_cout:
        w2 = sd['f.weight'].double().to(torch.bfloat16).double().reshape(fuse_cout, cout)
        ref, S, d = cb.fused_tail(ref, d, w2, sd['f.bias'].to(torch.float32), act=act)
        act = cfg.get('fuse_act', 'none')
    if out_f32:
        if not fuse_cout and act == 'none':  # the measurement behind cb.E4M3_BLOCK_U: fp32 outputs, no activation
            blk = float(((dst.cpu().double() - ref).abs() / S).max())
            FP8_BLOCK_ERR.append(blk)
            print(f'{name}: e4m3 block sum error max |got - ref| / S = {blk:.3e} = 2^{math.log2(max(blk, 1e-300)):.2f}')
        lo, hi = cb.f32_bounds(ref, d, act, 3.)
        got, ref = dst.cpu(), cb.apply_act(ref, act, 3.)
    else:
        codes = dst.cpu()
        pad = codes[..., cout:]
        assert bool(((pad == 0) | (pad == 0x80)).all()), \
            f'{name}: padded output codes not zero: {sorted(set(pad[(pad != 0) & (pad != 0x80)].tolist()))[:8]}'
        got = codes[..., :cout].permute(0, 3, 1, 2).contiguous().view(torch.float8_e4m3fn).double()
        inv = f32_(op_scales[0][1])
        lo, hi = cb.e4m3_bounds(ref, d, inv, act)
        ref = cb.apply_act(ref, act) * inv
    try:
        ratio = cb.check(name, got, lo, hi, ref, S)
    except cb.BoundError as e:
        e.got, e.lo, e.hi, e.ref = got, lo, hi, ref
        raise
    print(f'{name}: max |got - ref| / bound = {ratio:.3g}')
    return ratio


@pytest.mark.parametrize('name', list(FP8_CASES))
def test_conv_fp8_vs_dequantised_reference(dev, name):
    """Every FP8_CASES shape through run_conv_fp8: the e4m3 kernel within the rounding bound of the fp64 conv of the same e4m3
    operands (tests/test_gpu_conv_tiles.py runs the same check once per kernel instantiation)."""
    run_conv_fp8(dev, name, **FP8_CASES[name])


@pytest.mark.parametrize('nb', [6, 3])
def test_bucketed_local_refinement_vs_reference_golden(dev, nb):
    """ops.local_refinement(num_buckets=...) (refine_kernel with the bucket tables) bit-exact vs the reference's
    bucketed local_refinement (cpn.py:72-82) on the golden vectors."""
    from celldetection_amd import ops
    g = np.load(os.path.join(G, 'ops.npz'))
    got = ops.local_refinement(torch.as_tensor(g['refine_in']).to(dev), torch.as_tensor(g[f'refine_bucket_map_{nb}']).to(dev),
                               3, torch.as_tensor(g['refine_b']).to(dev), num_buckets=nb)
    np.testing.assert_array_equal(got.cpu().numpy(), g[f'refine_bucket_out_{nb}'])


@pytest.mark.parametrize('P,extent', [(1, 50), (700, 100), (5000, 200), (40000, 800), (40000, 120)])
def test_nms_binned_equals_dense_and_oracle(dev, P, extent):
    """Spatially binned NMS (slide-level path) = dense bit-mask NMS = CPU oracle: identical keep lists incl. ties,
    zero-area boxes (NaN IoU), duplicates and dense clusters (extent 120: ~thousands of overlaps per box)."""
    import cpn_oracle as orc
    from celldetection_amd import ops
    rng = np.random.default_rng(P + extent)
    xy = rng.uniform(0, extent, (P, 2)).astype(np.float32)
    wh = rng.uniform(0, 20, (P, 2)).astype(np.float32)
    boxes = np.concatenate((xy, xy + wh), 1)
    boxes[::17, 2:] = boxes[::17, :2]  # zero-area
    if P > 100:
        boxes[5] = boxes[4]
        boxes[50, :] = np.nan
    scores = rng.random(P).astype(np.float32)
    scores[::5] = scores[0]  # ties
    b, s = torch.as_tensor(boxes).to(dev), torch.as_tensor(scores).to(dev)
    for thr in (.2, 0.):
        got, st = ops.nms_binned(b, s, thr, return_stats=True)
        dense, cnt = ops._nms_segments(b, s, [0, P], thr)
        np.testing.assert_array_equal(got.cpu().numpy(), dense[:cnt[0]].cpu().numpy())
        if P <= 40000 and thr == .2:
            np.testing.assert_array_equal(got.cpu().numpy(), orc.nms(boxes, scores, thr))
        print(f'nms_binned P={P} extent={extent} thr={thr}: kept {got.numel()}, edges {st["edges"]}, sweeps {st["sweeps"]}, '
              f'workspace {st["workspace_bytes"] / 1e6:.1f} MB')


@pytest.mark.parametrize('n_big,chain', [(1, 0), (7, 0), (300, 0), (3, 400)])
def test_nms_binned_outliers_and_long_chains(dev, n_big, chain):
    """a few tile-sized outlier boxes among 40 000 cell-sized ones must not collapse the grid (they go through the
    oversized list: every box tests them, they scan every cell they reach), more outliers than the list holds fall back to
    the coarse grid, and a suppression chain of hundreds of links (box i suppresses i+1 only) resolves without one host
    round trip per four sweeps.  Keep lists = dense path = oracle in every case."""
    import cpn_oracle as orc
    from celldetection_amd import ops
    P = 40000
    rng = np.random.default_rng(n_big * 1000 + chain)
    xy = rng.uniform(0, 4000, (P, 2)).astype(np.float32)
    wh = rng.uniform(2, 20, (P, 2)).astype(np.float32)
    boxes = np.concatenate((xy, xy + wh), 1)
    scores = rng.random(P).astype(np.float32)
    big = rng.choice(P, n_big, replace=False)
    c = rng.uniform(500, 3500, (n_big, 2)).astype(np.float32)
    half = rng.uniform(300, 2000, (n_big, 2)).astype(np.float32)
    boxes[big] = np.concatenate((c - half, c + half), 1)
    scores[big[::2]] = 2. + rng.random(len(big[::2])).astype(np.float32)  # some outliers outrank everything, some do not
    if chain:  # boxes shifted by 45 % of their width: IoU(i, i+1) = 0.38 > thr, IoU(i, i+2) = 0.05 < thr; descending scores
        idx = rng.choice(np.setdiff1d(np.arange(P), big), chain, replace=False)
        x0 = 5000. + 4.5 * np.arange(chain, dtype=np.float32)
        boxes[idx] = np.stack((x0, np.full(chain, 5000., np.float32), x0 + 10., np.full(chain, 5010., np.float32)), 1)
        scores[idx] = 1.9 - 1e-3 * np.arange(chain, dtype=np.float32)
    b, s = torch.as_tensor(boxes).to(dev), torch.as_tensor(scores).to(dev)
    got, st = ops.nms_binned(b, s, .2, return_stats=True)
    dense, cnt = ops._nms_segments(b, s, [0, P], .2)
    np.testing.assert_array_equal(got.cpu().numpy(), dense[:cnt[0]].cpu().numpy())
    np.testing.assert_array_equal(got.cpu().numpy(), orc.nms(boxes, scores, .2))
    print(f'outliers {n_big} chain {chain}: kept {got.numel()}, edges {st["edges"]}, sweeps {st["sweeps"]}')
    if chain:
        assert st['sweeps'] >= chain // 2  # (the chain really is sequential: alternate links survive)
    if n_big <= 7:
        assert st['edges'] < 40 * P  # the grid did not collapse: a handful of candidates per box, not thousands


def test_nms_binned_slide_scale(dev):
    """10^6 detections spread like cells on a slide: < 1 GB of workspace (the dense mask would need 125 GB), the keep
    list is sorted by score, idempotent, and agrees with the dense path on a 60 000-box crop of the same set."""
    from celldetection_amd import ops
    P = 1_000_000
    g = torch.Generator().manual_seed(5)
    ctr = torch.rand(P, 2, generator=g) * 16384
    wh = torch.rand(P, 2, generator=g) * 24 + 4
    boxes = torch.cat((ctr - wh / 2, ctr + wh / 2), 1).to(dev)
    scores = torch.rand(P, generator=g).to(dev)
    keep, st = ops.nms_binned(boxes, scores, .2, return_stats=True)
    print(f'slide-scale NMS: kept {keep.numel()} of {P}, edges {st["edges"]}, sweeps {st["sweeps"]}, '
          f'workspace {st["workspace_bytes"] / 1e6:.0f} MB')
    assert st['workspace_bytes'] < 1e9
    ks = scores[keep]
    assert bool((ks[:-1] >= ks[1:]).all()) and 0 < keep.numel() < P
    again = ops.nms_binned(boxes[keep], ks, .2)
    assert torch.equal(again, torch.arange(keep.numel(), device=dev))
    sub = (ctr[:, 0] < 4000) & (ctr[:, 1] < 4000)
    idx = sub.nonzero().squeeze(1)[:60000].to(dev)
    a = ops.nms_binned(boxes[idx], scores[idx], .2)
    d, c = ops._nms_segments(boxes[idx], scores[idx], [0, idx.numel()], .2)
    assert torch.equal(a, d[:c[0]])


def test_border_batched_equals_per_tile(dev, gops):
    from celldetection_amd import ops
    con = torch.as_tensor(gops['border_in']).to(dev)  # [40, 12, 2]
    P = con.shape[0]
    img = torch.arange(P, dtype=torch.int32, device=dev) % 3
    sides = torch.tensor([15, 10, 5], dtype=torch.int32, device=dev)  # all / right+left / top+bottom
    offs = torch.tensor([[-3., 5.], [0., 0.], [2., -1.]], device=dev)
    got = ops.remove_border_contours_batched(con, img, sides, offs, (48, 64), 4).bool()
    for n, (top, right, bottom, left) in enumerate([(True, True, True, True), (False, True, False, True),
                                                    (True, False, True, False)]):
        m = img == n
        exp = ops.remove_border_contours(con[m], (48, 64), 4, top=top, right=right, bottom=bottom, left=left, offsets=offs[n])
        assert torch.equal(got[m], exp)
    np.testing.assert_array_equal(got[img == 0].cpu().numpy(), gops['border_keep_0'][(np.arange(P) % 3) == 0])


@pytest.mark.parametrize('shape,size', [((2, 1, 16, 24), (64, 96)), ((1, 3, 19, 26), (75, 101)), ((2, 2, 76, 102), (75, 101)),
                                        ((1, 1, 9, 9), (9, 31))])
def test_resize_bilinear_f32_vs_torch_cpu(dev, shape, size):
    """fp32 NCHW bilinear resize (score-bound masks, `_equal_size`) vs torch CPU's F.interpolate."""
    from celldetection_amd.cpn import _equal_size
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(1))
    ref = F.interpolate(x, size, mode='bilinear', align_corners=False)
    got = _equal_size(x.to(dev), torch.empty(1, 1, *size)).cpu()
    assert got.shape == ref.shape
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=0, atol=2e-6)  # a few ulp: torch may contract to FMA
    m = (x > .5).float()  # 0/1 masks: what the slide loop passes as score bounds
    np.testing.assert_array_equal(_equal_size(m.to(dev), torch.empty(1, 1, *size)).cpu().numpy() > .9,
                                  F.interpolate(m, size, mode='bilinear', align_corners=False).numpy() > .9)


@pytest.mark.parametrize('dtype', [torch.bool, torch.uint8, torch.float32, torch.int64, torch.float16])
def test_windows_any_equals_per_tile_any(dev, dtype):
    """Tile pre-filter of the slide loop (TileLoader skips tiles with an empty mask crop, cpn_inference.py:88-100): ONE window-any
    launch over the tiling table == ``mask[slices].any()`` per tile -- sparse seeds, seeds on window borders, -0.0 / NaN floats."""
    from celldetection_amd import ops, util
    H, W = 700, 1000
    slices = list(util.get_tiling_slices((H, W), (128, 160), (96, 100))[0])
    win = [[s[0].start, s[0].stop, s[1].start, s[1].stop] for s in slices]
    g = torch.Generator().manual_seed(5)
    mask = torch.zeros(H, W)
    ys, xs = torch.randint(0, H, (12,), generator=g), torch.randint(0, W, (12,), generator=g)
    mask[ys, xs] = 1.
    mask[127, 159] = 1.   # last pixel of the first window
    mask[H - 1, W - 1] = 1.
    m = mask.to(dtype).to(dev)
    if dtype == torch.float32:
        m[300, 500] = -0.      # zero
        m[5, 700] = float('nan')  # non-zero
    got = ops.windows_any(m, win)
    exp = [bool(torch.any(m[s])) for s in slices]
    assert got == exp and 0 < sum(exp) < len(exp)
    assert ops.windows_any(torch.zeros(H, W, dtype=dtype, device=dev), win) == [False] * len(win)
    assert ops.windows_any(m, []) == []
    with pytest.raises(ValueError):
        ops.windows_any(m, [[0, H + 1, 0, 10]])
