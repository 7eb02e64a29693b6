"""Weight packing for the HIP conv engine: (plan, state dict, precision, scales) -> what ``cpn_plan_create`` reads.

``pack`` turns the IR of a plan (``graph.Plan``: op dicts, tensors) and a state dict into the tensor descs, the ``cpn_op_desc``
array (include/cpn_hip.h), the weight blob and the float blob of biases (fp8: + multipliers).  It is a pure function of its
arguments, so two versions of it are compared byte for byte on the CPU (tools/pack_digest.py).

Blob layouts (stated here once; ``item`` = (chunk of KC input channels, filter tap), KC = 32 | fp8: 64):
  bf16   weight records [bundle][item][cout_b][32]; an odd item count gets one all-zero item (the kernel's pipeline step holds two)
  fp8    the same records with 64 channels, as e4m3 codes of ``w * input_scale / weight_scale[cout]``; channels are padded to 64;
         the float blob holds the biases and, behind ALL of them, the multipliers (= weight scales): a bias entry and its
         multiplier entry share their relative offset (``cpn_op_desc.mult_offset``)
  fp32   [bundle][tap][cin_b][cout_b] (verification path)
  stem7  [7][cout_b][8][4] bf16: filter row ky, output channel, (kx 0..7, c 0..3); kx = 7 and c >= in_channels are zero
  tail   the fused ReadOut tail's 1x1 conv [32][cout_b] bf16 + 32 biases, behind its conv's records
Every weight offset is a multiple of 16 bytes.  A bundle is a block of the block-diagonal weight matrix of a grouped conv
(``_bundle_geometry``), a phase of a sub-pixel decomposition (subpixel.py), or the whole dense matrix.

The work is split by job: ``_Precision`` (the facts of a number format), ``_Blobs`` (offsets, padding, alignment), the layout
functions ``_records`` / ``_records_inverse`` / ``_taps_f32``, ``_member_weights`` (an op's share of the conv its keys state),
``_assemble`` / ``_disassemble`` (padded dense matrix of an op), ``_quantise_e4m3``, and one packer per op kind (``_PACKERS``).
"""
from collections import namedtuple
from types import SimpleNamespace

import torch

from . import _lib

__all__ = ['pack']

_ACT = {'none': _lib.ACT_NONE, 'relu': _lib.ACT_RELU, 'sigmoid': _lib.ACT_SIGMOID, 'tanh_scaled': _lib.ACT_TANH_SCALED,
        'leaky_relu': _lib.ACT_LEAKY_RELU, 'silu': _lib.ACT_SILU, 'gelu': _lib.ACT_GELU, 'elu': _lib.ACT_ELU, 'tanh': _lib.ACT_TANH,
        'hardswish': _lib.ACT_HARDSWISH, 'mish': _lib.ACT_MISH, 'selu': _lib.ACT_SELU, 'softplus': _lib.ACT_SOFTPLUS}
_SUBPIXEL = {None: _lib.SUBPIXEL_NONE, 'head': _lib.SUBPIXEL_HEAD, 'phase': _lib.SUBPIXEL_PHASE, 'lateral': _lib.SUBPIXEL_LATERAL,
             'scatter': _lib.SUBPIXEL_SCATTER, 'blhead': _lib.SUBPIXEL_BL_HEAD, 'blphase': _lib.SUBPIXEL_BL_PHASE,
             'blframe': _lib.SUBPIXEL_BL_FRAME}
_PHASES = ('phase', 'scatter', 'blphase')  # ops that are four convs on a low-resolution map, one bundle per output phase


def _pad32(c):
    return (int(c) + 31) // 32 * 32


def _pad64(c):
    return (c + 63) // 64 * 64


def _sub_kind(sub):
    """Kind of an op's ``sub`` tag ('head' | 'phase' | 'lateral' | 'scatter' | 'blhead' | 'blphase' | 'blframe') or None: the tag is
    that string or a tuple (kind, parameter)."""
    return sub[0] if isinstance(sub, tuple) else sub


def _f64(sd, key):
    return sd[key].detach().double().cpu()


def _fold(sd, op):
    """Conv weight/bias with eval-mode BatchNorm (eps 1e-5) folded in, float64 math."""
    w = _f64(sd, op['w'] + 'weight')
    b = _f64(sd, op['w'] + 'bias') if op['bias'] else torch.zeros(w.shape[0], dtype=torch.float64)
    if op['bn'] is not None:
        g, beta, mu, var = (_f64(sd, op['bn'] + name) for name in ('weight', 'bias', 'running_mean', 'running_var'))
        s = g / torch.sqrt(var + 1e-5)
        w, b = w * s[:, None, None, None], (b - mu) * s + beta
    return w, b


def _bundle_geometry(cin, cout, groups, kc=32):
    """(bundles, cin_b, cout_b, groups_per_bundle) or None when the grouped conv must be densified
    (kc = channels per weight record: 32 bf16 | 64 fp8)."""
    if groups == 1:
        return None
    cig, cog = cin // groups, cout // groups
    if cig != cog:
        return None
    bw = cig if cig % kc == 0 else (kc if kc % cig == 0 else None)
    if bw is None or cin % bw:
        return None
    return cin // bw, bw, bw, bw // cig


# pad: channel padding of tensors; kc: channels per weight record; wdtype / align: element type of the weight blob and the
# number of ITS elements blob offsets are aligned to
_Precision = namedtuple('_Precision', 'name f32 fp8 pad kc wdtype align')


def _precision(name):
    if name == 'fp8':
        return _Precision(name, False, True, _pad64, 64, torch.uint8, 16)
    return _Precision(name, name == 'fp32', False, _pad32, 32, torch.float32 if name == 'fp32' else torch.bfloat16, 8)


class _Blobs:
    """The weight blob and the float blob (biases; fp8: + multipliers) under construction.  Every append returns the offset of
    what it appended: bytes in the weight blob, floats in the float blob."""

    def __init__(self, prec):
        self.prec, self.wparts, self.bparts, self.mparts = prec, [], [], []
        self.woff = self.boff = self.moff = 0

    def _append_weights(self, flat):
        off = self.woff
        assert off % 16 == 0, 'weight offsets are 16-byte aligned'
        self.wparts.append(flat)
        self.woff += flat.numel() * flat.element_size()
        return off

    def weights(self, packed):
        """Weight records [bundle][item][cout_b][KC] (values | e4m3 codes; an odd item count is padded with a zero slab: the
        kernel's pipeline step holds two items) or, fp32, [bundle][tap][cin_b][cout_b]; pads the blob to 16 bytes behind them."""
        if not self.prec.f32 and packed.shape[1] % 2:
            packed = torch.cat((packed, torch.zeros_like(packed[:, :1])), 1)
        flat = packed.contiguous().reshape(-1).to(self.prec.wdtype)
        tail = (-flat.numel()) % self.prec.align
        return self._append_weights(torch.cat((flat, flat.new_zeros(tail))) if tail else flat)

    def raw_bf16(self, w):
        """Weights a kernel reads as plain bf16 in every plan (stem, fused ReadOut tail); their sizes keep the alignment."""
        flat = w.reshape(-1).to(torch.bfloat16)
        off = self._append_weights(flat.view(torch.uint8) if self.prec.fp8 else flat)
        assert self.woff % 16 == 0
        return off

    def bias(self, b, mult=None):
        """Bias entries and, fp8, their multipliers (default: ones -- the kernel computes in bf16) at the same relative offset."""
        off = self.boff
        self.bparts.append(b.to(torch.float32))
        self.boff += b.numel()
        if self.prec.fp8:
            moff = self.multipliers(torch.ones(b.numel()) if mult is None else mult)
            assert moff == off and self.moff == self.boff, 'a bias entry and its multipliers share their relative offset'
        return off

    def multipliers(self, m):
        off = self.moff
        self.mparts.append(m.reshape(-1).to(torch.float32))
        self.moff += m.numel()
        return off

    def finish(self, device):
        """-> (weight blob, float blob, offset of the multipliers in it (fp8) | None)"""
        wblob, bblob = torch.cat(self.wparts).to(device), torch.cat(self.bparts).to(device)
        if not self.prec.fp8:
            return wblob, bblob, None
        return wblob, torch.cat((bblob, torch.cat(self.mparts).to(device))), bblob.numel()


# ---- layouts

def _records(dense, kc):
    """dense [bundle][cout_b][cin_b][k][k] -> weight records [bundle][item = (cin_b / kc, tap)][cout_b][kc]"""
    nb, co, ci, kh, kw = dense.shape
    return dense.reshape(nb, co, ci // kc, kc, kh * kw).permute(0, 2, 4, 1, 3).contiguous().reshape(nb, -1, co, kc)


def _records_inverse(records, cin_b, k):
    """weight records (without a zero slab) -> dense [bundle][cout_b][cin_b][k][k]"""
    nb, _, co, kc = records.shape
    return records.reshape(nb, cin_b // kc, k * k, co, kc).permute(0, 3, 1, 4, 2).reshape(nb, co, cin_b, k, k)


def _taps_f32(dense):
    """dense [bundle][cout_b][cin_b][k][k] -> the fp32 layout [bundle][tap][cin_b][cout_b]"""
    nb, co, ci, kh, kw = dense.shape
    return dense.reshape(nb, co, ci, kh * kw).permute(0, 3, 2, 1)


def _quantise_e4m3(records, shared=False):
    """records -> (e4m3 codes, weight scale [bundle][cout_b]); ``shared``: one scale per channel for all bundles (the four phases
    of a 'blphase' op share ONE bias and ONE multiplier per channel)."""
    wscale = (records.abs().amax((1, 3)) / 448.).clamp_min(1e-30)
    if shared:
        wscale = wscale.amax(0, keepdim=True).expand(records.shape[0], -1)
    return (records / wscale[:, None, :, None]).to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8), wscale


# ---- weights of one conv op

def _member_weights(op, w, b, c0=None, in_scales=None):
    """(op, folded weights and bias of the conv its keys state) -> the weights and bias THIS op applies: the lateral's channels,
    a ``share`` range (identity block in front when the first source is the running sum; the bias travels with ONE part), the four
    collapsed kernels [4][cout][cin][k2][k2] of a phase op (float64 tap sums, rounded once).  ``in_scales`` (fp8) = scales of the
    (first, second source | None), folded in: the MFMA then accumulates real-valued units / weight scale; ``c0`` = channels of the first."""
    kind, cin, cout = _sub_kind(op.get('sub')), op['cin'], op['cout']
    if kind == 'lateral':
        w = w[:, :op['sub'][1]]
    if op.get('share') is not None:
        lo, hi, with_bias = op['share'][:3]
        w = w[:, lo:hi]
        if len(op['share']) > 3:  # [running sum | feature] (Fuse2d over more than three features)
            w = torch.cat((torch.eye(cout, op['share'][3], dtype=w.dtype)[:, :, None, None], w), 1)
        if not with_bias:
            b = torch.zeros_like(b)
    if kind == 'blphase':
        from .subpixel import collapse_bilinear_taps
        w = collapse_bilinear_taps(w).reshape(4, cout, cin, op['k'], op['k'])
    elif kind in _PHASES:
        from .subpixel import collapse_upsampled_taps
        w = collapse_upsampled_taps(w[:, op['sub'][1]:]).reshape(4, cout, cin, 2, 2)
    if in_scales is not None:
        w = w.clone()
        if op['groups'] == 1 and in_scales[1] is not None:
            w[:, :c0] *= in_scales[0]
            w[:, c0:] *= in_scales[1]
        else:
            w *= in_scales[0]
    return w, b


# real channels of the two sources; padded channels of the first source, of the whole input and of the output
_ConvChannels = namedtuple('_ConvChannels', 'c0 c1 c0p cinp coutp')


def _conv_channels(op, tensors, prec):
    c0 = tensors[op['src0']]['c']
    c1 = tensors[op['src1']]['c'] if op['src1'] is not None else 0
    return _ConvChannels(c0, c1, prec.pad(c0), prec.pad(c0) + (prec.pad(c1) if op['src1'] is not None else 0),
                         prec.pad(op['cout']) if op['dst'] is not None else _pad32(op['cout']))


def _padded_bias(b, n):
    bias = torch.zeros(n, dtype=torch.float64)
    bias[:b.numel()] = b
    return bias


def _assemble(op, w, b, ch, prec):
    """(weights and bias the op applies, its channels) -> (bundles, cin_b, cout_b, dense [bundle][cout_b][cin_b][k][k], bias | None):
    the zero-padded matrices the kernel multiplies with, the second source's columns behind the PADDED first source."""
    kind, k, groups, cin, cout = _sub_kind(op.get('sub')), op['k'], op['groups'], op['cin'], op['cout']
    geo = _bundle_geometry(cin, cout, groups, prec.kc)
    if kind in _PHASES:
        dense = torch.zeros(4, ch.coutp, ch.cinp, w.shape[-1], w.shape[-1], dtype=torch.float64)  # 2 (nearest) | k2 (bilinear) taps
        dense[:, :cout, :cin] = w
        # 'phase': partial sums, the lateral op of the triple adds the bias (fp8: an all-zero one keeps the bias / multiplier
        # indices of the e4m3 kernel aligned); 'scatter' / 'blphase': one bias shared by the four phases
        zero_bias = torch.zeros(4 * ch.coutp, dtype=torch.float64) if prec.fp8 else None
        return 4, ch.cinp, ch.coutp, dense, zero_bias if kind == 'phase' else _padded_bias(b, ch.coutp)
    if geo is None:
        dense = torch.zeros(1, ch.coutp, ch.cinp, k, k, dtype=torch.float64)
        if groups == 1:
            dense[0, :cout, :ch.c0] = w[:, :ch.c0]
            if ch.c1:
                dense[0, :cout, ch.c0p:ch.c0p + ch.c1] = w[:, ch.c0:]
        else:  # densified grouped conv (block diagonal)
            cig, cog = cin // groups, cout // groups
            for g in range(groups):
                dense[0, g * cog:(g + 1) * cog, g * cig:(g + 1) * cig] = w[g * cog:(g + 1) * cog]
        return 1, ch.cinp, ch.coutp, dense, _padded_bias(b, ch.coutp)
    bundles, cin_b, cout_b, gpb = geo
    cig = cin // groups
    dense = torch.zeros(bundles, cout_b, cin_b, k, k, dtype=torch.float64)
    wg = w.reshape(bundles, gpb, cig, cig, k, k)  # [bundle, group-in-bundle, cout_g, cin_g, k, k]
    for g in range(gpb):
        dense[:, g * cig:(g + 1) * cig, g * cig:(g + 1) * cig] = wg[:, g]
    return bundles, cin_b, cout_b, dense, b.clone()


def _disassemble(op, dense, ch, prec, in_scales):
    """Inverse of ``_assemble`` for ops other than phase ops, the input scales divided out again: dense -> [cout, cin / groups, k, k]."""
    k, groups, cin, cout = op['k'], op['groups'], op['cin'], op['cout']
    geo = _bundle_geometry(cin, cout, groups, prec.kc)
    cig, cog = cin // groups, cout // groups
    if geo is not None:
        w = torch.stack([dense[:, g * cig:(g + 1) * cig, g * cig:(g + 1) * cig] for g in range(geo[3])], 1).reshape(cout, cig, k, k)
    elif groups > 1:
        w = torch.cat([dense[0, g * cog:(g + 1) * cog, g * cig:(g + 1) * cig] for g in range(groups)])
    else:
        w = torch.zeros(cout, cin, k, k, dtype=torch.float64)
        w[:, :ch.c0] = dense[0, :cout, :ch.c0] / in_scales[0]
        if ch.c1:
            w[:, ch.c0:] = dense[0, :cout, ch.c0p:ch.c0p + ch.c1] / in_scales[1]
        return w
    return w / in_scales[0]


# ---- one packer per op kind: (job, index of the op, op dict, its descriptor)

def _pack_input(job, i, op, d):
    d.op, d.dst, d.in_channels = (_lib.OP_INPUT if op['op'] == 'input' else _lib.OP_INPUT_STEM), op['dst'], op['in_channels']


def _pack_stem7(job, i, op, d):
    # the 7 taps of a filter row over a 4-channel NHWC input are 28 contiguous values.  fp8 plans: the stem computes in bf16 on
    # the bf16 input, too -- only its OUTPUT is e4m3 codes of the dst tensor's scale; no weight quantisation
    w, b = _fold(job.state_dict, op)
    cout, cin = op['cout'], op['cin']
    coutp = job.prec.pad(cout)
    wk = torch.zeros(7, coutp, 8, 4, dtype=torch.float64)
    wk[:, :cout, :7, :cin] = w.permute(2, 0, 3, 1)  # [cout, cin, ky, kx] -> [ky, cout, kx, cin]
    if job.prec.fp8:
        job.op_scales[i] = (0., 1. / float(job.act_scales[op['dst']]))
    d.op, d.src0, d.dst = _lib.OP_STEM7, op['src0'], op['dst']
    d.kh = d.kw = 7
    d.stride, d.pad, d.bundles, d.cin_b, d.cout_b = 2, 3, 1, 32, coutp
    d.weight_offset, d.bias_offset = job.blobs.raw_bf16(wk), job.blobs.bias(_padded_bias(b, coutp))
    d.act, d.cout_real, d.out_index = _lib.ACT_RELU, cout, -1
    d.fuse_weight_offset = d.fuse_bias_offset = -1


def _fused_pair(job, i, op, rejection):
    """-> the descriptors of the two convs a fused op restates: it shares their packed weights and biases."""
    if job.prec.f32 or job.prec.fp8:
        raise ValueError(rejection)
    assert op['first'] == i - 2
    return job.ops[op['first']], job.ops[op['first'] + 1]


def _pack_conv_pair(job, i, op, d):
    c1, c2 = _fused_pair(job, i, op, 'fused bottleneck heads are a bf16-plan feature')
    assert c2.bundles * c2.cout_b == c1.cout_b and c2.cin_b == c2.cout_b
    assert c1.dst == c2.src0 and op['w'].startswith(job.plan.ops[op['first']]['w']), 'conv_pair must directly follow its two convs'
    d.op, d.src0, d.dst = _lib.OP_CONV_PAIR, op['src0'], op['dst']
    d.kh = d.kw = 3
    d.stride, d.pad = c2.stride, 1
    d.bundles, d.cin_b, d.cout_b, d.c0_used = c2.bundles, c1.cin_b, c1.cout_b, c1.cin_b
    d.weight_offset, d.bias_offset = c1.weight_offset, c1.bias_offset
    d.fuse_weight_offset, d.fuse_bias_offset, d.fuse_cout = c2.weight_offset, c2.bias_offset, c2.cout_b
    d.act, d.fuse_act, d.out_index, d.cout_real = _lib.ACT_RELU, _lib.ACT_RELU, -1, c2.cout_real


def _pack_conv_bridge(job, i, op, d):
    c1, c2 = _fused_pair(job, i, op, 'the fused bridge level is a bf16-plan feature')
    assert c1.cout_b == c2.cin_b == c2.cout_b == 64
    assert c1.subpixel == _lib.SUBPIXEL_SCATTER and c1.dst == c2.src0 and \
        op['w'].startswith(job.plan.ops[op['first']]['w']), 'conv_bridge must directly follow its scatter conv + 3x3 conv'
    d.op, d.src0, d.dst, d.res = _lib.OP_CONV_BRIDGE, op['src0'], op['dst'], c2.res
    d.kh = d.kw = 3
    d.stride, d.pad, d.bundles, d.cin_b, d.cout_b, d.c0_used = 1, 1, 1, c1.cin_b, 64, c1.cin_b
    d.res_up, d.act, d.act_scale, d.out_index, d.cout_real = c2.res_up, c2.act, c2.act_scale, -1, c2.cout_real
    d.weight_offset, d.bias_offset = c1.weight_offset, c1.bias_offset
    d.fuse_weight_offset, d.fuse_bias_offset, d.fuse_cout = c2.weight_offset, c2.bias_offset, 0


def _pack_act(job, i, op, d):
    d.op, d.src0, d.dst, d.act = _lib.OP_ACT, op['src0'], op['dst'], _ACT[op['act']]


def _pack_maxpool(job, i, op, d):
    d.op, d.src0, d.dst = _lib.OP_MAXPOOL, op['src0'], op['dst']
    d.kh = d.kw = op['k']
    d.stride, d.pad = op['stride'], op['pad']


def _pack_bilinear(job, i, op, d):
    d.op, d.src0, d.dst = _lib.OP_BILINEAR, op['src0'], op['dst']
    d.act = 1 if op.get('mode') == 'bicubic' else 0  # (include/cpn_hip.h: a resize op's act selects the mode)
    if d.act and job.prec.fp8:
        raise NotImplementedError("refinement_interpolation='bicubic' is a bf16 / fp32-plan feature (bicubic weights are "
                                  'negative in places: the result leaves the e4m3 range of its source)')
    # feeds a bilinear sub-pixel triple: only the frame's neighbourhood of the map is needed when the phase convs run
    d.subpixel = _lib.SUBPIXEL_BL_FRAME if op.get('ring_for_bl') else _lib.SUBPIXEL_NONE


def _pack_conv(job, i, op, d):
    prec, blobs, tensors, scales = job.prec, job.blobs, job.plan.tensors, job.act_scales
    w, b = _fold(job.state_dict, op)
    kind = _sub_kind(op.get('sub'))
    if kind is not None and (prec.f32 or (prec.fp8 and kind == 'scatter')):
        raise ValueError('sub-pixel conv triples are a bf16 / fp8-plan feature (the scattered bridge form: bf16)')
    ch = _conv_channels(op, tensors, prec)
    in_scales = (scales[op['src0']], scales[op['src1']] if ch.c1 else None) if prec.fp8 else None
    w, b = _member_weights(op, w, b, ch.c0, in_scales)
    bundles, cin_b, cout_b, dense, bias = _assemble(op, w, b, ch, prec)
    mult = None
    if prec.fp8:
        records, wscale = _quantise_e4m3(_records(dense, prec.kc), shared=kind == 'blphase')
        mult = wscale[:1] if kind == 'blphase' else wscale
        wide = lambda t: tensors[t].get('phases', 1) == 4  # bf16 partial sums: values, no code scale
        job.op_scales[i] = ((1. if wide(op['res']) else float(scales[op['res']])) if op['res'] is not None else 0.,
                            (1. if wide(op['dst']) else 1. / float(scales[op['dst']])) if op['dst'] is not None else 0.)
        if job.effective_weights is not None and (kind in _PHASES or kind == 'lateral'):
            job.effective_weights.append(dict(w=None, b=None))  # (a member op: the simulator follows the head op it restates)
        elif job.effective_weights is not None:
            dq = records.view(torch.float8_e4m3fn).to(torch.float64) * wscale[:, None, :, None]
            weff = _disassemble(op, _records_inverse(dq, cin_b, op['k']), ch, prec, in_scales)
            job.effective_weights.append(dict(w=weff, b=b.clone()))
    else:
        records = _taps_f32(dense) if prec.f32 else _records(dense, prec.kc)
    d.op = _lib.OP_CONV_DEFERRED if op.get('deferred') else _lib.OP_CONV
    d.subpixel = _SUBPIXEL[kind]
    d.src0 = op['src0']
    d.src1 = -1 if op['src1'] is None else op['src1']
    d.res = -1 if op['res'] is None else op['res']
    d.dst = -1 if op['dst'] is None else op['dst']
    d.up0, d.up1 = (2 if op['up0'] == 'bilinear' else int(op['up0'])), int(op['up1'])
    d.res_up = 2 if op['res_up'] == 'shuffle' else int(op['res_up'])
    d.c0_used = ch.c0p if op['src1'] is not None else ch.cinp
    d.kh = d.kw = op['k']
    d.stride, d.pad = op['stride'], op['pad']
    d.bundles, d.cin_b, d.cout_b = bundles, cin_b, cout_b
    d.weight_offset, d.bias_offset = blobs.weights(records), (blobs.bias(bias, mult) if bias is not None else -1)
    d.act, d.act_scale = _ACT[op['act']], float(op['act_scale'])
    d.out_index = -1 if op['out_index'] is None else op['out_index']
    d.cout_real = op['cout']
    d.fuse_weight_offset = d.fuse_bias_offset = -1
    d.fuse_cout = 0
    if op.get('fuse'):  # fused ReadOut tail: the final 1x1 conv (bias) on this conv's activated output, <= 32 channels, bf16
        assert not prec.f32, 'fused heads are a bf16-only feature'
        fz = op['fuse']
        w2 = torch.zeros(32, ch.coutp, dtype=torch.float64)
        w2[:fz['cout'], :op['cout']] = _f64(job.state_dict, fz['w'] + 'weight').reshape(fz['cout'], op['cout'])
        b2 = _padded_bias(_f64(job.state_dict, fz['w'] + 'bias'), 32)
        d.fuse_weight_offset, d.fuse_bias_offset = blobs.raw_bf16(w2), blobs.bias(b2)
        d.fuse_cout, d.fuse_act, d.fuse_act_scale = fz['cout'], _ACT[fz['act']], float(fz['act_scale'])
        d.cout_real = fz['cout']


_PACKERS = {'input': _pack_input, 'input_stem': _pack_input, 'stem7': _pack_stem7, 'conv_pair': _pack_conv_pair,
            'conv_bridge': _pack_conv_bridge, 'act': _pack_act, 'maxpool': _pack_maxpool, 'bilinear': _pack_bilinear,
            'conv': _pack_conv}


def pack(plan, state_dict, device, precision: str = 'bf16', act_scales=None, effective_weights: list = None):
    """-> (tensor_descs, op_descs, weight_blob[bf16 | f32, device], bias_blob[f32, device]); layouts: see the module docstring.

    fp8 (e4m3): ``act_scales[tensor id]`` = value per activation code; returns additionally (mult_blob[f32] = weight_scale per
    output channel, a view of the float blob behind the biases, [(res_scale, out_inv_scale)] per op); the weight blob is a byte
    tensor.  ``effective_weights`` (tests): a list that receives, per conv op, the dequantised weights the fp8 kernel effectively
    applies to real-valued inputs (``[cout, cin/groups, k, k]`` float64) and the bias (None for the members of a triple)."""
    prec = _precision(precision)
    if prec.fp8 and act_scales is None:
        raise ValueError('fp8 packing needs the per-tensor activation scales')
    tens = (_lib.TensorDesc * len(plan.tensors))()
    for i, t in enumerate(plan.tensors):
        tens[i].channels, tens[i].down = prec.pad(t['c']) * t.get('phases', 1), t['down']
        # fp8 plans: the partial-sum tensor of a sub-pixel triple ([phase][c], ``phases`` == 4) is stored as bf16 -- flagged by a
        # negative scale (include/cpn_hip.h cpn_tensor_desc)
        tens[i].scale = (-1. if t.get('phases', 1) == 4 else float(act_scales[i])) if prec.fp8 else 0.
    ops = (_lib.OpDesc * len(plan.ops))()
    job = SimpleNamespace(plan=plan, state_dict=state_dict, prec=prec, blobs=_Blobs(prec), act_scales=act_scales, ops=ops,
                          op_scales=[(0., 0.)] * len(plan.ops), effective_weights=effective_weights)
    for i, op in enumerate(plan.ops):
        d = ops[i]
        d.src0 = d.src1 = d.res = d.dst = -1
        d.bias_offset = d.mult_offset = -1
        d.alt = int(op.get('alt', 0))
        if d.alt and prec.f32:
            raise ValueError('the stem fast path is a bf16 / fp8-plan feature')
        _PACKERS[op['op']](job, i, op, d)
    wblob, fblob, nb = job.blobs.finish(device)
    if not prec.fp8:
        return tens, ops, wblob, fblob
    for d in ops:
        if d.op == _lib.OP_CONV and d.bias_offset >= 0:
            d.mult_offset = nb + d.bias_offset
    return tens, ops, wblob, fblob, fblob[nb:], job.op_scales
