"""CPU tests of the native plan's validation: malformed descriptor arrays must be rejected with a stated code and message, by
cpn_plan_create (one case per rejection rule) or, for what depends on the input size, by the per-shape planner behind
cpn_plan_workspace_bytes (one case per message).  Every malformed plan is a valid plan from graph.build_plan + graph.pack with
exactly ONE field changed; host code only, no kernel runs.

Base plans (all tiny): CpnU22 base_channels=32 (HEAD triples), CpnResNet18FPN fpn_channels=16 base_channel=8 (BL triple, stem
alternatives; its fp8 pack carries the resize op), CpnResNeXt101UNet base_channel=8 (pair ops), CpnResNet18UNet base_channel=40
(bridge op: the bridge level of the tiny ResNeXt101UNet has 32 channels, the bridge fusion needs 64, so that plan holds none),
CpnU22 base_channels=8 with a SiLU head (activation ops).

Planner messages without a case, and why:
  'stem conv: missing tensors', 'activation op: missing tensors' -- cpn_plan_create rejects a CPN_OP_STEM7 / CPN_OP_ACT op
      without source or destination, so no created plan reaches them (the planner no longer carries these two checks);
  'negative tensor size' -- conv / max-pool sizes are floor((in + 2p - k) / s) + 1 behind an 'input too small' check: with k, s >= 1
      and p >= 0 they are >= 1.  Only a negative stride produced a negative size, and cpn_plan_create rejects that one now.
"""
import functools
from ctypes import c_void_p

import pytest

import celldetection_amd as cda
from celldetection_amd import _lib, graph
from celldetection_amd._lib import E_INVALID, E_UNSUPPORTED

PRECISION = {'bf16': _lib.PRECISION_BF16, 'fp32': _lib.PRECISION_F32, 'fp8': _lib.PRECISION_FP8}
_R8 = {'backbone_kwargs': {'base_channel': 8}}
BASES = {
    'u22': lambda: cda.models.CpnU22(3, backbone_kwargs={'backbone_kwargs': {'base_channels': 32}}),
    'fpn': lambda: cda.models.CpnResNet18FPN(3, backbone_kwargs=dict(_R8, fpn_channels=16)),
    'resnext': lambda: cda.models.CpnResNeXt101UNet(3, backbone_kwargs=_R8),
    'bridge': lambda: cda.models.CpnResNet18UNet(3, backbone_kwargs={'backbone_kwargs': {'base_channel': 40}}),
    'headact': lambda: cda.models.CpnU22(3, head_activation='silu', backbone_kwargs={'backbone_kwargs': {'base_channels': 8}}),
}


@functools.lru_cache(maxsize=None)
def packed(base, precision):
    """-> (tensor descs, op descs, weight blob, bias blob) of a valid plan; never modified (mutate() works on copies)."""
    model = BASES[base]()
    plan = model.plan_for(precision)
    kw = dict(act_scales=[.01] * len(plan.tensors)) if precision == 'fp8' else {}
    return graph.pack(plan, model.state_dict(), 'cpu', precision=precision, **kw)[:4]


def find(ops, nth=0, **fields):
    """Index of the nth op whose descriptor carries these field values."""
    hits = [i for i, o in enumerate(ops) if all(getattr(o, k) == v for k, v in fields.items())]
    return hits[nth]


def mutate(base, precision, target, field, value):
    """Copies of the base plan's descriptor arrays with one field changed.  target: ('op', field values that select it) |
    ('tensor', index) | None."""
    tens, ops, wblob, bblob = packed(base, precision)
    tens, ops = type(tens).from_buffer_copy(tens), type(ops).from_buffer_copy(ops)
    if target is not None:
        kind, sel = target
        item = tens[sel] if kind == 'tensor' else ops[find(ops, **sel)]
        assert getattr(item, field) != value, 'the mutation must change the plan'
        setattr(item, field, value)
    return tens, ops, wblob, bblob


def create(tens, ops, wblob, bblob, precision, n_tensors=None, n_ops=None):
    lib = _lib.load()
    handle = c_void_p()
    rc = lib.cpn_plan_create(handle, tens, len(tens) if n_tensors is None else n_tensors, ops, len(ops) if n_ops is None else n_ops,
                             _lib.ptr(wblob), wblob.numel() * wblob.element_size(), _lib.ptr(bblob), bblob.numel(), precision)
    return rc, lib.cpn_last_error().decode(), handle


def op(**sel):
    return 'op', sel


CONV, POOL, RESIZE = _lib.OP_CONV, _lib.OP_MAXPOOL, _lib.OP_BILINEAR
HEAD, PHASE, LATERAL, SCATTER = _lib.SUBPIXEL_HEAD, _lib.SUBPIXEL_PHASE, _lib.SUBPIXEL_LATERAL, _lib.SUBPIXEL_SCATTER
BL_HEAD, BL_PHASE, BL_FRAME = _lib.SUBPIXEL_BL_HEAD, _lib.SUBPIXEL_BL_PHASE, _lib.SUBPIXEL_BL_FRAME
PLAIN3 = dict(op=CONV, kh=3, subpixel=0, alt=0, src1=-1, res=-1)  # a plain 3x3 conv with a tensor destination
FUSED_HEAD = dict(op=CONV, kh=7, dst=-1, subpixel=0)               # a fused ReadOut head writing an external output

MSG_TENSOR = ('cpn_plan_create: tensor channels must be multiples of 32 (fp8: 64, with a positive scale, or a negative one for a bf16 '
              'partial-sum tensor), down a power of two <= 32')
MSG_WIDE = ('cpn_plan_create: a bf16 tensor of an fp8 plan (negative scale) is the destination of a sub-pixel PHASE op and the '
            'residual of its LATERAL op, nothing else')
MSG_STEM = 'cpn_plan_create: malformed stem fast-path op (bf16 / fp8 plans, alt = 2, <= 4 input channels, 32 | 64 output channels)'
MSG_PAIR = ('cpn_plan_create: a CPN_OP_CONV_PAIR op must follow the 1x1 conv + ReLU and the grouped 3x3 conv + ReLU (stride 1 | 2, '
            'bundles of 32 | 64 channels) it restates and share their offsets')
MSG_BRIDGE = ('cpn_plan_create: a CPN_OP_CONV_BRIDGE op must follow the scatter conv (32 | 64 -> 64 channels, ReLU) and the 3x3 conv '
              '(64 -> 64) it restates, share their offsets, and the tensor between them must have no other reader')
MSG_ACT = ('cpn_plan_create: an activation op needs source and destination tensors of equal channel count and one of the '
           'elementwise activations')
MSG_RESIZE = ('cpn_plan_create: a resize op takes act = 0 (bilinear) or 1 (bicubic; bf16 / fp32 plans only: bicubic weights are '
              'negative in places, the result leaves the e4m3 range of its source\'s scale)')
MSG_CONV_ACT = 'cpn_plan_create: conv ops take CPN_ACT_NONE .. CPN_ACT_TANH_SCALED (other activations are CPN_OP_ACT ops)'

# (id, base, precision, target, field, value, code, message): one case per rejection rule of cpn_plan_create, in rule order
CREATE_CASES = [
    ('tensor_channels', 'u22', 'bf16', ('tensor', 0), 'channels', 33, E_INVALID, MSG_TENSOR),
    ('tensor_down', 'u22', 'bf16', ('tensor', 3), 'down', 3, E_INVALID, MSG_TENSOR),
    ('tensor_scale_fp8', 'fpn', 'fp8', ('tensor', 2), 'scale', 0., E_INVALID, MSG_TENSOR),
    ('id_out_of_range', 'u22', 'bf16', op(**PLAIN3), 'src0', 31, E_INVALID, 'cpn_plan_create: tensor id out of range'),
    ('wide_tensor_elsewhere', 'fpn', 'fp8', ('tensor', 3), 'scale', -1., E_INVALID, MSG_WIDE),
    # (tensor 17: the phase tensor of the first sub-pixel triple, bf16 in the fp8 plan)
    ('phase_destination_narrow', 'u22', 'fp8', ('tensor', 17), 'scale', .01, E_INVALID, MSG_WIDE),
    ('head_triple_up1', 'u22', 'bf16', op(subpixel=HEAD), 'up1', 0, E_INVALID,
     'cpn_plan_create: malformed sub-pixel triple (HEAD, PHASE, LATERAL)'),
    ('head_triple_lateral_res', 'u22', 'bf16', op(subpixel=LATERAL), 'res_up', 1, E_INVALID,
     'cpn_plan_create: malformed sub-pixel triple (HEAD, PHASE, LATERAL)'),
    ('bl_triple_frame_kernel', 'fpn', 'bf16', op(subpixel=BL_FRAME), 'kh', 5, E_INVALID,
     'cpn_plan_create: malformed bilinear sub-pixel triple (BL_HEAD, BL_PHASE, BL_FRAME)'),
    ('bl_triple_fp8_fused_resize', 'fpn', 'fp8', op(op=CONV, subpixel=BL_HEAD), 'up0', 2, E_INVALID,
     'cpn_plan_create: malformed bilinear sub-pixel triple (BL_HEAD, BL_PHASE, BL_FRAME)'),
    ('bl_members_without_head', 'fpn', 'bf16', op(subpixel=BL_HEAD), 'subpixel', 0, E_INVALID,
     'cpn_plan_create: bilinear PHASE / FRAME ops must follow their BL_HEAD op'),
    ('members_without_head', 'u22', 'bf16', op(subpixel=HEAD), 'subpixel', 0, E_INVALID,
     'cpn_plan_create: sub-pixel PHASE / LATERAL ops must follow their HEAD op'),
    ('stem_input_channels', 'fpn', 'bf16', op(op=_lib.OP_INPUT_STEM), 'in_channels', 5, E_INVALID, MSG_STEM),
    ('stem_conv_channels', 'fpn', 'bf16', op(op=_lib.OP_STEM7), 'cout_b', 96, E_INVALID, MSG_STEM),
    ('pair_stride', 'resnext', 'bf16', op(op=_lib.OP_CONV_PAIR), 'stride', 1, E_INVALID, MSG_PAIR),
    ('pair_conv1_act', 'resnext', 'bf16', op(op=CONV, kh=1, cout_b=128, stride=1, act=_lib.ACT_RELU, res=-1), 'act', 0, E_INVALID, MSG_PAIR),
    ('bridge_channels', 'bridge', 'bf16', op(op=_lib.OP_CONV_BRIDGE), 'cout_b', 32, E_INVALID, MSG_BRIDGE),
    ('bridge_residual', 'bridge', 'bf16', op(op=_lib.OP_CONV_BRIDGE), 'res_up', 1, E_INVALID, MSG_BRIDGE),
    ('act_kind', 'headact', 'bf16', op(op=_lib.OP_ACT), 'act', _lib.ACT_TANH_SCALED, E_INVALID, MSG_ACT),
    ('act_missing_source', 'headact', 'bf16', op(op=_lib.OP_ACT), 'src0', -1, E_INVALID, MSG_ACT),
    ('resize_mode', 'fpn', 'fp8', op(op=RESIZE), 'act', 2, E_INVALID, MSG_RESIZE),
    ('resize_bicubic_fp8', 'fpn', 'fp8', op(op=RESIZE), 'act', 1, E_UNSUPPORTED, MSG_RESIZE),
    ('conv_act', 'u22', 'bf16', op(**PLAIN3), 'act', _lib.ACT_SILU, E_INVALID, MSG_CONV_ACT),
    ('conv_fuse_act', 'u22', 'bf16', op(**FUSED_HEAD), 'fuse_act', _lib.ACT_SILU, E_INVALID, MSG_CONV_ACT),
    ('alt', 'u22', 'bf16', op(**PLAIN3), 'alt', 3, E_INVALID, 'cpn_plan_create: alt must be 0, 1 or 2'),
    ('deferred_not_a_head', 'u22', 'bf16', op(**PLAIN3), 'op', _lib.OP_CONV_DEFERRED, E_INVALID,
     'cpn_plan_create: a deferred conv must be a fused ReadOut head of a bf16 plan'),
    ('fp8_mult_offset', 'fpn', 'fp8', op(**PLAIN3), 'mult_offset', 1 << 30, E_INVALID,
     'cpn_plan_create: fp8 conv needs cin_b % 64 == 0 and a valid mult_offset'),
    ('fp8_record_width', 'fpn', 'fp8', op(**PLAIN3), 'cin_b', 32, E_INVALID,
     'cpn_plan_create: fp8 conv needs cin_b % 64 == 0 and a valid mult_offset'),
    ('fp32_fused_head', 'fpn', 'fp32', op(**PLAIN3), 'fuse_cout', 1, E_INVALID, 'cpn_plan_create: fused heads are a bf16-only feature'),
    ('weight_offset', 'u22', 'bf16', op(**PLAIN3), 'weight_offset', -1, E_INVALID, 'cpn_plan_create: weight/bias offset out of range'),
    ('bias_offset', 'u22', 'bf16', op(**PLAIN3), 'bias_offset', 1 << 40, E_INVALID, 'cpn_plan_create: weight/bias offset out of range'),
    ('weight_bytes', 'u22', 'bf16', op(**FUSED_HEAD), 'bundles', 1 << 10, E_INVALID, 'cpn_plan_create: weight/bias offset out of range'),
]


@pytest.mark.parametrize('case', CREATE_CASES, ids=[c[0] for c in CREATE_CASES])
def test_create_rejects(case):
    _, base, precision, target, field, value, code, message = case
    rc, text, handle = create(*mutate(base, precision, target, field, value), PRECISION[precision])
    assert (rc, text) == (code, message)
    assert not handle.value


def test_create_rejects_its_arguments():
    """The two rejections in front of the descriptor rules: here the mutated 'field' is an argument of the call."""
    valid = mutate('u22', 'bf16', None, None, None)
    assert create(*valid, 7)[:2] == (E_INVALID, 'cpn_plan_create: unknown precision')
    assert create(*valid, _lib.PRECISION_BF16, n_ops=0)[:2] == (E_INVALID, 'cpn_plan_create: null/empty')
    assert create(*valid, _lib.PRECISION_BF16, n_tensors=0)[:2] == (E_INVALID, 'cpn_plan_create: null/empty')


def test_base_plans_are_accepted():
    lib = _lib.load()
    for base, precision in (('u22', 'bf16'), ('u22', 'fp8'), ('fpn', 'bf16'), ('fpn', 'fp32'), ('fpn', 'fp8'), ('resnext', 'bf16'),
                            ('bridge', 'bf16'), ('headact', 'bf16')):
        rc, text, handle = create(*mutate(base, precision, None, None, None), PRECISION[precision])
        assert rc == 0, (base, precision, text)
        assert lib.cpn_plan_workspace_bytes(handle, 2, 64, 96) > 0, (base, precision, lib.cpn_last_error())
        lib.cpn_plan_destroy(handle)


# (id, base, precision, target, field, value, (N, H, W), message): cpn_plan_create accepts the plan, planning the size does not --
# one case per message of the per-shape planner (all CPN_E_INVALID)
PLANNING_CASES = [
    # four 2x2 max-pools: 8 -> 4 -> 2 -> 1 -> nothing left
    ('maxpool_too_small', 'u22', 'bf16', None, None, None, (1, 8, 8), 'input too small for the max-pool'),
    ('both_sources_resized', 'u22', 'bf16', op(subpixel=HEAD), 'up0', 1, (1, 64, 64), 'conv: both sources resized'),
    ('scatter_without_tensor', 'u22', 'bf16', op(**FUSED_HEAD), 'subpixel', SCATTER, (1, 64, 64),
     'conv: a sub-pixel scatter conv needs a tensor destination'),
    # the second encoder level (stride 2) reads the full-resolution input tensor as its concat source
    ('concat_sizes', 'u22', 'bf16', op(**dict(PLAIN3, cin_b=32, cout_b=64)), 'src1', 0, (1, 64, 64), 'conv: concat sources differ in size'),
    # the unpadded 3x3 conv of the deepest level (stride 16) on a 16 x 16 input: one pixel
    ('conv_too_small', 'u22', 'bf16', op(**dict(PLAIN3, cin_b=256, cout_b=512)), 'pad', 0, (1, 16, 16),
     'input too small for a convolution of the graph'),
    ('residual_size', 'fpn', 'bf16', op(op=CONV, kh=3, res=2), 'res', 1, (1, 64, 64), 'conv: residual size mismatch'),
    # exact x2 level: the lateral conv runs, but strided it is half the size of the phase tensor it adds
    ('phase_tensor_size', 'u22', 'bf16', op(subpixel=LATERAL), 'stride', 2, (1, 64, 64), 'conv: phase tensor size mismatch'),
    ('unknown_op', 'u22', 'bf16', op(**PLAIN3), 'op', 42, (1, 64, 64), 'unknown op'),
]


@pytest.mark.parametrize('case', PLANNING_CASES, ids=[c[0] for c in PLANNING_CASES])
def test_planning_rejects(case):
    _, base, precision, target, field, value, (n, h, w), message = case
    lib = _lib.load()
    rc, text, handle = create(*mutate(base, precision, target, field, value), PRECISION[precision])
    assert rc == 0, text
    try:
        assert lib.cpn_plan_workspace_bytes(handle, n, h, w) == E_INVALID
        assert lib.cpn_last_error().decode() == message
        assert lib.cpn_plan_executed_flops(handle, n, h, w) == -1.  # the run refuses the same way
        assert lib.cpn_last_error().decode() == message
    finally:
        lib.cpn_plan_destroy(handle)


# ---- The index checks added with the executor's validation pass: these plans were ACCEPTED before (and read out of bounds or
# ---- divided by zero when a size was planned or run); the cases above hold for the earlier executor too, these do not.
MSG_IDS = 'cpn_plan_create: op without the source / destination tensor its kind needs'
MSG_OUT = 'cpn_plan_create: a conv without a destination tensor writes external output out_index = 0 .. 4'
MSG_GEOMETRY = 'cpn_plan_create: conv / max-pool ops need kh, kw, stride >= 1, pad >= 0 (convs: bundles >= 1)'
MSG_POOL_PAD = "cpn_plan_create: a max-pool's pad must be at most half its kernel size"
INDEX_CASES = [
    ('id_below_minus_one', 'u22', 'bf16', op(**PLAIN3), 'res', -2, 'cpn_plan_create: tensor id out of range'),
    ('id_below_minus_one_dst', 'u22', 'bf16', op(**PLAIN3), 'dst', -7, 'cpn_plan_create: tensor id out of range'),
    ('conv_without_source', 'u22', 'bf16', op(**PLAIN3), 'src0', -1, MSG_IDS),
    ('maxpool_without_source', 'u22', 'bf16', op(op=POOL), 'src0', -1, MSG_IDS),
    ('maxpool_without_destination', 'u22', 'bf16', op(op=POOL), 'dst', -1, MSG_IDS),
    ('resize_without_source', 'fpn', 'fp8', op(op=RESIZE), 'src0', -1, MSG_IDS),
    ('resize_without_destination', 'fpn', 'fp8', op(op=RESIZE), 'dst', -1, MSG_IDS),
    ('input_without_destination', 'u22', 'bf16', op(op=_lib.OP_INPUT), 'dst', -1, MSG_IDS),
    ('out_index_high', 'u22', 'bf16', op(**FUSED_HEAD), 'out_index', 5, MSG_OUT),
    ('out_index_negative', 'u22', 'bf16', op(**FUSED_HEAD), 'out_index', -1, MSG_OUT),
    ('conv_without_any_destination', 'u22', 'bf16', op(**PLAIN3), 'dst', -1, MSG_OUT),
    ('conv_kh', 'u22', 'bf16', op(**PLAIN3), 'kh', 0, MSG_GEOMETRY),
    ('conv_kw', 'u22', 'bf16', op(**PLAIN3), 'kw', 0, MSG_GEOMETRY),
    ('conv_stride_zero', 'u22', 'bf16', op(**PLAIN3), 'stride', 0, MSG_GEOMETRY),
    ('conv_stride_negative', 'u22', 'bf16', op(**PLAIN3), 'stride', -1, MSG_GEOMETRY),
    ('conv_pad', 'u22', 'bf16', op(**PLAIN3), 'pad', -1, MSG_GEOMETRY),
    ('conv_bundles', 'u22', 'bf16', op(**PLAIN3), 'bundles', 0, MSG_GEOMETRY),
    ('maxpool_kernel', 'u22', 'bf16', op(op=POOL), 'kh', 0, MSG_GEOMETRY),
    ('maxpool_stride', 'u22', 'bf16', op(op=POOL), 'stride', 0, MSG_GEOMETRY),
    ('maxpool_pad', 'u22', 'bf16', op(op=POOL), 'pad', -1, MSG_GEOMETRY),
    # (accepted before: a 2 x 2 window two pixels into the padding holds no valid tap, its maximum is -inf | -448 x scale)
    ('maxpool_pad_beyond_half_kernel', 'u22', 'bf16', op(op=POOL), 'pad', 2, MSG_POOL_PAD),
]


@pytest.mark.parametrize('case', INDEX_CASES, ids=[c[0] for c in INDEX_CASES])
def test_create_rejects_unchecked_indices(case):
    _, base, precision, target, field, value, message = case
    rc, text, handle = create(*mutate(base, precision, target, field, value), PRECISION[precision])
    assert (rc, text) == (E_INVALID, message)
    assert not handle.value
