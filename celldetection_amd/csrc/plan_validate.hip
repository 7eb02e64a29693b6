// Validation of a plan's descriptor arrays (cpn_plan_create): every index the planner and the executor dereference is checked
// here, and the positions of the members of fused units are established here and nowhere else (cpn_plan.h OpUnit).
// Rules run op by op in a fixed order: a plan that breaks two of them reports the first.
#include "cpn_plan.h"

namespace cpn {
namespace {

struct Validator {
    const cpn_plan &p;
    const int nt, no;
    const bool bf16, f32, fp8;
    explicit Validator(const cpn_plan &plan)
        : p(plan), nt((int) plan.tensors.size()), no((int) plan.ops.size()), bf16(plan.precision == CPN_PRECISION_BF16),
          f32(plan.precision == CPN_PRECISION_F32), fp8(plan.precision == CPN_PRECISION_FP8) {}

    const cpn_op_desc *op(int i) const { return i >= 0 && i < no ? &p.ops[i] : nullptr; }
    bool conv_with(const cpn_op_desc *o, int subpixel) const { return o && o->op == CPN_OP_CONV && o->subpixel == subpixel; }
    int channels(int t) const { return p.tensors[t].channels; }
    bool tensor(int t) const { return t >= 0 && t < nt; }
    bool wide(int t) const { return t >= 0 && p.tensors[t].scale < 0.f; }  // bf16 tensor of an fp8 plan

    bool tensors_ok() const {
        for (const auto &t : p.tensors)
            if (t.channels <= 0 || t.channels % (fp8 ? 64 : 32) || t.down < 1 || (t.down & (t.down - 1)) || t.down > 32 ||
                (fp8 && !(t.scale > 0.f || t.scale < 0.f)))
                return false;
        return true;
    }

    // bf16 partial-sum tensors (negative scale) exist between the PHASE and the LATERAL op of a sub-pixel triple only
    bool wide_tensors_ok(const cpn_op_desc &o) const {
        const bool phase_dst = o.op == CPN_OP_CONV && o.subpixel == CPN_SUBPIXEL_PHASE && o.dst >= 0;
        const bool lateral_res = o.op == CPN_OP_CONV && o.subpixel == CPN_SUBPIXEL_LATERAL && o.res_up == 2;
        return !wide(o.src0) && !wide(o.src1) && wide(o.dst) == phase_dst && (!wide(o.res) || lateral_res);
    }

    // conv3x3(cat(lateral, nearest_x2(top))) = head | phase (four 2x2 convs on top) + lateral (3x3 + pixel-shuffled residual)
    bool head_triple_ok(int i) const {
        const cpn_op_desc &head = p.ops[i], *phase = op(i + 1), *lateral = op(i + 2);
        if (head.op != CPN_OP_CONV || f32 || !lateral) return false;
        if (!conv_with(phase, CPN_SUBPIXEL_PHASE) || !conv_with(lateral, CPN_SUBPIXEL_LATERAL)) return false;
        const bool head_ok = head.up1 && head.src1 >= 0 && head.dst >= 0;
        const bool phase_ok = phase->src0 == head.src1 && phase->dst >= 0;
        const bool lateral_ok = lateral->src0 == head.src0 && lateral->dst == head.dst && lateral->res == phase->dst && lateral->res_up == 2;
        return head_ok && phase_ok && lateral_ok;
    }

    // fused ReadOut head over the x2 bilinear-resized map = head | phase (four k2 x k2 convs on the low-resolution map) + frame
    bool bl_triple_ok(int i) const {
        const cpn_op_desc &head = p.ops[i], *phase = op(i + 1), *frame = op(i + 2);
        if (head.op != CPN_OP_CONV || f32 || !frame) return false;
        const bool head_ok = head.dst < 0 && head.src0 >= 0 && (head.up0 == 0 || (head.up0 == 2 && !fp8)) &&  // (fp8: the resize is its own op)
                             head.fuse_cout > 0 && head.kh == head.kw && head.kh % 4 == 3;
        if (!head_ok || !conv_with(phase, CPN_SUBPIXEL_BL_PHASE) || !conv_with(frame, CPN_SUBPIXEL_BL_FRAME)) return false;
        const bool phase_ok = tensor(phase->src0) && (head.up0 != 2 || phase->src0 == head.src0) &&
                              channels(phase->src0) == channels(head.src0) && phase->out_index == head.out_index &&
                              phase->kh == (head.kh + 3) / 2 && phase->fuse_cout == head.fuse_cout;
        const bool frame_ok = frame->src0 == head.src0 && frame->out_index == head.out_index && frame->kh == head.kh &&
                              frame->up0 == head.up0 && frame->fuse_cout == head.fuse_cout;
        return phase_ok && frame_ok;
    }

    bool stem_fast_ok(const cpn_op_desc &o) const {
        if (f32 || o.alt != 2 || o.dst < 0) return false;
        if (o.op == CPN_OP_INPUT_STEM) return o.in_channels >= 1 && o.in_channels <= 4;
        return (o.cout_b == 32 || o.cout_b == 64) && o.src0 >= 0 && o.weight_offset >= 0 &&
               (size_t) o.weight_offset + (size_t) 7 * o.cout_b * 64 <= p.weight_bytes &&
               (o.bias_offset < 0 || (size_t) o.bias_offset + o.cout_b <= p.bias_count);
    }

    // 1x1 conv + ReLU (c1), grouped 3x3 conv + ReLU (c2) | the pair op that restates both
    bool pair_ok(int i) const {
        const cpn_op_desc &fused = p.ops[i], *c1 = op(i - 2), *c2 = op(i - 1);
        if (!bf16 || !c1 || c1->op != CPN_OP_CONV || c2->op != CPN_OP_CONV) return false;
        const bool c1_ok = c1->kh == 1 && c1->kw == 1 && c1->stride == 1 && c1->pad == 0 && c1->bundles == 1 && c1->src1 < 0 &&
                           c1->res < 0 && !c1->up0 && c1->act == CPN_ACT_RELU && !c1->subpixel && !c1->alt && c1->dst >= 0;
        const bool c2_ok = c2->src0 == c1->dst && c2->src1 < 0 && c2->res < 0 && !c2->up0 && c2->kh == 3 && c2->kw == 3 &&
                           (c2->stride == 1 || c2->stride == 2) && c2->pad == 1 && c2->act == CPN_ACT_RELU && !c2->subpixel &&
                           !c2->alt && c2->dst >= 0 && c2->cin_b == c2->cout_b && (c2->cout_b == 32 || c2->cout_b == 64) &&
                           c2->bundles * c2->cout_b == c1->cout_b;
        const bool restates = fused.src0 == c1->src0 && fused.dst == c2->dst && fused.stride == c2->stride && fused.cin_b == c1->cin_b &&
                              fused.cout_b == c1->cout_b && fused.fuse_cout == c2->cout_b && fused.bundles == c2->bundles &&
                              fused.weight_offset == c1->weight_offset && fused.bias_offset == c1->bias_offset &&
                              fused.fuse_weight_offset == c2->weight_offset && fused.fuse_bias_offset == c2->bias_offset;
        if (!c1_ok || !c2_ok || !restates || fused.cin_b % 32 || channels(fused.dst) != fused.cout_b) return false;
        const size_t it1 = (size_t) (fused.cin_b / 32), it2 = (size_t) (fused.fuse_cout / 32) * 9;
        return (size_t) fused.weight_offset + (it1 + (it1 & 1)) * fused.cout_b * 64 <= p.weight_bytes &&
               (size_t) fused.fuse_weight_offset + (size_t) fused.bundles * (it2 + (it2 & 1)) * fused.fuse_cout * 64 <= p.weight_bytes;
    }

    // scatter conv (c1: x2 upsampling as four 2x2 phase convs) + 3x3 conv (c2) | the bridge op that never stores c1's output
    bool bridge_ok(int i) const {
        const cpn_op_desc &fused = p.ops[i], *c1 = op(i - 2), *c2 = op(i - 1);
        if (!bf16 || !c1 || c1->op != CPN_OP_CONV || c2->op != CPN_OP_CONV) return false;
        const bool c1_ok = c1->subpixel == CPN_SUBPIXEL_SCATTER && c1->dst >= 0 && c1->act == CPN_ACT_RELU && c1->cout_b == 64 &&
                           (c1->cin_b == 32 || c1->cin_b == 64) && c1->bundles == 4 && c1->bias_offset >= 0;
        const bool c2_ok = c2->src0 == c1->dst && c2->src1 < 0 && !c2->up0 && c2->kh == 3 && c2->kw == 3 && c2->stride == 1 &&
                           c2->pad == 1 && c2->bundles == 1 && c2->cin_b == 64 && c2->cout_b == 64 && c2->subpixel == 0 && !c2->alt &&
                           c2->dst >= 0 && c2->res_up != 1 && c2->fuse_cout == 0;
        const bool restates = fused.src0 == c1->src0 && fused.dst == c2->dst && fused.res == c2->res && fused.res_up == c2->res_up &&
                              fused.act == c2->act && fused.cin_b == c1->cin_b && fused.cout_b == 64 && fused.kh == 3 && fused.kw == 3 &&
                              fused.weight_offset == c1->weight_offset && fused.bias_offset == c1->bias_offset &&
                              fused.fuse_weight_offset == c2->weight_offset && fused.fuse_bias_offset == c2->bias_offset;
        if (!c1_ok || !c2_ok || !restates || !tensor(fused.src0) || channels(fused.src0) < fused.cin_b) return false;
        for (int j = 0; j < no; ++j) {  // nothing else may read the tensor that is no longer stored
            const cpn_op_desc &q = p.ops[j];
            if (j != i - 1 && (q.src0 == c1->dst || q.src1 == c1->dst || q.res == c1->dst)) return false;
        }
        return true;
    }

    bool conv_blobs_ok(const cpn_op_desc &o) const {
        size_t wbytes = (size_t) o.bundles * o.cin_b * o.kh * o.kw * o.cout_b * 4;  // fp32 verification layout
        if (!f32) {  // [bundle][items (+1 zero slab if odd)][cout_b][32] bf16 | [..][64] e4m3 bytes
            const size_t items = (size_t) (o.cin_b / (fp8 ? 64 : 32)) * o.kh * o.kw;
            wbytes = (size_t) o.bundles * (items + (items & 1)) * o.cout_b * 64;
        }
        // (the four phases of a scatter / bilinear phase conv share one bias)
        const size_t biases = (size_t) ((o.subpixel == CPN_SUBPIXEL_SCATTER || o.subpixel == CPN_SUBPIXEL_BL_PHASE) ? 1 : o.bundles) * o.cout_b;
        return o.weight_offset >= 0 && (size_t) o.weight_offset + wbytes <= p.weight_bytes &&
               (o.bias_offset < 0 || (size_t) o.bias_offset + biases <= p.bias_count);
    }

    // the tensor ids an op kind cannot do without (planner and executor index with them unchecked)
    static bool required_ids_ok(const cpn_op_desc &o) {
        switch (o.op) {
            case CPN_OP_CONV:
            case CPN_OP_CONV_DEFERRED: return o.src0 >= 0;
            case CPN_OP_MAXPOOL:
            case CPN_OP_BILINEAR:
            case CPN_OP_ACT: return o.src0 >= 0 && o.dst >= 0;
            case CPN_OP_INPUT: return o.dst >= 0;
            default: return true;
        }
    }

    int check_op(int i, std::vector<OpUnit> &units) const {
        const cpn_op_desc &o = p.ops[i];
        const bool conv = o.op == CPN_OP_CONV || o.op == CPN_OP_CONV_DEFERRED;
        for (int s : {o.src0, o.src1, o.res, o.dst})
            if (s >= nt || s < -1) return fail(CPN_E_INVALID, "cpn_plan_create: tensor id out of range");
        if (fp8 && !wide_tensors_ok(o))
            return fail(CPN_E_INVALID, "cpn_plan_create: a bf16 tensor of an fp8 plan (negative scale) is the destination of a "
                                       "sub-pixel PHASE op and the residual of its LATERAL op, nothing else");
        if (o.subpixel == CPN_SUBPIXEL_HEAD) {
            if (!head_triple_ok(i)) return fail(CPN_E_INVALID, "cpn_plan_create: malformed sub-pixel triple (HEAD, PHASE, LATERAL)");
            units[i] = {UNIT_HEAD, i}; units[i + 1] = {UNIT_PHASE, i}; units[i + 2] = {UNIT_LATERAL, i};
        }
        if (o.subpixel == CPN_SUBPIXEL_BL_HEAD) {
            if (!bl_triple_ok(i)) return fail(CPN_E_INVALID, "cpn_plan_create: malformed bilinear sub-pixel triple (BL_HEAD, BL_PHASE, BL_FRAME)");
            units[i] = {UNIT_BL_HEAD, i}; units[i + 1] = {UNIT_BL_PHASE, i}; units[i + 2] = {UNIT_BL_FRAME, i};
        }
        // a member op is one that its head claimed (a resize op flagged BL_FRAME feeds the frame conv of a triple: propagate_dims)
        if ((o.subpixel == CPN_SUBPIXEL_BL_PHASE && units[i].role != UNIT_BL_PHASE) ||
            (o.subpixel == CPN_SUBPIXEL_BL_FRAME && o.op != CPN_OP_BILINEAR && units[i].role != UNIT_BL_FRAME))
            return fail(CPN_E_INVALID, "cpn_plan_create: bilinear PHASE / FRAME ops must follow their BL_HEAD op");
        if ((o.subpixel == CPN_SUBPIXEL_PHASE && units[i].role != UNIT_PHASE) || (o.subpixel == CPN_SUBPIXEL_LATERAL && units[i].role != UNIT_LATERAL))
            return fail(CPN_E_INVALID, "cpn_plan_create: sub-pixel PHASE / LATERAL ops must follow their HEAD op");
        if ((o.op == CPN_OP_INPUT_STEM || o.op == CPN_OP_STEM7) && !stem_fast_ok(o))
            return fail(CPN_E_INVALID, "cpn_plan_create: malformed stem fast-path op (bf16 / fp8 plans, alt = 2, <= 4 input "
                                       "channels, 32 | 64 output channels)");
        if (o.op == CPN_OP_CONV_PAIR) {
            if (!pair_ok(i))
                return fail(CPN_E_INVALID, "cpn_plan_create: a CPN_OP_CONV_PAIR op must follow the 1x1 conv + ReLU and the grouped "
                                           "3x3 conv + ReLU (stride 1 | 2, bundles of 32 | 64 channels) it restates and share their offsets");
            units[i - 2] = {UNIT_C1, i - 2}; units[i - 1] = {UNIT_C2, i - 2}; units[i] = {UNIT_PAIR, i - 2};
        }
        if (o.op == CPN_OP_CONV_BRIDGE) {
            if (!bridge_ok(i))
                return fail(CPN_E_INVALID, "cpn_plan_create: a CPN_OP_CONV_BRIDGE op must follow the scatter conv (32 | 64 -> 64 "
                                           "channels, ReLU) and the 3x3 conv (64 -> 64) it restates, share their offsets, and "
                                           "the tensor between them must have no other reader");
            units[i - 2] = {UNIT_C1, i - 2}; units[i - 1] = {UNIT_C2, i - 2}; units[i] = {UNIT_BRIDGE, i - 2};
        }
        if (o.op == CPN_OP_ACT && (o.src0 < 0 || o.dst < 0 || o.act < CPN_ACT_RELU || o.act > CPN_ACT_SOFTPLUS || o.act == CPN_ACT_TANH_SCALED ||
                                   channels(o.src0) != channels(o.dst)))
            return fail(CPN_E_INVALID, "cpn_plan_create: an activation op needs source and destination tensors of equal channel count "
                                       "and one of the elementwise activations");
        if (o.op == CPN_OP_BILINEAR && (o.act < 0 || o.act > 1 || (o.act == 1 && fp8)))
            return fail(o.act == 1 ? CPN_E_UNSUPPORTED : CPN_E_INVALID,
                        "cpn_plan_create: a resize op takes act = 0 (bilinear) or 1 (bicubic; bf16 / fp32 plans only: bicubic weights "
                        "are negative in places, the result leaves the e4m3 range of its source's scale)");
        if (conv && (o.act > CPN_ACT_TANH_SCALED || o.fuse_act > CPN_ACT_TANH_SCALED))
            return fail(CPN_E_INVALID, "cpn_plan_create: conv ops take CPN_ACT_NONE .. CPN_ACT_TANH_SCALED (other activations are CPN_OP_ACT ops)");
        if (o.alt < 0 || o.alt > 2) return fail(CPN_E_INVALID, "cpn_plan_create: alt must be 0, 1 or 2");
        if (o.op == CPN_OP_CONV_DEFERRED && (!bf16 || o.fuse_cout <= 0 || o.dst >= 0))
            return fail(CPN_E_INVALID, "cpn_plan_create: a deferred conv must be a fused ReadOut head of a bf16 plan");
        if (conv) {
            const size_t mults = (size_t) (o.subpixel == CPN_SUBPIXEL_BL_PHASE ? 1 : o.bundles) * o.cout_b;
            if (fp8 && (o.cin_b % 64 || (o.mult_offset >= 0 && (size_t) o.mult_offset + mults > p.bias_count)))
                return fail(CPN_E_INVALID, "cpn_plan_create: fp8 conv needs cin_b % 64 == 0 and a valid mult_offset");
            if (f32 && o.fuse_cout > 0) return fail(CPN_E_INVALID, "cpn_plan_create: fused heads are a bf16-only feature");
            if (!conv_blobs_ok(o)) return fail(CPN_E_INVALID, "cpn_plan_create: weight/bias offset out of range");
        }
        // the indices and divisors that planning and the run use unchecked
        if (!required_ids_ok(o)) return fail(CPN_E_INVALID, "cpn_plan_create: op without the source / destination tensor its kind needs");
        if (conv && o.dst < 0 && (o.out_index < 0 || o.out_index >= CPN_NUM_OUTPUTS))
            return fail(CPN_E_INVALID, "cpn_plan_create: a conv without a destination tensor writes external output out_index = 0 .. 4");
        if ((conv || o.op == CPN_OP_MAXPOOL) && (o.kh < 1 || o.kw < 1 || o.stride < 1 || o.pad < 0 || (conv && o.bundles < 1)))
            return fail(CPN_E_INVALID, "cpn_plan_create: conv / max-pool ops need kh, kw, stride >= 1, pad >= 0 (convs: bundles >= 1)");
        // (as torch.nn.MaxPool2d: with more padding a window can lie in the padding alone, and its maximum is -inf)
        if (o.op == CPN_OP_MAXPOOL && (o.pad > o.kh / 2 || o.pad > o.kw / 2))
            return fail(CPN_E_INVALID, "cpn_plan_create: a max-pool's pad must be at most half its kernel size");
        return 0;
    }
};

}  // namespace

int validate_plan(cpn_plan &plan) {
    const Validator v(plan);
    if (!v.tensors_ok())
        return fail(CPN_E_INVALID, "cpn_plan_create: tensor channels must be multiples of 32 (fp8: 64, with a "
                                   "positive scale, or a negative one for a bf16 partial-sum tensor), down a power of two <= 32");
    plan.units.assign(plan.ops.size(), OpUnit{});
    for (int i = 0; i < v.no; ++i)
        if (int rc = v.check_op(i, plan.units)) return rc;
    return 0;
}

}  // namespace cpn
