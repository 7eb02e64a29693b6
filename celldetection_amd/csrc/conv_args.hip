// ConvArgs / PairArgs from an op descriptor: the one statement of a conv launch's geometry, shared by the plan executor and the
// stand-alone entry points (host arithmetic only; no pointer is dereferenced).
#include <algorithm>

#include "cpn_plan.h"

namespace cpn {

ConvBinding plan_binding(const cpn_plan &p, const cpn_op_desc &o) {
    ConvBinding b;
    b.weights = p.weights;
    b.bias = p.bias;
    b.f32 = p.precision == CPN_PRECISION_F32;
    if (p.precision == CPN_PRECISION_FP8) {
        // (an fp8 plan's sources hold up to 2^31 one-byte elements; the stand-alone cpn_conv2d_fp8 passes record = 32 and so keeps
        //  the bf16 limit of 2^30 -- stricter than it has to be, left as it is)
        b.record = 64;
        b.mult = o.mult_offset >= 0 ? p.bias + o.mult_offset : nullptr;
        b.res_wide = o.res >= 0 && p.tensors[o.res].scale < 0.f;  // (bf16 partial sums of a sub-pixel triple)
        b.dst_wide = o.dst >= 0 && p.tensors[o.dst].scale < 0.f;
        b.res_scale = o.res >= 0 ? (b.res_wide ? 1.f : p.tensors[o.res].scale) : 0.f;
        b.out_inv_scale = o.dst >= 0 ? (b.dst_wide ? 1.f : 1.f / p.tensors[o.dst].scale) : 0.f;
    }
    return b;
}

static const float *at(const float *blob, int64_t offset) { return (blob && offset >= 0) ? blob + offset : nullptr; }

int build_conv_args(const ConvBinding &b, const cpn_op_desc &o, int N, ConvArgs &a, const void *s0, int c0s, const void *s1, int c1s,
                    const void *res, int rs, void *dst, int ds, int Hin, int Win, const int *stored) {
    a = ConvArgs{};
    a.src0 = s0; a.src1 = s1; a.c0_stride = c0s; a.c1_stride = c1s;
    a.c0_used = o.c0_used;
    a.up0 = o.up0; a.up1 = o.up1;
    a.N = N; a.Hin = Hin; a.Win = Win;
    a.Hs0 = stored ? stored[0] : (o.up0 ? Hin >> 1 : Hin); a.Ws0 = stored ? stored[1] : (o.up0 ? Win >> 1 : Win);
    a.Hs1 = stored ? stored[2] : (o.up1 ? Hin >> 1 : Hin); a.Ws1 = stored ? stored[3] : (o.up1 ? Win >> 1 : Win);
    if (!o.up0) { a.Hs0 = Hin; a.Ws0 = Win; }
    if (!o.up1) { a.Hs1 = Hin; a.Ws1 = Win; }
    if (a.Hs0 == Hin && a.Ws0 == Win) a.up0 = 0;  // same size: the resize (nearest or bilinear) is the identity
    if (a.Hs1 == Hin && a.Ws1 == Win) a.up1 = 0;
    if (Hin <= 0 || Win <= 0 || a.Hs0 <= 0 || a.Ws0 <= 0 || (s1 && (a.Hs1 <= 0 || a.Ws1 <= 0)))
        return fail(CPN_E_INVALID, "conv: empty input");
    a.sy0 = (float) a.Hs0 / (float) Hin; a.sx0 = (float) a.Ws0 / (float) Win;
    a.sy1 = (float) a.Hs1 / (float) Hin; a.sx1 = (float) a.Ws1 / (float) Win;
    a.KH = o.kh; a.KW = o.kw; a.stride = o.stride; a.pad = o.pad;
    a.Hout = (Hin + 2 * o.pad - o.kh) / o.stride + 1;
    a.Wout = (Win + 2 * o.pad - o.kw) / o.stride + 1;
    a.phase = o.subpixel == CPN_SUBPIXEL_PHASE ? 1 : (o.subpixel == CPN_SUBPIXEL_SCATTER ? 2 : 0);
    if (o.subpixel == CPN_SUBPIXEL_BL_PHASE) {
        // four k2 x k2 convs on the low-resolution map, one symmetric support (pad k2 / 2) and one bias for all phases, fused
        // ReadOut tail scattered to the [2 Hin][2 Win] planes; the frame of k2 / 2 low-resolution pixels belongs to BL_FRAME
        if (o.kh != o.kw || o.kh % 2 == 0 || o.pad != o.kh / 2 || o.stride != 1 || o.bundles != 4 || s1 || o.up0 || res ||
            o.fuse_cout <= 0 || o.dst >= 0)
            return fail(CPN_E_INVALID, "conv: a bilinear phase conv is k2 x k2, pad k2 / 2, stride 1, 4 bundles, one plain source, "
                                       "fused ReadOut tail");
        a.phase = 3;
        a.region = 1;
        a.region_margin = o.kh / 2;
        a.Hout = Hin; a.Wout = Win;
    }
    if (o.subpixel == CPN_SUBPIXEL_BL_FRAME) {  // the conv over the resized map, frame only: k = 2 k2 - 3 -> F = 2 (k2 / 2)
        if (o.fuse_cout <= 0 || o.dst >= 0) return fail(CPN_E_INVALID, "conv: a bilinear frame conv is a fused ReadOut head over a bilinear-resized source");
        a.region = 2;
        a.region_margin = 2 * ((o.kh / 2 + 1) / 2);
    }
    if (a.phase == 1 || a.phase == 2) {  // four 2 x 2 convs (one per output phase, padding (1 - py, 1 - px)) on the low-resolution map
        if (o.kh != 2 || o.kw != 2 || o.pad != 1 || o.stride != 1 || o.bundles != 4 || s1 || o.up0 || res)
            return fail(CPN_E_INVALID, "conv: a sub-pixel phase conv is 2x2, pad 1, stride 1, 4 bundles, one plain source");
        a.Hout = Hin; a.Wout = Win;
    }
    a.bundles = o.bundles; a.cin_b = o.cin_b; a.cout_b = o.cout_b;
    a.weights = (const unsigned char *) b.weights + o.weight_offset;
    a.bias = at(b.bias, o.bias_offset);
    a.res = res; a.res_stride = rs; a.res_up = o.res_up;
    a.Hr = (stored && o.res_up) ? stored[4] : (o.res_up ? a.Hout >> 1 : a.Hout);
    a.Wr = (stored && o.res_up) ? stored[5] : (o.res_up ? a.Wout >> 1 : a.Wout);
    if (o.res_up == 2) {
        if (!res || rs % 4 || 2 * a.Hr != a.Hout || 2 * a.Wr != a.Wout)
            return fail(CPN_E_INVALID, "conv: a pixel-shuffled residual is a [H/2, W/2, 4 * C] phase tensor");
        a.res_cph = rs / 4;
    }
    if (res && (a.Hr <= 0 || a.Wr <= 0)) return fail(CPN_E_INVALID, "conv: empty residual");
    a.ry = (float) a.Hr / (float) a.Hout; a.rx = (float) a.Wr / (float) a.Wout;
    a.act = o.act; a.act_scale = o.act_scale;
    a.out_mode = o.dst >= 0 ? OUT_BF16_NHWC : (o.fuse_cout > 0 ? OUT_FUSED_HEAD : OUT_F32_NCHW);
    if (o.fuse_cout > 0) {
        a.fuse_w = (const unsigned char *) b.weights + o.fuse_weight_offset;
        a.fuse_b = at(b.bias, o.fuse_bias_offset);
        a.fuse_cout = o.fuse_cout; a.fuse_act = o.fuse_act; a.fuse_scale = o.fuse_act_scale;
    }
    a.dst = dst; a.dst_stride = ds; a.dst_coff = o.dst_coff;
    a.cout_real = o.cout_real;
    const int kc = b.record;
    if (o.cin_b <= 0 || o.cin_b % kc || o.cout_b <= 0 || o.cout_b % 32 || o.c0_used % kc || o.bundles < 1)
        return fail(CPN_E_INVALID, "conv: channel counts must be positive multiples of 32 (64 input channels for fp8)");
    a.mult = b.mult;
    a.res_wide = b.res_wide; a.dst_wide = b.dst_wide;
    a.res_scale = b.res_scale; a.out_inv_scale = b.out_inv_scale;
    if (o.bundles > 1 && s1) return fail(CPN_E_INVALID, "conv: grouped conv with two sources");
    if (!s1 && o.c0_used < (a.phase ? 1 : o.bundles) * o.cin_b) return fail(CPN_E_INVALID, "conv: c0_used smaller than input channels");
    // sources are read through raw buffer descriptors whose out-of-range sentinel is byte offset 2^31 (conv_igemm.hip):
    // a source tensor may hold at most 2^31 BYTES (fp32 verification path: 2^31 elements); destinations are addressed
    // with 32-bit element offsets
    const int64_t src_limit = b.f32 ? (1ll << 31) : (1ll << 31) / (kc == 64 ? 1 : 2);
    if ((int64_t) N * a.Hs0 * a.Ws0 * c0s >= src_limit || (s1 && (int64_t) N * a.Hs1 * a.Ws1 * c1s >= src_limit) ||
        (int64_t) N * a.Hout * a.Wout * (a.phase == 2 ? 4 : 1) * std::max(ds, 1) >= (1ll << 31))
        return fail(CPN_E_UNSUPPORTED, "conv: tensor too large for one launch (sources: 2^31 bytes, destination: 2^31 "
                                       "elements); split the batch");
    // plain 1x1 convs are GEMMs over the flattened pixel axis: re-tile as [1, M/32, 32] so that narrow images
    // (16x16 at stride 32) still fill the 32-pixel MFMA column fragments
    if (o.kh == 1 && o.kw == 1 && o.stride == 1 && o.pad == 0 && !o.up0 && !o.up1 && !o.res_up &&
        a.out_mode == OUT_BF16_NHWC) {
        const int64_t M = (int64_t) N * Hin * Win;
        if (M % 32 == 0) {
            a.N = 1; a.Hin = a.Hout = a.Hs0 = a.Hs1 = a.Hr = (int) (M / 32); a.Win = a.Wout = a.Ws0 = a.Ws1 = a.Wr = 32;
        }
    }
    return 0;
}

int bridge_args(const ConvBinding &b, const cpn_op_desc &o, const cpn_op_desc &c2, int N, int Hp, int Wp, ConvArgs &a, const void *src,
                int c_stride, const void *res, int rs, void *dst, int ds) {
    static const char dummy = 0;
    const int stored[6] = {2 * Hp, 2 * Wp, 0, 0, 2 * Hp, 2 * Wp};
    cpn_op_desc main = c2;  // the 3x3 conv, with its weights and bias where the bridge op keeps them
    main.weight_offset = o.fuse_weight_offset;
    main.bias_offset = o.fuse_bias_offset;
    int rc = build_conv_args(b, main, N, a, &dummy, c2.cin_b, nullptr, 0, res, rs, dst, ds, 2 * Hp, 2 * Wp, stored);
    if (rc) return rc;
    a.src0 = src;  // (unused by the kernel: its halo tiles are computed from pre_src)
    a.pre_src = src; a.pre_stride = c_stride; a.pre_cin = o.cin_b; a.pre_H = Hp; a.pre_W = Wp;
    a.pre_w = (const unsigned char *) b.weights + o.weight_offset;
    a.pre_b = at(b.bias, o.bias_offset);
    return 0;
}

// FLOPs the bridge kernel's MFMA loops execute: the 3x3 conv + the scatter conv on every tile's 18 x 34 halo (20 fragments)
double bridge_executed_flops(const ConvArgs &a) {
    const double tiles = (double) a.N * ((a.Hout + 15) / 16) * ((a.Wout + 31) / 32);
    return conv_executed_flops(a) + tiles * 20. * 32. * 64. * a.pre_cin * 4. * 2.;
}

PairArgs pair_args(const cpn_op_desc &o, int N, int H, int W, int c_stride, int dst_stride, const void *weights, const float *bias) {
    PairArgs a{};
    a.N = N; a.H = H; a.W = W;
    a.cin = o.cin_b; a.cmid = o.cout_b; a.cb2 = o.fuse_cout; a.stride = o.stride;
    a.c_stride = c_stride;
    a.dst_stride = dst_stride;
    a.w1 = (const unsigned char *) weights + o.weight_offset;
    a.b1 = at(bias, o.bias_offset);
    a.w2 = (const unsigned char *) weights + o.fuse_weight_offset;
    a.b2 = at(bias, o.fuse_bias_offset);
    return a;
}

PairArgs plan_pair_args(const cpn_plan &p, const cpn_op_desc &o, int N, int H, int W) {
    return pair_args(o, N, H, W, p.tensors[o.src0].channels, p.tensors[o.dst].channels, p.weights, p.bias);
}

}  // namespace cpn
