// C ABI of the CPN conv stack + the native graph executor's run loop (see include/cpn_hip.h; the executor's other units:
// cpn_plan.h).  The executor owns no device memory: activations live in a caller-provided arena whose layout is planned once
// per input shape with a liveness-based first-fit allocator (static workspace planning instead of a caching
// allocator; 288 GB of HBM3E make arena reuse a locality optimisation, not a necessity).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "cpn_plan.h"

namespace cpn {

static thread_local std::string g_last_error;

int fail(int code, const char *msg) {
    g_last_error = msg;
    return code;
}
int check_hip(hipError_t e, const char *where) {
    if (e == hipSuccess) return 0;
    g_last_error = std::string(where) + ": " + hipGetErrorString(e);
    return (int) e;
}

// Argument building + validation of the single-conv entry points, shared with cpn_conv2d_kernel_info (which passes
// placeholder buffers: nothing here dereferences one)
static int conv2d_args(const cpn_op_desc *op, const void *src0, int c0_stride, const void *src1, int c1_stride, const void *res,
                       int res_stride, void *dst, int dst_stride, int N, int Hin, int Win, const void *weights, const float *bias,
                       ConvArgs &a, const int *stored = nullptr) {
    if (!op || !src0 || !dst || !weights) return fail(CPN_E_INVALID, "cpn_conv2d: null pointer");
    ConvBinding b;
    b.weights = weights; b.bias = bias;
    return build_conv_args(b, *op, N, a, src0, c0_stride, src1, c1_stride, res, res_stride, dst, dst_stride, Hin, Win, stored);
}

static int conv2d_fp8_args(const cpn_op_desc *op, const void *src0, int c0_stride, const void *src1, int c1_stride,
                           const void *res, int res_stride, void *dst, int dst_stride, int N, int Hin, int Win,
                           const void *weights, const float *bias, const float *mult, float res_scale, float out_inv_scale,
                           ConvArgs &a) {
    if (!op || !src0 || !dst || !weights) return fail(CPN_E_INVALID, "cpn_conv2d_fp8: null pointer");
    if (op->cin_b % 64 || op->c0_used % 64 || c0_stride % 64 || (src1 && c1_stride % 64))
        return fail(CPN_E_INVALID, "cpn_conv2d_fp8: input channel counts / strides must be multiples of 64");
    ConvBinding b;
    b.weights = weights; b.bias = bias;
    // record stays 32 here: the 64-channel records are checked above, and the source limit is the bf16 one (2^30 elements) where
    // an fp8 plan allows 2^31 (plan_binding) -- a difference this entry point has always had
    b.mult = (mult && op->bias_offset >= 0) ? mult + op->bias_offset : mult;  // (one multiplier per bias slot)
    b.res_scale = res_scale;
    b.out_inv_scale = out_inv_scale;
    return build_conv_args(b, *op, N, a, src0, c0_stride, src1, c1_stride, res, res_stride, dst, dst_stride, Hin, Win);
}

static int conv_bridge_args(const cpn_op_desc *op, const void *src, int c_stride, const void *res, int res_stride, void *dst,
                            int dst_stride, int N, int H, int W, const void *weights, const float *bias, ConvArgs &a) {
    if (!op || !src || !dst || !weights || op->op != CPN_OP_CONV_BRIDGE || N <= 0 || H <= 0 || W <= 0)
        return fail(CPN_E_INVALID, "cpn_conv_bridge: needs a CPN_OP_CONV_BRIDGE descriptor and non-null buffers");
    cpn_op_desc c2 = *op;  // the 3x3 conv the op restates: one plain 64-channel source, its own weights behind fuse_*_offset
    c2.op = CPN_OP_CONV; c2.src1 = -1; c2.up0 = c2.up1 = 0; c2.c0_used = 64; c2.cin_b = 64; c2.cout_b = 64; c2.bundles = 1;
    c2.kh = c2.kw = 3; c2.stride = 1; c2.pad = 1; c2.subpixel = 0; c2.fuse_cout = 0; c2.dst = 0; c2.dst_coff = 0;
    ConvBinding b;
    b.weights = weights; b.bias = bias;
    int rc = bridge_args(b, *op, c2, N, H, W, a, src, c_stride, res, res_stride, dst, dst_stride);
    if (rc) return rc;
    if (!conv_bridge_supported(a))
        return fail(CPN_E_UNSUPPORTED, "cpn_conv_bridge: needs 32 | 64 input channels, 64 output channels and an output of at "
                                       "least 16 x 32 pixels (run the two convs)");
    return 0;
}

}  // namespace cpn

using namespace cpn;

extern "C" {

const char *cpn_last_error(void) { return g_last_error.c_str(); }
int cpn_abi_version(void) { return CPN_ABI_VERSION; }

int cpn_plan_create(cpn_plan **plan, const cpn_tensor_desc *tensors, int32_t n_tensors, const cpn_op_desc *ops,
                    int32_t n_ops, const void *weights, size_t weight_bytes, const float *bias, size_t bias_count,
                    int32_t precision) {
    if (precision != CPN_PRECISION_BF16 && precision != CPN_PRECISION_F32 && precision != CPN_PRECISION_FP8)
        return fail(CPN_E_INVALID, "cpn_plan_create: unknown precision");
    if (!plan || !tensors || !ops || n_tensors <= 0 || n_ops <= 0) return fail(CPN_E_INVALID, "cpn_plan_create: null/empty");
    std::unique_ptr<cpn_plan> p(new cpn_plan());
    p->tensors.assign(tensors, tensors + n_tensors);
    p->ops.assign(ops, ops + n_ops);
    p->weights = (const unsigned char *) weights;
    p->weight_bytes = weight_bytes;
    p->bias = bias;
    p->bias_count = bias_count;
    p->precision = precision;
    if (int rc = validate_plan(*p)) return rc;
    *plan = p.release();
    return 0;
}

void cpn_plan_destroy(cpn_plan *plan) { delete plan; }

int64_t cpn_plan_workspace_bytes(cpn_plan *plan, int32_t N, int32_t H, int32_t W) {
    if (!plan || N <= 0 || H <= 0 || W <= 0) {
        fail(CPN_E_INVALID, "cpn_plan_workspace_bytes: N, H and W must be positive");
        return CPN_E_INVALID;
    }
    const ShapePlan &sp = get_shape_plan(plan, N, H, W);
    if (sp.error) return fail(sp.error, sp.message.c_str());
    return sp.total;
}

int cpn_plan_output_dims(cpn_plan *plan, int32_t H, int32_t W, int32_t out_index, int32_t *h, int32_t *w) {
    if (!plan || H <= 0 || W <= 0 || out_index < 0 || out_index >= CPN_NUM_OUTPUTS || !h || !w)
        return fail(CPN_E_INVALID, "cpn_plan_output_dims: bad arguments");
    const ShapePlan &sp = get_shape_plan(plan, 1, H, W);
    if (sp.error) return fail(sp.error, sp.message.c_str());
    *h = sp.out_h[out_index];
    *w = sp.out_w[out_index];
    return 0;
}

int cpn_plan_tensor_info(cpn_plan *plan, int32_t N, int32_t H, int32_t W, int32_t tensor, int64_t *byte_offset,
                         int32_t *h, int32_t *w, int32_t *channel_stride) {
    if (!plan || N <= 0 || H <= 0 || W <= 0 || tensor < 0 || tensor >= (int) plan->tensors.size() || !byte_offset || !h ||
        !w || !channel_stride)
        return fail(CPN_E_INVALID, "cpn_plan_tensor_info: bad arguments");
    const ShapePlan &sp = get_shape_plan(plan, N, H, W);
    if (sp.error) return fail(sp.error, sp.message.c_str());
    if (sp.offsets[tensor] < 0) return fail(CPN_E_INVALID, "cpn_plan_tensor_info: the tensor is never written");
    *byte_offset = sp.offsets[tensor];
    *h = sp.th[tensor];
    *w = sp.tw[tensor];
    *channel_stride = plan->tensors[tensor].channels;
    return 0;
}

int64_t cpn_plan_max_tensor_elements(cpn_plan *plan, int32_t H, int32_t W) {
    if (!plan || H <= 0 || W <= 0) {
        fail(CPN_E_INVALID, "cpn_plan_max_tensor_elements: bad arguments");
        return CPN_E_INVALID;
    }
    const ShapePlan &sp = get_shape_plan(plan, 1, H, W);
    if (sp.error) return fail(sp.error, sp.message.c_str());
    return sp.max_elems;
}

static int run_or_count(cpn_plan *plan, const void *input, int32_t in_dtype, int32_t N, int32_t H, int32_t W,
                        void *workspace, int64_t workspace_bytes, float *const *outputs, int32_t *range_flag,
                        hipStream_t st, double *flops, hipEvent_t *events = nullptr, double *op_flops = nullptr,
                        float *absmax = nullptr) {
    if (!plan || N <= 0 || H <= 0 || W <= 0) return fail(CPN_E_INVALID, "cpn_plan_run: N, H and W must be positive");
    const ShapePlan &sp = get_shape_plan(plan, N, H, W);
    if (sp.error) return fail(sp.error, sp.message.c_str());
    if (!flops && sp.total > workspace_bytes) return fail(CPN_E_WORKSPACE, "cpn_plan_run: workspace too small");
    const bool f32 = plan->precision == CPN_PRECISION_F32, fp8 = plan->precision == CPN_PRECISION_FP8;
    if (absmax && plan->precision != CPN_PRECISION_BF16) return fail(CPN_E_INVALID, "cpn_plan_run_stats: bf16 plans only");
    // (FLOP-count mode runs without a workspace: a non-null dummy base keeps "tensor at offset 0" distinguishable from "no tensor"
    //  in the argument checks -- nothing is launched in that mode)
    char *ws = (flops && !workspace) ? (char *) 256 : (char *) workspace;
    auto tptr = [&](int t) -> void * { return t >= 0 ? (void *) (ws + sp.offsets[t]) : nullptr; };
    auto tch = [&](int t) -> int { return t >= 0 ? plan->tensors[t].channels : 0; };
    for (size_t i = 0; i < plan->ops.size(); ++i) {
        const cpn_op_desc &o = plan->ops[i];
        int rc = 0;
        if (events) (void) hipEventRecord(events[i], st);
        if (sp.skip[i]) continue;
        switch (o.op) {
            case CPN_OP_INPUT: {
                if (flops) break;
                InputArgs a{input, tptr(o.dst), N, o.in_channels, H, W, tch(o.dst), in_dtype, range_flag};
                rc = check_hip((hipError_t) (f32 ? launch_input_f32(a, st)
                                                 : fp8 ? launch_input_fp8(a, 1.f / plan->tensors[o.dst].scale, st)
                                                       : launch_input(a, st)), "input kernel");
                break;
            }
            case CPN_OP_INPUT_STEM: {
                if (flops) break;
                InputArgs a{input, tptr(o.dst), N, o.in_channels, H, W, 4, in_dtype, range_flag};
                rc = check_hip((hipError_t) launch_input_stem(a, st), "stem input kernel");
                break;
            }
            case CPN_OP_STEM7: {
                StemArgs a{tptr(o.src0), tptr(o.dst), plan->weights + o.weight_offset,
                           o.bias_offset >= 0 ? plan->bias + o.bias_offset : nullptr, N, sp.th[o.src0], sp.tw[o.src0],
                           sp.th[o.dst], sp.tw[o.dst], o.cout_b, tch(o.dst),
                           fp8 ? 1.f / plan->tensors[o.dst].scale : 0.f};  // fp8 plans: e4m3 output codes
                const double fl = 2.0 * N * a.Hout * a.Wout * (double) o.cout_b * 7 * 32;
                if (op_flops) op_flops[i] = fl;
                if (flops) { *flops += fl; break; }
                rc = check_hip((hipError_t) launch_stem7(a, st), "stem conv kernel");
                break;
            }
            case CPN_OP_MAXPOOL: {
                if (flops) break;
                PoolArgs a{tptr(o.src0), tptr(o.dst), N, sp.th[o.src0], sp.tw[o.src0], sp.th[o.dst], sp.tw[o.dst],
                           tch(o.src0), o.kh, o.stride, o.pad};
                rc = check_hip((hipError_t) (f32 ? launch_maxpool_f32(a, st) : fp8 ? launch_maxpool_fp8(a, st)
                                                                                  : launch_maxpool(a, st)), "maxpool kernel");
                break;
            }
            case CPN_OP_ACT: {
                if (flops) break;
                ActArgs a{tptr(o.src0), tptr(o.dst), (long) N * sp.th[o.src0] * sp.tw[o.src0] * tch(o.src0), o.act,
                          fp8 ? plan->tensors[o.src0].scale : 1.f, fp8 ? 1.f / plan->tensors[o.dst].scale : 1.f};
                rc = check_hip((hipError_t) (f32 ? launch_act_f32(a, st) : fp8 ? launch_act_fp8(a, st) : launch_act(a, st)),
                               "activation kernel");
                break;
            }
            case CPN_OP_BILINEAR: {
                if (flops) break;
                if (sp.offsets[o.src0] == sp.offsets[o.dst]) break;  // same size: the planner aliased dst to src
                ResizeArgs a{tptr(o.src0), tptr(o.dst), N, sp.th[o.src0], sp.tw[o.src0], sp.th[o.dst], sp.tw[o.dst],
                             tch(o.src0), fp8 ? sp.ring[i] : 0,  // (ring: see propagate_dims, bilinear sub-pixel triple)
                             o.act == 1 ? 1 : 0};                // (CPN_OP_BILINEAR: act = 1 selects bicubic)
                rc = check_hip((hipError_t) (f32 ? launch_bilinear_f32(a, st) : fp8 ? launch_bilinear_fp8(a, st)
                                                                                   : launch_bilinear(a, st)), "bilinear kernel");
                break;
            }
            case CPN_OP_CONV_PAIR: {
                const int mid = plan->ops[plan->units[i].c1()].dst;
                PairArgs a = plan_pair_args(*plan, o, N, sp.th[mid], sp.tw[mid]);
                a.src = tptr(o.src0);
                a.dst = tptr(o.dst);
                const double fl = conv_pair_executed_flops(a);
                if (op_flops) op_flops[i] = fl;
                if (flops) { *flops += fl; break; }
                rc = check_hip((hipError_t) launch_conv_pair(a, st), "conv pair kernel");
                break;
            }
            case CPN_OP_CONV_BRIDGE: {
                ConvArgs a;
                rc = bridge_args(plan_binding(*plan, o), o, plan->ops[plan->units[i].c2()], N, sp.th[o.src0], sp.tw[o.src0], a,
                                 tptr(o.src0), tch(o.src0), tptr(o.res), tch(o.res), tptr(o.dst), tch(o.dst));
                if (rc) return rc;
                if (!conv_bridge_supported(a)) return fail(CPN_E_INVALID, "cpn_plan_run: bridge op at an unsupported size");
                const double fl = bridge_executed_flops(a);
                if (op_flops) op_flops[i] = fl;
                if (flops) { *flops += fl; break; }
                rc = check_hip((hipError_t) launch_conv(a, st), "conv bridge kernel");
                break;
            }
            case CPN_OP_CONV_DEFERRED: break;  // evaluated at the proposal pixels only (cpn_sparse_heads)
            case CPN_OP_CONV: {
                const ConvDims &cd = sp.conv[i];  // virtual input size + stored source sizes (propagate_dims)
                void *dst = o.dst >= 0 ? tptr(o.dst) : (outputs ? (void *) outputs[o.out_index] : nullptr);
                ConvArgs a;
                rc = build_conv_args(plan_binding(*plan, o), o, N, a, tptr(o.src0), tch(o.src0), tptr(o.src1), tch(o.src1),
                                     tptr(o.res), tch(o.res), dst, o.dst >= 0 ? tch(o.dst) : 0, cd.hin, cd.win, cd.stored);
                if (rc) return rc;
                if (o.dst >= 0) {
                    const int64_t M = (int64_t) N * sp.th[o.dst] * sp.tw[o.dst];
                    if ((int64_t) a.N * a.Hout * a.Wout * (a.phase == 2 ? 4 : 1) != M)
                        return fail(CPN_E_INVALID, "cpn_plan_run: conv output size mismatch");
                }
                if (op_flops) op_flops[i] = conv_executed_flops(a);
                if (flops) { *flops += conv_executed_flops(a); break; }
                if (!dst) return fail(CPN_E_INVALID, "cpn_plan_run: missing external output buffer");
                rc = check_hip((hipError_t) (f32 ? launch_conv_f32(a, st) : fp8 ? launch_conv_fp8(a, st) : launch_conv(a, st)),
                               "conv kernel");
                break;
            }
            default: return fail(CPN_E_INVALID, "cpn_plan_run: unknown op");
        }
        if (rc) return rc;
        if (absmax && o.dst >= 0 && o.op != CPN_OP_INPUT_STEM) {  // calibration: max |x| of the tensor this op produced
            // (the padded stem layout does not fill the input tensor's storage: its scale is set by the caller -- inputs
            // lie in [0, 1])
            const cpn_tensor_desc &t = plan->tensors[o.dst];
            const long count = (long) N * sp.th[o.dst] * sp.tw[o.dst] * t.channels;
            rc = check_hip((hipError_t) launch_absmax_bf16(tptr(o.dst), count, absmax + o.dst, st), "absmax kernel");
            if (rc) return rc;
        }
    }
    if (events) (void) hipEventRecord(events[plan->ops.size()], st);
    return 0;
}

int cpn_plan_num_ops(cpn_plan *plan) { return plan ? (int) plan->ops.size() : 0; }

int cpn_plan_run_timed(cpn_plan *plan, const void *input, int32_t in_dtype, int32_t N, int32_t H, int32_t W,
                       void *workspace, int64_t workspace_bytes, float *const *outputs, int32_t *range_flag,
                       void *stream, float *op_ms, double *op_flops) {
    if (!plan || !op_ms) return fail(CPN_E_INVALID, "cpn_plan_run_timed: null");
    const size_t n = plan->ops.size();
    std::vector<hipEvent_t> ev(n + 1);
    for (auto &e : ev)
        if (hipEventCreate(&e) != hipSuccess) return fail(CPN_E_INVALID, "cpn_plan_run_timed: event create failed");
    if (op_flops) std::fill(op_flops, op_flops + n, 0.);
    int rc = run_or_count(plan, input, in_dtype, N, H, W, workspace, workspace_bytes, outputs, range_flag,
                          (hipStream_t) stream, nullptr, ev.data(), op_flops);
    if (!rc) rc = check_hip(hipEventSynchronize(ev[n]), "cpn_plan_run_timed: sync");
    for (size_t i = 0; i < n && !rc; ++i) (void) hipEventElapsedTime(&op_ms[i], ev[i], ev[i + 1]);
    for (auto &e : ev) (void) hipEventDestroy(e);
    return rc;
}

int cpn_plan_run(cpn_plan *plan, const void *input, int32_t in_dtype, int32_t N, int32_t H, int32_t W,
                 void *workspace, int64_t workspace_bytes, float *const *outputs, int32_t *range_flag, void *stream) {
    return run_or_count(plan, input, in_dtype, N, H, W, workspace, workspace_bytes, outputs, range_flag,
                        (hipStream_t) stream, nullptr);
}

int cpn_plan_run_stats(cpn_plan *plan, const void *input, int32_t in_dtype, int32_t N, int32_t H, int32_t W,
                       void *workspace, int64_t workspace_bytes, float *const *outputs, int32_t *range_flag,
                       float *absmax, void *stream) {
    if (!absmax) return fail(CPN_E_INVALID, "cpn_plan_run_stats: null absmax");
    return run_or_count(plan, input, in_dtype, N, H, W, workspace, workspace_bytes, outputs, range_flag,
                        (hipStream_t) stream, nullptr, nullptr, nullptr, absmax);
}

double cpn_plan_executed_flops(cpn_plan *plan, int32_t N, int32_t H, int32_t W) {
    double f = 0.;
    if (run_or_count(plan, nullptr, 0, N, H, W, nullptr, 0, nullptr, nullptr, nullptr, &f)) return -1.;
    return f;
}

int cpn_conv2d(const cpn_op_desc *op, const void *src0, int32_t c0_stride, const void *src1, int32_t c1_stride,
               const void *res, int32_t res_stride, void *dst, int32_t dst_stride, int32_t N, int32_t Hin, int32_t Win,
               const void *weights, const float *bias, void *stream) {
    ConvArgs a;
    int rc = conv2d_args(op, src0, c0_stride, src1, c1_stride, res, res_stride, dst, dst_stride, N, Hin, Win, weights, bias, a);
    if (rc) return rc;
    return check_hip((hipError_t) launch_conv(a, (hipStream_t) stream), "cpn_conv2d");
}

int cpn_conv2d_sized(const cpn_op_desc *op, const void *src0, int32_t c0_stride, const void *src1, int32_t c1_stride,
                     const void *res, int32_t res_stride, void *dst, int32_t dst_stride, int32_t N, int32_t Hin, int32_t Win,
                     const int32_t stored[6], const void *weights, const float *bias, void *stream) {
    if (!stored) return fail(CPN_E_INVALID, "cpn_conv2d_sized: null pointer");
    if (op && ((op->up0 && (stored[0] < 1 || stored[1] < 1 || stored[0] > Hin || stored[1] > Win)) ||
               (op->up1 && src1 && (stored[2] < 1 || stored[3] < 1 || stored[2] > Hin || stored[3] > Win))))
        return fail(CPN_E_INVALID, "cpn_conv2d_sized: a resized source holds 1 ... Hin x 1 ... Win pixels");
    ConvArgs a;
    int rc = conv2d_args(op, src0, c0_stride, src1, c1_stride, res, res_stride, dst, dst_stride, N, Hin, Win, weights, bias, a, stored);
    if (rc) return rc;
    return check_hip((hipError_t) launch_conv(a, (hipStream_t) stream), "cpn_conv2d_sized");
}

int cpn_conv2d_fp8(const cpn_op_desc *op, const void *src0, int32_t c0_stride, const void *src1, int32_t c1_stride,
                   const void *res, int32_t res_stride, void *dst, int32_t dst_stride, int32_t N, int32_t Hin,
                   int32_t Win, const void *weights, const float *bias, const float *mult, float res_scale,
                   float out_inv_scale, void *stream) {
    ConvArgs a;
    int rc = conv2d_fp8_args(op, src0, c0_stride, src1, c1_stride, res, res_stride, dst, dst_stride, N, Hin, Win, weights, bias,
                             mult, res_scale, out_inv_scale, a);
    if (rc) return rc;
    return check_hip((hipError_t) launch_conv_fp8(a, (hipStream_t) stream), "cpn_conv2d_fp8");
}

int cpn_conv_pair(const cpn_op_desc *op, const void *src, int32_t c_stride, void *dst, int32_t dst_stride, int32_t N,
                  int32_t H, int32_t W, const void *weights, const float *bias, void *stream) {
    if (!op || !src || !dst || !weights || op->op != CPN_OP_CONV_PAIR || N <= 0 || H <= 0 || W <= 0)
        return fail(CPN_E_INVALID, "cpn_conv_pair: needs a CPN_OP_CONV_PAIR descriptor and non-null buffers");
    PairArgs a = pair_args(*op, N, H, W, c_stride, dst_stride, weights, bias);
    a.src = src; a.dst = dst;
    if (!conv_pair_supported(a))
        return fail(CPN_E_UNSUPPORTED, "cpn_conv_pair: needs W = 16 or W >= 32, conv1 output channels a multiple of 256 (128 at "
                                       "W > 32 and for a stride-2 conv2), conv2 bundles of 32 | 64 channels (32 on stride-1 generic tiles)");
    return check_hip((hipError_t) launch_conv_pair(a, (hipStream_t) stream), "cpn_conv_pair");
}

int cpn_conv_bridge(const cpn_op_desc *op, const void *src, int32_t c_stride, const void *res, int32_t res_stride, void *dst,
                    int32_t dst_stride, int32_t N, int32_t H, int32_t W, const void *weights, const float *bias, void *stream) {
    ConvArgs a;
    int rc = conv_bridge_args(op, src, c_stride, res, res_stride, dst, dst_stride, N, H, W, weights, bias, a);
    if (rc) return rc;
    return check_hip((hipError_t) launch_conv(a, (hipStream_t) stream), "cpn_conv_bridge");
}

int cpn_conv2d_kernel_info(const cpn_op_desc *op, int32_t precision, int32_t c0_stride, int32_t c1_stride, int32_t res_stride,
                           int32_t dst_stride, int32_t N, int32_t Hin, int32_t Win, int32_t info[5]) {
    static char dummy[8] = {};  // stands for every buffer: the argument building stores pointers, the selection tests them for null
    if (!op || !info) return fail(CPN_E_INVALID, "cpn_conv2d_kernel_info: null pointer");
    const void *src1 = op->src1 >= 0 ? dummy : nullptr, *res = op->res >= 0 ? dummy : nullptr;
    ConvArgs a;
    ConvKernelSel s{};
    int rc;
    if (precision == CPN_PRECISION_BF16 && op->op == CPN_OP_CONV_BRIDGE) {
        rc = conv_bridge_args(op, dummy, c0_stride, res, res_stride, dummy, dst_stride, N, Hin, Win, dummy, nullptr, a);
        if (!rc) rc = select_conv_kernel(a, s);
    } else if (precision == CPN_PRECISION_BF16) {
        rc = conv2d_args(op, dummy, c0_stride, src1, c1_stride, res, res_stride, dummy, dst_stride, N, Hin, Win, dummy, nullptr, a);
        if (!rc) rc = select_conv_kernel(a, s);
    } else if (precision == CPN_PRECISION_FP8) {
        rc = conv2d_fp8_args(op, dummy, c0_stride, src1, c1_stride, res, res_stride, dummy, dst_stride, N, Hin, Win, dummy, nullptr,
                             nullptr, 1.f, 1.f, a);
        if (!rc) rc = select_conv_kernel_fp8(a, s);
    } else {
        return fail(CPN_E_INVALID, "cpn_conv2d_kernel_info: precision must be CPN_PRECISION_BF16 or CPN_PRECISION_FP8");
    }
    if (rc > 0) return fail(rc, "cpn_conv2d_kernel_info: the conv kernels do not run this call (hipErrorInvalidValue from the launch)");
    if (rc) return rc;
    info[0] = s.mode; info[1] = s.TH; info[2] = s.BN; info[3] = s.WM; info[4] = s.WN;
    return 0;
}

int cpn_convert_input_stem(const void *src, int32_t in_dtype, void *dst, int32_t N, int32_t C, int32_t H, int32_t W,
                           int32_t *range_flag, void *stream) {
    if (!src || !dst || N <= 0 || H <= 0 || W <= 0 || C < 1 || C > 4 || (in_dtype != 0 && in_dtype != 1))
        return fail(CPN_E_INVALID, "cpn_convert_input_stem: bad arguments (1..4 channels, dtype 0 = f32 | 1 = u8)");
    InputArgs a{src, dst, N, C, H, W, 4, in_dtype, range_flag};
    return check_hip((hipError_t) launch_input_stem(a, (hipStream_t) stream), "cpn_convert_input_stem");
}

int cpn_stem7(const cpn_op_desc *op, const void *src, void *dst, int32_t dst_stride, int32_t N, int32_t H, int32_t W,
              const void *weights, const float *bias, float out_inv_scale, void *stream) {
    if (!op || !src || !dst || !weights || N <= 0 || H <= 0 || W <= 0) return fail(CPN_E_INVALID, "cpn_stem7: bad arguments");
    if (op->op != CPN_OP_STEM7 || (op->cout_b != 32 && op->cout_b != 64) || dst_stride < op->cout_b || dst_stride % 8)
        return fail(CPN_E_INVALID, "cpn_stem7: needs a CPN_OP_STEM7 descriptor with 32 | 64 output channels");
    StemArgs a{src, dst, (const unsigned char *) weights + op->weight_offset,
               (bias && op->bias_offset >= 0) ? bias + op->bias_offset : nullptr, N, H, W, (H - 1) / 2 + 1, (W - 1) / 2 + 1,
               op->cout_b, dst_stride, out_inv_scale > 0.f ? out_inv_scale : 0.f};
    return check_hip((hipError_t) launch_stem7(a, (hipStream_t) stream), "cpn_stem7");
}

int cpn_maxpool2d(const void *src, void *dst, int32_t N, int32_t Hin, int32_t Win, int32_t C, int32_t k, int32_t stride,
                  int32_t pad, void *stream) {
    if (C % 8) return fail(CPN_E_INVALID, "cpn_maxpool2d: C must be a multiple of 8");
    PoolArgs a{src, dst, N, Hin, Win, (Hin + 2 * pad - k) / stride + 1, (Win + 2 * pad - k) / stride + 1, C, k, stride, pad};
    return check_hip((hipError_t) launch_maxpool(a, (hipStream_t) stream), "cpn_maxpool2d");
}

int cpn_resize_bilinear(const void *src, void *dst, int32_t N, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout,
                        int32_t C, void *stream) {
    if (C % 8) return fail(CPN_E_INVALID, "cpn_resize_bilinear: C must be a multiple of 8");
    ResizeArgs a{src, dst, N, Hin, Win, Hout, Wout, C};
    return check_hip((hipError_t) launch_bilinear(a, (hipStream_t) stream), "cpn_resize_bilinear");
}

int cpn_convert_input(const void *src, int32_t in_dtype, void *dst, int32_t N, int32_t C, int32_t H, int32_t W,
                      int32_t Cpad, int32_t *range_flag, void *stream) {
    if (Cpad % 8 || Cpad < C) return fail(CPN_E_INVALID, "cpn_convert_input: bad Cpad");
    InputArgs a{src, dst, N, C, H, W, Cpad, in_dtype, range_flag};
    return check_hip((hipError_t) launch_input(a, (hipStream_t) stream), "cpn_convert_input");
}

int cpn_histogram(const void *x, int32_t dtype, int64_t n, uint32_t *hist, void *stream) {
    if (!x || !hist || n < 0 || (dtype != 1 && dtype != 2)) return fail(CPN_E_INVALID, "cpn_histogram: dtype 1 (u8) or 2 (u16)");
    if (n == 0) return 0;
    return check_hip((hipError_t) launch_histogram(x, dtype, (long) n, hist, (hipStream_t) stream), "cpn_histogram");
}

int cpn_window_any(const void *mask, int32_t dtype, int32_t H, int32_t W, const int32_t *windows, int32_t n, int32_t *out,
                   void *stream) {
    if (!mask || (n > 0 && (!windows || !out)) || n < 0 || H <= 0 || W <= 0 || (dtype != 0 && dtype != 1))
        return fail(CPN_E_INVALID, "cpn_window_any: dtype 0 (f32) or 1 (u8 / bool), H, W > 0");
    return check_hip((hipError_t) launch_window_any(mask, dtype, W, windows, n, out, (hipStream_t) stream), "cpn_window_any");
}

int cpn_rescale_to_uint8(const void *x, int32_t dtype, int64_t n, double low, double high, uint8_t *out, void *stream) {
    if (!x || !out || n < 0 || dtype < 0 || dtype > 2) return fail(CPN_E_INVALID, "cpn_rescale_to_uint8: dtype 0 (f32), 1 (u8), 2 (u16)");
    if (!(high > low)) return fail(CPN_E_INVALID, "cpn_rescale_to_uint8: needs high > low");
    if (n == 0) return 0;
    return check_hip((hipError_t) launch_rescale_u8(x, dtype, (long) n, low, high, out, (hipStream_t) stream), "cpn_rescale_to_uint8");
}

}  // extern "C"
