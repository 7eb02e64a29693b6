// Launch trace of the native plan executor on a machine without a GPU (driver: tools/plan_trace.py, which also says how this
// program is built).  It links the executor's host units and the conv kernel objects (select_conv_kernel, conv_pair_supported,
// conv_pair_blocks and the FLOP functions are the real ones), but the unit with the run loop is compiled with every launch_* name
// renamed to trace_launch_* (-Dlaunch_conv=trace_launch_conv ...): the stand-ins below print the argument struct they are handed,
// field by field, pointers as offsets from the fake bases the run was given.  No HIP call is reached.
//
// Input: a file of plan records (plan_trace.py export()).  Per record: cpn_plan_create, then per size cpn_plan_workspace_bytes and
// cpn_plan_run; return codes and cpn_last_error() texts are part of the trace.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/cpn_hip.h"
#include "../celldetection_amd/csrc/cpn_kernels.h"

namespace {

// fake device addresses: far apart, never dereferenced
constexpr uintptr_t SPAN = (uintptr_t) 1 << 40;
constexpr uintptr_t WEIGHTS = 1 * SPAN, BIAS = 2 * SPAN, INPUT = 3 * SPAN, ARENA = 4 * SPAN, FLAG = 5 * SPAN, OUTPUT0 = 8 * SPAN;

std::string ptr(const void *p) {
    static const char *names[] = {"?", "weights", "bias", "input", "arena", "flag", "?", "?"};
    const uintptr_t v = (uintptr_t) p;
    if (!p) return "null";
    char buf[64];
    if (v >= OUTPUT0) snprintf(buf, sizeof buf, "out%d+%" PRIuPTR, (int) ((v - OUTPUT0) / SPAN), (v - OUTPUT0) % SPAN);
    else snprintf(buf, sizeof buf, "%s+%" PRIuPTR, names[v / SPAN], v % SPAN);
    return buf;
}
#define P(x) ptr(x).c_str()

}  // namespace

namespace cpn {

static int trace_conv(const char *which, const ConvArgs &a) {
    printf("  %s src0 %s src1 %s c_stride %d %d c0_used %d up %d %d Hs %d %d %d %d s %.9g %.9g %.9g %.9g N %d in %d x %d out %d x %d "
           "k %d %d stride %d pad %d bundles %d cin_b %d cout_b %d weights %s bias %s phase %d region %d %d narrow %d res %s "
           "res_stride %d res_up %d res_cph %d Hr %d Wr %d r %.9g %.9g act %d %.9g out_mode %d dst %s dst_stride %d dst_coff %d "
           "cout_real %d fuse_w %s fuse_b %s fuse %d %d %.9g mult %s scales %.9g %.9g wide %d %d pre %s %s %s %d %d %d %d\n",
           which, P(a.src0), P(a.src1), a.c0_stride, a.c1_stride, a.c0_used, a.up0, a.up1, a.Hs0, a.Ws0, a.Hs1, a.Ws1, a.sy0, a.sx0,
           a.sy1, a.sx1, a.N, a.Hin, a.Win, a.Hout, a.Wout, a.KH, a.KW, a.stride, a.pad, a.bundles, a.cin_b, a.cout_b, P(a.weights),
           P(a.bias), a.phase, a.region, a.region_margin, a.narrow, P(a.res), a.res_stride, a.res_up, a.res_cph, a.Hr, a.Wr, a.ry,
           a.rx, a.act, a.act_scale, a.out_mode, P(a.dst), a.dst_stride, a.dst_coff, a.cout_real, P(a.fuse_w), P(a.fuse_b),
           a.fuse_cout, a.fuse_act, a.fuse_scale, P(a.mult), a.res_scale, a.out_inv_scale, a.dst_wide, a.res_wide, P(a.pre_src),
           P(a.pre_w), P(a.pre_b), a.pre_stride, a.pre_cin, a.pre_H, a.pre_W);
    return 0;
}
int trace_launch_conv(const ConvArgs &a, hipStream_t) { return trace_conv("conv", a); }
int trace_launch_conv_fp8(const ConvArgs &a, hipStream_t) { return trace_conv("conv_fp8", a); }
int trace_launch_conv_f32(const ConvArgs &a, hipStream_t) { return trace_conv("conv_f32", a); }

int trace_launch_conv_pair(const PairArgs &a, hipStream_t) {
    printf("  conv_pair src %s c_stride %d N %d %d x %d cin %d cmid %d w1 %s b1 %s w2 %s b2 %s cb2 %d dst %s dst_stride %d stride %d\n",
           P(a.src), a.c_stride, a.N, a.H, a.W, a.cin, a.cmid, P(a.w1), P(a.b1), P(a.w2), P(a.b2), a.cb2, P(a.dst), a.dst_stride, a.stride);
    return 0;
}

static int trace_pool(const char *which, const PoolArgs &a) {
    printf("  %s src %s dst %s N %d in %d x %d out %d x %d C %d k %d stride %d pad %d\n", which, P(a.src), P(a.dst), a.N, a.Hin, a.Win,
           a.Hout, a.Wout, a.C, a.k, a.stride, a.pad);
    return 0;
}
int trace_launch_maxpool(const PoolArgs &a, hipStream_t) { return trace_pool("maxpool", a); }
int trace_launch_maxpool_f32(const PoolArgs &a, hipStream_t) { return trace_pool("maxpool_f32", a); }
int trace_launch_maxpool_fp8(const PoolArgs &a, hipStream_t) { return trace_pool("maxpool_fp8", a); }

static int trace_act(const char *which, const ActArgs &a) {
    printf("  %s src %s dst %s count %ld act %d scales %.9g %.9g\n", which, P(a.src), P(a.dst), a.count, a.act, a.in_scale, a.out_inv_scale);
    return 0;
}
int trace_launch_act(const ActArgs &a, hipStream_t) { return trace_act("act", a); }
int trace_launch_act_f32(const ActArgs &a, hipStream_t) { return trace_act("act_f32", a); }
int trace_launch_act_fp8(const ActArgs &a, hipStream_t) { return trace_act("act_fp8", a); }

static int trace_resize(const char *which, const ResizeArgs &a) {
    printf("  %s src %s dst %s N %d in %d x %d out %d x %d C %d ring %d mode %d\n", which, P(a.src), P(a.dst), a.N, a.Hin, a.Win, a.Hout,
           a.Wout, a.C, a.ring, a.mode);
    return 0;
}
int trace_launch_bilinear(const ResizeArgs &a, hipStream_t) { return trace_resize("bilinear", a); }
int trace_launch_bilinear_f32(const ResizeArgs &a, hipStream_t) { return trace_resize("bilinear_f32", a); }
int trace_launch_bilinear_fp8(const ResizeArgs &a, hipStream_t) { return trace_resize("bilinear_fp8", a); }

static int trace_input(const char *which, const InputArgs &a, float inv_scale) {
    printf("  %s src %s dst %s N %d C %d %d x %d Cpad %d dtype %d flag %s inv_scale %.9g\n", which, P(a.src), P(a.dst), a.N, a.C, a.H, a.W,
           a.Cpad, a.dtype, P(a.range_flag), inv_scale);
    return 0;
}
int trace_launch_input(const InputArgs &a, hipStream_t) { return trace_input("input", a, 0.f); }
int trace_launch_input_f32(const InputArgs &a, hipStream_t) { return trace_input("input_f32", a, 0.f); }
int trace_launch_input_fp8(const InputArgs &a, float inv_scale, hipStream_t) { return trace_input("input_fp8", a, inv_scale); }
int trace_launch_input_stem(const InputArgs &a, hipStream_t) { return trace_input("input_stem", a, 0.f); }

int trace_launch_stem7(const StemArgs &a, hipStream_t) {
    printf("  stem7 src %s dst %s weights %s bias %s N %d in %d x %d out %d x %d coutp %d dst_stride %d out_inv_scale %.9g\n", P(a.src),
           P(a.dst), P(a.weights), P(a.bias), a.N, a.H, a.W, a.Hout, a.Wout, a.coutp, a.dst_stride, a.out_inv_scale);
    return 0;
}

// referenced by entry points this program never calls
int trace_launch_absmax_bf16(const void *, long, float *, hipStream_t) { abort(); }
int trace_launch_histogram(const void *, int, long, unsigned int *, hipStream_t) { abort(); }
int trace_launch_window_any(const void *, int, int, const int *, int, int *, hipStream_t) { abort(); }
int trace_launch_rescale_u8(const void *, int, long, double, double, unsigned char *, hipStream_t) { abort(); }

}  // namespace cpn

static bool read(FILE *f, void *dst, size_t bytes) { return fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    if (argc != 2 && argc != 3) { fprintf(stderr, "usage: plan_trace RECORDS [NAME of the one record to run]\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    int32_t sizes[2];
    if (!f || !read(f, sizes, sizeof sizes) || sizes[0] != (int32_t) sizeof(cpn_tensor_desc) || sizes[1] != (int32_t) sizeof(cpn_op_desc)) {
        fprintf(stderr, "plan_trace: cannot read %s, or its descriptor sizes are not this build's\n", argv[1]);
        return 2;
    }
    float *outputs[CPN_NUM_OUTPUTS];
    for (int i = 0; i < CPN_NUM_OUTPUTS; ++i) outputs[i] = (float *) (OUTPUT0 + i * SPAN);
    int32_t name_len;
    while (read(f, &name_len, sizeof name_len)) {
        std::string name(name_len, ' ');
        int32_t head[4];  // precision, n_tensors, n_ops, n_sizes
        int64_t blobs[2];  // weight bytes, bias count
        if (!read(f, &name[0], name_len) || !read(f, head, sizeof head) || !read(f, blobs, sizeof blobs)) return 2;
        std::vector<int32_t> nhw(3 * head[3]);
        std::vector<cpn_tensor_desc> tensors(head[1]);
        std::vector<cpn_op_desc> ops(head[2]);
        if (!read(f, nhw.data(), nhw.size() * sizeof(int32_t)) || !read(f, tensors.data(), tensors.size() * sizeof(cpn_tensor_desc)) ||
            !read(f, ops.data(), ops.size() * sizeof(cpn_op_desc)))
            return 2;
        if (argc == 3 && name != argv[2]) continue;
        cpn_plan *plan = nullptr;
        int rc = cpn_plan_create(&plan, tensors.data(), head[1], ops.data(), head[2], (const void *) WEIGHTS, (size_t) blobs[0],
                                 (const float *) BIAS, (size_t) blobs[1], head[0]);
        printf("# %s: create %d%s%s\n", name.c_str(), rc, rc ? " " : "", rc ? cpn_last_error() : "");
        if (rc) continue;
        for (int s = 0; s < head[3]; ++s) {
            const int N = nhw[3 * s], H = nhw[3 * s + 1], W = nhw[3 * s + 2];
            const int64_t bytes = cpn_plan_workspace_bytes(plan, N, H, W);
            printf("## %s N=%d H=%d W=%d workspace %" PRId64 "%s%s\n", name.c_str(), N, H, W, bytes, bytes < 0 ? " " : "",
                   bytes < 0 ? cpn_last_error() : "");
            rc = cpn_plan_run(plan, (const void *) INPUT, 0, N, H, W, (void *) ARENA, INT64_MAX, outputs, (int32_t *) FLAG, nullptr);
            printf("## run %d%s%s\n", rc, rc ? " " : "", rc ? cpn_last_error() : "");
        }
        cpn_plan_destroy(plan);
    }
    fclose(f);
    return 0;
}
