// Trainable bilinear resize on the GPU (gfx950): the backward pieces behind celldetection_amd.nn.bilinear_resize and
// nn.resized_conv2d that csrc/misc_kernels.hip, csrc/conv_igemm.hip and csrc/conv_train.hip do not provide.  The rule is the
// "Trainable bilinear resize" section of include/cpn_hip.h; the index arithmetic is csrc/bilinear_adjoint.h.  This unit is compiled
// with -ffp-contract=off: the blend and the sums have one stated order of operations.
//
//   bl_sum_kernel:         the adjoint of the resize on bf16 NHWC activations.  A lane owns 16 bytes (8 channels) of one source pixel,
//                          walks its footprint (rows x columns, ascending row-major) and adds ba_weight_y * ba_weight_x * t in
//                          fp32 -- the coefficient first, then one multiply and one add -- and rounds once.
//   bl_sum_planes_kernel:  the same adjoint on fp32 NCHW planes (the head maps): one lane per source pixel of one plane, fp32 out.
//   BlSource:              the weight gradient of a k x k stride-1 conv whose input is the VIRTUAL tensor resize(x) is the dense one
//                          (csrc/wgrad_dense.h: ct_wgrad_slab_kernel, ct_wgrad_reduce_kernel and the host path around them,
//                          compiled here under this unit's flags) with this Source.  Once per 128-pixel chunk the kernel's per-row
//                          LDS table takes the four source pixels (negative outside the tensor) and the two lambdas of every staged
//                          pixel; every 16-byte item then loads its four source items, blends
//                          hy * (hx * a00 + lx * a01) + ly * (hx * a10 + lx * a11) in fp32, rounds to bf16 (RNE) and writes the LDS
//                          row.  Neither the resized tensor nor a workspace of its size exists.
// The bias gradient is that of csrc/wgrad_bias.h.  No floating-point atomics, no scatter: results are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"
#include "bilinear_adjoint.h"
#include "cpn_error.h"
#include "wgrad_dense.h"  // the dense weight gradient: slab kernel, reduce kernel, check, workspace, launches; ct_bf16_rne
#include "wgrad_slabs.h"

namespace {

__device__ __forceinline__ float bl_lo(uint32_t v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float bl_hi(uint32_t v) { return __uint_as_float(v & 0xffff0000u); }

// hy * (hx * a00 + lx * a01) + ly * (hx * a10 + lx * a11): four products, two sums, two products, one sum
__device__ __forceinline__ float bl_blend(float a00, float a01, float a10, float a11, float hy, float ly, float hx, float lx) {
    return hy * (hx * a00 + lx * a01) + ly * (hx * a10 + lx * a11);
}

// resize(x): the table entry of a staged row is its four source pixels (int32; negative outside the tensor), lambda_y, lambda_x
// (fp32), 8 bytes unused
struct BlSource {
    static constexpr int ENTRY = 32, KMIN = 3;
    const uint16_t *x;  // [N][h][w][C]
    int C, h, w;
    float sy, sx;       // ba_scale(h, H), ba_scale(w, W)
    __device__ __forceinline__ int channels() const { return C; }
    __device__ __forceinline__ void fill(char *entry, int64_t f, long P, int H, int W) const {
        int g[4] = {-1, -1, -1, -1};
        float ly = 0.f, lx = 0.f;
        if (f >= 0 && f < P) {
            const unsigned row = (unsigned) f / (unsigned) W;
            const int px = (int) ((unsigned) f - row * (unsigned) W);
            const unsigned n = row / (unsigned) H;
            const int py = (int) (row - n * (unsigned) H);
            int y0, y1, x0, x1;
            ba_tap(py, sy, h, true, &y0, &y1, &ly);  // (fused: the conv loader's form of the coordinate)
            ba_tap(px, sx, w, true, &x0, &x1, &lx);
            y0 = min(y0, h - 1), y1 = min(y1, h - 1);  // (they are inside already for h <= H: a guard, not a rule)
            x0 = min(x0, w - 1), x1 = min(x1, w - 1);
            const int r0 = ((int) n * h + y0) * w, r1 = ((int) n * h + y1) * w;
            g[0] = r0 + x0, g[1] = r0 + x1, g[2] = r1 + x0, g[3] = r1 + x1;
        }
        *(u32x4 *) entry = u32x4{(unsigned) g[0], (unsigned) g[1], (unsigned) g[2], (unsigned) g[3]};
        *(float *) (entry + 16) = ly;
        *(float *) (entry + 20) = lx;
    }
    __device__ __forceinline__ u32x4 item(const char *entry, int64_t, long, int ch, int q) const {
        const u32x4 g = *(const u32x4 *) entry;
        u32x4 v = {0, 0, 0, 0};
        if ((int) g[0] >= 0 && ch < C) {
            const float ly = *(const float *) (entry + 16), lx = *(const float *) (entry + 20);
            const float hy = 1.f - ly, hx = 1.f - lx;
            const uint16_t *base = x + ch + q * 8;
            const u32x4 a00 = *(const u32x4 *) (base + (int64_t) (int) g[0] * C), a01 = *(const u32x4 *) (base + (int64_t) (int) g[1] * C);
            const u32x4 a10 = *(const u32x4 *) (base + (int64_t) (int) g[2] * C), a11 = *(const u32x4 *) (base + (int64_t) (int) g[3] * C);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float lo = bl_blend(bl_lo(a00[e]), bl_lo(a01[e]), bl_lo(a10[e]), bl_lo(a11[e]), hy, ly, hx, lx);
                const float hi = bl_blend(bl_hi(a00[e]), bl_hi(a01[e]), bl_hi(a10[e]), bl_hi(a11[e]), hy, ly, hx, lx);
                v[e] = (uint32_t) ct_bf16_rne(lo) | ((uint32_t) ct_bf16_rne(hi) << 16);
            }
        }
        return v;
    }
};

// The column weights of a footprint do not depend on the row: the first BL_WX of them are computed once, before the row loop, and
// kept in registers (read with compile-time indices only); a wider footprint computes the rest where it uses them.  The values and
// the order of the operations are those of the plain double loop.
constexpr int BL_WX = 8;

template <bool FUSED>
__device__ __forceinline__ void bl_column_weights(float (&wx)[BL_WX], int x0, int x1, float sx, int w, int j) {
#pragma unroll
    for (int a = 0; a < BL_WX; ++a) wx[a] = x0 + a < x1 ? ba_weight(x0 + a, sx, w, FUSED, j) : 0.f;
}

// t [N][H][W][C] -> dst [N][h][w][C]: dst[n][i][j] = sum over the footprint of (i, j) of weight_y(y, i) weight_x(x, j) t[n][y][x],
// 8 channels per lane; the coordinate fused, as bilinear_kernel and the conv loader compute it
__global__ __launch_bounds__(256) void bl_sum_kernel(const uint16_t *__restrict__ t, uint16_t *__restrict__ dst, int H, int W, int C8,
                                                      int h, int w, float sy, float sx, long total) {
    constexpr bool FUSED = true;
    const long o = (long) blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int c8 = (int) (o % C8);
    const long pix = o / C8;
    const int j = (int) (pix % w), i = (int) ((pix / w) % h);
    const long n = pix / ((long) w * h);
    const int y0 = ba_first(i - 1, sy, h, H, FUSED), y1 = ba_first(i + 1, sy, h, H, FUSED);
    const int x0 = ba_first(j - 1, sx, w, W, FUSED), x1 = ba_first(j + 1, sx, w, W, FUSED);
    float wx[BL_WX];
    bl_column_weights<FUSED>(wx, x0, x1, sx, w, j);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const auto add = [&](float c, const uint16_t *p) {
        const u32x4 v = *(const u32x4 *) p;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[2 * e] = acc[2 * e] + c * bl_lo(v[e]);
            acc[2 * e + 1] = acc[2 * e + 1] + c * bl_hi(v[e]);
        }
    };
    for (int y = y0; y < y1; ++y) {
        const float wy = ba_weight(y, sy, h, FUSED, i);
        const uint16_t *row = t + (((n * H + y) * W + x0) * C8 + c8) * 8;
#pragma unroll
        for (int a = 0; a < BL_WX; ++a)
            if (x0 + a < x1) add(wy * wx[a], row + (long) a * C8 * 8);
        for (int x = x0 + BL_WX; x < x1; ++x) add(wy * ba_weight(x, sx, w, FUSED, j), row + (long) (x - x0) * C8 * 8);
    }
    u32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (uint32_t) ct_bf16_rne(acc[2 * e]) | ((uint32_t) ct_bf16_rne(acc[2 * e + 1]) << 16);
    *(u32x4 *) (dst + o * 8) = r;
}

// t [P][H][W] -> dst [P][h][w], fp32: the same sum, one lane per source pixel of one plane; the coordinate split, as
// resize_f32_kernel computes it
__global__ __launch_bounds__(256) void bl_sum_planes_kernel(const float *__restrict__ t, float *__restrict__ dst, int H, int W, int h,
                                                             int w, float sy, float sx, long total) {
    constexpr bool FUSED = false;
    const long o = (long) blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int j = (int) (o % w), i = (int) ((o / w) % h);
    const long plane = o / ((long) w * h);
    const int y0 = ba_first(i - 1, sy, h, H, FUSED), y1 = ba_first(i + 1, sy, h, H, FUSED);
    const int x0 = ba_first(j - 1, sx, w, W, FUSED), x1 = ba_first(j + 1, sx, w, W, FUSED);
    const float *src = t + plane * H * W;
    float wx[BL_WX];
    bl_column_weights<FUSED>(wx, x0, x1, sx, w, j);
    float acc = 0.f;
    for (int y = y0; y < y1; ++y) {
        const float wy = ba_weight(y, sy, h, FUSED, i);
        const float *row = src + (long) y * W + x0;
#pragma unroll
        for (int a = 0; a < BL_WX; ++a)
            if (x0 + a < x1) {
                const float c = wy * wx[a];
                acc = acc + c * row[a];
            }
        for (int x = x0 + BL_WX; x < x1; ++x) {
            const float c = wy * ba_weight(x, sx, w, FUSED, j);
            acc = acc + c * row[x - x0];
        }
    }
    dst[o] = acc;
}

// 0, or the error code with its message recorded; the partition of an accepted call
int bl_check(const char *who, int N, int H, int W, int cin, int h, int w, int cout, int k, int slab_rows, WgSlabs *part) {
    static thread_local char msg[200];
    const char *bad = nullptr;
    if (N < 1 || H < 1 || W < 1) bad = "N, H and W must be at least 1";
    else if (h < 1 || w < 1 || h > H || w > W) bad = "h and w must lie in 1 ... H and 1 ... W";
    else if (cin < 32 || cin % 32 || cout < 32 || cout % 32) bad = "cin and cout must be positive multiples of 32";
    else if (k != 3 && k != 5 && k != 7) bad = "k must be 3, 5 or 7";
    else if (slab_rows < 0) bad = "slab_rows must be 0 (auto) or positive";
    if (bad) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return cpn::fail(CPN_E_INVALID, msg);
    }
    return ct_check_partition(who, N, H, W, cin, cout, k, slab_rows, part);
}

// the shared argument checks of the two footprint sums (N: images or planes; per_pixel: lanes per source pixel; align: bytes)
int bl_sum_check(const char *who, int64_t N, int H, int W, int h, int w, const void *t, const void *dst, int per_pixel, int align) {
    static thread_local char msg[200];
    const char *bad = nullptr;
    int code = CPN_E_INVALID;
    const int64_t hw = (int64_t) H * W;
    if (N < 1 || H < 1 || W < 1 || h < 1 || w < 1 || h > H || w > W) bad = "N, H, W at least 1, h and w in 1 ... H and 1 ... W";
    else if (hw > 0x7fffffffll || N > 0x7fffffffll / hw) bad = "more than 2^31 - 1 pixels", code = CPN_E_UNSUPPORTED;
    else if (!t || !dst) bad = "null pointer";
    else if (((uintptr_t) t | (uintptr_t) dst) & (uintptr_t) (align - 1))
        bad = align == 16 ? "t and dst must start at 16-byte aligned addresses" : "t and dst must start at 4-byte aligned addresses";
    else if ((N * h * w * per_pixel + 255) / 256 > 0x7fffffffll) bad = "more than 2^31 - 1 workgroups", code = CPN_E_UNSUPPORTED;
    if (!bad) return 0;
    snprintf(msg, sizeof msg, "%s: %s", who, bad);
    return cpn::fail(code, msg);
}

}  // namespace

extern "C" {

int64_t cpn_resized_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t h, int32_t w, int32_t cout,
                                               int32_t k, int32_t slab_rows) {
    WgSlabs part;
    if (bl_check("cpn_resized_conv_wgrad_workspace_bytes", N, H, W, cin, h, w, cout, k, slab_rows, &part)) return 0;
    return ct_workspace_bytes(part.slabs, cin, cout, k);
}

int cpn_resized_conv_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t k,
                                int32_t slab_rows, int32_t info[5]) {
    WgSlabs part;
    if (const int rc = bl_check("cpn_resized_conv_wgrad_info", N, H, W, cin, h, w, cout, k, slab_rows, &part)) return rc;
    if (!info) return cpn::fail(CPN_E_INVALID, "cpn_resized_conv_wgrad_info: null pointer");
    wgs_info(part, info);
    return 0;
}

int cpn_resized_conv_wgrad(const void *x, const void *dy, int32_t N, int32_t H, int32_t W, int32_t cin, int32_t h, int32_t w,
                           int32_t cout, int32_t k, int32_t slab_rows, void *dw, int32_t dw_dtype, void *db, int32_t db_dtype,
                           void *workspace, int64_t workspace_bytes, void *stream) {
    WgSlabs part;
    if (const int rc = bl_check("cpn_resized_conv_wgrad", N, H, W, cin, h, w, cout, k, slab_rows, &part)) return rc;
    if (!x || !dy || !workspace || (!dw && !db)) return cpn::fail(CPN_E_INVALID, "cpn_resized_conv_wgrad: null pointer");
    if (((uintptr_t) x | (uintptr_t) dy) & 15)
        return cpn::fail(CPN_E_INVALID, "cpn_resized_conv_wgrad: x and dy must start at 16-byte aligned addresses");
    if ((dw && dw_dtype != CT_F32 && dw_dtype != CT_BF16) || (db && db_dtype != CT_F32 && db_dtype != CT_BF16))
        return cpn::fail(CPN_E_INVALID, "cpn_resized_conv_wgrad: an output dtype must be 0 (fp32) or 1 (bf16)");
    if (workspace_bytes < ct_workspace_bytes(part.slabs, cin, cout, k))
        return cpn::fail(CPN_E_WORKSPACE, "cpn_resized_conv_wgrad: workspace smaller than cpn_resized_conv_wgrad_workspace_bytes");
    const BlSource src{(const uint16_t *) x, cin, h, w, ba_scale(h, H), ba_scale(w, W)};
    ct_launch_wgrad(part, dy, src, H, cin, cout, k, dw, dw_dtype, db, db_dtype, workspace, (hipStream_t) stream);
    return cpn::check_hip(hipGetLastError(), "cpn_resized_conv_wgrad");
}

int cpn_bilinear_sum(const void *t, int32_t N, int32_t H, int32_t W, int32_t C, void *dst, int32_t h, int32_t w, void *stream) {
    if (C < 8 || C % 8) return cpn::fail(CPN_E_INVALID, "cpn_bilinear_sum: C must be a positive multiple of 8");
    if (const int rc = bl_sum_check("cpn_bilinear_sum", N, H, W, h, w, t, dst, C / 8, 16)) return rc;
    const long total = (long) N * h * w * (C / 8);
    hipLaunchKernelGGL(bl_sum_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, (hipStream_t) stream, (const uint16_t *) t,
                       (uint16_t *) dst, H, W, C / 8, h, w, ba_scale(h, H), ba_scale(w, W), total);
    return cpn::check_hip(hipGetLastError(), "cpn_bilinear_sum");
}

int cpn_bilinear_sum_f32(const float *t, int64_t planes, int32_t H, int32_t W, float *dst, int32_t h, int32_t w, void *stream) {
    if (const int rc = bl_sum_check("cpn_bilinear_sum_f32", planes, H, W, h, w, t, dst, 1, 4)) return rc;
    const long total = (long) planes * h * w;
    hipLaunchKernelGGL(bl_sum_planes_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, (hipStream_t) stream, t, dst, H, W, h,
                       w, ba_scale(h, H), ba_scale(w, W), total);
    return cpn::check_hip(hipGetLastError(), "cpn_bilinear_sum_f32");
}

}  // extern "C"
