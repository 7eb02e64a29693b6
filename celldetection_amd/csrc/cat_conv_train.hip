// Trainable concat convolution on the GPU (gfx950): the two backward pieces behind celldetection_amd.nn.cat_conv2d that
// csrc/conv_igemm.hip and csrc/conv_train.hip do not provide.  The rule is the "Trainable concat convolution" section of
// include/cpn_hip.h.  The conv's input is the VIRTUAL tensor cat(x0, resize(x1)): x0 [N][H][W][C0] and x1 [N][h][w][C1] read
// through the nearest map of csrc/nearest_adjoint.h; neither the resized nor the concatenated tensor exists in memory.
//
//   CcSources:             the weight gradient over the virtual concat is the dense one (csrc/wgrad_dense.h: ct_wgrad_slab_kernel,
//                          ct_wgrad_reduce_kernel and the host path around them) with this Source; it writes
//                          dW [Cout][C0 + C1][k][k].  A 32-channel block of the 64-channel tile belongs to ONE source
//                          (C0 % 32 == 0; the two blocks of a tile may belong to different ones).  A block of x0 is staged as it
//                          lies; a block of x1 is gathered: the source pixel of each of the CT_CH + K - 1 staged pixels is computed
//                          once per chunk into the kernel's LDS table, and every 16-byte item of the row looks its pixel up there.
//   cc_nearest_sum_kernel:  the adjoint of the resize.  A lane owns 16 bytes (8 channels) of one source pixel, adds the pixels of
//                          its footprint in ascending row-major order in fp32 and rounds once; an empty footprint gives zeros.
// The bias gradient is that of csrc/wgrad_bias.h.  No floating-point atomics: results are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "nearest_adjoint.h"
#include "wgrad_dense.h"  // the dense weight gradient: slab kernel, reduce kernel, check, workspace, launches; ct_bf16_rne
#include "wgrad_slabs.h"

namespace {

// cat(x0, resize(x1)): the table entry of a staged row is its x1 pixel (int32; negative outside the tensor)
struct CcSources {
    static constexpr int ENTRY = 4, KMIN = 1;
    const uint16_t *x0, *x1;  // x0 may be null with C0 == 0 (the bridge level)
    int C0, C1, h1, w1;
    float sy, sx;             // na_scale(h1, H), na_scale(w1, W)
    __device__ __forceinline__ int channels() const { return C0 + C1; }
    __device__ __forceinline__ void fill(char *entry, int64_t f, long P, int H, int W) const {
        int g = -1;
        if (f >= 0 && f < P) g = na_pixel_src((int32_t) f, H, W, h1, w1, sy, sx);
        *(int *) entry = g;
    }
    __device__ __forceinline__ u32x4 item(const char *entry, int64_t f, long, int ch, int q) const {
        const int g = *(const int *) entry;
        u32x4 v = {0, 0, 0, 0};
        if (g >= 0 && ch < C0 + C1) {  // (one offset per load: two loads under their branches, not one load of a chosen address)
            if (ch < C0) v = *(const u32x4 *) (x0 + (f * C0 + ch + q * 8));
            else v = *(const u32x4 *) (x1 + ((int64_t) g * C1 + (ch - C0) + q * 8));
        }
        return v;
    }
};

// t [N][H][W][C] -> dst [N][h][w][C]: dst[n][i][j] = sum of t[n][y][x] over the footprint of (i, j), 8 channels per lane
__global__ __launch_bounds__(256) void cc_nearest_sum_kernel(const uint16_t *__restrict__ t, uint16_t *__restrict__ dst, int H, int W,
                                                              int C8, int h, int w, float sy, float sx, long total) {
    const long o = (long) blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int c8 = (int) (o % C8);
    const long pix = o / C8;
    const int j = (int) (pix % w), i = (int) ((pix / w) % h);
    const long n = pix / ((long) w * h);
    const int y0 = na_first(i, sy, h, H), y1 = na_first(i + 1, sy, h, H);
    const int x0 = na_first(j, sx, w, W), x1 = na_first(j + 1, sx, w, W);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            const u32x4 v = *(const u32x4 *) (t + (((n * H + y) * W + x) * C8 + c8) * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[2 * e] += __uint_as_float(v[e] << 16);
                acc[2 * e + 1] += __uint_as_float(v[e] & 0xffff0000u);
            }
        }
    u32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (uint32_t) ct_bf16_rne(acc[2 * e]) | ((uint32_t) ct_bf16_rne(acc[2 * e + 1]) << 16);
    *(u32x4 *) (dst + o * 8) = r;
}

// 0, or the error code with its message recorded; the partition of an accepted call (the dense weight gradient's, on the C0 + C1
// channels of the virtual concat)
int cc_check(const char *who, int N, int H, int W, int c0, int c1, int h1, int w1, int cout, int k, int slab_rows, WgSlabs *part) {
    static thread_local char msg[200];
    const char *bad = nullptr;
    if (N < 1 || H < 1 || W < 1) bad = "N, H and W must be at least 1";
    else if (h1 < 1 || w1 < 1 || h1 > H || w1 > W) bad = "h1 and w1 must lie in 1 ... H and 1 ... W";
    else if (c0 < 0 || c0 % 32 || c1 < 32 || c1 % 32 || cout < 32 || cout % 32)
        bad = "c0 must be 0 or a positive multiple of 32, c1 and cout positive multiples of 32";
    else if (k != 1 && k != 3 && k != 5 && k != 7) bad = "k must be 1, 3, 5 or 7";
    else if (slab_rows < 0) bad = "slab_rows must be 0 (auto) or positive";
    if (bad) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return cpn::fail(CPN_E_INVALID, msg);
    }
    return ct_check_partition(who, N, H, W, (int64_t) c0 + c1, cout, k, slab_rows, part);
}

}  // namespace

extern "C" {

int64_t cpn_cat_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t c0, int32_t c1, int32_t h1, int32_t w1,
                                           int32_t cout, int32_t k, int32_t slab_rows) {
    WgSlabs part;
    if (cc_check("cpn_cat_conv_wgrad_workspace_bytes", N, H, W, c0, c1, h1, w1, cout, k, slab_rows, &part)) return 0;
    return ct_workspace_bytes(part.slabs, c0 + c1, cout, k);
}

int cpn_cat_conv_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t c0, int32_t c1, int32_t h1, int32_t w1, int32_t cout, int32_t k,
                            int32_t slab_rows, int32_t info[5]) {
    WgSlabs part;
    if (const int rc = cc_check("cpn_cat_conv_wgrad_info", N, H, W, c0, c1, h1, w1, cout, k, slab_rows, &part)) return rc;
    if (!info) return cpn::fail(CPN_E_INVALID, "cpn_cat_conv_wgrad_info: null pointer");
    wgs_info(part, info);
    return 0;
}

int cpn_cat_conv_wgrad(const void *x0, const void *x1, const void *dy, int32_t N, int32_t H, int32_t W, int32_t c0, int32_t c1,
                       int32_t h1, int32_t w1, int32_t cout, int32_t k, int32_t slab_rows, void *dw, int32_t dw_dtype, void *db,
                       int32_t db_dtype, void *workspace, int64_t workspace_bytes, void *stream) {
    WgSlabs part;
    if (const int rc = cc_check("cpn_cat_conv_wgrad", N, H, W, c0, c1, h1, w1, cout, k, slab_rows, &part)) return rc;
    if ((c0 > 0) != (x0 != nullptr)) return cpn::fail(CPN_E_INVALID, "cpn_cat_conv_wgrad: x0 must be null exactly when c0 is 0");
    if (!x1 || !dy || !workspace || (!dw && !db)) return cpn::fail(CPN_E_INVALID, "cpn_cat_conv_wgrad: null pointer");
    if (((uintptr_t) x0 | (uintptr_t) x1 | (uintptr_t) dy) & 15)
        return cpn::fail(CPN_E_INVALID, "cpn_cat_conv_wgrad: x0, x1 and dy must start at 16-byte aligned addresses");
    if ((dw && dw_dtype != CT_F32 && dw_dtype != CT_BF16) || (db && db_dtype != CT_F32 && db_dtype != CT_BF16))
        return cpn::fail(CPN_E_INVALID, "cpn_cat_conv_wgrad: an output dtype must be 0 (fp32) or 1 (bf16)");
    if (workspace_bytes < ct_workspace_bytes(part.slabs, c0 + c1, cout, k))
        return cpn::fail(CPN_E_WORKSPACE, "cpn_cat_conv_wgrad: workspace smaller than cpn_cat_conv_wgrad_workspace_bytes");
    const CcSources src{(const uint16_t *) x0, (const uint16_t *) x1, c0, c1, h1, w1, na_scale(h1, H), na_scale(w1, W)};
    ct_launch_wgrad(part, dy, src, H, c0 + c1, cout, k, dw, dw_dtype, db, db_dtype, workspace, (hipStream_t) stream);
    return cpn::check_hip(hipGetLastError(), "cpn_cat_conv_wgrad");
}

int cpn_nearest_sum(const void *t, int32_t N, int32_t H, int32_t W, int32_t C, void *dst, int32_t h, int32_t w, void *stream) {
    if (N < 1 || H < 1 || W < 1 || h < 1 || w < 1 || h > H || w > W)
        return cpn::fail(CPN_E_INVALID, "cpn_nearest_sum: N, H, W at least 1, h and w in 1 ... H and 1 ... W");
    if (C < 8 || C % 8) return cpn::fail(CPN_E_INVALID, "cpn_nearest_sum: C must be a positive multiple of 8");
    if ((int64_t) N * H * W > 0x7fffffffll) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_nearest_sum: more than 2^31 - 1 pixels");
    if (!t || !dst) return cpn::fail(CPN_E_INVALID, "cpn_nearest_sum: null pointer");
    if (((uintptr_t) t | (uintptr_t) dst) & 15)
        return cpn::fail(CPN_E_INVALID, "cpn_nearest_sum: t and dst must start at 16-byte aligned addresses");
    const long total = (long) N * h * w * (C / 8);
    if ((total + 255) / 256 > 0x7fffffffl) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_nearest_sum: more than 2^31 - 1 workgroups");
    hipLaunchKernelGGL(cc_nearest_sum_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, (hipStream_t) stream,
                       (const uint16_t *) t, (uint16_t *) dst, H, W, C / 8, h, w, na_scale(h, H), na_scale(w, W), total);
    return cpn::check_hip(hipGetLastError(), "cpn_nearest_sum");
}

}  // extern "C"
