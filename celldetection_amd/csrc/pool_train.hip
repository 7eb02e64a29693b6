// Max-pool with its tap index and gather gradient on the GPU (gfx950): what celldetection_amd.nn.max_pool2d runs.  The rule is the
// max-pool part of the "Trainable stem and max-pool" section of include/cpn_hip.h; the index arithmetic is csrc/pool_adjoint.h.
//
//   mp_pool_kernel:          max-pool (3, 2, 1) | (2, 2, 0) with the tap index of the first maximum, 16 bytes per lane.
//   mp_pool_backward_kernel: the gradient as a gather: a lane owns 16 bytes of one input pixel and visits the windows that cover
//                            it (csrc/pool_adjoint.h) in raster order.
// No floating-point atomics: results are bit-identical from run to run.  Inputs are finite: NaN is outside the contract (a NaN never
// takes a window over, so a window of NaNs alone yields -inf).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "mfma_frag.h"  // u32x4
#include "pool_adjoint.h"
#include "wgrad_bias.h"  // ct_bf16_rne, the dtype codes

namespace {

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// ---- max-pool -------------------------------------------------------------------------------------------------------------
// A lane owns 16 bytes of one pixel: E = 8 bf16 or 4 fp32 channels.
template <bool BF16>
struct MpLane {
    static constexpr int E = BF16 ? 8 : 4;
    static __device__ __forceinline__ void load(const void *base, long item, float v[E]) {
        const u32x4 u = *(const u32x4 *) ((const unsigned char *) base + item * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (BF16) {
                v[2 * e] = __uint_as_float(u[e] << 16);
                v[2 * e + 1] = __uint_as_float(u[e] & 0xffff0000u);
            } else {
                v[e] = __uint_as_float(u[e]);
            }
        }
    }
};

template <bool BF16>
__global__ __launch_bounds__(256) void mp_pool_kernel(const void *__restrict__ x, void *__restrict__ y, unsigned char *__restrict__ index,
                                                      int H, int W, int G, int Hout, int Wout, int k, int s, int pad, long total) {
    constexpr int E = MpLane<BF16>::E;
    const long o = (long) blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int g = (int) (o % G);
    const long pix = o / G;
    const int ox = (int) (pix % Wout), oy = (int) ((pix / Wout) % Hout);
    const long n = pix / ((long) Wout * Hout);
    float best[E];
    int tap[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        best[e] = -__builtin_inff();
        tap[e] = 0;
    }
    bool first = true;
    for (int ty = 0; ty < k; ++ty) {
        const int iy = pa_position(oy, ty, s, pad);
        if (iy < 0 || iy >= H) continue;
        for (int tx = 0; tx < k; ++tx) {
            const int ix = pa_position(ox, tx, s, pad);
            if (ix < 0 || ix >= W) continue;
            float v[E];
            MpLane<BF16>::load(x, ((n * H + iy) * W + ix) * G + g, v);
            const int t = pa_index(ty, tx, k);
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (first || v[e] > best[e]) {  // strictly greater: the first maximum in raster order keeps the window
                    best[e] = v[e];
                    tap[e] = t;
                }
            first = false;
        }
    }
    u32x4 r;
    if constexpr (BF16) {  // (the values are the input's own: nothing is rounded)
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = (__float_as_uint(best[2 * e]) >> 16) | (__float_as_uint(best[2 * e + 1]) & 0xffff0000u);
        u32x2 ti;
        ti.x = (unsigned) tap[0] | ((unsigned) tap[1] << 8) | ((unsigned) tap[2] << 16) | ((unsigned) tap[3] << 24);
        ti.y = (unsigned) tap[4] | ((unsigned) tap[5] << 8) | ((unsigned) tap[6] << 16) | ((unsigned) tap[7] << 24);
        *(u32x2 *) (index + o * 8) = ti;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = __float_as_uint(best[e]);
        *(unsigned *) (index + o * 4) = (unsigned) tap[0] | ((unsigned) tap[1] << 8) | ((unsigned) tap[2] << 16) | ((unsigned) tap[3] << 24);
    }
    *(u32x4 *) ((unsigned char *) y + o * 16) = r;
}

template <bool BF16>
__global__ __launch_bounds__(256) void mp_pool_backward_kernel(const void *__restrict__ dy, const unsigned char *__restrict__ index,
                                                               void *__restrict__ dx, int H, int W, int G, int Hout, int Wout, int k,
                                                               int s, int pad, long total) {
    constexpr int E = MpLane<BF16>::E;
    const long o = (long) blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int g = (int) (o % G);
    const long pix = o / G;
    const int ix = (int) (pix % W), iy = (int) ((pix / W) % H);
    const long n = pix / ((long) W * H);
    const int oy0 = pa_first(iy, k, s, pad), oy1 = pa_last(iy, s, pad, Hout);
    const int ox0 = pa_first(ix, k, s, pad), ox1 = pa_last(ix, s, pad, Wout);
    float acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    for (int oy = oy0; oy <= oy1; ++oy)
        for (int ox = ox0; ox <= ox1; ++ox) {  // the windows that cover the pixel, in raster order
            const unsigned mine = (unsigned) pa_index(pa_tap(iy, oy, s, pad), pa_tap(ix, ox, s, pad), k);
            const long item = ((n * Hout + oy) * Wout + ox) * G + g;
            float v[E];
            MpLane<BF16>::load(dy, item, v);
            unsigned t[2];
            if constexpr (BF16) {
                const u32x2 ti = *(const u32x2 *) (index + item * 8);
                t[0] = ti.x; t[1] = ti.y;
            } else {
                t[0] = *(const unsigned *) (index + item * 4); t[1] = 0;
            }
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (((t[e >> 2] >> (8 * (e & 3))) & 0xffu) == mine) acc[e] += v[e];
        }
    u32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if constexpr (BF16) r[e] = (unsigned) ct_bf16_rne(acc[2 * e]) | ((unsigned) ct_bf16_rne(acc[2 * e + 1]) << 16);
        else r[e] = __float_as_uint(acc[e]);
    }
    *(u32x4 *) ((unsigned char *) dx + o * 16) = r;
}

// ---- argument checks (0, or the error code with its message recorded) -------------------------------------------------------
int mp_pool_check(const char *who, int dtype, int N, int H, int W, int C, int k, int s, int pad, int *Hout, int *Wout) {
    static thread_local char msg[200];
    const char *bad = nullptr;
    if (N < 1 || H < 1 || W < 1) bad = "N, H and W must be at least 1";
    else if (C < 8 || C % 8) bad = "C must be a positive multiple of 8";
    else if (dtype != CT_F32 && dtype != CT_BF16) bad = "dtype must be 0 (fp32) or 1 (bf16)";
    else if (!((k == 3 && s == 2 && pad == 1) || (k == 2 && s == 2 && pad == 0))) bad = "(k, stride, pad) must be (3, 2, 1) or (2, 2, 0)";
    else if (pa_out(H, k, s, pad) < 1 || pa_out(W, k, s, pad) < 1) bad = "H and W must hold at least one window";
    if (bad) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return cpn::fail(CPN_E_INVALID, msg);
    }
    if ((int64_t) N * H > 0x7fffffffll || (int64_t) N * H * W > 0x7fffffffll || (int64_t) N * H * W * (C / 4) > 0x7fffffffll * 256) {
        snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 pixels or workgroups", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    *Hout = pa_out(H, k, s, pad);
    *Wout = pa_out(W, k, s, pad);
    return 0;
}

}  // namespace

extern "C" {

int cpn_maxpool2d_indexed(const void *x, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride,
                          int32_t pad, void *y, void *index, void *stream) {
    int Hout, Wout;
    if (const int rc = mp_pool_check("cpn_maxpool2d_indexed", dtype, N, H, W, C, k, stride, pad, &Hout, &Wout)) return rc;
    if (!x || !y || !index) return cpn::fail(CPN_E_INVALID, "cpn_maxpool2d_indexed: null pointer");
    if (((uintptr_t) x | (uintptr_t) y | (uintptr_t) index) & 15)
        return cpn::fail(CPN_E_INVALID, "cpn_maxpool2d_indexed: x, y and index must start at 16-byte aligned addresses");
    const int G = dtype == CT_BF16 ? C / 8 : C / 4;
    const long total = (long) N * Hout * Wout * G;
    const dim3 grid((unsigned) ((total + 255) / 256));
    if (dtype == CT_BF16)
        hipLaunchKernelGGL((mp_pool_kernel<true>), grid, dim3(256), 0, (hipStream_t) stream, x, y, (unsigned char *) index, H, W, G, Hout,
                           Wout, k, stride, pad, total);
    else
        hipLaunchKernelGGL((mp_pool_kernel<false>), grid, dim3(256), 0, (hipStream_t) stream, x, y, (unsigned char *) index, H, W, G, Hout,
                           Wout, k, stride, pad, total);
    return cpn::check_hip(hipGetLastError(), "cpn_maxpool2d_indexed");
}

int cpn_maxpool2d_backward(const void *dy, const void *index, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k,
                           int32_t stride, int32_t pad, void *dx, void *stream) {
    int Hout, Wout;
    if (const int rc = mp_pool_check("cpn_maxpool2d_backward", dtype, N, H, W, C, k, stride, pad, &Hout, &Wout)) return rc;
    if (!dy || !index || !dx) return cpn::fail(CPN_E_INVALID, "cpn_maxpool2d_backward: null pointer");
    if (((uintptr_t) dy | (uintptr_t) index | (uintptr_t) dx) & 15)
        return cpn::fail(CPN_E_INVALID, "cpn_maxpool2d_backward: dy, index and dx must start at 16-byte aligned addresses");
    const int G = dtype == CT_BF16 ? C / 8 : C / 4;
    const long total = (long) N * H * W * G;
    const dim3 grid((unsigned) ((total + 255) / 256));
    if (dtype == CT_BF16)
        hipLaunchKernelGGL((mp_pool_backward_kernel<true>), grid, dim3(256), 0, (hipStream_t) stream, dy, (const unsigned char *) index, dx,
                           H, W, G, Hout, Wout, k, stride, pad, total);
    else
        hipLaunchKernelGGL((mp_pool_backward_kernel<false>), grid, dim3(256), 0, (hipStream_t) stream, dy, (const unsigned char *) index,
                           dx, H, W, G, Hout, Wout, k, stride, pad, total);
    return cpn::check_hip(hipGetLastError(), "cpn_maxpool2d_backward");
}

}  // extern "C"
