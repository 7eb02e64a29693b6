// Trainable concat convolution on the GPU (gfx950): the two backward pieces behind celldetection_amd.nn.cat_conv2d that
// csrc/conv_igemm.hip and csrc/conv_train.hip do not provide.  The rule is the "Trainable concat convolution" section of
// include/cpn_hip.h.  The conv's input is the VIRTUAL tensor cat(x0, resize(x1)): x0 [N][H][W][C0] and x1 [N][h][w][C1] read
// through the nearest map of csrc/nearest_adjoint.h; neither the resized nor the concatenated tensor exists in memory.
//
//   cc_wgrad_slab_kernel:  the weight gradient over the virtual concat.  Workgroup, fragments, LDS image, operand reads
//                          (ds_read_b64_tr_b16), MFMA (v_mfma_f32_32x32x16_bf16), rows of zeros instead of masks and the
//                          partition are those of ct_wgrad_slab_kernel (csrc/conv_train.hip); what differs is where a staged X row
//                          comes from.  A 32-channel block of the 64-channel tile belongs to ONE source (C0 % 32 == 0; the two
//                          blocks of a tile may belong to different ones).  A block of x0 is staged as it lies; a block of x1 is
//                          gathered: the source pixel of each of the CT_CH + K - 1 staged pixels is computed once per chunk into an
//                          LDS table (next to the column table), and every 16-byte item of the row looks its pixel up there.
//   ct_wgrad_reduce_kernel (csrc/wgrad_dense.h, the dense conv's): adds the slabs in ascending order and rounds once; writes
//                          dW [Cout][C0 + C1][k][k].
//   cc_nearest_sum_kernel:  the adjoint of the resize.  A lane owns 16 bytes (8 channels) of one source pixel, adds the pixels of
//                          its footprint in ascending row-major order in fp32 and rounds once; an empty footprint gives zeros.
// The bias gradient is that of csrc/wgrad_bias.h.  No floating-point atomics: results are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "nearest_adjoint.h"
#include "wgrad_bias.h"  // ct_bias_slab_kernel / ct_bias_reduce_kernel, ct_bf16_rne, the dtype codes
#include "wgrad_dense.h"  // ct_wgrad_reduce_kernel, ct_mt, ct_tiles_co, ct_slabs_wanted
#include "wgrad_slabs.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int CC_CH = 128;   // pixels per staged chunk (8 MFMA steps)
constexpr int CC_ROW = 64;   // bytes of an LDS row: 32 channels

// LDS image: dY [2 MT blocks][CC_CH rows], X [2 blocks][CC_CH + K - 1 rows], one row of zeros, the column of every chunk pixel
// (int32; a large negative number where no tap of this filter row applies), the x1 pixel of every staged X row (int32; negative
// outside the tensor).  Every offset is a multiple of 16.
template <int K, int MT>
struct CcLds {
    static constexpr int XR = CC_CH + K - 1;
    static constexpr int DY = 0, X = DY + 2 * MT * CC_CH * CC_ROW, ZERO = X + 2 * XR * CC_ROW, META = ZERO + CC_ROW,
                         SRC = META + CC_CH * 4, TOTAL = SRC + (XR * 4 + 15) / 16 * 16;
};
constexpr int CC_NO_TAP = -(1 << 24);

__device__ __forceinline__ s16x4 cc_read_tr(const char *smem, int byte_offset) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *) (smem + byte_offset));
}

struct CcSources {
    const uint16_t *x0, *x1;  // x0 may be null with C0 == 0 (the bridge level)
    int C0, C1, h1, w1;
    float sy, sx;             // na_scale(h1, H), na_scale(w1, W)
};

template <int K, int MT>
__global__ __launch_bounds__(256) void cc_wgrad_slab_kernel(const uint16_t *__restrict__ dy, CcSources src, float *__restrict__ ws,
                                                             WgSlabs part, int H, int Cout, long P, int tiles_ci) {
    typedef CcLds<K, MT> L;
    __shared__ __attribute__((aligned(16))) char smem[L::TOTAL];
    constexpr int PAD = K / 2, KK = K * K;
    const int tid = threadIdx.x, W = part.W, Cin = src.C0 + src.C1;
    const int slab = blockIdx.x, ky = blockIdx.z;
    const int co0 = (int) (blockIdx.y / tiles_ci) * 64 * MT, ci0 = (int) (blockIdx.y % tiles_ci) * 64;
    int64_t p0, p1;
    wgs_range(part, slab, &p0, &p1);

    const int wave = tid >> 6, lane = tid & 63;
    const int wco = wave >> 1, wci = wave & 1;
    const int half = lane >> 5, wq = (lane >> 2) & 3;
    const int cb = (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;  // byte offset of the lane's four channels in a row
    const int a_base = L::DY + wco * MT * CC_CH * CC_ROW + cb, b_base = L::X + wci * L::XR * CC_ROW + cb, z_addr = L::ZERO + cb;

    f32x16 acc[MT][K];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][kx][r] = 0.f;

    if (tid < CC_ROW / 16) *(u32x4 *) (smem + L::ZERO + tid * 16) = u32x4{0, 0, 0, 0};
    const long x_shift = (long) (ky - PAD) * W - PAD;  // flat pixel offset of X row 0 of a chunk from the chunk's first pixel

    for (int64_t c0 = p0; c0 < p1; c0 += CC_CH) {
        // ---- tables: the column of every chunk pixel, the x1 pixel of every staged X row (once per chunk, not per item)
        if (tid < CC_CH) {
            const int64_t p = c0 + tid;
            int m = CC_NO_TAP;
            if (p < p1) {  // (p <= 2^31 - 1: 32-bit division)
                const unsigned row = (unsigned) p / (unsigned) W;
                const int y = (int) (row % (unsigned) H) + ky - PAD;
                if (y >= 0 && y < H) m = (int) ((unsigned) p - row * (unsigned) W);
            }
            *(int *) (smem + L::META + tid * 4) = m;
        }
        if (tid < L::XR) {
            const int64_t f = c0 + tid + x_shift;
            int g = -1;
            if (f >= 0 && f < P) g = na_pixel_src((int32_t) f, H, W, src.h1, src.w1, src.sy, src.sx);
            *(int *) (smem + L::SRC + tid * 4) = g;
        }
        __syncthreads();
        // ---- stage (16 bytes = 8 channels per item; per pixel 2 MT blocks x 4 items of dY, 2 x 4 of X)
        for (int i = tid; i < CC_CH * 8 * MT; i += 256) {
            const int t = i / (8 * MT), blk = (i % (8 * MT)) >> 2, q = i & 3;
            const int64_t p = c0 + t;
            const int ch = co0 + blk * 32;
            u32x4 v = {0, 0, 0, 0};
            if (p < p1 && ch < Cout) v = *(const u32x4 *) (dy + p * Cout + ch + q * 8);
            *(u32x4 *) (smem + L::DY + (blk * CC_CH + t) * CC_ROW + q * 16) = v;
        }
        for (int i = tid; i < L::XR * 8; i += 256) {
            const int u = i >> 3, blk = (i >> 2) & 1, q = i & 3;
            const int g = *(const int *) (smem + L::SRC + u * 4);
            const int ch = ci0 + blk * 32;
            u32x4 v = {0, 0, 0, 0};
            if (g >= 0 && ch < Cin) {
                if (ch < src.C0) v = *(const u32x4 *) (src.x0 + (c0 + u + x_shift) * src.C0 + ch + q * 8);
                else v = *(const u32x4 *) (src.x1 + (int64_t) g * src.C1 + (ch - src.C0) + q * 8);
            }
            *(u32x4 *) (smem + L::X + (blk * L::XR + u) * CC_ROW + q * 16) = v;
        }
        __syncthreads();
        // ---- multiply: all 64 lanes of all four waves, whatever the tile's real extent (rows of zeros stand for the rest)
        const int64_t left = p1 - c0;
        const int steps = left >= CC_CH ? CC_CH / WGS_STEP : wgs_steps(left);
        for (int s = 0; s < steps; ++s) {
            const int t0 = WGS_STEP * s + 8 * half + wq, t1 = t0 + 4;
            bf16x8 A[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const s16x4 a0 = cc_read_tr(smem, a_base + (m * CC_CH + t0) * CC_ROW);
                const s16x4 a1 = cc_read_tr(smem, a_base + (m * CC_CH + t1) * CC_ROW);
                A[m] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
            }
            const int m0 = *(const int *) (smem + L::META + t0 * 4), m1 = *(const int *) (smem + L::META + t1 * 4);
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const bool ok0 = (unsigned) (m0 + kx - PAD) < (unsigned) W, ok1 = (unsigned) (m1 + kx - PAD) < (unsigned) W;
                const s16x4 b0 = cc_read_tr(smem, ok0 ? b_base + (t0 + kx) * CC_ROW : z_addr);
                const s16x4 b1 = cc_read_tr(smem, ok1 ? b_base + (t1 + kx) * CC_ROW : z_addr);
                const bf16x8 B = __builtin_bit_cast(bf16x8, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m][kx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[m], B, acc[m][kx], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // ---- partial sums: D[i = co][j = ci], lane -> j = lane % 32, register r -> i = 8 * (r / 4) + 4 * (lane / 32) + r % 4
    const int ci = ci0 + wci * 32 + (lane & 31);
    if (ci < Cin) {
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            float *out = ws + ((int64_t) slab * KK + ky * K + kx) * Cout * Cin;
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + (wco * MT + m) * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
                    if (co < Cout) out[(int64_t) co * Cin + ci] = acc[m][kx][r];
                }
        }
    }
}

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

// (The kernel per filter size and the slabs of the auto partition are those of the dense weight gradient on the C0 + C1 channels of
//  the virtual concat: ct_mt, ct_tiles_co and ct_slabs_wanted of csrc/wgrad_dense.h.)

// 0, or the error code with its message recorded; the partition of an accepted call
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
    const int64_t cin = (int64_t) c0 + c1;
    if ((int64_t) N * H * W > 0x7fffffffll || cin * cout * k * k > 0x7fffffffll || ((cout + 63) / 64) * ((cin + 63) / 64) > 65535) {
        snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 pixels or weights, or more than 65535 tiles of 64 x 64 channels", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    const WgSlabs s = wgs_partition((int64_t) N * H, W, slab_rows, ct_slabs_wanted((int) cin, cout, k));
    if (wgs_chain(s) > 0x7fffffffll || wgs_bias_chain(s) > 0x7fffffffll) {
        snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 steps in a chain (raise slab_rows)", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    if (part) *part = s;
    return 0;
}

template <int K>
void cc_launch_slabs(const WgSlabs &part, const void *dy, const CcSources &src, float *ws, int H, int cout, hipStream_t st) {
    const int tco = ct_tiles_co(cout, K), tci = (src.C0 + src.C1 + 63) / 64;
    hipLaunchKernelGGL((cc_wgrad_slab_kernel<K, ct_mt(K)>), dim3((unsigned) part.slabs, (unsigned) (tco * tci), (unsigned) K), dim3(256), 0,
                       st, (const uint16_t *) dy, src, ws, part, H, cout, (long) (part.rows * part.W), tci);
}

}  // namespace

extern "C" {

int64_t cpn_cat_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t c0, int32_t c1, int32_t h1, int32_t w1,
                                           int32_t cout, int32_t k, int32_t slab_rows) {
    WgSlabs part;
    if (cc_check("cpn_cat_conv_wgrad_workspace_bytes", N, H, W, c0, c1, h1, w1, cout, k, slab_rows, &part)) return 0;
    return (int64_t) part.slabs * ((int64_t) (c0 + c1) * cout * k * k + cout) * 4;
}

int cpn_cat_conv_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t c0, int32_t c1, int32_t h1, int32_t w1, int32_t cout, int32_t k,
                            int32_t slab_rows, int32_t info[5]) {
    WgSlabs part;
    if (const int rc = cc_check("cpn_cat_conv_wgrad_info", N, H, W, c0, c1, h1, w1, cout, k, slab_rows, &part)) return rc;
    if (!info) return cpn::fail(CPN_E_INVALID, "cpn_cat_conv_wgrad_info: null pointer");
    info[0] = part.slabs;
    info[1] = part.slab_rows;
    info[2] = part.steps;
    info[3] = part.slabs;  // the reduce chain: one add per slab
    info[4] = (int32_t) wgs_bias_chain(part);
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
    const int cin = c0 + c1;
    const int64_t per = (int64_t) cin * cout * k * k;
    if (workspace_bytes < (int64_t) part.slabs * (per + cout) * 4)
        return cpn::fail(CPN_E_WORKSPACE, "cpn_cat_conv_wgrad: workspace smaller than cpn_cat_conv_wgrad_workspace_bytes");
    hipStream_t st = (hipStream_t) stream;
    float *ws = (float *) workspace, *wsb = ws + (int64_t) part.slabs * per;
    if (dw) {
        const CcSources src{(const uint16_t *) x0, (const uint16_t *) x1, c0, c1, h1, w1, na_scale(h1, H), na_scale(w1, W)};
        switch (k) {
            case 1: cc_launch_slabs<1>(part, dy, src, ws, H, cout, st); break;
            case 3: cc_launch_slabs<3>(part, dy, src, ws, H, cout, st); break;
            case 5: cc_launch_slabs<5>(part, dy, src, ws, H, cout, st); break;
            default: cc_launch_slabs<7>(part, dy, src, ws, H, cout, st); break;
        }
        hipLaunchKernelGGL(ct_wgrad_reduce_kernel, dim3((unsigned) ((per + 255) / 256)), dim3(256), 0, st, ws, part.slabs, k * k, cout,
                           cin, dw, dw_dtype);
    }
    if (db) {
        hipLaunchKernelGGL(ct_bias_slab_kernel, dim3((unsigned) part.slabs, (unsigned) (cout / 32)), dim3(256), 0, st,
                           (const uint16_t *) dy, wsb, part, cout);
        hipLaunchKernelGGL(ct_bias_reduce_kernel, dim3((unsigned) ((cout + 255) / 256)), dim3(256), 0, st, wsb, part.slabs, cout, db,
                           db_dtype);
    }
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
