// Trainable bilinear resize on the GPU (gfx950): the backward pieces behind celldetection_amd.nn.bilinear_resize and
// nn.resized_conv2d that csrc/misc_kernels.hip, csrc/conv_igemm.hip and csrc/conv_train.hip do not provide.  The rule is the
// "Trainable bilinear resize" section of include/cpn_hip.h; the index arithmetic is csrc/bilinear_adjoint.h.  This unit is compiled
// with -ffp-contract=off: the blend and the sums have one stated order of operations.
//
//   bl_sum_kernel:         the adjoint of the resize on bf16 NHWC activations.  A lane owns 16 bytes (8 channels) of one source pixel,
//                          walks its footprint (rows x columns, ascending row-major) and adds ba_weight_y * ba_weight_x * t in
//                          fp32 -- the coefficient first, then one multiply and one add -- and rounds once.
//   bl_sum_planes_kernel:  the same adjoint on fp32 NCHW planes (the head maps): one lane per source pixel of one plane, fp32 out.
//   bl_wgrad_slab_kernel:  the weight gradient of a k x k stride-1 conv whose input is the VIRTUAL tensor resize(x).  Workgroup,
//                          fragments, LDS image, operand reads (ds_read_b64_tr_b16), MFMA (v_mfma_f32_32x32x16_bf16), rows of zeros
//                          instead of masks and the partition are those of cc_wgrad_slab_kernel (csrc/cat_conv_train.hip); what
//                          differs is the staging of an X row: once per 128-pixel chunk a per-row LDS table takes the four source
//                          pixels (negative outside the tensor) and the two lambdas of every staged pixel; every 16-byte item then
//                          loads its four source items, blends hy * (hx * a00 + lx * a01) + ly * (hx * a10 + lx * a11) in fp32,
//                          rounds to bf16 (RNE) and writes the LDS row.  Neither the resized tensor nor a workspace of its size
//                          exists.
//   ct_wgrad_reduce_kernel (csrc/wgrad_dense.h, the dense conv's): adds the slabs in ascending order and rounds once.
// The bias gradient is that of csrc/wgrad_bias.h.  No floating-point atomics, no scatter: results are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"
#include "bilinear_adjoint.h"
#include "cpn_error.h"
#include "wgrad_bias.h"  // ct_bias_slab_kernel / ct_bias_reduce_kernel, ct_bf16_rne, the dtype codes
#include "wgrad_dense.h"  // ct_wgrad_reduce_kernel, ct_mt, ct_tiles_co, ct_slabs_wanted
#include "wgrad_slabs.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int BL_CH = 128;   // pixels per staged chunk (8 MFMA steps)
constexpr int BL_ROW = 64;   // bytes of an LDS row: 32 channels
constexpr int BL_TAP = 32;   // bytes of a table entry: four source pixels (int32), lambda_y, lambda_x (fp32), 8 unused

// LDS image: dY [2 MT blocks][BL_CH rows], X [2 blocks][BL_CH + K - 1 rows], one row of zeros, the column of every chunk pixel
// (int32; a large negative number where no tap of this filter row applies), the taps of every staged X row.  Every offset is a
// multiple of 16.
template <int K, int MT>
struct BlLds {
    static constexpr int XR = BL_CH + K - 1;
    static constexpr int DY = 0, X = DY + 2 * MT * BL_CH * BL_ROW, ZERO = X + 2 * XR * BL_ROW, META = ZERO + BL_ROW,
                         TAP = META + BL_CH * 4, TOTAL = TAP + XR * BL_TAP;
};
constexpr int BL_NO_TAP = -(1 << 24);

__device__ __forceinline__ s16x4 bl_read_tr(const char *smem, int byte_offset) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *) (smem + byte_offset));
}

struct BlSource {
    const uint16_t *x;  // [N][h][w][C]
    int C, h, w;
    float sy, sx;       // ba_scale(h, H), ba_scale(w, W)
};

__device__ __forceinline__ float bl_lo(uint32_t v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float bl_hi(uint32_t v) { return __uint_as_float(v & 0xffff0000u); }

// hy * (hx * a00 + lx * a01) + ly * (hx * a10 + lx * a11): four products, two sums, two products, one sum
__device__ __forceinline__ float bl_blend(float a00, float a01, float a10, float a11, float hy, float ly, float hx, float lx) {
    return hy * (hx * a00 + lx * a01) + ly * (hx * a10 + lx * a11);
}

template <int K, int MT>
__global__ __launch_bounds__(256) void bl_wgrad_slab_kernel(const uint16_t *__restrict__ dy, BlSource src, float *__restrict__ ws,
                                                             WgSlabs part, int H, int Cout, long P, int tiles_ci) {
    typedef BlLds<K, MT> L;
    __shared__ __attribute__((aligned(16))) char smem[L::TOTAL];
    constexpr int PAD = K / 2, KK = K * K;
    const int tid = threadIdx.x, W = part.W, Cin = src.C;
    const int slab = blockIdx.x, ky = blockIdx.z;
    const int co0 = (int) (blockIdx.y / tiles_ci) * 64 * MT, ci0 = (int) (blockIdx.y % tiles_ci) * 64;
    int64_t p0, p1;
    wgs_range(part, slab, &p0, &p1);

    const int wave = tid >> 6, lane = tid & 63;
    const int wco = wave >> 1, wci = wave & 1;
    const int half = lane >> 5, wq = (lane >> 2) & 3;
    const int cb = (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;  // byte offset of the lane's four channels in a row
    const int a_base = L::DY + wco * MT * BL_CH * BL_ROW + cb, b_base = L::X + wci * L::XR * BL_ROW + cb, z_addr = L::ZERO + cb;

    f32x16 acc[MT][K];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][kx][r] = 0.f;

    if (tid < BL_ROW / 16) *(u32x4 *) (smem + L::ZERO + tid * 16) = u32x4{0, 0, 0, 0};
    const long x_shift = (long) (ky - PAD) * W - PAD;  // flat pixel offset of X row 0 of a chunk from the chunk's first pixel

    for (int64_t c0 = p0; c0 < p1; c0 += BL_CH) {
        // ---- tables: the column of every chunk pixel, the taps of every staged X row (once per chunk, not per item)
        if (tid < BL_CH) {
            const int64_t p = c0 + tid;
            int m = BL_NO_TAP;
            if (p < p1) {  // (p <= 2^31 - 1: 32-bit division)
                const unsigned row = (unsigned) p / (unsigned) W;
                const int y = (int) (row % (unsigned) H) + ky - PAD;
                if (y >= 0 && y < H) m = (int) ((unsigned) p - row * (unsigned) W);
            }
            *(int *) (smem + L::META + tid * 4) = m;
        }
        if (tid < L::XR) {
            const int64_t f = c0 + tid + x_shift;
            int g[4] = {-1, -1, -1, -1};
            float ly = 0.f, lx = 0.f;
            if (f >= 0 && f < P) {
                const unsigned row = (unsigned) f / (unsigned) W;
                const int x = (int) ((unsigned) f - row * (unsigned) W);
                const unsigned n = row / (unsigned) H;
                const int y = (int) (row - n * (unsigned) H);
                int y0, y1, x0, x1;
                ba_tap(y, src.sy, src.h, true, &y0, &y1, &ly);  // (fused: the conv loader's form of the coordinate)
                ba_tap(x, src.sx, src.w, true, &x0, &x1, &lx);
                y0 = min(y0, src.h - 1), y1 = min(y1, src.h - 1);  // (they are inside already for h <= H: a guard, not a rule)
                x0 = min(x0, src.w - 1), x1 = min(x1, src.w - 1);
                const int r0 = ((int) n * src.h + y0) * src.w, r1 = ((int) n * src.h + y1) * src.w;
                g[0] = r0 + x0, g[1] = r0 + x1, g[2] = r1 + x0, g[3] = r1 + x1;
            }
            *(u32x4 *) (smem + L::TAP + tid * BL_TAP) = u32x4{(unsigned) g[0], (unsigned) g[1], (unsigned) g[2], (unsigned) g[3]};
            *(float *) (smem + L::TAP + tid * BL_TAP + 16) = ly;
            *(float *) (smem + L::TAP + tid * BL_TAP + 20) = lx;
        }
        __syncthreads();
        // ---- stage (16 bytes = 8 channels per item; per pixel 2 MT blocks x 4 items of dY, 2 x 4 of X)
        for (int i = tid; i < BL_CH * 8 * MT; i += 256) {
            const int t = i / (8 * MT), blk = (i % (8 * MT)) >> 2, q = i & 3;
            const int64_t p = c0 + t;
            const int ch = co0 + blk * 32;
            u32x4 v = {0, 0, 0, 0};
            if (p < p1 && ch < Cout) v = *(const u32x4 *) (dy + p * Cout + ch + q * 8);
            *(u32x4 *) (smem + L::DY + (blk * BL_CH + t) * BL_ROW + q * 16) = v;
        }
        for (int i = tid; i < L::XR * 8; i += 256) {
            const int u = i >> 3, blk = (i >> 2) & 1, q = i & 3;
            const u32x4 g = *(const u32x4 *) (smem + L::TAP + u * BL_TAP);
            const int ch = ci0 + blk * 32;
            u32x4 v = {0, 0, 0, 0};
            if ((int) g[0] >= 0 && ch < Cin) {
                const float ly = *(const float *) (smem + L::TAP + u * BL_TAP + 16), lx = *(const float *) (smem + L::TAP + u * BL_TAP + 20);
                const float hy = 1.f - ly, hx = 1.f - lx;
                const uint16_t *base = src.x + ch + q * 8;
                const u32x4 a00 = *(const u32x4 *) (base + (int64_t) (int) g[0] * Cin), a01 = *(const u32x4 *) (base + (int64_t) (int) g[1] * Cin);
                const u32x4 a10 = *(const u32x4 *) (base + (int64_t) (int) g[2] * Cin), a11 = *(const u32x4 *) (base + (int64_t) (int) g[3] * Cin);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float lo = bl_blend(bl_lo(a00[e]), bl_lo(a01[e]), bl_lo(a10[e]), bl_lo(a11[e]), hy, ly, hx, lx);
                    const float hi = bl_blend(bl_hi(a00[e]), bl_hi(a01[e]), bl_hi(a10[e]), bl_hi(a11[e]), hy, ly, hx, lx);
                    v[e] = (uint32_t) ct_bf16_rne(lo) | ((uint32_t) ct_bf16_rne(hi) << 16);
                }
            }
            *(u32x4 *) (smem + L::X + (blk * L::XR + u) * BL_ROW + q * 16) = v;
        }
        __syncthreads();
        // ---- multiply: all 64 lanes of all four waves, whatever the tile's real extent (rows of zeros stand for the rest)
        const int64_t left = p1 - c0;
        const int steps = left >= BL_CH ? BL_CH / WGS_STEP : wgs_steps(left);
        for (int s = 0; s < steps; ++s) {
            const int t0 = WGS_STEP * s + 8 * half + wq, t1 = t0 + 4;
            bf16x8 A[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const s16x4 a0 = bl_read_tr(smem, a_base + (m * BL_CH + t0) * BL_ROW);
                const s16x4 a1 = bl_read_tr(smem, a_base + (m * BL_CH + t1) * BL_ROW);
                A[m] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
            }
            const int m0 = *(const int *) (smem + L::META + t0 * 4), m1 = *(const int *) (smem + L::META + t1 * 4);
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const bool ok0 = (unsigned) (m0 + kx - PAD) < (unsigned) W, ok1 = (unsigned) (m1 + kx - PAD) < (unsigned) W;
                const s16x4 b0 = bl_read_tr(smem, ok0 ? b_base + (t0 + kx) * BL_ROW : z_addr);
                const s16x4 b1 = bl_read_tr(smem, ok1 ? b_base + (t1 + kx) * BL_ROW : z_addr);
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
    if ((int64_t) N * H > 0x7fffffffll || (int64_t) N * H * W > 0x7fffffffll || (int64_t) cin * cout * k * k > 0x7fffffffll ||
        (int64_t) ((cout + 63) / 64) * ((cin + 63) / 64) > 65535) {
        snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 pixels or weights, or more than 65535 tiles of 64 x 64 channels", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    const WgSlabs s = wgs_partition((int64_t) N * H, W, slab_rows, ct_slabs_wanted(cin, cout, k));
    if (wgs_chain(s) > 0x7fffffffll || wgs_bias_chain(s) > 0x7fffffffll) {
        snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 steps in a chain (raise slab_rows)", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    if (part) *part = s;
    return 0;
}

template <int K>
void bl_launch_slabs(const WgSlabs &part, const void *dy, const BlSource &src, float *ws, int H, int cout, hipStream_t st) {
    const int tco = ct_tiles_co(cout, K), tci = (src.C + 63) / 64;
    hipLaunchKernelGGL((bl_wgrad_slab_kernel<K, ct_mt(K)>), dim3((unsigned) part.slabs, (unsigned) (tco * tci), (unsigned) K), dim3(256), 0,
                       st, (const uint16_t *) dy, src, ws, part, H, cout, (long) (part.rows * part.W), tci);
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
    return (int64_t) part.slabs * ((int64_t) cin * cout * k * k + cout) * 4;
}

int cpn_resized_conv_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t k,
                                int32_t slab_rows, int32_t info[5]) {
    WgSlabs part;
    if (const int rc = bl_check("cpn_resized_conv_wgrad_info", N, H, W, cin, h, w, cout, k, slab_rows, &part)) return rc;
    if (!info) return cpn::fail(CPN_E_INVALID, "cpn_resized_conv_wgrad_info: null pointer");
    info[0] = part.slabs;
    info[1] = part.slab_rows;
    info[2] = part.steps;
    info[3] = part.slabs;  // the reduce chain: one add per slab
    info[4] = (int32_t) wgs_bias_chain(part);
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
    const int64_t per = (int64_t) cin * cout * k * k;
    if (workspace_bytes < (int64_t) part.slabs * (per + cout) * 4)
        return cpn::fail(CPN_E_WORKSPACE, "cpn_resized_conv_wgrad: workspace smaller than cpn_resized_conv_wgrad_workspace_bytes");
    hipStream_t st = (hipStream_t) stream;
    float *ws = (float *) workspace, *wsb = ws + (int64_t) part.slabs * per;
    if (dw) {
        const BlSource src{(const uint16_t *) x, cin, h, w, ba_scale(h, H), ba_scale(w, W)};
        switch (k) {
            case 3: bl_launch_slabs<3>(part, dy, src, ws, H, cout, st); break;
            case 5: bl_launch_slabs<5>(part, dy, src, ws, H, cout, st); break;
            default: bl_launch_slabs<7>(part, dy, src, ws, H, cout, st); break;
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
