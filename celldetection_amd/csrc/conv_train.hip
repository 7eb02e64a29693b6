// Trainable convolution on the GPU (gfx950): the kernels behind celldetection_amd.nn.conv2d that csrc/conv_igemm.hip does not
// already provide.  The rule is the "Trainable convolution" section of include/cpn_hip.h.
//
// Forward and input gradient are calls of cpn_conv2d; what they need per step is the weight tensor in that kernel's record layout:
//   ct_pack_kernel:        [Cout][Cin][k][k] fp32 | bf16 -> [item][out channel][32] bf16, forward (item = (chunk of Cin, tap)) or
//                          dgrad (item = (chunk of Cout, tap), tap flipped, channel roles swapped); one zero item behind an odd count.
// Weight gradient, dW[co][ci][ky][kx] = sum over pixels p of dY[p][co] * X[p + (ky - pad) * W + (kx - pad)][ci] with zeros outside
// the image.  The reduction index is the pixel, which is the ROW index of both operands as they lie in memory ([pixel][channel]):
//   ct_wgrad_slab_kernel:  one workgroup = (slab of the pixel range, 64 MT x 64 tile of (co, ci), filter row ky); four waves, each
//                          MT fragments of 32 x 32 and k accumulators per fragment (one per kx); MT = 2 for k <= 3, else 1.  Per chunk of 128 pixels it stages the dY rows and the X rows
//                          of the flat range [chunk + (ky - pad) * W - pad, ... + 128 + k - 1) in LDS as they lie (32-channel rows of
//                          64 B: the four pixel rows of a transposed read cover the 64 banks once), and reads both as operands of
//                          v_mfma_f32_32x32x16_bf16 with ds_read_b64_tr_b16: a lane supplies the address of ITS pixel row, so the
//                          staged X segment serves all k taps of the filter row (row index + kx), and a tap that falls outside the
//                          image (or a pixel behind the slab's end) points at a row of zeros instead: padded, never masked -- EXEC
//                          stays all ones, every address is 8-byte aligned.  Partial sums go to workspace[slab][tap][co][ci].
//   ct_wgrad_reduce_kernel: adds the slabs in ascending order (one fp32 chain per element) and rounds once to the output dtype.
//   ct_bias_slab_kernel / ct_bias_reduce_kernel: sum of dY per channel, eight interleaved chains per slab added in order, then the
//                          slabs in ascending order.
// No floating-point atomics: results are bit-identical from run to run.  The partition is csrc/wgrad_slabs.h.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "wgrad_bias.h"  // ct_bias_slab_kernel / ct_bias_reduce_kernel, ct_bf16_rne, the dtype codes
#include "wgrad_dense.h"  // ct_wgrad_reduce_kernel, ct_mt, ct_slabs_wanted
#include "wgrad_slabs.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int CT_CH = 128;   // pixels per staged chunk (8 MFMA steps)
constexpr int CT_ROW = 64;   // bytes of an LDS row: 32 channels

__global__ __launch_bounds__(256) void ct_pack_kernel(const void *w, int w_dtype, int Cout, int Cin, int K, int dgrad,
                                                       uint16_t *packed, long total) {
    const long o = (long) blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int CO = dgrad ? Cin : Cout, CR = dgrad ? Cout : Cin, KK = K * K;
    const int c = (int) (o & 31), oc = (int) ((o >> 5) % CO), item = (int) ((o >> 5) / CO);
    uint16_t v = 0;
    if (item < CR / 32 * KK) {  // (the item behind an odd count is zeros)
        const int rc = item / KK * 32 + c, tap = item % KK;
        int ky = tap / K, kx = tap % K;
        long idx;
        if (dgrad) {
            ky = K - 1 - ky;
            kx = K - 1 - kx;
            idx = (((long) rc * Cin + oc) * K + ky) * K + kx;
        } else {
            idx = (((long) oc * Cin + rc) * K + ky) * K + kx;
        }
        v = w_dtype == CT_BF16 ? ((const uint16_t *) w)[idx] : ct_bf16_rne(((const float *) w)[idx]);
    }
    packed[o] = v;
}

// LDS image of the slab kernel: dY [2 blocks][CT_CH rows], X [2 blocks][CT_CH + K - 1 rows], one row of zeros, the column of every
// chunk pixel (int32; a large negative number where no tap of this filter row applies).  Every offset is a multiple of 16.
template <int K, int MT>
struct CtLds {
    static constexpr int XR = CT_CH + K - 1;
    static constexpr int DY = 0, X = DY + 2 * MT * CT_CH * CT_ROW, ZERO = X + 2 * XR * CT_ROW, META = ZERO + CT_ROW,
                         TOTAL = META + CT_CH * 4;
};
constexpr int CT_NO_TAP = -(1 << 24);

__device__ __forceinline__ s16x4 ct_read_tr(const char *smem, int byte_offset) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *) (smem + byte_offset));
}

template <int K, int MT>
__global__ __launch_bounds__(256) void ct_wgrad_slab_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                             float *__restrict__ ws, WgSlabs part, int H, int Cin, int Cout,
                                                             long P, int tiles_ci) {
    typedef CtLds<K, MT> L;
    __shared__ __attribute__((aligned(16))) char smem[L::TOTAL];
    constexpr int PAD = K / 2, KK = K * K;
    const int tid = threadIdx.x, W = part.W;
    const int slab = blockIdx.x, ky = blockIdx.z;
    const int co0 = (int) (blockIdx.y / tiles_ci) * 64 * MT, ci0 = (int) (blockIdx.y % tiles_ci) * 64;
    int64_t p0, p1;
    wgs_range(part, slab, &p0, &p1);

    const int wave = tid >> 6, lane = tid & 63;
    const int wco = wave >> 1, wci = wave & 1;
    const int half = lane >> 5, wq = (lane >> 2) & 3;
    const int cb = (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;  // byte offset of the lane's four channels in a row
    const int a_base = L::DY + wco * MT * CT_CH * CT_ROW + cb, b_base = L::X + wci * L::XR * CT_ROW + cb, z_addr = L::ZERO + cb;

    f32x16 acc[MT][K];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][kx][r] = 0.f;

    if (tid < CT_ROW / 16) *(u32x4 *) (smem + L::ZERO + tid * 16) = u32x4{0, 0, 0, 0};
    const long x_shift = (long) (ky - PAD) * W - PAD;  // flat pixel offset of X row 0 of a chunk from the chunk's first pixel

    for (int64_t c0 = p0; c0 < p1; c0 += CT_CH) {
        // ---- stage (16 bytes = 8 channels per item; per pixel 2 MT blocks x 4 items of dY, 2 x 4 of X)
        for (int i = tid; i < CT_CH * 8 * MT; i += 256) {
            const int t = i / (8 * MT), blk = (i % (8 * MT)) >> 2, q = i & 3;
            const int64_t p = c0 + t;
            const int ch = co0 + blk * 32;
            u32x4 v = {0, 0, 0, 0};
            if (p < p1 && ch < Cout) v = *(const u32x4 *) (dy + p * Cout + ch + q * 8);
            *(u32x4 *) (smem + L::DY + (blk * CT_CH + t) * CT_ROW + q * 16) = v;
        }
        for (int i = tid; i < L::XR * 8; i += 256) {
            const int u = i >> 3, blk = (i >> 2) & 1, q = i & 3;
            const int64_t f = c0 + u + x_shift;
            const int ch = ci0 + blk * 32;
            u32x4 v = {0, 0, 0, 0};
            if (f >= 0 && f < P && ch < Cin) v = *(const u32x4 *) (x + f * Cin + ch + q * 8);
            *(u32x4 *) (smem + L::X + (blk * L::XR + u) * CT_ROW + q * 16) = v;
        }
        if (tid < CT_CH) {
            const int64_t p = c0 + tid;
            int m = CT_NO_TAP;
            if (p < p1) {  // (p <= 2^31 - 1: 32-bit division)
                const unsigned row = (unsigned) p / (unsigned) W;
                const int y = (int) (row % (unsigned) H) + ky - PAD;
                if (y >= 0 && y < H) m = (int) ((unsigned) p - row * (unsigned) W);
            }
            *(int *) (smem + L::META + tid * 4) = m;
        }
        __syncthreads();
        // ---- multiply: all 64 lanes of all four waves, whatever the tile's real extent (rows of zeros stand for the rest)
        const int64_t left = p1 - c0;
        const int steps = left >= CT_CH ? CT_CH / WGS_STEP : wgs_steps(left);
        for (int s = 0; s < steps; ++s) {
            const int t0 = WGS_STEP * s + 8 * half + wq, t1 = t0 + 4;
            bf16x8 A[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const s16x4 a0 = ct_read_tr(smem, a_base + (m * CT_CH + t0) * CT_ROW);
                const s16x4 a1 = ct_read_tr(smem, a_base + (m * CT_CH + t1) * CT_ROW);
                A[m] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
            }
            const int m0 = *(const int *) (smem + L::META + t0 * 4), m1 = *(const int *) (smem + L::META + t1 * 4);
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const bool ok0 = (unsigned) (m0 + kx - PAD) < (unsigned) W, ok1 = (unsigned) (m1 + kx - PAD) < (unsigned) W;
                const s16x4 b0 = ct_read_tr(smem, ok0 ? b_base + (t0 + kx) * CT_ROW : z_addr);
                const s16x4 b1 = ct_read_tr(smem, ok1 ? b_base + (t1 + kx) * CT_ROW : z_addr);
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

// (ct_wgrad_reduce_kernel, ct_mt and ct_slabs_wanted -- the kernel per filter size and the slabs of the auto partition -- are in
//  csrc/wgrad_dense.h, shared with csrc/cat_conv_train.hip)

// 0, or the error code with its message recorded; the partition of an accepted call
int ct_check(const char *who, int N, int H, int W, int cin, int cout, int k, int slab_rows, WgSlabs *part) {
    static thread_local char msg[160];
    const char *bad = nullptr;
    if (N < 1 || H < 1 || W < 1) bad = "N, H and W must be at least 1";
    else if (cin < 32 || cin % 32 || cout < 32 || cout % 32) bad = "cin and cout must be positive multiples of 32";
    else if (k != 1 && k != 3 && k != 5 && k != 7) bad = "k must be 1, 3, 5 or 7";
    else if (slab_rows < 0) bad = "slab_rows must be 0 (auto) or positive";
    if (bad) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return cpn::fail(CPN_E_INVALID, msg);
    }
    if ((int64_t) N * H * W > 0x7fffffffll || (int64_t) cin * cout * k * k > 0x7fffffffll ||
        (int64_t) ((cout + 63) / 64) * ((cin + 63) / 64) > 65535) {  // (an upper bound of the tile count of every kernel)
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
void ct_launch_slabs(const WgSlabs &part, const void *dy, const void *x, float *ws, int H, int cin, int cout, hipStream_t st) {
    const int tco = ct_tiles_co(cout, K), tci = (cin + 63) / 64;
    hipLaunchKernelGGL((ct_wgrad_slab_kernel<K, ct_mt(K)>), dim3((unsigned) part.slabs, (unsigned) (tco * tci), (unsigned) K), dim3(256), 0, st,
                       (const uint16_t *) dy, (const uint16_t *) x, ws, part, H, cin, cout, (long) (part.rows * part.W), tci);
}

}  // namespace

extern "C" {

int cpn_conv_train_pack(const void *w, int32_t w_dtype, int32_t cout, int32_t cin, int32_t k, int32_t mode, void *packed,
                        void *stream) {
    if (const int rc = ct_check("cpn_conv_train_pack", 1, 1, 1, cin, cout, k, 0, nullptr)) return rc;
    if (!w || !packed) return cpn::fail(CPN_E_INVALID, "cpn_conv_train_pack: null pointer");
    if (w_dtype != CT_F32 && w_dtype != CT_BF16) return cpn::fail(CPN_E_INVALID, "cpn_conv_train_pack: w_dtype must be 0 (fp32) or 1 (bf16)");
    if (mode != CPN_CONV_PACK_FORWARD && mode != CPN_CONV_PACK_DGRAD)
        return cpn::fail(CPN_E_INVALID, "cpn_conv_train_pack: mode must be CPN_CONV_PACK_FORWARD or CPN_CONV_PACK_DGRAD");
    const int reduced = mode == CPN_CONV_PACK_DGRAD ? cout : cin, outc = mode == CPN_CONV_PACK_DGRAD ? cin : cout;
    const long items = (long) reduced / 32 * k * k, total = (items + (items & 1)) * outc * 32;
    hipLaunchKernelGGL(ct_pack_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, (hipStream_t) stream, w, w_dtype, cout,
                       cin, k, mode == CPN_CONV_PACK_DGRAD ? 1 : 0, (uint16_t *) packed, total);
    return cpn::check_hip(hipGetLastError(), "cpn_conv_train_pack");
}

int64_t cpn_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t k, int32_t slab_rows) {
    WgSlabs part;
    if (ct_check("cpn_conv_wgrad_workspace_bytes", N, H, W, cin, cout, k, slab_rows, &part)) return 0;
    return (int64_t) part.slabs * ((int64_t) cin * cout * k * k + cout) * 4;
}

int cpn_conv_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t k, int32_t slab_rows, int32_t info[5]) {
    WgSlabs part;
    if (const int rc = ct_check("cpn_conv_wgrad_info", N, H, W, cin, cout, k, slab_rows, &part)) return rc;
    if (!info) return cpn::fail(CPN_E_INVALID, "cpn_conv_wgrad_info: null pointer");
    info[0] = part.slabs;
    info[1] = part.slab_rows;
    info[2] = part.steps;
    info[3] = part.slabs;  // the reduce chain: one add per slab
    info[4] = (int32_t) wgs_bias_chain(part);
    return 0;
}

int cpn_conv_wgrad(const void *x, const void *dy, int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t k,
                   int32_t slab_rows, void *dw, int32_t dw_dtype, void *db, int32_t db_dtype, void *workspace,
                   int64_t workspace_bytes, void *stream) {
    WgSlabs part;
    if (const int rc = ct_check("cpn_conv_wgrad", N, H, W, cin, cout, k, slab_rows, &part)) return rc;
    if (!x || !dy || !workspace || (!dw && !db)) return cpn::fail(CPN_E_INVALID, "cpn_conv_wgrad: null pointer");
    if ((dw && dw_dtype != CT_F32 && dw_dtype != CT_BF16) || (db && db_dtype != CT_F32 && db_dtype != CT_BF16))
        return cpn::fail(CPN_E_INVALID, "cpn_conv_wgrad: an output dtype must be 0 (fp32) or 1 (bf16)");
    const int64_t per = (int64_t) cin * cout * k * k;
    if (workspace_bytes < (int64_t) part.slabs * (per + cout) * 4)
        return cpn::fail(CPN_E_WORKSPACE, "cpn_conv_wgrad: workspace smaller than cpn_conv_wgrad_workspace_bytes");
    hipStream_t st = (hipStream_t) stream;
    float *ws = (float *) workspace, *wsb = ws + (int64_t) part.slabs * per;
    if (dw) {
        switch (k) {
            case 1: ct_launch_slabs<1>(part, dy, x, ws, H, cin, cout, st); break;
            case 3: ct_launch_slabs<3>(part, dy, x, ws, H, cin, cout, st); break;
            case 5: ct_launch_slabs<5>(part, dy, x, ws, H, cin, cout, st); break;
            default: ct_launch_slabs<7>(part, dy, x, ws, H, cin, cout, st); break;
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
    return cpn::check_hip(hipGetLastError(), "cpn_conv_wgrad");
}

}  // extern "C"
