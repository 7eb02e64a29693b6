// The whole dense weight gradient, dW[co][ci][ky][kx] = sum over pixels p of dY[p][co] * X[p + (ky - pad) * W + (kx - pad)][ci] with
// zeros outside the image: the slab kernel, the kernel that adds the slabs' partial sums, the choice of fragments per wave and of
// slabs per filter size, and the host path around them (partition check, workspace size, launches).  Three units include it and
// differ only in their Source, the struct that says where a staged X row comes from: csrc/conv_train.hip (X as it lies),
// csrc/cat_conv_train.hip (the virtual concat of a lateral and a nearest-resized top), csrc/bilinear_train.hip (the virtual bilinear
// resize; compiled with -ffp-contract=off).  The partition is csrc/wgrad_slabs.h, the bias kernels are csrc/wgrad_bias.h.  Device
// code with internal linkage: every unit that includes this header gets its own copy, compiled with that unit's flags.
//
//   ct_wgrad_slab_kernel:  one workgroup = (slab of the pixel range, 64 MT x 64 tile of (co, ci), filter row ky); four waves, each
//                          MT fragments of 32 x 32 and k accumulators per fragment (one per kx); MT = 2 for k <= 3, else 1.  The
//                          reduction index is the pixel, which is the ROW index of both operands as they lie in memory
//                          ([pixel][channel]).  Per chunk of 128 pixels it stages the dY rows and the X rows of the flat range
//                          [chunk + (ky - pad) * W - pad, ... + 128 + k - 1) in LDS (32-channel rows of 64 B: the four pixel rows
//                          of a transposed read cover the 64 banks once), and reads both as operands of v_mfma_f32_32x32x16_bf16
//                          with ds_read_b64_tr_b16: a lane supplies the address of ITS pixel row, so the staged X segment serves
//                          all k taps of the filter row (row index + kx), and a tap that falls outside the image (or a pixel behind
//                          the slab's end) points at a row of zeros instead: padded, never masked -- EXEC stays all ones, every
//                          address is 8-byte aligned.  Partial sums go to workspace[slab][tap][co][ci].
//   ct_wgrad_reduce_kernel: adds the slabs in ascending order (one fp32 chain per element) and rounds once to the output dtype.
// No floating-point atomics: results are bit-identical from run to run.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"  // the error codes
#include "cpn_error.h"
#include "wgrad_bias.h"  // ct_bias_slab_kernel / ct_bias_reduce_kernel, ct_bf16_rne, the dtype codes
#include "wgrad_slabs.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int CT_CH = 128;   // pixels per staged chunk (8 MFMA steps)
constexpr int CT_ROW = 64;   // bytes of an LDS row: 32 channels
constexpr int CT_NO_TAP = -(1 << 24);

// A Source is passed to the slab kernel by value and answers four questions:
//   int channels() const                                  the input channels Cin of the (virtual) X
//   static constexpr int ENTRY                            bytes of its LDS table entry per staged X row (0: no table)
//   void fill(char *entry, int64_t f, long P, int H, int W) const
//                                                         writes the entry of flat pixel f (once per chunk and row; ENTRY > 0 only)
//   u32x4 item(const char *entry, int64_t f, long P, int ch, int q) const
//                                                         the 16 bytes (channels ch + 8 q ... + 8) of flat pixel f; zeros unless
//                                                         0 <= f < P and ch < channels()
// and names the smallest filter size its unit accepts (KMIN: no kernel is built below it).  A Source with a table pays one more
// barrier per chunk (tables, barrier, stage, barrier); one without stages first and writes the column table behind it.

// LDS image of the slab kernel: dY [2 MT blocks][CT_CH rows], X [2 blocks][CT_CH + K - 1 rows], one row of zeros, the column of
// every chunk pixel (int32; a large negative number where no tap of this filter row applies), the Source's entry of every staged X
// row.  Every offset is a multiple of 16.
template <int K, int MT, int ENTRY>
struct CtLds {
    static constexpr int XR = CT_CH + K - 1;
    static constexpr int DY = 0, X = DY + 2 * MT * CT_CH * CT_ROW, ZERO = X + 2 * XR * CT_ROW, META = ZERO + CT_ROW,
                         SRC = META + CT_CH * 4, TOTAL = SRC + (XR * ENTRY + 15) / 16 * 16;
};

__device__ __forceinline__ s16x4 ct_read_tr(const char *smem, int byte_offset) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *) (smem + byte_offset));
}

template <int K, int MT, class Source>
__global__ __launch_bounds__(256) void ct_wgrad_slab_kernel(const uint16_t *__restrict__ dy, Source src, float *__restrict__ ws,
                                                             WgSlabs part, int H, int Cout, long P, int tiles_ci) {
    typedef CtLds<K, MT, Source::ENTRY> L;
    __shared__ __attribute__((aligned(16))) char smem[L::TOTAL];
    constexpr int PAD = K / 2, KK = K * K;
    constexpr bool TABLE = Source::ENTRY > 0;
    const int tid = threadIdx.x, W = part.W, Cin = src.channels();
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
        const auto column_table = [&] {
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
        };
        // ---- tables: the column of every chunk pixel, the Source's entry of every staged X row (once per chunk, not per item)
        if constexpr (TABLE) {
            column_table();
            if (tid < L::XR) src.fill(smem + L::SRC + tid * Source::ENTRY, c0 + tid + x_shift, P, H, W);
            __syncthreads();
        }
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
            const u32x4 v = src.item(smem + L::SRC + u * Source::ENTRY, c0 + u + x_shift, P, ci0 + blk * 32, q);
            *(u32x4 *) (smem + L::X + (blk * L::XR + u) * CT_ROW + q * 16) = v;
        }
        if constexpr (!TABLE) column_table();
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

// workspace [slab][tap][co][ci] -> dw [co][ci][tap]: the slabs in ascending order (one fp32 chain per element), one rounding
__global__ __launch_bounds__(256) void ct_wgrad_reduce_kernel(const float *__restrict__ ws, int slabs, int KK, int Cout, int Cin,
                                                               void *dw, int dw_dtype) {
    const long per = (long) KK * Cout * Cin;
    const long e = (long) blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    float sum = ws[e];
    for (int s = 1; s < slabs; ++s) sum += ws[s * per + e];
    const long cc = e % ((long) Cout * Cin);
    const long o = cc * KK + e / ((long) Cout * Cin);
    if (dw_dtype == CT_BF16) ((uint16_t *) dw)[o] = ct_bf16_rne(sum);
    else ((float *) dw)[o] = sum;
}

// The kernel per filter size: MT fragments of 32 output channels per wave (a workgroup: 64 MT output x 64 input channels), and the
// slabs of the auto partition, both as measured on an MI355X (profiles/conv_train.txt).  k <= 3: two fragments share every X
// operand read (half the LDS traffic per MFMA; 84 / 204 registers, 50 KB of LDS: 3 / 2 workgroups per CU) and the slabs fill the
// 256 CUs once.  k >= 5: one fragment (two would leave one workgroup per CU with nothing to overlap its staging: 13.5 ms instead
// of 9.8 ms on 7x7 256 -> 256 at 8 x 256^2) and about 1024 workgroups (11.8 ms with the 448 that fill the CUs once).
constexpr int CT_CUS = 256, CT_GROUPS = 1024;
constexpr int ct_mt(int k) { return k <= 3 ? 2 : 1; }
constexpr int ct_resident(int k) { return k == 3 ? 2 : 3; }
inline int ct_tiles_co(int cout, int k) { return (cout + 64 * ct_mt(k) - 1) / (64 * ct_mt(k)); }
inline int ct_slabs_wanted(int cin, int cout, int k) {
    const int per_slab = ct_tiles_co(cout, k) * ((cin + 63) / 64) * k;
    const int want = k <= 3 ? CT_CUS * ct_resident(k) / per_slab : (CT_GROUPS + per_slab - 1) / per_slab;
    return want < 1 ? 1 : want;
}

// ---- the host path: every unit checks its own arguments (each in its int range, cin and cout multiples of 32, k one of its
// filter sizes) and then calls these

// The size limits and the partition of an accepted call: 0, or the error code with its message recorded
int ct_check_partition(const char *who, int N, int H, int W, int64_t cin, int cout, int k, int slab_rows, WgSlabs *part) {
    static thread_local char msg[200];
    if ((int64_t) N * H * W > 0x7fffffffll || cin * cout * k * k > 0x7fffffffll ||
        (int64_t) ((cout + 63) / 64) * ((cin + 63) / 64) > 65535) {  // (an upper bound of the tile count of every kernel)
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

// bytes of the workspace: per slab the partial sums of dW and of db, fp32
inline int64_t ct_workspace_bytes(int slabs, int64_t cin, int cout, int k) { return (int64_t) slabs * (cin * cout * k * k + cout) * 4; }

template <int K, class Source>
void ct_launch_slabs(const WgSlabs &part, const void *dy, const Source &src, float *ws, int H, int cin, int cout, hipStream_t st) {
    const int tco = ct_tiles_co(cout, K), tci = (cin + 63) / 64;
    hipLaunchKernelGGL((ct_wgrad_slab_kernel<K, ct_mt(K), Source>), dim3((unsigned) part.slabs, (unsigned) (tco * tci), (unsigned) K),
                       dim3(256), 0, st, (const uint16_t *) dy, src, ws, part, H, cout, (long) (part.rows * part.W), tci);
}

// dW (slab kernel of the filter size, then the reduce) and db (bias slab, bias reduce), whichever is asked for, on one stream;
// workspace as ct_workspace_bytes lays it out
template <class Source>
void ct_launch_wgrad(const WgSlabs &part, const void *dy, const Source &src, int H, int cin, int cout, int k, void *dw, int dw_dtype,
                     void *db, int db_dtype, void *workspace, hipStream_t st) {
    const int64_t per = (int64_t) cin * cout * k * k;
    float *ws = (float *) workspace, *wsb = ws + (int64_t) part.slabs * per;
    if (dw) {
        switch (k) {
            case 1:
                if constexpr (Source::KMIN <= 1) ct_launch_slabs<1>(part, dy, src, ws, H, cin, cout, st);
                break;
            case 3: ct_launch_slabs<3>(part, dy, src, ws, H, cin, cout, st); break;
            case 5: ct_launch_slabs<5>(part, dy, src, ws, H, cin, cout, st); break;
            default: ct_launch_slabs<7>(part, dy, src, ws, H, cin, cout, st); break;
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
}

}  // namespace
