// The whole dense weight gradient, dW[co][ci][ky][kx] = sum over pixels p of dY[p][co] * X[p + (ky - pad) * W + (kx - pad)][ci] with
// zeros outside the image: the slab kernel, the kernel that adds the slabs' partial sums, the choice of fragments per wave and of
// slabs per filter size, and the host path around them (partition check, workspace size, launches).  Three units include it for
// all of that and differ only in their Source, the struct that says where a staged X row comes from: csrc/conv_train.hip (X as it
// lies, CtDense below), csrc/cat_conv_train.hip (the virtual concat of a lateral and a nearest-resized top), csrc/bilinear_train.hip
// (the virtual bilinear resize; compiled with -ffp-contract=off).  A fourth, csrc/grouped_conv_train.hip, includes it for the slab
// kernel alone, with CtDense and a Tiling of its own: the diagonal fragments of a grouped conv.  The partition is
// csrc/wgrad_slabs.h, the bias kernels are csrc/wgrad_bias.h, the fragment idiom is csrc/mfma_frag.h.  Device code with internal
// linkage: every unit that includes this header gets its own copy, compiled with that unit's flags.
//
//   ct_wgrad_slab_kernel:  one workgroup = (slab of the pixel range, tile of (co, ci) as the Tiling says, filter row ky); four
//                          waves, each FR fragments of 32 x 32 and k accumulators per fragment (one per kx).  The dense grid
//                          (CtGrid): a 64 MT x 64 tile, MT fragments per wave; MT = 2 for k <= 3, else 1.  The
//                          reduction index is the pixel, which is the ROW index of both operands as they lie in memory
//                          ([pixel][channel]).  Per chunk of CH pixels (dense: 128) it stages the dY rows and the X rows of the
//                          flat range [chunk + (ky - pad) * W - pad, ... + CH + k - 1) in LDS (32-channel rows of 64 B: the four
//                          pixel rows of a transposed read cover the 64 banks once), and reads both as operands of
//                          v_mfma_f32_32x32x16_bf16 with ds_read_b64_tr_b16: a lane supplies the address of ITS pixel row, so the
//                          staged X segment serves all k taps of the filter row (row index + kx), and a tap that falls outside the
//                          image (or a pixel behind the slab's end) points at a row of zeros instead: padded, never masked -- EXEC
//                          stays all ones, every address is 8-byte aligned.  Dense partial sums go to workspace[slab][tap][co][ci].
//   ct_wgrad_reduce_kernel: adds the slabs in ascending order (one fp32 chain per element) and rounds once to the output dtype.
// No floating-point atomics: results are bit-identical from run to run.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"  // the error codes
#include "cpn_error.h"
#include "mfma_frag.h"
#include "wgrad_bias.h"  // ct_launch_bias, ct_bf16_rne, the dtype codes
#include "wgrad_slabs.h"

namespace {

constexpr int CT_CH = 128;   // pixels per staged chunk of the dense grid (8 MFMA steps)
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

// X as it lies: [pixel][Cin]
struct CtDense {
    static constexpr int ENTRY = 0, KMIN = 1;
    const uint16_t *x;
    int C;
    __device__ __forceinline__ int channels() const { return C; }
    __device__ __forceinline__ u32x4 item(const char *, int64_t f, long P, int ch, int q) const {
        u32x4 v = {0, 0, 0, 0};
        if (f >= 0 && f < P && ch < C) v = *(const u32x4 *) (x + f * C + ch + q * 8);
        return v;
    }
};

// A Tiling is passed by value next to the Source and says which 32-channel blocks a workgroup stages and a wave multiplies:
//   static constexpr int CH, FR, DYB, XB                  pixels per chunk (a multiple of 16, at most 256); fragments per wave; the
//                                                         blocks of dY and of X the LDS image has room for
//   Tile tile(unsigned by, int wave, int lane) const      the place of blockIdx.y's workgroup and of one of its lanes:
//     int dy_blocks, x_blocks                               blocks it stages (<= DYB, XB), every one of them in full: zeros behind
//                                                           the channels
//     int dy0, x0                                           first channel of staged block 0 of dY and of X
//     int a_block, b_block                                  the wave multiplies the FR staged dY blocks from a_block by X block b_block
//     void store(float *ws, int slab, int ky, const f32x16 (&acc)[FR][K], int Cout, int Cin) const
//                                                           the wave's partial sums (D[i = co][j = ci]: lane -> j = lane % 32,
//                                                           register r -> i = mf_row(r, lane / 32)) into its unit's workspace
// The dense grid: blockIdx.y = (tile of 64 MT output channels, tile of 64 input channels), wave = (MT fragments of co, fragment
// of ci), partial sums to workspace[slab][tap][co][ci] where co and ci exist.
template <int MT>
struct CtGrid {
    static constexpr int CH = CT_CH, FR = MT, DYB = 2 * MT, XB = 2;
    int tiles_ci;
    struct Tile {
        static constexpr int dy_blocks = DYB, x_blocks = XB;
        int dy0, x0, a_block, b_block, half, col;
        template <int K>
        __device__ __forceinline__ void store(float *ws, int slab, int ky, const f32x16 (&acc)[MT][K], int Cout, int Cin) const {
            const int ci = x0 + b_block * 32 + col;
            if (ci < Cin) {
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    float *out = ws + ((int64_t) slab * K * K + ky * K + kx) * Cout * Cin;
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int co = dy0 + (a_block + m) * 32 + mf_row(r, half);
                            if (co < Cout) out[(int64_t) co * Cin + ci] = acc[m][kx][r];
                        }
                }
            }
        }
    };
    __device__ __forceinline__ Tile tile(unsigned by, int wave, int lane) const {
        const int co0 = (int) (by / tiles_ci) * 64 * MT, ci0 = (int) (by % tiles_ci) * 64;
        return Tile{co0, ci0, (wave >> 1) * MT, wave & 1, lane >> 5, lane & 31};
    }
};

// LDS image of the slab kernel: dY [DYB blocks][CH rows], X [XB blocks][CH + K - 1 rows], one row of zeros, the column of
// every chunk pixel (int32; a large negative number where no tap of this filter row applies), the Source's entry of every staged X
// row.  Every offset is a multiple of 16.
template <int K, class Tiling, int ENTRY>
struct CtLds {
    static constexpr int CH = Tiling::CH, XR = CH + K - 1;
    static constexpr int DY = 0, X = DY + Tiling::DYB * CH * CT_ROW, ZERO = X + Tiling::XB * XR * CT_ROW, META = ZERO + CT_ROW,
                         SRC = META + CH * 4, TOTAL = SRC + (XR * ENTRY + 15) / 16 * 16;
};

// (MT does nothing but pick the default Tiling, so that the dense family reads <K, MT, Source>; a unit with a Tiling of its own
// passes that Tiling's FR.)
template <int K, int MT, class Source, class Tiling = CtGrid<MT>>
__global__ __launch_bounds__(256) void ct_wgrad_slab_kernel(const uint16_t *__restrict__ dy, Source src, float *__restrict__ ws,
                                                             WgSlabs part, int H, int Cout, long P, Tiling tiling) {
    typedef CtLds<K, Tiling, Source::ENTRY> L;
    __shared__ __attribute__((aligned(16))) char smem[L::TOTAL];
    constexpr int PAD = K / 2, CH = Tiling::CH, FR = Tiling::FR;
    constexpr bool TABLE = Source::ENTRY > 0;
    static_assert(FR == MT && CH % WGS_STEP == 0 && CH <= 256, "one accumulator set per fragment; whole steps; a thread per chunk pixel");
    const int tid = threadIdx.x, W = part.W, Cin = src.channels();
    const int slab = blockIdx.x, ky = blockIdx.z;
    int64_t p0, p1;
    wgs_range(part, slab, &p0, &p1);

    const int wave = tid >> 6, lane = tid & 63;
    const auto tile = tiling.tile(blockIdx.y, wave, lane);
    const int half = lane >> 5, wq = (lane >> 2) & 3;
    const int cb = mf_lane_bytes(lane);
    const int a_base = L::DY + tile.a_block * CH * CT_ROW + cb, b_base = L::X + tile.b_block * L::XR * CT_ROW + cb, z_addr = L::ZERO + cb;

    f32x16 acc[FR][K];
#pragma unroll
    for (int m = 0; m < FR; ++m)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) mf_zero(acc[m][kx]);

    if (tid < CT_ROW / 16) *(u32x4 *) (smem + L::ZERO + tid * 16) = u32x4{0, 0, 0, 0};
    const long x_shift = (long) (ky - PAD) * W - PAD;  // flat pixel offset of X row 0 of a chunk from the chunk's first pixel

    for (int64_t c0 = p0; c0 < p1; c0 += CH) {
        const auto column_table = [&] {
            if (tid < CH) {
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
        // ---- stage (16 bytes = 8 channels per item; per pixel 4 items of every staged block of dY and of X)
        for (int i = tid; i < CH * 4 * tile.dy_blocks; i += 256) {
            const int t = i / (4 * tile.dy_blocks), blk = (i % (4 * tile.dy_blocks)) >> 2, q = i & 3;
            const int64_t p = c0 + t;
            const int ch = tile.dy0 + blk * 32;
            u32x4 v = {0, 0, 0, 0};
            if (p < p1 && ch < Cout) v = *(const u32x4 *) (dy + p * Cout + ch + q * 8);
            *(u32x4 *) (smem + L::DY + (blk * CH + t) * CT_ROW + q * 16) = v;
        }
        for (int i = tid; i < L::XR * 4 * tile.x_blocks; i += 256) {
            const int u = i / (4 * tile.x_blocks), blk = (i % (4 * tile.x_blocks)) >> 2, q = i & 3;
            const u32x4 v = src.item(smem + L::SRC + u * Source::ENTRY, c0 + u + x_shift, P, tile.x0 + blk * 32, q);
            *(u32x4 *) (smem + L::X + (blk * L::XR + u) * CT_ROW + q * 16) = v;
        }
        if constexpr (!TABLE) column_table();
        __syncthreads();
        // ---- multiply: all 64 lanes of all four waves, whatever the tile's real extent (rows of zeros stand for the rest)
        const int64_t left = p1 - c0;
        const int steps = left >= CH ? CH / WGS_STEP : wgs_steps(left);
        for (int s = 0; s < steps; ++s) {
            const int t0 = WGS_STEP * s + 8 * half + wq, t1 = t0 + 4;
            bf16x8 A[FR];
#pragma unroll
            for (int m = 0; m < FR; ++m) A[m] = mf_operand(smem, a_base + (m * CH + t0) * CT_ROW, a_base + (m * CH + t1) * CT_ROW);
            const int m0 = *(const int *) (smem + L::META + t0 * 4), m1 = *(const int *) (smem + L::META + t1 * 4);
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const bool ok0 = (unsigned) (m0 + kx - PAD) < (unsigned) W, ok1 = (unsigned) (m1 + kx - PAD) < (unsigned) W;
                const bf16x8 B = mf_operand(smem, ok0 ? b_base + (t0 + kx) * CT_ROW : z_addr, ok1 ? b_base + (t1 + kx) * CT_ROW : z_addr);
#pragma unroll
                for (int m = 0; m < FR; ++m) acc[m][kx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[m], B, acc[m][kx], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    tile.store(ws, slab, ky, acc, Cout, Cin);
}

// The chains of a partition of the weight gradient and of the bias gradient (the same one unless the conv is strided) fit 31 bits:
// 0, or the error code with its message recorded
int ct_check_chains(const char *who, const WgSlabs &part, const WgSlabs &bias_part) {
    static thread_local char msg[200];
    if (wgs_chain(part) > 0x7fffffffll || wgs_bias_chain(bias_part) > 0x7fffffffll) {
        snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 steps in a chain (raise slab_rows)", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    return 0;
}

// ---- The dense family alone: the reduce kernel, the choice of fragments and slabs per filter size and the host path.  A unit that
// wants the slab kernel with a Tiling of its own (csrc/grouped_conv_train.hip) defines WGRAD_SLAB_KERNEL_ONLY before it includes
// this header and gets none of it: no kernel it never launches in its code object.
#ifndef WGRAD_SLAB_KERNEL_ONLY

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
    if (const int rc = ct_check_chains(who, s, s)) return rc;
    if (part) *part = s;
    return 0;
}

// bytes of the workspace: per slab the partial sums of dW and of db, fp32
inline int64_t ct_workspace_bytes(int slabs, int64_t cin, int cout, int k) { return (int64_t) slabs * (cin * cout * k * k + cout) * 4; }

template <int K, class Source>
void ct_launch_slabs(const WgSlabs &part, const void *dy, const Source &src, float *ws, int H, int cin, int cout, hipStream_t st) {
    const int tco = ct_tiles_co(cout, K), tci = (cin + 63) / 64;
    hipLaunchKernelGGL((ct_wgrad_slab_kernel<K, ct_mt(K), Source>), dim3((unsigned) part.slabs, (unsigned) (tco * tci), (unsigned) K),
                       dim3(256), 0, st, (const uint16_t *) dy, src, ws, part, H, cout, (long) (part.rows * part.W),
                       CtGrid<ct_mt(K)>{tci});
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
    if (db) ct_launch_bias(part, dy, wsb, cout, db, db_dtype, st);
}

#endif  // WGRAD_SLAB_KERNEL_ONLY

}  // namespace
