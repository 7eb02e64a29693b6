// Trainable grouped 3x3 convolution on the GPU (gfx950): the kernels behind celldetection_amd.nn.grouped_conv2d that
// csrc/conv_igemm.hip does not already provide.  The rule is the "Trainable grouped convolution" section of include/cpn_hip.h; the
// index arithmetic is csrc/grouped_conv.h.
//
// Forward and input gradient are calls of cpn_conv2d on `bundles` block-diagonal dense convs of bw -> bw channels; per step they need
//   gc_pack_kernel:        [C][cig][3][3] fp32 | bf16 -> [bundle][item][bw][32] bf16, forward or dgrad (taps flipped, channel roles
//                          swapped inside the group); off-group entries and the padding item of every bundle are exact zeros.
//   gc_dilate_kernel:      stride 2: dZ [N][Hin][Win][C], dZ[2 i][2 j] = dY[i][j] and zero elsewhere, 16 bytes per lane; every unit
//                          of dZ is written exactly once (no separate clear).
//   gc_subsample_kernel:   the gather back, xs[i][j] = x[2 i][2 j], 16 bytes per lane: the operand of the strided 1x1 shortcut's
//                          weight gradient (cpn_subsample2d, "Trainable bottleneck block" of include/cpn_hip.h).
// Weight gradient, dW[co][cl][ky][kx] = sum over pixels p of dZ[p][co] * X[p + (ky - 1) * W + (kx - 1)][g(co) * cig + cl]:
//   gc_wgrad_slab_kernel:  the method of ct_wgrad_slab_kernel (csrc/wgrad_dense.h) on the diagonal fragments only.  One workgroup =
//                          (slab of the pixel range, span of four fragments, filter row ky); a wave owns ONE diagonal 32 x 32
//                          fragment and three accumulators of it (one per kx).  Per chunk of 64 pixels it stages the dZ rows of
//                          the span's 32-channel chunks and the X rows of the flat range
//                          [chunk + (ky - 1) * W - 1, ... + 64 + 2) in LDS as they lie (64-byte rows), and reads both as operands of
//                          v_mfma_f32_32x32x16_bf16 with ds_read_b64_tr_b16.  A tap outside the image, or a pixel behind the slab,
//                          points at a row of zeros: EXEC stays all ones, every address is 8-byte aligned.  Partial sums go to
//                          workspace[slab][tap][fragment][32 co][32 ci].
//   gc_wgrad_reduce_kernel: per dW element: the slabs in ascending order (one fp32 chain), rounded once.  It reads only the
//                          entries whose input and output channel share a group: the off-group products of a 32-wide bundle
//                          never reach dW.
//   bias gradient:         ct_bias_slab_kernel / ct_bias_reduce_kernel (csrc/wgrad_bias.h) on dY itself.
// No floating-point atomics: results are bit-identical from run to run.  The partition is csrc/wgrad_slabs.h.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "grouped_conv.h"
#include "wgrad_bias.h"
#include "wgrad_slabs.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int GC_ROW = 64;  // bytes of an LDS row: 32 channels
constexpr int GC_NO_TAP = -(1 << 24);

__global__ __launch_bounds__(256) void gc_pack_kernel(const void *w, int w_dtype, GcGeo geo, int dgrad, uint16_t *packed,
                                                       long total) {
    const long o = (long) blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int64_t idx = gc_pack_source(geo, o, dgrad);
    uint16_t v = 0;
    if (idx >= 0) v = w_dtype == CT_BF16 ? ((const uint16_t *) w)[idx] : ct_bf16_rne(((const float *) w)[idx]);
    packed[o] = v;
}

__global__ __launch_bounds__(256) void gc_dilate_kernel(const u32x4 *__restrict__ dy, u32x4 *__restrict__ dz, unsigned Hin,
                                                         unsigned Win, unsigned C8, unsigned total) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    const int64_t s = gc_dilate_source(u, Hin, Win, C8);
    u32x4 v = {0, 0, 0, 0};
    if (s >= 0) v = dy[s];
    dz[u] = v;
}

// xs [N][Hout][Wout][C], xs[i][j] = x[stride i][stride j]: every unit of xs written exactly once
__global__ __launch_bounds__(256) void gc_subsample_kernel(const u32x4 *__restrict__ x, u32x4 *__restrict__ xs, unsigned Hin,
                                                            unsigned Win, unsigned C8, unsigned stride, unsigned total) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    xs[u] = x[gc_subsample_source(u, Hin, Win, C8, stride)];
}

// LDS image of the slab kernel: dZ [4 blocks][CH rows], X [4 blocks][CH + 2 rows], one row of zeros, the column of every chunk
// pixel (int32; a large negative number where no tap of this filter row applies).  Every offset is a multiple of 16.
constexpr int GC_CH = 64;  // pixels per staged chunk (4 MFMA steps)
struct GcLds {
    static constexpr int XR = GC_CH + 2;
    static constexpr int DY = 0, X = DY + 4 * GC_CH * GC_ROW, ZERO = X + 4 * XR * GC_ROW, META = ZERO + GC_ROW, TOTAL = META + GC_CH * 4;
};

__device__ __forceinline__ s16x4 gc_read_tr(const char *smem, int byte_offset) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *) (smem + byte_offset));
}

__global__ __launch_bounds__(256) void gc_wgrad_slab_kernel(const uint16_t *__restrict__ dz, const uint16_t *__restrict__ x,
                                                             float *__restrict__ ws, WgSlabs part, GcGeo geo, int H, long P) {
    typedef GcLds L;
    constexpr int CH = GC_CH;
    __shared__ __attribute__((aligned(16))) char smem[L::TOTAL];
    const int tid = threadIdx.x, W = part.W, C = geo.C;
    const int slab = blockIdx.x, span = blockIdx.y, ky = blockIdx.z;
    const int NB = gc_span_chunks(geo), ch0 = gc_span_first_chunk(geo, span) * 32;
    int64_t p0, p1;
    wgs_range(part, slab, &p0, &p1);

    const int wave = tid >> 6, lane = tid & 63;
    const int frag = gc_wave_frag(geo, span, wave);  // (wave-uniform; -1: this wave multiplies rows of zeros and stores nothing)
    int co_chunk = 0, ci_chunk = 0;
    gc_frag_chunks(geo, frag < 0 ? 0 : frag, &co_chunk, &ci_chunk);
    const int a_blk = frag < 0 ? wave : co_chunk - ch0 / 32, b_blk = frag < 0 ? wave : ci_chunk - ch0 / 32;
    const int half = lane >> 5, wq = (lane >> 2) & 3;
    const int cb = (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;  // byte offset of the lane's four channels in a row
    const int a_base = L::DY + a_blk * CH * GC_ROW + cb, b_base = L::X + b_blk * L::XR * GC_ROW + cb, z_addr = L::ZERO + cb;

    f32x16 acc[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[kx][e] = 0.f;

    if (tid < GC_ROW / 16) *(u32x4 *) (smem + L::ZERO + tid * 16) = u32x4{0, 0, 0, 0};
    const long x_shift = (long) (ky - 1) * W - 1;  // flat pixel offset of X row 0 of a chunk from the chunk's first pixel

    for (int64_t c0 = p0; c0 < p1; c0 += CH) {
        // ---- stage (16 bytes = 8 channels per item; per pixel NB blocks x 4 items); blocks behind C hold zeros
        for (int i = tid; i < CH * 4 * NB; i += 256) {
            const int t = i / (4 * NB), blk = (i % (4 * NB)) >> 2, q = i & 3;
            const int64_t p = c0 + t;
            const int ch = ch0 + blk * 32;
            u32x4 v = {0, 0, 0, 0};
            if (p < p1 && ch < C) v = *(const u32x4 *) (dz + p * C + ch + q * 8);
            *(u32x4 *) (smem + L::DY + (blk * CH + t) * GC_ROW + q * 16) = v;
        }
        for (int i = tid; i < L::XR * 4 * NB; i += 256) {
            const int u = i / (4 * NB), blk = (i % (4 * NB)) >> 2, q = i & 3;
            const int64_t f = c0 + u + x_shift;
            const int ch = ch0 + blk * 32;
            u32x4 v = {0, 0, 0, 0};
            if (f >= 0 && f < P && ch < C) v = *(const u32x4 *) (x + f * C + ch + q * 8);
            *(u32x4 *) (smem + L::X + (blk * L::XR + u) * GC_ROW + q * 16) = v;
        }
        if (tid < CH) {
            const int64_t p = c0 + tid;
            int m = GC_NO_TAP;
            if (p < p1) {  // (p <= 2^31 - 1: 32-bit division)
                const unsigned row = (unsigned) p / (unsigned) W;
                const int y = (int) (row % (unsigned) H) + ky - 1;
                if (y >= 0 && y < H) m = (int) ((unsigned) p - row * (unsigned) W);
            }
            *(int *) (smem + L::META + tid * 4) = m;
        }
        __syncthreads();
        // ---- multiply: all 64 lanes of all four waves (rows of zeros stand for what does not exist)
        const int64_t left = p1 - c0;
        const int steps = left >= CH ? CH / WGS_STEP : wgs_steps(left);
        for (int s = 0; s < steps; ++s) {
            const int t0 = WGS_STEP * s + 8 * half + wq, t1 = t0 + 4;
            const s16x4 a0 = gc_read_tr(smem, a_base + t0 * GC_ROW);
            const s16x4 a1 = gc_read_tr(smem, a_base + t1 * GC_ROW);
            const bf16x8 A = __builtin_bit_cast(bf16x8, __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
            const int m0 = *(const int *) (smem + L::META + t0 * 4), m1 = *(const int *) (smem + L::META + t1 * 4);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const bool ok0 = (unsigned) (m0 + kx - 1) < (unsigned) W, ok1 = (unsigned) (m1 + kx - 1) < (unsigned) W;
                const s16x4 b0 = gc_read_tr(smem, ok0 ? b_base + (t0 + kx) * GC_ROW : z_addr);
                const s16x4 b1 = gc_read_tr(smem, ok1 ? b_base + (t1 + kx) * GC_ROW : z_addr);
                const bf16x8 B = __builtin_bit_cast(bf16x8, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
                acc[kx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, acc[kx], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // ---- partial sums: D[i = co][j = ci], lane -> j = lane % 32, register e -> i = 8 * (e / 4) + 4 * (lane / 32) + e % 4
    if (frag >= 0) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            float *out = ws + (((int64_t) slab * GCV_TAPS + ky * 3 + kx) * geo.frags + frag) * 1024 + (lane & 31);
#pragma unroll
            for (int e = 0; e < 16; ++e) out[(8 * (e >> 2) + 4 * half + (e & 3)) * 32] = acc[kx][e];
        }
    }
}

// workspace [slab][tap][fragment][32][32] -> dw [co][cl][tap]
__global__ __launch_bounds__(256) void gc_wgrad_reduce_kernel(const float *__restrict__ ws, int slabs, GcGeo geo, void *dw,
                                                               int dw_dtype) {
    const long total = (long) geo.C * geo.cig * GCV_TAPS;
    const long o = (long) blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int tap = (int) (o % GCV_TAPS), cl = (int) (o / GCV_TAPS % geo.cig), co = (int) (o / GCV_TAPS / geo.cig);
    int f, i, j;
    gc_locate(geo, co, cl, &f, &i, &j);
    const long per = (long) GCV_TAPS * geo.frags * 1024;
    const float *src = ws + ((long) tap * geo.frags + f) * 1024 + i * 32 + j;
    float sum = src[0];
    for (int s = 1; s < slabs; ++s) sum += src[s * per];
    if (dw_dtype == CT_BF16) ((uint16_t *) dw)[o] = ct_bf16_rne(sum);
    else ((float *) dw)[o] = sum;
}

// One workgroup per filter row (blockIdx.z), as in the dense kernel.  Keeping the accumulators of all nine taps in one workgroup, so
// that dZ is staged once, was measured and lost on every encoder shape by 1.6 to 1.9 x (profiles/grouped_conv.txt).  34 KB of LDS:
// four workgroups per CU, and the auto partition asks for as many slabs as fill the 256 CUs with them.
constexpr int GC_CUS = 256, GC_RESIDENT = 4;
int gc_slabs_wanted(const GcGeo &g) {
    const int per_slab = g.spans * 3;
    const int want = GC_CUS * GC_RESIDENT / per_slab;
    return want < 1 ? 1 : want;
}

struct GcCall {
    GcGeo geo;
    int Hout, Wout;
    WgSlabs part;   // of the weight gradient: the N * Hin image rows of x and dZ
    WgSlabs bpart;  // of the bias gradient: the N * Hout image rows of dY (stride 1: the same)
};

// 0, or the error code with its message recorded; the geometry and the partitions of an accepted call
int gc_check(const char *who, int N, int Hin, int Win, int C, int cig, int stride, int slab_rows, GcCall *call) {
    static thread_local char msg[200];
    const char *bad = nullptr;
    GcGeo geo;
    if (N < 1 || Hin < 1 || Win < 1) bad = "N, H and W must be at least 1";
    else if (!gc_geometry(C, cig, &geo)) bad = "channels per group must be 4, 8, 16, 32 or 64 and C a positive multiple of the bundle width (32; 64 for 64 per group)";
    else if (stride != 1 && stride != 2) bad = "stride must be 1 or 2";
    else if (slab_rows < 0) bad = "slab_rows must be 0 (auto) or positive";
    if (bad) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return cpn::fail(CPN_E_INVALID, msg);
    }
    // (activations: 2^31 bytes per tensor, the limit of cpn_conv2d's sources, which also keeps the dilation's unit index in 32 bits)
    if ((int64_t) N * Hin * Win > 0x7fffffffll || (int64_t) N * Hin * Win * C >= (1ll << 30) || C / 32 > 65535) {
        snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 pixels, 2^30 or more activation elements, or more than 65535 * 32 channels", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    GcCall c;
    c.geo = geo;
    c.Hout = gc_out_size(Hin, stride);
    c.Wout = gc_out_size(Win, stride);
    c.part = wgs_partition((int64_t) N * Hin, Win, slab_rows, gc_slabs_wanted(geo));
    c.bpart = wgs_partition((int64_t) N * c.Hout, c.Wout, slab_rows, gc_slabs_wanted(geo));
    if (wgs_chain(c.part) > 0x7fffffffll || wgs_bias_chain(c.bpart) > 0x7fffffffll) {
        snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 steps in a chain (raise slab_rows)", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    if (call) *call = c;
    return 0;
}

int64_t gc_ws_floats(const GcCall &c) {
    return (int64_t) c.part.slabs * GCV_TAPS * c.geo.frags * 1024 + (int64_t) c.bpart.slabs * c.geo.C;
}

}  // namespace

extern "C" {

int cpn_grouped_conv_pack(const void *w, int32_t w_dtype, int32_t C, int32_t cig, int32_t mode, void *packed, void *stream) {
    GcCall c;
    if (const int rc = gc_check("cpn_grouped_conv_pack", 1, 1, 1, C, cig, 1, 0, &c)) return rc;
    if (!w || !packed) return cpn::fail(CPN_E_INVALID, "cpn_grouped_conv_pack: null pointer");
    if (w_dtype != CT_F32 && w_dtype != CT_BF16) return cpn::fail(CPN_E_INVALID, "cpn_grouped_conv_pack: w_dtype must be 0 (fp32) or 1 (bf16)");
    if (mode != CPN_CONV_PACK_FORWARD && mode != CPN_CONV_PACK_DGRAD)
        return cpn::fail(CPN_E_INVALID, "cpn_grouped_conv_pack: mode must be CPN_CONV_PACK_FORWARD or CPN_CONV_PACK_DGRAD");
    const long total = (long) gc_packed_elements(c.geo);
    hipLaunchKernelGGL(gc_pack_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, (hipStream_t) stream, w, w_dtype, c.geo,
                       mode == CPN_CONV_PACK_DGRAD ? 1 : 0, (uint16_t *) packed, total);
    return cpn::check_hip(hipGetLastError(), "cpn_grouped_conv_pack");
}

int cpn_grouped_conv_dilate(const void *dy, int32_t N, int32_t Hin, int32_t Win, int32_t C, void *dz, void *stream) {
    GcCall c;
    if (const int rc = gc_check("cpn_grouped_conv_dilate", N, Hin, Win, C, 32, 2, 0, &c)) return rc;
    if (!dy || !dz) return cpn::fail(CPN_E_INVALID, "cpn_grouped_conv_dilate: null pointer");
    if (((uintptr_t) dy | (uintptr_t) dz) & 15) return cpn::fail(CPN_E_INVALID, "cpn_grouped_conv_dilate: dy and dz must be 16-byte aligned");
    const unsigned total = (unsigned) ((int64_t) N * Hin * Win * (C / 8));
    hipLaunchKernelGGL(gc_dilate_kernel, dim3((total + 255u) / 256u), dim3(256), 0, (hipStream_t) stream, (const u32x4 *) dy,
                       (u32x4 *) dz, (unsigned) Hin, (unsigned) Win, (unsigned) (C / 8), total);
    return cpn::check_hip(hipGetLastError(), "cpn_grouped_conv_dilate");
}

int cpn_subsample2d(const void *x, int32_t N, int32_t Hin, int32_t Win, int32_t C, int32_t stride, void *xs, void *stream) {
    if (N < 1 || Hin < 1 || Win < 1) return cpn::fail(CPN_E_INVALID, "cpn_subsample2d: N, H and W must be at least 1");
    if (C < 8 || C % 8) return cpn::fail(CPN_E_INVALID, "cpn_subsample2d: C must be a positive multiple of 8");
    if (stride != 2) return cpn::fail(CPN_E_INVALID, "cpn_subsample2d: stride must be 2");
    // (the limits of the dilation: x is a source of cpn_conv2d, and the unit index stays in 32 bits)
    if ((int64_t) N * Hin * Win > 0x7fffffffll || (int64_t) N * Hin * Win * C >= (1ll << 30))
        return cpn::fail(CPN_E_UNSUPPORTED, "cpn_subsample2d: more than 2^31 - 1 pixels or 2^30 or more activation elements");
    if (!x || !xs) return cpn::fail(CPN_E_INVALID, "cpn_subsample2d: null pointer");
    if (((uintptr_t) x | (uintptr_t) xs) & 15) return cpn::fail(CPN_E_INVALID, "cpn_subsample2d: x and xs must be 16-byte aligned");
    const unsigned total = (unsigned) ((int64_t) N * gc_out_size(Hin, stride) * gc_out_size(Win, stride) * (C / 8));
    hipLaunchKernelGGL(gc_subsample_kernel, dim3((total + 255u) / 256u), dim3(256), 0, (hipStream_t) stream, (const u32x4 *) x,
                       (u32x4 *) xs, (unsigned) Hin, (unsigned) Win, (unsigned) (C / 8), (unsigned) stride, total);
    return cpn::check_hip(hipGetLastError(), "cpn_subsample2d");
}

int64_t cpn_grouped_conv_wgrad_workspace_bytes(int32_t N, int32_t Hin, int32_t Win, int32_t C, int32_t cig, int32_t stride,
                                               int32_t slab_rows) {
    GcCall c;
    if (gc_check("cpn_grouped_conv_wgrad_workspace_bytes", N, Hin, Win, C, cig, stride, slab_rows, &c)) return 0;
    return gc_ws_floats(c) * 4;
}

int cpn_grouped_conv_wgrad_info(int32_t N, int32_t Hin, int32_t Win, int32_t C, int32_t cig, int32_t stride, int32_t slab_rows,
                                int32_t info[5]) {
    GcCall c;
    if (const int rc = gc_check("cpn_grouped_conv_wgrad_info", N, Hin, Win, C, cig, stride, slab_rows, &c)) return rc;
    if (!info) return cpn::fail(CPN_E_INVALID, "cpn_grouped_conv_wgrad_info: null pointer");
    info[0] = c.part.slabs;
    info[1] = c.part.slab_rows;
    info[2] = c.part.steps;
    info[3] = c.part.slabs;  // the reduce chain: one add per slab
    info[4] = (int32_t) wgs_bias_chain(c.bpart);
    return 0;
}

int cpn_grouped_conv_wgrad(const void *x, const void *dz, const void *dy, int32_t N, int32_t Hin, int32_t Win, int32_t C, int32_t cig,
                           int32_t stride, int32_t slab_rows, void *dw, int32_t dw_dtype, void *db, int32_t db_dtype, void *workspace,
                           int64_t workspace_bytes, void *stream) {
    GcCall c;
    if (const int rc = gc_check("cpn_grouped_conv_wgrad", N, Hin, Win, C, cig, stride, slab_rows, &c)) return rc;
    if (!workspace || (!dw && !db) || (dw && (!x || !dz)) || (db && !dy))
        return cpn::fail(CPN_E_INVALID, "cpn_grouped_conv_wgrad: null pointer");
    if ((dw && dw_dtype != CT_F32 && dw_dtype != CT_BF16) || (db && db_dtype != CT_F32 && db_dtype != CT_BF16))
        return cpn::fail(CPN_E_INVALID, "cpn_grouped_conv_wgrad: an output dtype must be 0 (fp32) or 1 (bf16)");
    if (dw && (((uintptr_t) x | (uintptr_t) dz) & 15))
        return cpn::fail(CPN_E_INVALID, "cpn_grouped_conv_wgrad: x and dz must be 16-byte aligned");
    if (workspace_bytes < gc_ws_floats(c) * 4)
        return cpn::fail(CPN_E_WORKSPACE, "cpn_grouped_conv_wgrad: workspace smaller than cpn_grouped_conv_wgrad_workspace_bytes");
    hipStream_t st = (hipStream_t) stream;
    float *ws = (float *) workspace, *wsb = ws + (int64_t) c.part.slabs * GCV_TAPS * c.geo.frags * 1024;
    if (dw) {
        hipLaunchKernelGGL(gc_wgrad_slab_kernel, dim3((unsigned) c.part.slabs, (unsigned) c.geo.spans, 3u), dim3(256), 0, st,
                           (const uint16_t *) dz, (const uint16_t *) x, ws, c.part, c.geo, Hin, (long) (c.part.rows * c.part.W));
        const long total = (long) C * cig * GCV_TAPS;
        hipLaunchKernelGGL(gc_wgrad_reduce_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, st, ws, c.part.slabs, c.geo, dw,
                           dw_dtype);
    }
    if (db) {
        hipLaunchKernelGGL(ct_bias_slab_kernel, dim3((unsigned) c.bpart.slabs, (unsigned) (C / 32)), dim3(256), 0, st,
                           (const uint16_t *) dy, wsb, c.bpart, C);
        hipLaunchKernelGGL(ct_bias_reduce_kernel, dim3((unsigned) ((C + 255) / 256)), dim3(256), 0, st, wsb, c.bpart.slabs, C, db,
                           db_dtype);
    }
    return cpn::check_hip(hipGetLastError(), "cpn_grouped_conv_wgrad");
}

}  // extern "C"
