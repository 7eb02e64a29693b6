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
//   ct_wgrad_slab_kernel<3, 1, CtDense, GcSpans>: the slab kernel of csrc/wgrad_dense.h, its text unchanged, on the diagonal
//                          fragments only; what is the grouped conv's own is the Tiling GcSpans below.  One workgroup = (slab of the
//                          pixel range, span of four fragments, filter row ky); a wave owns ONE diagonal 32 x 32 fragment and three
//                          accumulators of it (one per kx); chunks of 64 pixels; x and dZ are staged as they lie (CtDense).
//                          Partial sums go to workspace[slab][tap][fragment][32 co][32 ci].
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
#define WGRAD_SLAB_KERNEL_ONLY  // the slab kernel, CtDense and ct_check_chains; not the dense reduce kernel and host path
#include "wgrad_dense.h"
#include "wgrad_slabs.h"

namespace {

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

// The Tiling of ct_wgrad_slab_kernel for the diagonal fragments (the contract is written in csrc/wgrad_dense.h): blockIdx.y = span.
// A workgroup stages the span's 32-channel chunks of dZ and of X (two or four; chunks behind C hold zeros), wave w multiplies the two
// chunks of fragment 4 span + w; a wave behind the last fragment multiplies chunk w by chunk w -- zeros, or a product nobody reads
// -- and stores nothing.  LDS: dZ [4 blocks][64 rows], X [4 blocks][66 rows], the zero row, the column table: 33600 bytes.
struct GcSpans {
    static constexpr int CH = 64, FR = 1, DYB = 4, XB = 4;
    GcGeo geo;
    struct Tile {
        int dy_blocks, x_blocks, dy0, x0, a_block, b_block, frag, frags, half, col;
        template <int K>
        __device__ __forceinline__ void store(float *ws, int slab, int ky, const f32x16 (&acc)[1][K], int, int) const {
            if (frag >= 0) {
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    float *out = ws + (((int64_t) slab * GCV_TAPS + ky * K + kx) * frags + frag) * 1024 + col;
#pragma unroll
                    for (int r = 0; r < 16; ++r) out[mf_row(r, half) * 32] = acc[0][kx][r];
                }
            }
        }
    };
    __device__ __forceinline__ Tile tile(unsigned span, int wave, int lane) const {
        const int nb = gc_span_chunks(geo), first = gc_span_first_chunk(geo, (int) span);
        const int frag = gc_wave_frag(geo, (int) span, wave);  // (wave-uniform)
        int co_chunk = 0, ci_chunk = 0;
        gc_frag_chunks(geo, frag < 0 ? 0 : frag, &co_chunk, &ci_chunk);
        return Tile{nb, nb, first * 32, first * 32, frag < 0 ? wave : co_chunk - first, frag < 0 ? wave : ci_chunk - first, frag,
                    geo.frags, lane >> 5, lane & 31};
    }
};

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
    if (const int rc = ct_check_chains(who, c.part, c.bpart)) return rc;
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
    wgs_info(c.part, c.bpart, info);
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
        hipLaunchKernelGGL((ct_wgrad_slab_kernel<3, 1, CtDense, GcSpans>), dim3((unsigned) c.part.slabs, (unsigned) c.geo.spans, 3u),
                           dim3(256), 0, st, (const uint16_t *) dz, CtDense{(const uint16_t *) x, C}, ws, c.part, Hin, C,
                           (long) (c.part.rows * c.part.W), GcSpans{c.geo});
        const long total = (long) C * cig * GCV_TAPS;
        hipLaunchKernelGGL(gc_wgrad_reduce_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, st, ws, c.part.slabs, c.geo, dw,
                           dw_dtype);
    }
    if (db) ct_launch_bias(c.bpart, dy, wsb, C, db, db_dtype, st);
    return cpn::check_hip(hipGetLastError(), "cpn_grouped_conv_wgrad");
}

}  // extern "C"
