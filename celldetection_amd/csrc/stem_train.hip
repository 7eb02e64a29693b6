// Trainable ResNet stem and max-pool on the GPU (gfx950): what celldetection_amd.nn.stem_conv2d and nn.max_pool2d run.  The rule
// is the "Trainable stem and max-pool" section of include/cpn_hip.h.  The stem is Conv2d(C <= 4 -> 32 | 64, 7x7, stride 2, pad 3)
// on the padded 4-channel input bf16 [N][H + 6][W + 8][4] that cpn_convert_input_stem writes (csrc/stem.hip): the 32 values
// (kx 0..7, c 0..3) that output pixel (oy, ox) meets in filter row ky are the 64 contiguous bytes at Xp[n][2 oy + ky][2 ox].
//
//   st_pack_kernel:        weight [Cout][C][7][7] (fp32 | bf16) -> [7][Cout][32] bf16, zeros at kx = 7 and c >= C.
//   st_forward_kernel:     the MFMA loop of stem7_kernel (csrc/stem_mfma.h, one text for both): 14 v_mfma_f32_32x32x16_bf16 steps
//                          per 32-pixel fragment, operands straight from global memory, + bias, with this unit's epilogue: no
//                          ReLU, bf16 by ct_bf16_rne, 16-byte stores.
//   st_wgrad_slab_kernel:  dW_ky[Cout][32] = dY^T R_ky per filter row, the flat output pixel as the reduction index, 16 pixels per
//                          MFMA step.  A workgroup owns a slab of output rows (csrc/wgrad_slabs.h) and all seven filter rows: per
//                          chunk of 128 pixels the dY rows are staged in LDS once, wave w stages the 64-byte X rows of filter row
//                          w (then 4 + w) into its own region, and both operands are read with ds_read_b64_tr_b16.  Pixels behind
//                          the slab's end are staged as zeros in both operands (no masks, no uninitialised LDS).
//   st_wgrad_reduce_kernel: adds the slabs in ascending order, rounds once, writes the real 7 x C of the 32 columns only.
//   st_pool_kernel:        max-pool (3, 2, 1) | (2, 2, 0) with the tap index of the first maximum, 16 bytes per lane.
//   st_pool_backward_kernel: the gradient as a gather: a lane owns 16 bytes of one input pixel and visits the windows that cover
//                          it (csrc/pool_adjoint.h) in raster order.
// The bias gradient is that of csrc/wgrad_bias.h.  No floating-point atomics: results are bit-identical from run to run.  Inputs of
// the pool are finite: NaN is outside the contract (a NaN never takes a window over, so a window of NaNs alone yields -inf).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "mfma_frag.h"
#include "pool_adjoint.h"
#include "stem_mfma.h"
#include "wgrad_bias.h"  // ct_bias_slab_kernel / ct_bias_reduce_kernel, ct_bf16_rne, the dtype codes
#include "wgrad_slabs.h"

namespace {

typedef u32x4 __attribute__((aligned(8))) u32x4_a8;  // a row of the padded input starts at a multiple of 8 bytes (odd W)

constexpr int ST_PAD_ROWS = 6, ST_PAD_COLS = 8;  // STEM_PAD_ROWS / STEM_PAD_COLS of csrc/cpn_kernels.h
constexpr int ST_CH = 128;   // pixels per staged chunk (8 MFMA steps)
constexpr int ST_ROW = 64;   // bytes of an LDS row: 32 channels of dY, or the 32 values (kx, c) of one pixel and filter row
constexpr int ST_SLABS = 256;  // slabs of the auto partition: one workgroup per slab and CU (512 measured no faster: profiles/stem.txt)

// ---- weight pack ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void st_pack_kernel(const void *__restrict__ w, int w_dtype, int Cout, int C, uint16_t *__restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 7 * Cout * 32) return;
    const int v = e & 31, co = (e >> 5) % Cout, ky = (e >> 5) / Cout;
    const int kx = v >> 2, c = v & 3;
    uint16_t r = 0;
    if (kx < 7 && c < C) {
        const int si = ((co * C + c) * 7 + ky) * 7 + kx;
        r = w_dtype == CT_BF16 ? ((const uint16_t *) w)[si] : ct_bf16_rne(((const float *) w)[si]);
    }
    out[e] = r;
}

// ---- forward: stem_mfma_loop with an epilogue that has no activation -----------------------------------------------------------
__device__ __forceinline__ unsigned int st_pack2(float lo, float hi) {
    return (unsigned int) ct_bf16_rne(lo) | ((unsigned int) ct_bf16_rne(hi) << 16);
}

struct StBf16 {
    unsigned char *dst;
    size_t stride;  // bytes per output pixel
    __device__ __forceinline__ void operator()(const float (&v0)[4], const float (&v1)[4], int ch, size_t pixel, bool ok) const {
        stem_store_bf16(dst + pixel * stride + (size_t) ch * 2, ok, st_pack2(v0[0], v0[1]), st_pack2(v0[2], v0[3]), st_pack2(v1[0], v1[1]),
                        st_pack2(v1[2], v1[3]));
    }
};

template <int NF>
__global__ __launch_bounds__(256, 2) void st_forward_kernel(const unsigned char *__restrict__ xp, const unsigned char *__restrict__ wts,
                                                            const float *__restrict__ bias_p, unsigned char *__restrict__ dst, int N,
                                                            int H, int W, int Hout, int Wout) {
    const int wave = (int) ((blockIdx.x * (unsigned) blockDim.x + threadIdx.x) >> 6);
    const int nwaves = (int) ((gridDim.x * (unsigned) blockDim.x) >> 6);
    stem_mfma_loop<NF>(xp, wts, bias_p, N, H + ST_PAD_ROWS, W + ST_PAD_COLS, Hout, Wout, wave, nwaves, StBf16{dst, (size_t) NF * 32 * 2});
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
// LDS image: dY [NF blocks][ST_CH rows], X [4 waves][ST_CH rows]; rows of ST_ROW bytes, every offset a multiple of 16
template <int NF>
__global__ __launch_bounds__(256) void st_wgrad_slab_kernel(const uint16_t *__restrict__ dy, const unsigned char *__restrict__ xp,
                                                             float *__restrict__ ws, WgSlabs part, int Hout, int H, int W) {
    constexpr int DY = 0, X = NF * ST_CH * ST_ROW, TOTAL = X + 4 * ST_CH * ST_ROW, Cout = NF * 32;
    __shared__ __attribute__((aligned(16))) char smem[TOTAL];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int half = lane >> 5, wq = (lane >> 2) & 3;
    const int cb = mf_lane_bytes(lane);
    const int a_base = DY + cb, b_base = X + wave * ST_CH * ST_ROW + cb;
    const unsigned Wout = (unsigned) part.W;
    const int Wp = W + ST_PAD_COLS, Hp = H + ST_PAD_ROWS;
    const int slab = blockIdx.x;
    int64_t p0, p1;
    wgs_range(part, slab, &p0, &p1);

    f32x16 acc[2][NF];  // [pass]: wave w owns filter rows w and 4 + w (wave 3: row 3 alone)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int m = 0; m < NF; ++m) mf_zero(acc[g][m]);

    for (int64_t c0 = p0; c0 < p1; c0 += ST_CH) {
        // ---- stage dY: 16 bytes = 8 channels per item, 4 NF items per pixel; zeros behind the slab's end
        // (every load is issued before the first store: a pixel behind the end reads the slab's last pixel and is zeroed in registers)
        {
            constexpr int ITEMS = ST_CH * 4 * NF / 256;
            u32x4 v[ITEMS];
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                const int i = tid + 256 * j, t = i / (4 * NF), blk = (i % (4 * NF)) >> 2, q = i & 3;
                const int64_t p = c0 + t;
                v[j] = *(const u32x4 *) (dy + (p < p1 ? p : p1 - 1) * Cout + blk * 32 + q * 8);
                if (p >= p1) v[j] = u32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                const int i = tid + 256 * j, t = i / (4 * NF), blk = (i % (4 * NF)) >> 2, q = i & 3;
                *(u32x4 *) (smem + DY + (blk * ST_CH + t) * ST_ROW + q * 16) = v[j];
            }
        }
        const int64_t left = p1 - c0;
        const int steps = left >= ST_CH ? ST_CH / WGS_STEP : wgs_steps(left);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int ky = 4 * g + wave;  // (wave-uniform)
            // ---- stage X: the 64 bytes at Xp[n][2 oy + ky][2 ox] of every chunk pixel, 4 items per pixel; zeros behind the end
            if (ky < 7) {
                constexpr int ITEMS = ST_CH * 4 / 64;
                u32x4 v[ITEMS];
#pragma unroll
                for (int j = 0; j < ITEMS; ++j) {
                    const int i = lane + 64 * j, t = i >> 2, q = i & 3;
                    const int64_t p = c0 + t;
                    const unsigned pc = (unsigned) (p < p1 ? p : p1 - 1);  // (p <= 2^31 - 1: 32-bit division)
                    const unsigned row = pc / Wout, ox = pc - row * Wout;
                    const unsigned n = row / (unsigned) Hout, oy = row - n * (unsigned) Hout;
                    v[j] = *(const u32x4_a8 *) (xp + (((size_t) n * Hp + 2 * oy + ky) * Wp + 2 * ox) * 8 + q * 16);
                    if (p >= p1) v[j] = u32x4{0, 0, 0, 0};
                }
#pragma unroll
                for (int j = 0; j < ITEMS; ++j) {
                    const int i = lane + 64 * j, t = i >> 2, q = i & 3;
                    *(u32x4 *) (smem + X + (wave * ST_CH + t) * ST_ROW + q * 16) = v[j];
                }
            }
            __syncthreads();
            // ---- multiply: all 64 lanes, rows of zeros stand for the pixels behind the end
            if (ky < 7) {
                for (int s = 0; s < steps; ++s) {
                    const int t0 = WGS_STEP * s + 8 * half + wq, t1 = t0 + 4;
                    const bf16x8 B = mf_operand(smem, b_base + t0 * ST_ROW, b_base + t1 * ST_ROW);
#pragma unroll
                    for (int m = 0; m < NF; ++m) {
                        const bf16x8 A = mf_operand(smem, a_base + (m * ST_CH + t0) * ST_ROW, a_base + (m * ST_CH + t1) * ST_ROW);
                        acc[g][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, acc[g][m], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }
    }
    // ---- partial sums: D[i = co][j = (kx, c)], lane -> j = lane % 32, register r -> i = mf_row(r, lane / 32)
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int ky = 4 * g + wave;
        if (ky < 7) {
            float *out = ws + ((int64_t) slab * 7 + ky) * Cout * 32;
#pragma unroll
            for (int m = 0; m < NF; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) out[(m * 32 + mf_row(r, half)) * 32 + (lane & 31)] = acc[g][m][r];
        }
    }
}

// workspace [slab][7][Cout][32] -> dw [Cout][C][7][7]: the slabs in ascending order, one rounding; columns kx = 7 and c >= C unread
__global__ __launch_bounds__(256) void st_wgrad_reduce_kernel(const float *__restrict__ ws, int slabs, int Cout, int C, void *dw,
                                                               int dw_dtype) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Cout * C * 49) return;
    const int kx = e % 7, ky = (e / 7) % 7, c = (e / 49) % C, co = e / (49 * C);
    const long per = 7l * Cout * 32, at = ((long) ky * Cout + co) * 32 + kx * 4 + c;
    float sum = ws[at];
#pragma unroll 16
    for (int s = 1; s < slabs; ++s) sum += ws[s * per + at];  // (the loads of 16 slabs in flight, the adds in order)
    if (dw_dtype == CT_BF16) ((uint16_t *) dw)[e] = ct_bf16_rne(sum);
    else ((float *) dw)[e] = sum;
}

// ---- max-pool -------------------------------------------------------------------------------------------------------------
// A lane owns 16 bytes of one pixel: E = 8 bf16 or 4 fp32 channels.
template <bool BF16>
struct StLane {
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
__global__ __launch_bounds__(256) void st_pool_kernel(const void *__restrict__ x, void *__restrict__ y, unsigned char *__restrict__ index,
                                                      int H, int W, int G, int Hout, int Wout, int k, int s, int pad, long total) {
    constexpr int E = StLane<BF16>::E;
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
            StLane<BF16>::load(x, ((n * H + iy) * W + ix) * G + g, v);
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
__global__ __launch_bounds__(256) void st_pool_backward_kernel(const void *__restrict__ dy, const unsigned char *__restrict__ index,
                                                               void *__restrict__ dx, int H, int W, int G, int Hout, int Wout, int k,
                                                               int s, int pad, long total) {
    constexpr int E = StLane<BF16>::E;
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
            StLane<BF16>::load(dy, item, v);
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
int st_check(const char *who, int N, int H, int W, int cout, int slab_rows, WgSlabs *part) {
    static thread_local char msg[200];
    const char *bad = nullptr;
    if (N < 1 || H < 1 || W < 1) bad = "N, H and W must be at least 1";
    else if (cout != 32 && cout != 64) bad = "cout must be 32 or 64";
    else if (slab_rows < 0) bad = "slab_rows must be 0 (auto) or positive";
    if (bad) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return cpn::fail(CPN_E_INVALID, msg);
    }
    if ((int64_t) N * (H + ST_PAD_ROWS) > 0x7fffffffll || (int64_t) N * (H + ST_PAD_ROWS) * (W + ST_PAD_COLS) > 0x7fffffffll) {
        snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 pixels in the padded input", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    if (part) *part = wgs_partition((int64_t) N * ((H - 1) / 2 + 1), (W - 1) / 2 + 1, slab_rows, ST_SLABS);
    return 0;
}

int st_pool_check(const char *who, int dtype, int N, int H, int W, int C, int k, int s, int pad, int *Hout, int *Wout) {
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

int cpn_stem_train_pack(const void *weight, int32_t weight_dtype, int32_t cout, int32_t cin, void *packed, void *stream) {
    if (cout != 32 && cout != 64) return cpn::fail(CPN_E_INVALID, "cpn_stem_train_pack: cout must be 32 or 64");
    if (cin < 1 || cin > 4) return cpn::fail(CPN_E_INVALID, "cpn_stem_train_pack: cin must lie in 1 ... 4");
    if (weight_dtype != CT_F32 && weight_dtype != CT_BF16)
        return cpn::fail(CPN_E_INVALID, "cpn_stem_train_pack: weight_dtype must be 0 (fp32) or 1 (bf16)");
    if (!weight || !packed) return cpn::fail(CPN_E_INVALID, "cpn_stem_train_pack: null pointer");
    hipLaunchKernelGGL(st_pack_kernel, dim3((unsigned) ((7 * cout * 32 + 255) / 256)), dim3(256), 0, (hipStream_t) stream, weight,
                       weight_dtype, cout, cin, (uint16_t *) packed);
    return cpn::check_hip(hipGetLastError(), "cpn_stem_train_pack");
}

int cpn_stem_train_forward(const void *xp, const void *packed, const float *bias, int32_t N, int32_t H, int32_t W, int32_t cout,
                           void *y, void *stream) {
    if (const int rc = st_check("cpn_stem_train_forward", N, H, W, cout, 0, nullptr)) return rc;
    if (!xp || !packed || !y) return cpn::fail(CPN_E_INVALID, "cpn_stem_train_forward: null pointer");
    if (((uintptr_t) xp | (uintptr_t) packed | (uintptr_t) y) & 15)
        return cpn::fail(CPN_E_INVALID, "cpn_stem_train_forward: xp, packed and y must start at 16-byte aligned addresses");
    const int Hout = (H - 1) / 2 + 1, Wout = (W - 1) / 2 + 1;
    const long nfrag = (long) N * Hout * ((Wout + 31) / 32);
    long blocks = (nfrag + 3) / 4;           // 4 waves per block, one fragment per wave and pass
    if (blocks > 256 * 2) blocks = 256 * 2;  // persistent: two blocks per CU (the A-fragments are loaded once per wave)
    if (cout == 64)
        hipLaunchKernelGGL((st_forward_kernel<2>), dim3((unsigned) blocks), dim3(256), 0, (hipStream_t) stream, (const unsigned char *) xp,
                           (const unsigned char *) packed, bias, (unsigned char *) y, N, H, W, Hout, Wout);
    else
        hipLaunchKernelGGL((st_forward_kernel<1>), dim3((unsigned) blocks), dim3(256), 0, (hipStream_t) stream, (const unsigned char *) xp,
                           (const unsigned char *) packed, bias, (unsigned char *) y, N, H, W, Hout, Wout);
    return cpn::check_hip(hipGetLastError(), "cpn_stem_train_forward");
}

int64_t cpn_stem_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t cout, int32_t slab_rows) {
    WgSlabs part;
    if (st_check("cpn_stem_wgrad_workspace_bytes", N, H, W, cout, slab_rows, &part)) return 0;
    return (int64_t) part.slabs * (7 * cout * 32 + cout) * 4;
}

int cpn_stem_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t cout, int32_t slab_rows, int32_t info[5]) {
    WgSlabs part;
    if (const int rc = st_check("cpn_stem_wgrad_info", N, H, W, cout, slab_rows, &part)) return rc;
    if (!info) return cpn::fail(CPN_E_INVALID, "cpn_stem_wgrad_info: null pointer");
    wgs_info(part, info);
    return 0;
}

int cpn_stem_wgrad(const void *xp, const void *dy, int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t slab_rows,
                   void *dw, int32_t dw_dtype, void *db, int32_t db_dtype, void *workspace, int64_t workspace_bytes, void *stream) {
    WgSlabs part;
    if (const int rc = st_check("cpn_stem_wgrad", N, H, W, cout, slab_rows, &part)) return rc;
    if (cin < 1 || cin > 4) return cpn::fail(CPN_E_INVALID, "cpn_stem_wgrad: cin must lie in 1 ... 4");
    if (!xp || !dy || !workspace || (!dw && !db)) return cpn::fail(CPN_E_INVALID, "cpn_stem_wgrad: null pointer");
    if (((uintptr_t) xp | (uintptr_t) dy | (uintptr_t) workspace) & 15)
        return cpn::fail(CPN_E_INVALID, "cpn_stem_wgrad: xp, dy and workspace must start at 16-byte aligned addresses");
    if ((dw && dw_dtype != CT_F32 && dw_dtype != CT_BF16) || (db && db_dtype != CT_F32 && db_dtype != CT_BF16))
        return cpn::fail(CPN_E_INVALID, "cpn_stem_wgrad: an output dtype must be 0 (fp32) or 1 (bf16)");
    const int64_t per = 7ll * cout * 32;
    if (workspace_bytes < (int64_t) part.slabs * (per + cout) * 4)
        return cpn::fail(CPN_E_WORKSPACE, "cpn_stem_wgrad: workspace smaller than cpn_stem_wgrad_workspace_bytes");
    hipStream_t st = (hipStream_t) stream;
    float *ws = (float *) workspace, *wsb = ws + (int64_t) part.slabs * per;
    const int Hout = (H - 1) / 2 + 1;
    if (dw) {
        if (cout == 64)
            hipLaunchKernelGGL((st_wgrad_slab_kernel<2>), dim3((unsigned) part.slabs), dim3(256), 0, st, (const uint16_t *) dy,
                               (const unsigned char *) xp, ws, part, Hout, H, W);
        else
            hipLaunchKernelGGL((st_wgrad_slab_kernel<1>), dim3((unsigned) part.slabs), dim3(256), 0, st, (const uint16_t *) dy,
                               (const unsigned char *) xp, ws, part, Hout, H, W);
        hipLaunchKernelGGL(st_wgrad_reduce_kernel, dim3((unsigned) ((cout * cin * 49 + 255) / 256)), dim3(256), 0, st, ws, part.slabs, cout,
                           cin, dw, dw_dtype);
    }
    if (db) {
        hipLaunchKernelGGL(ct_bias_slab_kernel, dim3((unsigned) part.slabs, (unsigned) (cout / 32)), dim3(256), 0, st,
                           (const uint16_t *) dy, wsb, part, cout);
        hipLaunchKernelGGL(ct_bias_reduce_kernel, dim3((unsigned) ((cout + 255) / 256)), dim3(256), 0, st, wsb, part.slabs, cout, db,
                           db_dtype);
    }
    return cpn::check_hip(hipGetLastError(), "cpn_stem_wgrad");
}

int cpn_maxpool2d_indexed(const void *x, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride,
                          int32_t pad, void *y, void *index, void *stream) {
    int Hout, Wout;
    if (const int rc = st_pool_check("cpn_maxpool2d_indexed", dtype, N, H, W, C, k, stride, pad, &Hout, &Wout)) return rc;
    if (!x || !y || !index) return cpn::fail(CPN_E_INVALID, "cpn_maxpool2d_indexed: null pointer");
    if (((uintptr_t) x | (uintptr_t) y | (uintptr_t) index) & 15)
        return cpn::fail(CPN_E_INVALID, "cpn_maxpool2d_indexed: x, y and index must start at 16-byte aligned addresses");
    const int G = dtype == CT_BF16 ? C / 8 : C / 4;
    const long total = (long) N * Hout * Wout * G;
    const dim3 grid((unsigned) ((total + 255) / 256));
    if (dtype == CT_BF16)
        hipLaunchKernelGGL((st_pool_kernel<true>), grid, dim3(256), 0, (hipStream_t) stream, x, y, (unsigned char *) index, H, W, G, Hout,
                           Wout, k, stride, pad, total);
    else
        hipLaunchKernelGGL((st_pool_kernel<false>), grid, dim3(256), 0, (hipStream_t) stream, x, y, (unsigned char *) index, H, W, G, Hout,
                           Wout, k, stride, pad, total);
    return cpn::check_hip(hipGetLastError(), "cpn_maxpool2d_indexed");
}

int cpn_maxpool2d_backward(const void *dy, const void *index, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k,
                           int32_t stride, int32_t pad, void *dx, void *stream) {
    int Hout, Wout;
    if (const int rc = st_pool_check("cpn_maxpool2d_backward", dtype, N, H, W, C, k, stride, pad, &Hout, &Wout)) return rc;
    if (!dy || !index || !dx) return cpn::fail(CPN_E_INVALID, "cpn_maxpool2d_backward: null pointer");
    if (((uintptr_t) dy | (uintptr_t) index | (uintptr_t) dx) & 15)
        return cpn::fail(CPN_E_INVALID, "cpn_maxpool2d_backward: dy, index and dx must start at 16-byte aligned addresses");
    const int G = dtype == CT_BF16 ? C / 8 : C / 4;
    const long total = (long) N * H * W * G;
    const dim3 grid((unsigned) ((total + 255) / 256));
    if (dtype == CT_BF16)
        hipLaunchKernelGGL((st_pool_backward_kernel<true>), grid, dim3(256), 0, (hipStream_t) stream, dy, (const unsigned char *) index, dx,
                           H, W, G, Hout, Wout, k, stride, pad, total);
    else
        hipLaunchKernelGGL((st_pool_backward_kernel<false>), grid, dim3(256), 0, (hipStream_t) stream, dy, (const unsigned char *) index,
                           dx, H, W, G, Hout, Wout, k, stride, pad, total);
    return cpn::check_hip(hipGetLastError(), "cpn_maxpool2d_backward");
}

}  // extern "C"
