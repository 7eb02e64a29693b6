// Trainable image conv on the GPU (gfx950): what celldetection_amd.nn.image_conv2d runs, the first conv of the U-Net encoders,
// Conv2d(C <= 4 -> 32 | 64 | 128, 3x3, stride 1, padding 1) on the image itself.  The rule is the "Trainable image conv" section of
// include/cpn_hip.h.  The image becomes the padded 4-channel tensor Xq, bf16 [N][H + 2][W + 3][4], in which the 16 values
// (kx 0..3, c 0..3) that output pixel (y, x) meets in filter row ky are the 32 contiguous bytes at Xq[n][y + ky][x].
//
//   ic_pad_kernel:          fp32 NCHW -> Xq: zero border (one row and one column in front), zeros in the channels >= C.
//   ic_pack_kernel:         weight [Cout][C][3][3] (fp32 | bf16) -> [3][Cout][16] bf16, zeros at kx = 3 and c >= C.
//   ic_forward_kernel:      one v_mfma_f32_32x32x16_bf16 step per filter row and 32-channel block on a fragment of 32 pixels of an
//                           image row, operands straight from global memory (the next fragment's are loaded before this one's
//                           products), + bias, bf16 by ct_bf16_rne, 16-byte stores (the swap-and-store of csrc/stem_mfma.h).
//   ic_wgrad_slab_kernel:   dW_ky[Cout][16] = dY^T R_ky per filter row, the flat output pixel as the reduction index, 16 pixels per
//                           MFMA step.  A workgroup owns a slab of image rows (csrc/wgrad_slabs.h) and all three filter rows.  Per
//                           chunk of 128 pixels the dY rows are staged in LDS once for all three filter rows, next to two images
//                           of the pixels' Xq values: image 0 holds the 32 bytes of filter row 0 and of filter row 1 side by side
//                           in a 64-byte row, image 1 those of filter row 2 and 32 bytes of zeros.  Wave w owns image w % 2 and
//                           the 32-channel blocks w / 2, w / 2 + 2 of dY from the slab's first pixel to its last; both operands
//                           are read with ds_read_b64_tr_b16.  The next chunk's global loads are issued before this chunk's
//                           products.  Pixels behind the slab's end are staged as zeros in both operands.
//   ic_wgrad_reduce_kernel: adds the slabs in ascending order, rounds once, writes the real 3 x C of the 16 columns only.
// The bias gradient is that of csrc/wgrad_bias.h.  No floating-point atomics: results are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "mfma_frag.h"
#include "stem_mfma.h"   // stem_store_bf16, u32x2, bf16x8_a8
#include "wgrad_bias.h"  // ct_bias_slab_kernel / ct_bias_reduce_kernel, ct_bf16_rne, the dtype codes
#include "wgrad_slabs.h"

namespace {

typedef u32x4 __attribute__((aligned(8))) u32x4_a8;  // a pixel of the padded input starts at a multiple of 8 bytes

constexpr int IC_PAD_ROWS = 2, IC_PAD_COLS = 3;  // Xq is [N][H + 2][W + 3][4]
constexpr int IC_CH = 128;     // pixels per staged chunk (8 MFMA steps)
constexpr int IC_ROW = 64;     // bytes of an LDS row: 32 channels of dY, or the 2 x 16 values (kx, c) of one pixel and two filter rows
constexpr int IC_SLABS = 512;  // slabs of the auto partition: two workgroups per CU, each busy while the other one stages

// ---- input pad ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ic_pad_kernel(const float *__restrict__ src, unsigned char *__restrict__ dst, int N, int C, int H,
                                                     int W) {
    const int Hq = H + IC_PAD_ROWS, Wq = W + IC_PAD_COLS;
    const long total = (long) N * Hq * Wq, HW = (long) H * W;
    for (long i = blockIdx.x * 256l + threadIdx.x; i < total; i += (long) gridDim.x * 256) {
        const int xq = (int) (i % Wq);
        const long r = i / Wq;
        const int yq = (int) (r % Hq);
        const long n = r / Hq;
        const int y = yq - 1, x = xq - 1;
        uint16_t v[4] = {0, 0, 0, 0};
        if (y >= 0 && y < H && x >= 0 && x < W) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) v[c] = ct_bf16_rne(src[(n * C + c) * HW + (long) y * W + x]);
        }
        u32x2 o;
        o.x = (unsigned) v[0] | ((unsigned) v[1] << 16);
        o.y = (unsigned) v[2] | ((unsigned) v[3] << 16);
        *(u32x2 *) (dst + i * 8) = o;
    }
}

// ---- weight pack ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ic_pack_kernel(const void *__restrict__ w, int w_dtype, int Cout, int C, uint16_t *__restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * Cout * 16) return;
    const int v = e & 15, co = (e >> 4) % Cout, ky = (e >> 4) / Cout;
    const int kx = v >> 2, c = v & 3;
    uint16_t r = 0;
    if (kx < 3 && c < C) {
        const int si = ((co * C + c) * 3 + ky) * 3 + kx;
        r = w_dtype == CT_BF16 ? ((const uint16_t *) w)[si] : ct_bf16_rne(((const float *) w)[si]);
    }
    out[e] = r;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int ic_pack2(float lo, float hi) {
    return (unsigned int) ct_bf16_rne(lo) | ((unsigned int) ct_bf16_rne(hi) << 16);
}

// the lane's 8 K-values of the three filter rows of fragment f: 16 contiguous bytes of Xq each (lanes past the row's end read its
// last pixel and store nothing)
__device__ __forceinline__ void ic_load_fragment(const unsigned char *__restrict__ xq, long f, int fx, int H, int W, int l31, int lhi,
                                                 bf16x8 (&bx)[3]) {
    const int Hq = H + IC_PAD_ROWS, Wq = W + IC_PAD_COLS;
    const int tx = (int) (f % fx);
    const long r = f / fx;
    const int y = (int) (r % H);
    const long n = r / H;
    const int x = tx * 32 + l31;
    const int xc = x < W ? x : W - 1;
    const unsigned char *p = xq + (((size_t) n * Hq + y) * Wq + xc) * 8 + lhi * 16;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) bx[ky] = *(const bf16x8_a8 *) (p + (size_t) ky * Wq * 8);
}

// NF = 32-channel output fragments (1 | 2 | 4); weights [3][NF * 32][16] bf16.  One wave = one 32-pixel row fragment at a time
// (persistent waves, grid-stride); the A fragments stay in registers.
template <int NF>
__global__ __launch_bounds__(256) void ic_forward_kernel(const unsigned char *__restrict__ xq, const unsigned char *__restrict__ wts,
                                                         const float *__restrict__ bias_p, unsigned char *__restrict__ dst, int N, int H,
                                                         int W) {
    constexpr int Cout = NF * 32;
    const int wave = (int) ((blockIdx.x * 256u + threadIdx.x) >> 6);
    const int nwaves = (int) ((gridDim.x * 256u) >> 6);
    const int lane = threadIdx.x & 63;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int fx = (W + 31) >> 5;  // fragments per image row
    const long nfrag = (long) N * H * fx;

    // A-fragments: lane -> output channel j * 32 + l31, K-octet lhi of filter row ky
    bf16x8 wf[NF][3];
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) wf[j][ky] = *(const bf16x8 *) (wts + ((size_t) (ky * Cout + j * 32 + l31) * 16 + lhi * 8) * 2);
    float bias[NF][4][4];
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) bias[j][q][e] = bias_p ? bias_p[j * 32 + mf_row(4 * q + e, lhi)] : 0.f;

    bf16x8 bx[3], nx[3];
    if (wave < nfrag) ic_load_fragment(xq, wave, fx, H, W, l31, lhi, bx);
    for (long f = wave; f < nfrag; f += nwaves) {
        const bool more = f + nwaves < nfrag;  // (wave-uniform)
        if (more) ic_load_fragment(xq, f + nwaves, fx, H, W, l31, lhi, nx);
        f32x16 acc[NF];
#pragma unroll
        for (int j = 0; j < NF; ++j) mf_zero(acc[j]);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int j = 0; j < NF; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[j][ky], bx[ky], acc[j], 0, 0, 0);
        const int x = (int) (f % fx) * 32 + l31;
        const size_t pixel = (size_t) (f / fx) * W + x;  // (f / fx = n * H + y)
        unsigned char *at = dst + pixel * (Cout * 2);
#pragma unroll
        for (int j = 0; j < NF; ++j)
#pragma unroll
            for (int qp = 0; qp < 2; ++qp) {
                const int q0 = 2 * qp, q1 = q0 + 1;
                float v0[4], v1[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v0[e] = acc[j][q0 * 4 + e] + bias[j][q0][e];
                    v1[e] = acc[j][q1 * 4 + e] + bias[j][q1][e];
                }
                // the lane halves swap the quads they do not keep: the lane owns channels j * 32 + 8 (2 qp + lhi) ... + 7
                stem_store_bf16(at + (j * 32 + 8 * (lhi ? q1 : q0)) * 2, x < W, ic_pack2(v0[0], v0[1]), ic_pack2(v0[2], v0[3]),
                                ic_pack2(v1[0], v1[1]), ic_pack2(v1[2], v1[3]));
            }
        if (more) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) bx[ky] = nx[ky];
        }
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
// LDS image: dY [NF blocks][IC_CH rows], X [2 images][IC_CH rows]; rows of IC_ROW bytes, every offset a multiple of 16.
// Wave w owns X image g = w % 2 and the dY blocks m = w / 2 + 2 k (k < KI) that exist.
template <int NF>
struct IcStage {
    static constexpr int DY_ITEMS = IC_CH * 4 * NF / 256;  // 16 bytes = 8 channels per item, 4 NF items per pixel
    u32x4 dy[DY_ITEMS];
    u32x4 x[3];  // item tid of filter row ky: pixel tid / 2, half tid % 2 of its 32 bytes
};

template <int NF>
__device__ __forceinline__ void ic_stage_load(IcStage<NF> &s, const uint16_t *__restrict__ dy, const unsigned char *__restrict__ xq,
                                              int64_t c0, int64_t p1, int tid, int H, int W) {
    constexpr int Cout = NF * 32;
    // (a pixel behind the slab's end reads the slab's last pixel and is zeroed in registers)
#pragma unroll
    for (int j = 0; j < IcStage<NF>::DY_ITEMS; ++j) {
        const int i = tid + 256 * j, t = i / (4 * NF), blk = (i % (4 * NF)) >> 2, q = i & 3;
        const int64_t p = c0 + t;
        s.dy[j] = *(const u32x4 *) (dy + (p < p1 ? p : p1 - 1) * Cout + blk * 32 + q * 8);
        if (p >= p1) s.dy[j] = u32x4{0, 0, 0, 0};
    }
    const int t = tid >> 1, q = tid & 1;
    const int64_t p = c0 + t;
    const unsigned pc = (unsigned) (p < p1 ? p : p1 - 1);  // (p <= 2^31 - 1: 32-bit division)
    const unsigned row = pc / (unsigned) W, x = pc - row * (unsigned) W;  // row = n * H + y
    const unsigned n = row / (unsigned) H;
    const int Wq = W + IC_PAD_COLS;
    const unsigned char *at = xq + (((size_t) row + IC_PAD_ROWS * n) * Wq + x) * 8 + q * 16;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        s.x[ky] = *(const u32x4_a8 *) (at + (size_t) ky * Wq * 8);
        if (p >= p1) s.x[ky] = u32x4{0, 0, 0, 0};
    }
}

template <int NF>
__global__ __launch_bounds__(256) void ic_wgrad_slab_kernel(const uint16_t *__restrict__ dy, const unsigned char *__restrict__ xq,
                                                             float *__restrict__ ws, WgSlabs part, int H) {
    constexpr int DY = 0, X = NF * IC_CH * IC_ROW, TOTAL = X + 2 * IC_CH * IC_ROW, Cout = NF * 32;
    constexpr int KI = NF == 4 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) char smem[TOTAL];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int half = lane >> 5, wq = (lane >> 2) & 3;
    const int g = wave & 1, m0 = wave >> 1;
    const bool works = m0 < NF;  // (wave-uniform; with one block of channels waves 2 and 3 stage only)
    const int cb = mf_lane_bytes(lane);
    const int a_base = DY + cb, b_base = X + g * IC_CH * IC_ROW + cb;
    const int W = part.W;
    const int slab = blockIdx.x;
    int64_t p0, p1;
    wgs_range(part, slab, &p0, &p1);

    f32x16 acc[KI];
#pragma unroll
    for (int k = 0; k < KI; ++k) mf_zero(acc[k]);
    // the upper half of image 1's rows is written once: zeros
    if (tid < IC_CH * 2) *(u32x4 *) (smem + X + (IC_CH + (tid >> 1)) * IC_ROW + 32 + (tid & 1) * 16) = u32x4{0, 0, 0, 0};

    IcStage<NF> st;
    ic_stage_load<NF>(st, dy, xq, p0, p1, tid, H, W);
    for (int64_t c0 = p0; c0 < p1; c0 += IC_CH) {
#pragma unroll
        for (int j = 0; j < IcStage<NF>::DY_ITEMS; ++j) {
            const int i = tid + 256 * j, t = i / (4 * NF), blk = (i % (4 * NF)) >> 2, q = i & 3;
            *(u32x4 *) (smem + DY + (blk * IC_CH + t) * IC_ROW + q * 16) = st.dy[j];
        }
        {
            const int t = tid >> 1, q = tid & 1;
            *(u32x4 *) (smem + X + t * IC_ROW + q * 16) = st.x[0];
            *(u32x4 *) (smem + X + t * IC_ROW + 32 + q * 16) = st.x[1];
            *(u32x4 *) (smem + X + (IC_CH + t) * IC_ROW + q * 16) = st.x[2];
        }
        __syncthreads();
        if (c0 + IC_CH < p1) ic_stage_load<NF>(st, dy, xq, c0 + IC_CH, p1, tid, H, W);  // in flight during the products
        const int64_t left = p1 - c0;
        const int steps = left >= IC_CH ? IC_CH / WGS_STEP : wgs_steps(left);
        // ---- multiply: all 64 lanes, rows of zeros stand for the pixels behind the end
        if (works) {
            for (int s = 0; s < steps; ++s) {
                const int t0 = WGS_STEP * s + 8 * half + wq, t1 = t0 + 4;
                const bf16x8 B = mf_operand(smem, b_base + t0 * IC_ROW, b_base + t1 * IC_ROW);
#pragma unroll
                for (int k = 0; k < KI; ++k) {
                    const int m = m0 + 2 * k;
                    const bf16x8 A = mf_operand(smem, a_base + (m * IC_CH + t0) * IC_ROW, a_base + (m * IC_CH + t1) * IC_ROW);
                    acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, acc[k], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // ---- partial sums: D[i = co][j], lane -> j = lane % 32 = 16 (filter row - 2 g) + (kx, c), register r -> i = mf_row(r, lane / 32)
    const int j = lane & 31, ky = 2 * g + (j >> 4);
    if (works && ky < 3) {
        float *out = ws + ((int64_t) slab * 3 + ky) * Cout * 16;
#pragma unroll
        for (int k = 0; k < KI; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) out[((m0 + 2 * k) * 32 + mf_row(r, half)) * 16 + (j & 15)] = acc[k][r];
    }
}

// workspace [slab][3][Cout][16] -> dw [Cout][C][3][3]: the slabs in ascending order, one rounding; columns kx = 3 and c >= C unread
__global__ __launch_bounds__(256) void ic_wgrad_reduce_kernel(const float *__restrict__ ws, int slabs, int Cout, int C, void *dw,
                                                               int dw_dtype) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Cout * C * 9) return;
    const int kx = e % 3, ky = (e / 3) % 3, c = (e / 9) % C, co = e / (9 * C);
    const long per = 3l * Cout * 16, at = ((long) ky * Cout + co) * 16 + kx * 4 + c;
    float sum = ws[at];
#pragma unroll 16
    for (int s = 1; s < slabs; ++s) sum += ws[s * per + at];  // (the loads of 16 slabs in flight, the adds in order)
    if (dw_dtype == CT_BF16) ((uint16_t *) dw)[e] = ct_bf16_rne(sum);
    else ((float *) dw)[e] = sum;
}

// ---- argument checks (0, or the error code with its message recorded) -------------------------------------------------------
int ic_check(const char *who, int N, int H, int W, int cout, int slab_rows, WgSlabs *part) {
    static thread_local char msg[200];
    const char *bad = nullptr;
    if (N < 1 || H < 1 || W < 1) bad = "N, H and W must be at least 1";
    else if (cout != 32 && cout != 64 && cout != 128) bad = "cout must be 32, 64 or 128";
    else if (slab_rows < 0) bad = "slab_rows must be 0 (auto) or positive";
    if (bad) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return cpn::fail(CPN_E_INVALID, msg);
    }
    if ((int64_t) N * (H + IC_PAD_ROWS) > 0x7fffffffll || (int64_t) N * (H + IC_PAD_ROWS) * (W + IC_PAD_COLS) > 0x7fffffffll) {
        snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 pixels in the padded input", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    if (part) *part = wgs_partition((int64_t) N * H, W, slab_rows, IC_SLABS);
    return 0;
}

}  // namespace

extern "C" {

int cpn_image_conv_pad(const float *src, int32_t N, int32_t C, int32_t H, int32_t W, void *xq, void *stream) {
    if (const int rc = ic_check("cpn_image_conv_pad", N, H, W, 32, 0, nullptr)) return rc;
    if (C < 1 || C > 4) return cpn::fail(CPN_E_INVALID, "cpn_image_conv_pad: C must lie in 1 ... 4");
    if (!src || !xq) return cpn::fail(CPN_E_INVALID, "cpn_image_conv_pad: null pointer");
    if (((uintptr_t) src & 3) || ((uintptr_t) xq & 15))
        return cpn::fail(CPN_E_INVALID, "cpn_image_conv_pad: src must start at a 4-byte, xq at a 16-byte aligned address");
    const long total = (long) N * (H + IC_PAD_ROWS) * (W + IC_PAD_COLS);
    long blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(ic_pad_kernel, dim3((unsigned) blocks), dim3(256), 0, (hipStream_t) stream, src, (unsigned char *) xq, N, C, H, W);
    return cpn::check_hip(hipGetLastError(), "cpn_image_conv_pad");
}

int cpn_image_conv_pack(const void *weight, int32_t weight_dtype, int32_t cout, int32_t cin, void *packed, void *stream) {
    if (cout != 32 && cout != 64 && cout != 128) return cpn::fail(CPN_E_INVALID, "cpn_image_conv_pack: cout must be 32, 64 or 128");
    if (cin < 1 || cin > 4) return cpn::fail(CPN_E_INVALID, "cpn_image_conv_pack: cin must lie in 1 ... 4");
    if (weight_dtype != CT_F32 && weight_dtype != CT_BF16)
        return cpn::fail(CPN_E_INVALID, "cpn_image_conv_pack: weight_dtype must be 0 (fp32) or 1 (bf16)");
    if (!weight || !packed) return cpn::fail(CPN_E_INVALID, "cpn_image_conv_pack: null pointer");
    hipLaunchKernelGGL(ic_pack_kernel, dim3((unsigned) ((3 * cout * 16 + 255) / 256)), dim3(256), 0, (hipStream_t) stream, weight,
                       weight_dtype, cout, cin, (uint16_t *) packed);
    return cpn::check_hip(hipGetLastError(), "cpn_image_conv_pack");
}

int cpn_image_conv_forward(const void *xq, const void *packed, const float *bias, int32_t N, int32_t H, int32_t W, int32_t cout,
                           void *y, void *stream) {
    if (const int rc = ic_check("cpn_image_conv_forward", N, H, W, cout, 0, nullptr)) return rc;
    if (!xq || !packed || !y) return cpn::fail(CPN_E_INVALID, "cpn_image_conv_forward: null pointer");
    if (((uintptr_t) xq | (uintptr_t) packed | (uintptr_t) y) & 15)
        return cpn::fail(CPN_E_INVALID, "cpn_image_conv_forward: xq, packed and y must start at 16-byte aligned addresses");
    const long nfrag = (long) N * H * ((W + 31) / 32);
    long blocks = (nfrag + 3) / 4;           // 4 waves per block, one fragment per wave and pass
    // persistent: as many workgroups per CU as the kernel's registers let run at once (74 / 102 / 158 VGPRs), so that every wave
    // gets the same share of the fragments
    const long per_cu = cout == 128 ? 2 : cout == 64 ? 3 : 4;
    if (blocks > 256 * per_cu) blocks = 256 * per_cu;
    const dim3 grid((unsigned) blocks);
    hipStream_t st = (hipStream_t) stream;
    const unsigned char *x = (const unsigned char *) xq, *w = (const unsigned char *) packed;
    if (cout == 128) hipLaunchKernelGGL((ic_forward_kernel<4>), grid, dim3(256), 0, st, x, w, bias, (unsigned char *) y, N, H, W);
    else if (cout == 64) hipLaunchKernelGGL((ic_forward_kernel<2>), grid, dim3(256), 0, st, x, w, bias, (unsigned char *) y, N, H, W);
    else hipLaunchKernelGGL((ic_forward_kernel<1>), grid, dim3(256), 0, st, x, w, bias, (unsigned char *) y, N, H, W);
    return cpn::check_hip(hipGetLastError(), "cpn_image_conv_forward");
}

int64_t cpn_image_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t cout, int32_t slab_rows) {
    WgSlabs part;
    if (ic_check("cpn_image_conv_wgrad_workspace_bytes", N, H, W, cout, slab_rows, &part)) return 0;
    return (int64_t) part.slabs * (3 * cout * 16 + cout) * 4;
}

int cpn_image_conv_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t cout, int32_t slab_rows, int32_t info[5]) {
    WgSlabs part;
    if (const int rc = ic_check("cpn_image_conv_wgrad_info", N, H, W, cout, slab_rows, &part)) return rc;
    if (!info) return cpn::fail(CPN_E_INVALID, "cpn_image_conv_wgrad_info: null pointer");
    wgs_info(part, info);
    return 0;
}

int cpn_image_conv_wgrad(const void *xq, const void *dy, int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t slab_rows,
                         void *dw, int32_t dw_dtype, void *db, int32_t db_dtype, void *workspace, int64_t workspace_bytes,
                         void *stream) {
    WgSlabs part;
    if (const int rc = ic_check("cpn_image_conv_wgrad", N, H, W, cout, slab_rows, &part)) return rc;
    if (cin < 1 || cin > 4) return cpn::fail(CPN_E_INVALID, "cpn_image_conv_wgrad: cin must lie in 1 ... 4");
    if (!xq || !dy || !workspace || (!dw && !db)) return cpn::fail(CPN_E_INVALID, "cpn_image_conv_wgrad: null pointer");
    if (((uintptr_t) xq | (uintptr_t) dy | (uintptr_t) workspace) & 15)
        return cpn::fail(CPN_E_INVALID, "cpn_image_conv_wgrad: xq, dy and workspace must start at 16-byte aligned addresses");
    if ((dw && dw_dtype != CT_F32 && dw_dtype != CT_BF16) || (db && db_dtype != CT_F32 && db_dtype != CT_BF16))
        return cpn::fail(CPN_E_INVALID, "cpn_image_conv_wgrad: an output dtype must be 0 (fp32) or 1 (bf16)");
    const int64_t per = 3ll * cout * 16;
    if (workspace_bytes < (int64_t) part.slabs * (per + cout) * 4)
        return cpn::fail(CPN_E_WORKSPACE, "cpn_image_conv_wgrad: workspace smaller than cpn_image_conv_wgrad_workspace_bytes");
    hipStream_t st = (hipStream_t) stream;
    float *ws = (float *) workspace, *wsb = ws + (int64_t) part.slabs * per;
    if (dw) {
        const dim3 grid((unsigned) part.slabs);
        const uint16_t *g = (const uint16_t *) dy;
        const unsigned char *x = (const unsigned char *) xq;
        if (cout == 128) hipLaunchKernelGGL((ic_wgrad_slab_kernel<4>), grid, dim3(256), 0, st, g, x, ws, part, H);
        else if (cout == 64) hipLaunchKernelGGL((ic_wgrad_slab_kernel<2>), grid, dim3(256), 0, st, g, x, ws, part, H);
        else hipLaunchKernelGGL((ic_wgrad_slab_kernel<1>), grid, dim3(256), 0, st, g, x, ws, part, H);
        hipLaunchKernelGGL(ic_wgrad_reduce_kernel, dim3((unsigned) ((cout * cin * 9 + 255) / 256)), dim3(256), 0, st, ws, part.slabs, cout,
                           cin, dw, dw_dtype);
    }
    if (db) {
        hipLaunchKernelGGL(ct_bias_slab_kernel, dim3((unsigned) part.slabs, (unsigned) (cout / 32)), dim3(256), 0, st,
                           (const uint16_t *) dy, wsb, part, cout);
        hipLaunchKernelGGL(ct_bias_reduce_kernel, dim3((unsigned) ((cout + 255) / 256)), dim3(256), 0, st, wsb, part.slabs, cout, db,
                           db_dtype);
    }
    return cpn::check_hip(hipGetLastError(), "cpn_image_conv_wgrad");
}

}  // extern "C"
