// Trainable image conv on the GPU (gfx950): what celldetection_amd.nn.image_conv2d runs, the first conv of the U-Net encoders,
// Conv2d(C <= 4 -> 32 | 64 | 128, 3x3, stride 1, padding 1) on the image itself.  The rule is the "Trainable image conv" section of
// include/cpn_hip.h.  The image becomes the padded 4-channel tensor Xq, bf16 [N][H + 2][W + 3][4], in which the 16 values
// (kx 0..3, c 0..3) that output pixel (y, x) meets in filter row ky are the 32 contiguous bytes at Xq[n][y + ky][x].
//
//   ic_pad_kernel:          fp32 NCHW -> Xq: zero border (one row and one column in front), zeros in the channels >= C.
//   ic_forward_kernel:      one v_mfma_f32_32x32x16_bf16 step per filter row and 32-channel block on a fragment of 32 pixels of an
//                           image row, operands straight from global memory (the next fragment's are loaded before this one's
//                           products), + bias, bf16 by ct_bf16_rne, 16-byte stores (the epilogue StBf16 of csrc/stem_mfma.h).
//   ic_wgrad_slab_kernel:   dW_ky[Cout][16] = dY^T R_ky per filter row, the flat output pixel as the reduction index, 16 pixels per
//                           MFMA step.  A workgroup owns a slab of image rows (csrc/wgrad_slabs.h) and all three filter rows.  Per
//                           chunk of 128 pixels the dY rows are staged in LDS once for all three filter rows, next to two images
//                           of the pixels' Xq values: image 0 holds the 32 bytes of filter row 0 and of filter row 1 side by side
//                           in a 64-byte row, image 1 those of filter row 2 and 32 bytes of zeros.  Wave w owns image w % 2 and
//                           the 32-channel blocks w / 2, w / 2 + 2 of dY from the slab's first pixel to its last; both operands
//                           are read with ds_read_b64_tr_b16.  The next chunk's global loads are issued before this chunk's
//                           products.  Pixels behind the slab's end are staged as zeros in both operands.
// What it shares with the trainable stem is csrc/image_train.h: the weight pack ([3][Cout][16] bf16, zeros at kx = 3 and c >= C), the
// kernel that adds the slabs in ascending order, rounds once and writes the real 3 x C of the 16 columns only, the dY staging, the
// checks and the host path.  The bias gradient is that of csrc/wgrad_bias.h.  No floating-point atomics: results are bit-identical
// from run to run.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/cpn_hip.h"
#include "image_train.h"
#include "mfma_frag.h"
#include "stem_mfma.h"  // StBf16, u32x2, bf16x8_a8

namespace {

struct IcGeo {
    static constexpr int K = 3, STRIDE = 1;
    static constexpr int PAD_ROWS = 2, PAD_COLS = 3;  // Xq is [N][H + 2][W + 3][4]
    static constexpr int REC = 16;
    static constexpr int COUTS[] = {32, 64, 128};
    static constexpr int SLABS = 512;  // two workgroups per CU, each busy while the other one stages
    static constexpr const char *X = "xq";
};

// ---- input pad ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ic_pad_kernel(const float *__restrict__ src, unsigned char *__restrict__ dst, int N, int C, int H,
                                                     int W) {
    const int Hq = H + IcGeo::PAD_ROWS, Wq = W + IcGeo::PAD_COLS;
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

// ---- forward ------------------------------------------------------------------------------------------------------------------
// the lane's 8 K-values of the three filter rows of fragment f: 16 contiguous bytes of Xq each (lanes past the row's end read its
// last pixel and store nothing)
__device__ __forceinline__ void ic_load_fragment(const unsigned char *__restrict__ xq, long f, int fx, int H, int W, int l31, int lhi,
                                                 bf16x8 (&bx)[3]) {
    const int Hq = H + IcGeo::PAD_ROWS, Wq = W + IcGeo::PAD_COLS;
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
    const StBf16 epilogue{dst, (size_t) Cout * 2};

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
                epilogue(v0, v1, j * 32 + 8 * (lhi ? q1 : q0), pixel, x < W);
            }
        if (more) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) bx[ky] = nx[ky];
        }
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
// LDS image: dY [NF blocks][IT_CH rows], X [2 images][IT_CH rows]; rows of IT_ROW bytes, every offset a multiple of 16.
// Wave w owns X image g = w % 2 and the dY blocks m = w / 2 + 2 k (k < KI) that exist.
template <int NF>
struct IcStage {
    u32x4 dy[IT_DY_ITEMS<NF>];
    u32x4 x[3];  // item tid of filter row ky: pixel tid / 2, half tid % 2 of its 32 bytes
};

template <int NF>
__device__ __forceinline__ void ic_stage_load(IcStage<NF> &s, const uint16_t *__restrict__ dy, const unsigned char *__restrict__ xq,
                                              int64_t c0, int64_t p1, int tid, int H, int W) {
    // (a pixel behind the slab's end reads the slab's last pixel and is zeroed in registers)
#pragma unroll
    for (int j = 0; j < IT_DY_ITEMS<NF>; ++j) s.dy[j] = ItDyItem<NF>(tid + 256 * j).load(dy, c0, p1);
    const int t = tid >> 1, q = tid & 1;
    const int64_t p = c0 + t;
    const unsigned pc = (unsigned) (p < p1 ? p : p1 - 1);  // (p <= 2^31 - 1: 32-bit division)
    const unsigned row = pc / (unsigned) W, x = pc - row * (unsigned) W;  // row = n * H + y
    const unsigned n = row / (unsigned) H;
    const int Wq = W + IcGeo::PAD_COLS;
    const unsigned char *at = xq + (((size_t) row + IcGeo::PAD_ROWS * n) * Wq + x) * 8 + q * 16;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        s.x[ky] = *(const u32x4_a8 *) (at + (size_t) ky * Wq * 8);
        if (p >= p1) s.x[ky] = u32x4{0, 0, 0, 0};
    }
}

template <int NF>
__global__ __launch_bounds__(256) void ic_wgrad_slab_kernel(const uint16_t *__restrict__ dy, const unsigned char *__restrict__ xq,
                                                             float *__restrict__ ws, WgSlabs part, int H) {
    constexpr int DY = 0, X = NF * IT_CH * IT_ROW, TOTAL = X + 2 * IT_CH * IT_ROW, Cout = NF * 32;
    constexpr int KI = NF == 4 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) char smem[TOTAL];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int half = lane >> 5, wq = (lane >> 2) & 3;
    const int g = wave & 1, m0 = wave >> 1;
    const bool works = m0 < NF;  // (wave-uniform; with one block of channels waves 2 and 3 stage only)
    const int cb = mf_lane_bytes(lane);
    const int a_base = DY + cb, b_base = X + g * IT_CH * IT_ROW + cb;
    const int W = part.W;
    const int slab = blockIdx.x;
    int64_t p0, p1;
    wgs_range(part, slab, &p0, &p1);

    f32x16 acc[KI];
#pragma unroll
    for (int k = 0; k < KI; ++k) mf_zero(acc[k]);
    // the upper half of image 1's rows is written once: zeros
    if (tid < IT_CH * 2) *(u32x4 *) (smem + X + (IT_CH + (tid >> 1)) * IT_ROW + 32 + (tid & 1) * 16) = u32x4{0, 0, 0, 0};

    IcStage<NF> st;
    ic_stage_load<NF>(st, dy, xq, p0, p1, tid, H, W);
    for (int64_t c0 = p0; c0 < p1; c0 += IT_CH) {
#pragma unroll
        for (int j = 0; j < IT_DY_ITEMS<NF>; ++j) ItDyItem<NF>(tid + 256 * j).store(smem + DY, st.dy[j]);
        {
            const int t = tid >> 1, q = tid & 1;
            *(u32x4 *) (smem + X + t * IT_ROW + q * 16) = st.x[0];
            *(u32x4 *) (smem + X + t * IT_ROW + 32 + q * 16) = st.x[1];
            *(u32x4 *) (smem + X + (IT_CH + t) * IT_ROW + q * 16) = st.x[2];
        }
        __syncthreads();
        if (c0 + IT_CH < p1) ic_stage_load<NF>(st, dy, xq, c0 + IT_CH, p1, tid, H, W);  // in flight during the products
        const int64_t left = p1 - c0;
        const int steps = left >= IT_CH ? IT_CH / WGS_STEP : wgs_steps(left);
        // ---- multiply: all 64 lanes, rows of zeros stand for the pixels behind the end
        if (works) {
            for (int s = 0; s < steps; ++s) {
                const int t0 = WGS_STEP * s + 8 * half + wq, t1 = t0 + 4;
                const bf16x8 B = mf_operand(smem, b_base + t0 * IT_ROW, b_base + t1 * IT_ROW);
#pragma unroll
                for (int k = 0; k < KI; ++k) {
                    const int m = m0 + 2 * k;
                    const bf16x8 A = mf_operand(smem, a_base + (m * IT_CH + t0) * IT_ROW, a_base + (m * IT_CH + t1) * IT_ROW);
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

// ---- the launches of an accepted call (csrc/image_train.h checks and calls) ------------------------------------------------------
void ic_launch_forward(const unsigned char *xq, const unsigned char *packed, const float *bias, unsigned char *y, int N, int H, int W,
                       int cout, hipStream_t st) {
    const long nfrag = (long) N * H * ((W + 31) / 32);
    long blocks = (nfrag + 3) / 4;           // 4 waves per block, one fragment per wave and pass
    // persistent: as many workgroups per CU as the kernel's registers let run at once (74 / 102 / 158 VGPRs), so that every wave
    // gets the same share of the fragments
    const long per_cu = cout == 128 ? 2 : cout == 64 ? 3 : 4;
    if (blocks > 256 * per_cu) blocks = 256 * per_cu;
    const dim3 grid((unsigned) blocks);
    if (cout == 128) hipLaunchKernelGGL((ic_forward_kernel<4>), grid, dim3(256), 0, st, xq, packed, bias, y, N, H, W);
    else if (cout == 64) hipLaunchKernelGGL((ic_forward_kernel<2>), grid, dim3(256), 0, st, xq, packed, bias, y, N, H, W);
    else hipLaunchKernelGGL((ic_forward_kernel<1>), grid, dim3(256), 0, st, xq, packed, bias, y, N, H, W);
}

void ic_launch_slabs(const WgSlabs &part, const uint16_t *dy, const unsigned char *xq, float *ws, int H, int, int cout, hipStream_t st) {
    const dim3 grid((unsigned) part.slabs);
    if (cout == 128) hipLaunchKernelGGL((ic_wgrad_slab_kernel<4>), grid, dim3(256), 0, st, dy, xq, ws, part, H);
    else if (cout == 64) hipLaunchKernelGGL((ic_wgrad_slab_kernel<2>), grid, dim3(256), 0, st, dy, xq, ws, part, H);
    else hipLaunchKernelGGL((ic_wgrad_slab_kernel<1>), grid, dim3(256), 0, st, dy, xq, ws, part, H);
}

}  // namespace

extern "C" {

int cpn_image_conv_pad(const float *src, int32_t N, int32_t C, int32_t H, int32_t W, void *xq, void *stream) {
    if (const int rc = it_check<IcGeo>("cpn_image_conv_pad", N, H, W, IcGeo::COUTS[0], 0, nullptr)) return rc;
    if (C < 1 || C > 4) return cpn::fail(CPN_E_INVALID, "cpn_image_conv_pad: C must lie in 1 ... 4");
    if (!src || !xq) return cpn::fail(CPN_E_INVALID, "cpn_image_conv_pad: null pointer");
    if (((uintptr_t) src & 3) || ((uintptr_t) xq & 15))
        return cpn::fail(CPN_E_INVALID, "cpn_image_conv_pad: src must start at a 4-byte, xq at a 16-byte aligned address");
    const long total = (long) N * (H + IcGeo::PAD_ROWS) * (W + IcGeo::PAD_COLS);
    long blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(ic_pad_kernel, dim3((unsigned) blocks), dim3(256), 0, (hipStream_t) stream, src, (unsigned char *) xq, N, C, H, W);
    return cpn::check_hip(hipGetLastError(), "cpn_image_conv_pad");
}

int cpn_image_conv_pack(const void *weight, int32_t weight_dtype, int32_t cout, int32_t cin, void *packed, void *stream) {
    return it_pack<IcGeo>("cpn_image_conv_pack", weight, weight_dtype, cout, cin, packed, stream);
}

int cpn_image_conv_forward(const void *xq, const void *packed, const float *bias, int32_t N, int32_t H, int32_t W, int32_t cout,
                           void *y, void *stream) {
    return it_forward<IcGeo>("cpn_image_conv_forward", xq, packed, bias, N, H, W, cout, y, stream, ic_launch_forward);
}

int64_t cpn_image_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t cout, int32_t slab_rows) {
    return it_wgrad_workspace_bytes<IcGeo>("cpn_image_conv_wgrad_workspace_bytes", N, H, W, cout, slab_rows);
}

int cpn_image_conv_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t cout, int32_t slab_rows, int32_t info[5]) {
    return it_wgrad_info<IcGeo>("cpn_image_conv_wgrad_info", N, H, W, cout, slab_rows, info);
}

int cpn_image_conv_wgrad(const void *xq, const void *dy, int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t slab_rows,
                         void *dw, int32_t dw_dtype, void *db, int32_t db_dtype, void *workspace, int64_t workspace_bytes,
                         void *stream) {
    return it_wgrad<IcGeo>("cpn_image_conv_wgrad", xq, dy, N, H, W, cin, cout, slab_rows, dw, dw_dtype, db, db_dtype, workspace,
                           workspace_bytes, stream, ic_launch_slabs);
}

}  // extern "C"
