// Trainable ResNet stem on the GPU (gfx950): what celldetection_amd.nn.stem_conv2d runs (the max-pool is csrc/pool_train.hip).  The rule
// is the "Trainable stem and max-pool" section of include/cpn_hip.h.  The stem is Conv2d(C <= 4 -> 32 | 64, 7x7, stride 2, pad 3)
// on the padded 4-channel input bf16 [N][H + 6][W + 8][4] that cpn_convert_input_stem writes (csrc/stem.hip): the 32 values
// (kx 0..7, c 0..3) that output pixel (oy, ox) meets in filter row ky are the 64 contiguous bytes at Xp[n][2 oy + ky][2 ox].
//
// What it shares with the trainable image conv is csrc/image_train.h: the weight pack ([7][Cout][32] bf16, zeros at kx = 7 and
// c >= C), the kernel that adds the slabs, the dY staging, the checks and the host path.  Its own:
//   st_forward_kernel:     the MFMA loop of stem7_kernel (csrc/stem_mfma.h, one text for both): 14 v_mfma_f32_32x32x16_bf16 steps
//                          per 32-pixel fragment, operands straight from global memory, + bias, with the epilogue StBf16: no
//                          ReLU, bf16 by ct_bf16_rne, 16-byte stores.
//   st_wgrad_slab_kernel:  dW_ky[Cout][32] = dY^T R_ky per filter row, the flat output pixel as the reduction index, 16 pixels per
//                          MFMA step.  A workgroup owns a slab of output rows (csrc/wgrad_slabs.h) and all seven filter rows: per
//                          chunk of 128 pixels the dY rows are staged in LDS once, wave w stages the 64-byte X rows of filter row
//                          w (then 4 + w) into its own region, and both operands are read with ds_read_b64_tr_b16.  Pixels behind
//                          the slab's end are staged as zeros in both operands (no masks, no uninitialised LDS).
// The slabs' sums are added in ascending order and rounded once; only the real 7 x C of the 32 columns are written.
// The bias gradient is that of csrc/wgrad_bias.h.  No floating-point atomics: results are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/cpn_hip.h"
#include "image_train.h"
#include "mfma_frag.h"
#include "stem_mfma.h"

namespace {

struct StGeo {
    static constexpr int K = 7, STRIDE = 2;
    static constexpr int PAD_ROWS = 6, PAD_COLS = 8;  // STEM_PAD_ROWS / STEM_PAD_COLS of csrc/cpn_kernels.h
    static constexpr int REC = 32;
    static constexpr int COUTS[] = {32, 64};
    static constexpr int SLABS = 256;  // one workgroup per slab and CU (512 measured no faster: profiles/stem.txt)
    static constexpr const char *X = "xp";
};

// ---- forward: stem_mfma_loop with the epilogue that has no activation -----------------------------------------------------------
template <int NF>
__global__ __launch_bounds__(256, 2) void st_forward_kernel(const unsigned char *__restrict__ xp, const unsigned char *__restrict__ wts,
                                                            const float *__restrict__ bias_p, unsigned char *__restrict__ dst, int N,
                                                            int H, int W, int Hout, int Wout) {
    const int wave = (int) ((blockIdx.x * (unsigned) blockDim.x + threadIdx.x) >> 6);
    const int nwaves = (int) ((gridDim.x * (unsigned) blockDim.x) >> 6);
    stem_mfma_loop<NF>(xp, wts, bias_p, N, H + StGeo::PAD_ROWS, W + StGeo::PAD_COLS, Hout, Wout, wave, nwaves, StBf16{dst, (size_t) NF * 32 * 2});
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
// LDS image: dY [NF blocks][IT_CH rows], X [4 waves][IT_CH rows]; rows of IT_ROW bytes, every offset a multiple of 16
template <int NF>
__global__ __launch_bounds__(256) void st_wgrad_slab_kernel(const uint16_t *__restrict__ dy, const unsigned char *__restrict__ xp,
                                                             float *__restrict__ ws, WgSlabs part, int Hout, int H, int W) {
    constexpr int DY = 0, X = NF * IT_CH * IT_ROW, TOTAL = X + 4 * IT_CH * IT_ROW, Cout = NF * 32;
    __shared__ __attribute__((aligned(16))) char smem[TOTAL];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int half = lane >> 5, wq = (lane >> 2) & 3;
    const int cb = mf_lane_bytes(lane);
    const int a_base = DY + cb, b_base = X + wave * IT_CH * IT_ROW + cb;
    const unsigned Wout = (unsigned) part.W;
    const int Wp = W + StGeo::PAD_COLS, Hp = H + StGeo::PAD_ROWS;
    const int slab = blockIdx.x;
    int64_t p0, p1;
    wgs_range(part, slab, &p0, &p1);

    f32x16 acc[2][NF];  // [pass]: wave w owns filter rows w and 4 + w (wave 3: row 3 alone)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int m = 0; m < NF; ++m) mf_zero(acc[g][m]);

    for (int64_t c0 = p0; c0 < p1; c0 += IT_CH) {
        // ---- stage dY (every load is issued before the first store)
        {
            u32x4 v[IT_DY_ITEMS<NF>];
#pragma unroll
            for (int j = 0; j < IT_DY_ITEMS<NF>; ++j) v[j] = ItDyItem<NF>(tid + 256 * j).load(dy, c0, p1);
#pragma unroll
            for (int j = 0; j < IT_DY_ITEMS<NF>; ++j) ItDyItem<NF>(tid + 256 * j).store(smem + DY, v[j]);
        }
        const int64_t left = p1 - c0;
        const int steps = left >= IT_CH ? IT_CH / WGS_STEP : wgs_steps(left);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int ky = 4 * g + wave;  // (wave-uniform)
            // ---- stage X: the 64 bytes at Xp[n][2 oy + ky][2 ox] of every chunk pixel, 4 items per pixel; zeros behind the end
            if (ky < 7) {
                constexpr int ITEMS = IT_CH * 4 / 64;
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
                    *(u32x4 *) (smem + X + (wave * IT_CH + t) * IT_ROW + q * 16) = v[j];
                }
            }
            __syncthreads();
            // ---- multiply: all 64 lanes, rows of zeros stand for the pixels behind the end
            if (ky < 7) {
                for (int s = 0; s < steps; ++s) {
                    const int t0 = WGS_STEP * s + 8 * half + wq, t1 = t0 + 4;
                    const bf16x8 B = mf_operand(smem, b_base + t0 * IT_ROW, b_base + t1 * IT_ROW);
#pragma unroll
                    for (int m = 0; m < NF; ++m) {
                        const bf16x8 A = mf_operand(smem, a_base + (m * IT_CH + t0) * IT_ROW, a_base + (m * IT_CH + t1) * IT_ROW);
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

// ---- the launches of an accepted call (csrc/image_train.h checks and calls) ------------------------------------------------------
void st_launch_forward(const unsigned char *xp, const unsigned char *packed, const float *bias, unsigned char *y, int N, int H, int W,
                       int cout, hipStream_t st) {
    const int Hout = it_out<StGeo>(H), Wout = it_out<StGeo>(W);
    const long nfrag = (long) N * Hout * ((Wout + 31) / 32);
    long blocks = (nfrag + 3) / 4;           // 4 waves per block, one fragment per wave and pass
    if (blocks > 256 * 2) blocks = 256 * 2;  // persistent: two blocks per CU (the A-fragments are loaded once per wave)
    if (cout == 64) hipLaunchKernelGGL((st_forward_kernel<2>), dim3((unsigned) blocks), dim3(256), 0, st, xp, packed, bias, y, N, H, W, Hout, Wout);
    else hipLaunchKernelGGL((st_forward_kernel<1>), dim3((unsigned) blocks), dim3(256), 0, st, xp, packed, bias, y, N, H, W, Hout, Wout);
}

void st_launch_slabs(const WgSlabs &part, const uint16_t *dy, const unsigned char *xp, float *ws, int H, int W, int cout, hipStream_t st) {
    const int Hout = it_out<StGeo>(H);
    if (cout == 64) hipLaunchKernelGGL((st_wgrad_slab_kernel<2>), dim3((unsigned) part.slabs), dim3(256), 0, st, dy, xp, ws, part, Hout, H, W);
    else hipLaunchKernelGGL((st_wgrad_slab_kernel<1>), dim3((unsigned) part.slabs), dim3(256), 0, st, dy, xp, ws, part, Hout, H, W);
}

}  // namespace

extern "C" {

int cpn_stem_train_pack(const void *weight, int32_t weight_dtype, int32_t cout, int32_t cin, void *packed, void *stream) {
    return it_pack<StGeo>("cpn_stem_train_pack", weight, weight_dtype, cout, cin, packed, stream);
}

int cpn_stem_train_forward(const void *xp, const void *packed, const float *bias, int32_t N, int32_t H, int32_t W, int32_t cout,
                           void *y, void *stream) {
    return it_forward<StGeo>("cpn_stem_train_forward", xp, packed, bias, N, H, W, cout, y, stream, st_launch_forward);
}

int64_t cpn_stem_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t cout, int32_t slab_rows) {
    return it_wgrad_workspace_bytes<StGeo>("cpn_stem_wgrad_workspace_bytes", N, H, W, cout, slab_rows);
}

int cpn_stem_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t cout, int32_t slab_rows, int32_t info[5]) {
    return it_wgrad_info<StGeo>("cpn_stem_wgrad_info", N, H, W, cout, slab_rows, info);
}

int cpn_stem_wgrad(const void *xp, const void *dy, int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t slab_rows,
                   void *dw, int32_t dw_dtype, void *db, int32_t db_dtype, void *workspace, int64_t workspace_bytes, void *stream) {
    return it_wgrad<StGeo>("cpn_stem_wgrad", xp, dy, N, H, W, cin, cout, slab_rows, dw, dw_dtype, db, db_dtype, workspace, workspace_bytes,
                           stream, st_launch_slabs);
}

}  // extern "C"
