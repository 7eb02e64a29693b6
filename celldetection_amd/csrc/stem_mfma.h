// The MFMA loop of the 7x7 stride-2 stem on the padded 4-channel input bf16 [N][Hp = H + 6][Wp = W + 8][4] (csrc/stem.hip says why
// that layout): K = 7 filter rows x 32 values (8 pixels x 4 channels) = 14 steps of v_mfma_f32_32x32x16_bf16 per fragment of 32
// output pixels, both operands straight from global memory.  Two kernels are wrappers around it and differ in their Epilogue:
// stem7_kernel (csrc/stem.hip: ReLU, then bf16 or e4m3) and st_forward_kernel (csrc/stem_train.hip: bf16, no activation).
//
// An Epilogue is called once per (fragment, 32-channel block j, pair qp of accumulator quads) with
//   void operator()(const float (&v0)[4], const float (&v1)[4], int ch, size_t pixel, bool ok) const
// v0 / v1: the sums + bias of channels j * 32 + 8 q + 4 lhi + e of the lane's pixel, q = 2 qp and 2 qp + 1 (lhi = lane / 32).  ch:
// the first of the 8 consecutive channels the lane owns once the lane halves have swapped the quads they do not keep,
// j * 32 + 8 (2 qp + lhi).  pixel: the flat output pixel; ok: false in the lanes behind the row's end, which store nothing.  The
// epilogue applies its activation, converts, swaps and stores; stem_store_bf16 is the swap and the store of the bf16 layouts and
// StBf16 the epilogue without an activation, which the trainable image conv (csrc/image_conv_train.hip) stores through as well: its
// loop prefetches and is its own.
// Device code with internal linkage: every unit that includes this header gets its own copy, compiled with that unit's flags.
#pragma once
#include <hip/hip_runtime.h>

#include "mfma_frag.h"
#include "wgrad_bias.h"  // ct_bf16_rne

namespace {

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef bf16x8 __attribute__((aligned(8))) bf16x8_a8;  // a row of the padded input starts at a multiple of 8 bytes (odd W)

// a0, a1: the lane's quad q0 as two packed bf16 pairs, b0, b1: its quad q1.  v_permlane32_swap(x, y): x of lanes 32..63 <-> y of
// lanes 0..31, so the lower lanes end with (own q0, the upper lanes' q0) = channels 8 q0 ... + 7 and the upper lanes with (the
// lower lanes' q1, own q1) = channels 8 q1 ... + 7: one 16-byte store at `at`
__device__ __forceinline__ void stem_store_bf16(unsigned char *at, bool ok, unsigned a0, unsigned a1, unsigned b0, unsigned b1) {
    const u32x2 s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
    const u32x2 s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
    u32x4 o;
    o.x = s0.x; o.y = s1.x; o.z = s0.y; o.w = s1.y;
    if (ok) *(u32x4 *) at = o;
}

__device__ __forceinline__ unsigned int stem_pack2(float lo, float hi) {
    return (unsigned int) ct_bf16_rne(lo) | ((unsigned int) ct_bf16_rne(hi) << 16);
}

// the Epilogue of the trainable convs: no activation, bf16 by ct_bf16_rne, one 16-byte store
struct StBf16 {
    unsigned char *dst;
    size_t stride;  // bytes per output pixel
    __device__ __forceinline__ void operator()(const float (&v0)[4], const float (&v1)[4], int ch, size_t pixel, bool ok) const {
        stem_store_bf16(dst + pixel * stride + (size_t) ch * 2, ok, stem_pack2(v0[0], v0[1]), stem_pack2(v0[2], v0[3]),
                        stem_pack2(v1[0], v1[1]), stem_pack2(v1[2], v1[3]));
    }
};

// NF = 32-channel output fragments (1 | 2); weights [7][NF * 32][32] bf16.  One wave = one 32-pixel row fragment at a time
// (persistent waves, grid-stride: this one is wave `wave` of `nwaves`, which the kernel works out itself -- there the compiler
// folds blockDim into the launch bounds, inside an inlined function it costs a load); the A fragments stay in registers (28 KB
// for 64 outputs).
template <int NF, class Epilogue>
__device__ __forceinline__ void stem_mfma_loop(const unsigned char *__restrict__ src, const unsigned char *__restrict__ weights,
                                               const float *__restrict__ bias_p, int N, int Hp, int Wp, int Hout, int Wout,
                                               int wave, int nwaves, const Epilogue &epilogue) {
    const int lane = threadIdx.x & 63;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int fx = (Wout + 31) >> 5;  // fragments per output row
    const long nfrag = (long) N * Hout * fx;
    constexpr int coutp = NF * 32;

    // A-fragments: lane -> output channel j * 32 + l31, K-octet (half, lhi) of filter row ky
    bf16x8 wf[NF][14];
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
        for (int ks = 0; ks < 14; ++ks)
            wf[j][ks] = *(const bf16x8 *) (weights + ((size_t) ((ks >> 1) * coutp + j * 32 + l31) * 32 + (ks & 1) * 16 + lhi * 8) * 2);
    float bias[NF][4][4];
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) bias[j][q][e] = bias_p ? bias_p[j * 32 + mf_row(4 * q + e, lhi)] : 0.f;

    for (long f = wave; f < nfrag; f += nwaves) {
        const int tx = (int) (f % fx);
        const long r = f / fx;
        const int oy = (int) (r % Hout);
        const int n = (int) (r / Hout);
        const int ox = tx * 32 + l31;
        const int oxc = ox < Wout ? ox : Wout - 1;  // lanes past the row end recompute its last pixel (never stored)
        // B-fragments: this lane's 8 K-values of filter row ky are 16 contiguous bytes of the padded input
        const unsigned char *p = src + (((size_t) n * Hp + 2 * oy) * Wp + 2 * oxc) * 8 + lhi * 16;
        bf16x8 bx[14];
#pragma unroll
        for (int ks = 0; ks < 14; ++ks) bx[ks] = *(const bf16x8_a8 *) (p + (size_t) (ks >> 1) * Wp * 8 + (ks & 1) * 32);
        f32x16 acc[NF];
#pragma unroll
        for (int j = 0; j < NF; ++j) mf_zero(acc[j]);
#pragma unroll
        for (int ks = 0; ks < 14; ++ks)
#pragma unroll
            for (int j = 0; j < NF; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[j][ks], bx[ks], acc[j], 0, 0, 0);
        const size_t pixel = ((size_t) n * Hout + oy) * Wout + ox;
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
                epilogue(v0, v1, j * 32 + 8 * (lhi ? q1 : q0), pixel, ox < Wout);
            }
    }
}

}  // namespace
