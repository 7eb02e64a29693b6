// Device arithmetic of the Fourier-to-contour decode and of local refinement, shared by decode_nms.hip (inference) and
// cpn_objective.hip (training objective) so that both give the same bits.  Include only from files compiled with
// -ffp-contract=off: every product and sum below is rounded on its own, in the reference's order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cpn_dec {

// x/y of one contour sample: ((loc + sum_k f[k][sincol]*sin[k][s]) + sum_k f[k][coscol]*cos[k][s]), ops/cpn.py:91-94
__device__ __forceinline__ float synth(const float *coef, int order, int samples, int s, int sincol, int coscol,
                                       const float *__restrict__ cos_t, const float *__restrict__ sin_t, float loc) {
    float a = __fmul_rn(coef[sincol], sin_t[s]);
    for (int k = 1; k < order; ++k) a = __fadd_rn(a, __fmul_rn(coef[k * 4 + sincol], sin_t[k * samples + s]));
    float v = __fadd_rn(loc, a);
    float c = __fmul_rn(coef[coscol], cos_t[s]);
    for (int k = 1; k < order; ++k) c = __fadd_rn(c, __fmul_rn(coef[k * 4 + coscol], cos_t[k * samples + s]));
    return __fadd_rn(v, c);
}

// bucketed refinement (models/cpn.py:72-82, ops/cpn.py:238-255): sample s blends the channel pairs of three
// neighbouring buckets; idx/w are host-built [3][samples] tables (bucket index, weight) in the reference's order a,b,c
struct Buckets {
    int n;               // refinement_buckets (1 = plain two-channel map)
    const int32_t *idx;  // [3][samples]
    const float *w;      // [3][samples]
    int samples;
};

// one iteration of models/cpn.py:63-85: round (half to even) -> clamp -> gather -> add; returns the gathered pixel iy * W + ix
__device__ __forceinline__ size_t refine_step(float &cx, float &cy, const float *__restrict__ ref_b, int H, int W,
                                              const Buckets &B, int s) {
    const size_t plane = (size_t) H * W;
    cx = fminf(fmaxf(rintf(cx), 0.f), (float) (W - 1));
    cy = fminf(fmaxf(rintf(cy), 0.f), (float) (H - 1));
    const int ix = (int) cx, iy = (int) cy;
    const size_t o = (size_t) iy * W + ix;
    if (B.n <= 1) {
        cx = __fadd_rn(cx, ref_b[o]);
        cy = __fadd_rn(cy, ref_b[plane + o]);
    } else {  // responses = (r_a*w_a + r_b*w_b) + r_c*w_c, every product and sum rounded (cpn.py:76-81)
        float rx = 0.f, ry = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int bi = B.idx[k * B.samples + s];
            const float wk = B.w[k * B.samples + s];
            const float tx = __fmul_rn(ref_b[(size_t) (2 * bi) * plane + o], wk);
            const float ty = __fmul_rn(ref_b[(size_t) (2 * bi + 1) * plane + o], wk);
            rx = k == 0 ? tx : __fadd_rn(rx, tx);
            ry = k == 0 ? ty : __fadd_rn(ry, ty);
        }
        cx = __fadd_rn(cx, rx);
        cy = __fadd_rn(cy, ry);
    }
    return o;
}

__device__ __forceinline__ void refine_point(float &cx, float &cy, const float *__restrict__ ref_b, int H, int W,
                                             int iterations, const Buckets &B, int s) {
    for (int it = 0; it < iterations; ++it) refine_step(cx, cy, ref_b, H, W, B, s);
}

}  // namespace cpn_dec
