// Index arithmetic of the bilinear resize (align_corners = False) and of its adjoint (csrc/bilinear_train.hip).  The forward kernels
// read output index dst of an axis through
//     f = fmaxf(scale * ((float) dst + 0.5f) - 0.5f, 0.f),  i0 = (int) f,  i1 = i0 + (i0 < in_size - 1),  lambda = f - (float) i0
// with scale = (float) in / (float) out, as (1 - lambda) * src[i0] + lambda * src[i1].  ba_tap restates that token for token.  What
// the source text leaves open is how often the coordinate is rounded, and the forward kernels differ in it:
//   fused:  bilinear_kernel (csrc/misc_kernels.hip) and the conv loader's halo_bilinear_store (csrc/conv_igemm.hip) are compiled with
//           contraction, which turns the product and the difference into ONE v_fma_f32 (one rounding);
//   split:  resize_f32_kernel (csrc/decode_nms.hip, the fp32 planes) rounds the product and the difference each (__fmul_rn, __fsub_rn).
// The two agree wherever the product is exact (the exact x2 of the models among them) and differ by its rounding elsewhere, which
// moves lambda by up to 2^-24 * in and, where f falls on an integer, the tap pair.  ba_tap therefore takes the form as an argument
// and states both explicitly (fmaf / two statements under contract(off)), so that what a backward sums is the adjoint of what ITS
// forward read at EVERY size.
//
// i0 is non-decreasing in dst (a float product with a positive constant is monotone, so are the fma, the difference, fmaxf and the
// truncation of a non-negative number), and an output reads i0 and i0 + 1 at most, hence the dst indices that touch source index i
// -- its footprint -- are those with i0 in {i - 1, i}: one contiguous range [ba_first(i - 1), ba_first(i + 1)), never empty for
// 1 <= in <= out (i0 takes every value 0 ... in - 1, because f advances by scale <= 1 per step from 0).  ba_first finds a range's
// start from a float estimate that it then corrects by stepping, so its answer does not depend on how the estimate is rounded.
// ba_weight is the coefficient with which dst reads i: 1 - lambda if i == i0, plus lambda if i == i1 -- at the clamped last index
// both apply -- and 0 for every other i, so a footprint may be walked generously.
// Supported: 1 <= in <= out; in == out is the identity (scale 1, f = dst, lambda = 0).
// Compiles for the device and for the host (tests/bilinear_adjoint_host.cpp runs it against brute force under sanitizers).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BA_HD __host__ __device__ __forceinline__
#else
#define BA_HD inline
#endif

BA_HD float ba_scale(int in_size, int out_size) { return (float) in_size / (float) out_size; }

// the two taps of output index dst and the weight of the second; fused: the coordinate's product and difference in one fma
BA_HD void ba_tap(int dst, float scale, int in_size, bool fused, int *i0, int *i1, float *lambda) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float f = fused ? fmaxf(fmaf(scale, (float) dst + 0.5f, -0.5f), 0.f) : fmaxf(scale * ((float) dst + 0.5f) - 0.5f, 0.f);
    *i0 = (int) f;
    *i1 = *i0 + (*i0 < in_size - 1);
    *lambda = f - (float) *i0;
}

BA_HD int ba_i0(int dst, float scale, int in_size, bool fused) {
    int i0, i1;
    float lambda;
    ba_tap(dst, scale, in_size, fused, &i0, &i1, &lambda);
    return i0;
}

// the smallest dst in [0, out_size] whose i0 is >= i (out_size: none); any i, 1 <= in_size <= out_size
BA_HD int ba_first(int i, float scale, int in_size, int out_size, bool fused) {
    if (i <= 0) return 0;
    if (i >= in_size) return out_size;
    const float e = ceilf(((float) i + 0.5f) / scale - 0.5f);
    int d = e >= (float) out_size ? out_size : (e <= 0.f ? 0 : (int) e);
    while (d > 0 && ba_i0(d - 1, scale, in_size, fused) >= i) --d;
    while (d < out_size && ba_i0(d, scale, in_size, fused) < i) ++d;
    return d;
}

// the coefficient with which output index dst reads source index i
BA_HD float ba_weight(int dst, float scale, int in_size, bool fused, int i) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int i0, i1;
    float lambda;
    ba_tap(dst, scale, in_size, fused, &i0, &i1, &lambda);
    float w = 0.f;
    if (i == i0) w = 1.f - lambda;
    if (i == i1) w += lambda;
    return w;
}
