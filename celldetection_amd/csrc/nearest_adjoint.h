// Index arithmetic of the nearest resize and of its adjoint (csrc/cat_conv_train.hip).  The forward loader of the conv kernels
// reads a resized source through nearest_src of csrc/cpn_kernels.h: src(dst) = min((int) floorf((float) dst * scale), in - 1) with
// scale = (float) in / (float) out -- PyTorch's legacy 'nearest' rule.  na_src restates it token for token, so that what the
// backward sums is the exact adjoint of what the forward read at EVERY size, including those where the float product and the
// integer quotient dst * in / out disagree.
//
// src is non-decreasing in dst (a float product with a positive constant is monotone, so is floorf, so is the clamp), hence the
// dst pixels that read source pixel i -- its footprint -- are one contiguous range [na_first(i), na_first(i + 1)), possibly empty,
// and the footprints of i = 0 ... in - 1 partition [0, out).  na_first finds the range's start from a float estimate that it then
// corrects by stepping, so its answer does not depend on how the estimate is rounded.
// Compiles for the device and for the host (tests/nearest_adjoint_host.cpp runs it against brute force under sanitizers).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NA_HD __host__ __device__ __forceinline__
#else
#define NA_HD inline
#endif

NA_HD float na_scale(int in_size, int out_size) { return (float) in_size / (float) out_size; }

// nearest_src of csrc/cpn_kernels.h
NA_HD int na_src(int dst, float scale, int in_size) {
    const int s = (int) floorf((float) dst * scale);
    return s < in_size - 1 ? s : in_size - 1;
}

// the smallest dst in [0, out_size] with na_src(dst) >= i (out_size: none); 0 <= i <= in_size, 1 <= in_size <= out_size
NA_HD int na_first(int i, float scale, int in_size, int out_size) {
    if (i <= 0) return 0;
    if (i >= in_size) return out_size;
    float e = ceilf((float) i / scale);
    int d = e >= (float) out_size ? out_size : (e <= 0.f ? 0 : (int) e);
    while (d > 0 && na_src(d - 1, scale, in_size) >= i) --d;
    while (d < out_size && na_src(d, scale, in_size) < i) ++d;
    return d;
}

// flat pixel f = (n * H + y) * W + x of the [N][H][W] map -> the flat pixel of the [N][h][w] source it reads through the resize
// (0 <= f < N * H * W <= 2^31 - 1; sy = na_scale(h, H), sx = na_scale(w, W))
NA_HD int32_t na_pixel_src(int32_t f, int32_t H, int32_t W, int32_t h, int32_t w, float sy, float sx) {
    const uint32_t row = (uint32_t) f / (uint32_t) W;
    const int32_t x = (int32_t) ((uint32_t) f - row * (uint32_t) W);
    const uint32_t n = row / (uint32_t) H;
    const int32_t y = (int32_t) (row - n * (uint32_t) H);
    return (int32_t) ((n * (uint32_t) h + (uint32_t) na_src(y, sy, h)) * (uint32_t) w + (uint32_t) na_src(x, sx, w));
}
