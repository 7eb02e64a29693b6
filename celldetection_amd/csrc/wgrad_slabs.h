// The slab partition of the weight-gradient reduction (csrc/wgrad_dense.h).  The reduction index of dW is the pixel
// p = (n * H + y) * W + x of the NHWC tensors; R = N * H image rows of W pixels each.  A slab is `slab_rows` consecutive image rows
// (the last slab may be partial; a slab may cross from one image of the batch into the next), i.e. the pixel range
// [s * slab_rows * W, min(R, (s + 1) * slab_rows) * W).  A workgroup reduces the pixels of its slab in ascending order, 16 per MFMA
// step, in ONE fp32 accumulator per output; the reduce kernel then adds the slabs' partial sums in ascending slab order.
// Integer arithmetic only; compiles for the device and for the host (tests/wgrad_slabs_host.cpp runs it against brute force under
// sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WGS_HD __host__ __device__ __forceinline__
#else
#define WGS_HD inline
#endif

constexpr int WGS_STEP = 16;           // pixels per MFMA step (v_mfma_f32_32x32x16_bf16)
constexpr int WGS_BIAS_LANES = 8;      // the bias gradient's slab sum: 8 interleaved chains per channel, then added in order

struct WgSlabs {
    int64_t rows;       // R = N * H
    int32_t W;
    int32_t slab_rows;  // image rows per slab (>= 1)
    int32_t slabs;      // ceil(R / slab_rows)
    int32_t steps;      // MFMA steps of the largest (= first) slab: ceil(slab_rows * W / 16)
};

WGS_HD int64_t wgs_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// requested: rows per slab, 0 = auto: at most slabs_wanted >= 1 slabs of equal size (the caller knows how many workgroups a slab
// takes and how many the device holds at once).  Needs rows >= 1, W >= 1, rows * W <= 2^31 - 1.
WGS_HD WgSlabs wgs_partition(int64_t rows, int32_t W, int32_t requested, int32_t slabs_wanted) {
    WgSlabs s;
    s.rows = rows;
    s.W = W;
    int64_t sr;
    if (requested > 0) {
        sr = requested < rows ? requested : rows;
    } else {
        sr = wgs_ceil_div(rows, slabs_wanted < 1 ? 1 : slabs_wanted);
    }
    s.slab_rows = (int32_t) sr;
    s.slabs = (int32_t) wgs_ceil_div(rows, sr);
    s.steps = (int32_t) wgs_ceil_div(sr * W, WGS_STEP);
    return s;
}

// pixel range [p0, p1) of slab `slab` (0 <= slab < slabs)
WGS_HD void wgs_range(const WgSlabs &s, int32_t slab, int64_t *p0, int64_t *p1) {
    const int64_t r0 = (int64_t) slab * s.slab_rows;
    int64_t r1 = r0 + s.slab_rows;
    if (r1 > s.rows) r1 = s.rows;
    *p0 = r0 * s.W;
    *p1 = r1 * s.W;
}

// MFMA steps of a slab of `pixels` pixels
WGS_HD int32_t wgs_steps(int64_t pixels) { return (int32_t) wgs_ceil_div(pixels, WGS_STEP); }

// length of the fp32 chain of one weight-gradient element: the MFMA steps of a slab, + 2 for the MFMA-internal sum, + one add
// per slab in the reduce kernel (64-bit: 2^31 - 1 slabs of one pixel are a valid partition)
WGS_HD int64_t wgs_chain(const WgSlabs &s) { return (int64_t) s.steps + 2 + s.slabs; }

// ... and of one bias-gradient element: ceil(slab pixels / 8) adds per interleaved chain, 8 adds across them, one per slab
WGS_HD int64_t wgs_bias_chain(const WgSlabs &s) {
    return wgs_ceil_div((int64_t) s.slab_rows * s.W, WGS_BIAS_LANES) + WGS_BIAS_LANES + s.slabs;
}

// the five numbers of a *_wgrad_info call: slabs, rows per slab, MFMA steps of the largest slab, and the two chains that the slabs
// add to it -- the reduce chain (one add per slab) and the bias chain, of the bias gradient's own partition where a strided conv
// gives dY other rows than x
WGS_HD void wgs_info(const WgSlabs &s, const WgSlabs &bias, int32_t info[5]) {
    info[0] = s.slabs;
    info[1] = s.slab_rows;
    info[2] = s.steps;
    info[3] = s.slabs;
    info[4] = (int32_t) wgs_bias_chain(bias);
}
WGS_HD void wgs_info(const WgSlabs &s, int32_t info[5]) { wgs_info(s, s, info); }
