// The slab partition and the lane mapping of the batch-normalisation kernels (csrc/batch_norm.hip).  x is [M pixels][C channels],
// C = 8 V: a pixel is V vectors of 8 channels.  The vectors are cut into channel blocks of at most BNS_LANES = 256 (blockIdx.y);
// a workgroup of 256 lanes owns one block of vb vectors and, per step, R = 256 / vb (floor) consecutive pixels: lane l holds vector
// l % vb of the pixel `first pixel of the step + l / vb`, lanes >= R * vb idle.  A lane keeps its 8 channels for the whole kernel.
// The pixel range is cut into slabs of slab_pixels consecutive pixels (the last may be partial); one workgroup per (slab, block).
// The fp64 sums of a channel: every lane adds its own pixels in ascending order (a chain of at most ceil(slab pixels / R) terms),
// the min(R, slab pixels) lane partials that hold a pixel are added in ascending lane order, then the slabs in ascending order.
// Integer arithmetic only; compiles for the device and for the host (tests/bn_slabs_host.cpp runs it against brute force under
// sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BNS_HD __host__ __device__ __forceinline__
#else
#define BNS_HD inline
#endif

constexpr int BNS_LANES = 256;        // lanes of a workgroup = the most vectors of a channel block
constexpr int BNS_VEC = 8;            // channels per vector (16 B of bf16)
constexpr int BNS_MIN_SLAB = 64;      // auto partition: no slab below this many pixels (workspace traffic <= 1 / 8 of bf16 x's)

struct BnSlabs {
    int64_t M;            // pixels
    int32_t V;            // vectors per pixel = C / 8
    int32_t blocks;       // channel blocks = ceil(V / 256)
    int32_t slab_pixels;  // pixels per slab (>= 1)
    int32_t slabs;        // ceil(M / slab_pixels)
};

BNS_HD int64_t bns_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// vectors of channel block `block` (0 <= block < blocks): 256, the last block what is left
BNS_HD int32_t bns_block_vectors(const BnSlabs &s, int32_t block) {
    const int32_t left = s.V - block * BNS_LANES;
    return left < BNS_LANES ? left : BNS_LANES;
}

// pixels per step of a block of vb vectors
BNS_HD int32_t bns_rows(int32_t vb) { return BNS_LANES / vb; }

// requested: pixels per slab, 0 = auto: at most slabs_wanted >= 1 slabs of equal size and none below BNS_MIN_SLAB pixels.
// Needs 1 <= M <= 2^31 - 1, V >= 1.
BNS_HD BnSlabs bns_partition(int64_t M, int32_t V, int32_t requested, int32_t slabs_wanted) {
    BnSlabs s;
    s.M = M;
    s.V = V;
    s.blocks = (int32_t) bns_ceil_div(V, BNS_LANES);
    int64_t sp;
    if (requested > 0) {
        sp = requested;
    } else {
        sp = bns_ceil_div(M, slabs_wanted < 1 ? 1 : slabs_wanted);
        if (sp < BNS_MIN_SLAB) sp = BNS_MIN_SLAB;
    }
    if (sp > M) sp = M;
    s.slab_pixels = (int32_t) sp;
    s.slabs = (int32_t) bns_ceil_div(M, sp);
    return s;
}

// pixel range [p0, p1) of slab `slab` (0 <= slab < slabs)
BNS_HD void bns_range(const BnSlabs &s, int32_t slab, int64_t *p0, int64_t *p1) {
    *p0 = (int64_t) slab * s.slab_pixels;
    int64_t e = *p0 + s.slab_pixels;
    *p1 = e > s.M ? s.M : e;
}

// lane -> (pixel row of the step, vector of the block); false for an idle lane
BNS_HD bool bns_lane(int32_t vb, int32_t lane, int32_t *row, int32_t *vec) {
    *row = lane / vb;
    *vec = lane - *row * vb;
    return *row < bns_rows(vb);
}

// steps a workgroup takes over a slab of `pixels` pixels, and the terms of the chain of the lanes of pixel row `row`
BNS_HD int64_t bns_steps(int64_t pixels, int32_t vb) { return bns_ceil_div(pixels, bns_rows(vb)); }
BNS_HD int64_t bns_lane_terms(int64_t pixels, int32_t vb, int32_t row) {
    return row < pixels ? bns_ceil_div(pixels - row, bns_rows(vb)) : 0;
}

// lane partials added per channel for a slab of `pixels` pixels: the pixel rows that hold a pixel
BNS_HD int32_t bns_partials(int64_t pixels, int32_t vb) {
    const int32_t R = bns_rows(vb);
    return pixels < R ? (int32_t) pixels : R;
}

// length of the fp64 chain of one channel sum in block `block`: the longest lane chain of the largest (= first) slab, one add per
// lane partial, one add per slab.  Never more than M + 1 + slabs.
BNS_HD int64_t bns_sum_chain(const BnSlabs &s, int32_t block) {
    const int32_t vb = bns_block_vectors(s, block);
    return bns_steps(s.slab_pixels, vb) + bns_partials(s.slab_pixels, vb) + s.slabs;
}

// ... and of a per-channel result: the sum and the at most BNS_FINALISE_OPS fp64 operations of the finalise kernels behind it
// (mean, var and invstd: / M, mean * mean, -, + eps, sqrt, 1 /; dgamma: *, -, *).  Never more than M + 7 + slabs.
constexpr int BNS_FINALISE_OPS = 6;
BNS_HD int64_t bns_chain(const BnSlabs &s, int32_t block) { return bns_sum_chain(s, block) + BNS_FINALISE_OPS; }

// ... and the longest over the blocks (the last block, whose R is the largest, or the first)
BNS_HD int64_t bns_chain_max(const BnSlabs &s) {
    const int64_t a = bns_chain(s, 0), b = bns_chain(s, s.blocks - 1);
    return a > b ? a : b;
}
