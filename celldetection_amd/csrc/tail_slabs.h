// The partitions of the ReadOut-tail kernels (csrc/readout_tail.hip).  x is [N images][HW pixels][Cin channels]; a pixel of the
// batch is (n, q), q its index inside image n.  Neither partition ever crosses an image: the keep mask is per image, so a workgroup
// has one mask.
//
// Backward: image n is cut into `per_image` slabs of slab_pixels consecutive pixels (the last slab of an image may be partial);
// slab index = n * per_image + (slab of the image).  A workgroup reduces the pixels of its slab in ascending order, 16 per MFMA
// step, in ONE fp32 accumulator per weight-gradient element; the reduce kernel adds the slabs' partial sums in ascending slab
// index, i.e. ascending (n, slab) order, and multiplies by s once.  The bias gradient sums a slab in 8 interleaved chains per
// channel (pixel index inside the slab mod 8, ascending), adds the eight in order, then the slabs in ascending order.
//
// Forward: image n is cut into tiles of 32 consecutive pixels (the last tile of an image may be partial); a workgroup takes
// group_tiles consecutive tiles of one image.
// Integer arithmetic only; compiles for the device and for the host (tests/tail_slabs_host.cpp runs it against brute force under
// sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TLS_HD __host__ __device__ __forceinline__
#else
#define TLS_HD inline
#endif

constexpr int TLS_STEP = 16;         // pixels per MFMA step of the weight gradient (v_mfma_f32_32x32x16_bf16)
constexpr int TLS_TILE = 32;         // pixels per forward tile (the lanes of one MFMA column index)
constexpr int TLS_BIAS_LANES = 8;    // the bias gradient's slab sum: 8 interleaved chains per channel
constexpr int TLS_MIN_SLAB = 64;     // auto partition: no slab below this many pixels unless the image is smaller

struct TailSlabs {
    int32_t N;            // images
    int64_t HW;           // pixels per image
    int64_t slab_pixels;  // pixels per slab (1 ... HW)
    int64_t per_image;    // slabs per image = ceil(HW / slab_pixels)
    int64_t slabs;        // N * per_image
    int64_t steps;        // MFMA steps of the largest (= first) slab: ceil(slab_pixels / 16)
};

TLS_HD int64_t tls_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// requested: pixels per slab, 0 = auto: about slabs_wanted >= 1 slabs over the batch, of equal size inside an image, a multiple of
// 64 pixels.  Needs N >= 1, HW >= 1, N * HW <= 2^31 - 1.
TLS_HD TailSlabs tls_partition(int32_t N, int64_t HW, int64_t requested, int64_t slabs_wanted) {
    TailSlabs s;
    s.N = N;
    s.HW = HW;
    int64_t sp;
    if (requested > 0) {
        sp = requested;
    } else {
        const int64_t per = tls_ceil_div(slabs_wanted < 1 ? 1 : slabs_wanted, N);
        sp = tls_ceil_div(tls_ceil_div(HW, per), TLS_MIN_SLAB) * TLS_MIN_SLAB;
    }
    if (sp > HW) sp = HW;
    s.slab_pixels = sp;
    s.per_image = tls_ceil_div(HW, sp);
    s.slabs = s.per_image * N;
    s.steps = tls_ceil_div(sp, TLS_STEP);
    return s;
}

// slab `slab` (0 <= slab < slabs) -> its image and its pixel range [q0, q1) inside that image
TLS_HD void tls_range(const TailSlabs &s, int64_t slab, int32_t *n, int64_t *q0, int64_t *q1) {
    *n = (int32_t) (slab / s.per_image);
    *q0 = (slab - (int64_t) *n * s.per_image) * s.slab_pixels;
    const int64_t e = *q0 + s.slab_pixels;
    *q1 = e > s.HW ? s.HW : e;
}

// MFMA steps of a slab of `pixels` pixels
TLS_HD int64_t tls_steps(int64_t pixels) { return tls_ceil_div(pixels, TLS_STEP); }

// adds of the reduce kernel per weight-gradient element: one per slab (a slab of an image whose channel was dropped is multiplied
// by 0, exactly), and the one multiplication by s
TLS_HD int64_t tls_reduce_chain(const TailSlabs &s) { return s.slabs + 1; }

// length of the fp32 chain of one weight-gradient element: the MFMA steps of a slab, + 2 for the MFMA-internal sum, + the reduce
TLS_HD int64_t tls_chain(const TailSlabs &s) { return s.steps + 2 + tls_reduce_chain(s); }

// ... and of one bias-gradient element: ceil(slab pixels / 8) adds per interleaved chain, 8 adds across them, one per slab
TLS_HD int64_t tls_bias_chain(const TailSlabs &s) {
    return tls_ceil_div(s.slab_pixels, TLS_BIAS_LANES) + TLS_BIAS_LANES + s.slabs;
}

// ... and of one forward output: one MFMA step per 16 input channels, + 2 for the MFMA-internal sum (the fma with s and the bias
// and the rounding to the output dtype come on top)
TLS_HD int64_t tls_forward_chain(int32_t cin) { return cin / 16 + 2; }

// ---- forward tiles
struct TailTiles {
    int64_t per_image;    // tiles per image = ceil(HW / 32)
    int64_t group_tiles;  // tiles per workgroup (>= 1)
    int64_t groups;       // workgroups per image = ceil(per_image / group_tiles)
};

// about groups_wanted workgroups over the batch, each a multiple of 4 tiles (one per wave)
TLS_HD TailTiles tls_tiles(int32_t N, int64_t HW, int64_t groups_wanted) {
    TailTiles t;
    t.per_image = tls_ceil_div(HW, TLS_TILE);
    const int64_t per = tls_ceil_div(groups_wanted < 1 ? 1 : groups_wanted, N);
    t.group_tiles = tls_ceil_div(tls_ceil_div(t.per_image, per), 4) * 4;
    t.groups = tls_ceil_div(t.per_image, t.group_tiles);
    return t;
}

// workgroup `group` (0 <= group < N * groups) -> its image and its tile range [t0, t1) inside that image; tile t holds the pixels
// [32 t, min(32 t + 32, HW))
TLS_HD void tls_tile_range(const TailTiles &t, int64_t group, int32_t *n, int64_t *t0, int64_t *t1) {
    *n = (int32_t) (group / t.groups);
    *t0 = (group - (int64_t) *n * t.groups) * t.group_tiles;
    const int64_t e = *t0 + t.group_tiles;
    *t1 = e > t.per_image ? t.per_image : e;
}
