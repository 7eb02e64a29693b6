// Connected components of label images on the GPU (gfx950): the pass that csrc/label_contours.hip (labels2contours) and
// csrc/components.hip (label_components / relabel_ / masks2labels) share.  Every kernel lives in an unnamed namespace: each
// translation unit that includes this file gets instantiations of its own.
//
// Rule (include/cpn_hip.h, "Component labelling").  A pixel takes part if it is foreground; two neighbouring foreground pixels are
// linked if they are equal.  CC_EQUAL: foreground is v > 0, equal is the same value.  CC_NONZERO: foreground is v != 0 and any two
// foreground pixels are equal (the tile kernel and the seam kernel read such an image as v != 0 ? 1 : 0 and go on as CC_EQUAL).
// CONN = 8: the 8 neighbours; CONN = 4: the 4 edge neighbours.
//
// The image is read through explicit strides, element (y, x, c) at labels[(y * W + x) * pixel_stride + c * channel_stride]: the
// channel-interleaved [H][W][C] image is (C, 1), a [N][H][W] mask stack is (1, H * W).  roots = int32 [C][H][W].
//   cc_local_kernel:   a workgroup owns a 32 x 32 tile of one channel and runs a union-find in LDS (8 KiB: the 32-wave limit of a
//                      CU is reached before its LDS) over the links of every pixel to its W and N neighbour, and for CONN = 8 to
//                      its NW and NE neighbour (those that follow from other pixels' links left out); it writes the image index
//                      (y * W + x) of the pixel's local root, -1 for a pixel that takes no part.
//   cc_seam_kernel:    one thread per pixel of a tile's first column or first row links it to its neighbours in the tile to the
//                      left or above: the pixel directly across the seam, and for CONN = 8 the two diagonal ones.  Every access
//                      to a parent word in this launch is an agent-scope atomic (relaxed loads, atomicMin): no plain load reads a
//                      word that another workgroup writes, and no workgroup waits for another.  A stale parent is still an
//                      ancestor, so freshness is not needed for correctness, atomicity is.
//   cc_flatten_kernel: every pixel follows its chain to the root and stores it (atomic loads and stores again: chains are shortened
//                      under the readers, and either value is an ancestor); root words are never written.  Counts the roots.
// The larger index is always linked under the smaller (atomicMin on the parent word), so parent <= self everywhere, every chain
// strictly decreases (the bound of every find loop), a union either ends or continues with a strictly smaller maximum of its two
// indices (the bound of the union loop), and the root of a component is its smallest image index: its raster-first pixel.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/cpn_hip.h"

namespace {

typedef unsigned long long cc_u64;

constexpr int CC_T = CPN_CONTOURS_TILE, CC_SHIFT = 5;
static_assert((1 << CC_SHIFT) == CC_T && CC_T * CC_T == 1024, "tile geometry: 256 threads own 4 pixels each");
constexpr int CC_EQUAL = CPN_COMPONENTS_EQUAL, CC_NONZERO = CPN_COMPONENTS_NONZERO;

constexpr int SCOPE_WG = __HIP_MEMORY_SCOPE_WORKGROUP, SCOPE_AGENT = __HIP_MEMORY_SCOPE_AGENT;

// the value the union-find sees: > 0 takes part, equal values link
template <int MODE>
__device__ __forceinline__ int32_t cc_value(int32_t v) {
    return MODE == CC_NONZERO ? (int32_t) (v != 0) : v;
}

// parent <= self: the chain strictly decreases, so the loop ends after at most x steps
template <int SCOPE>
__device__ __forceinline__ int uf_find(int *L, int x) {
    for (;;) {
        const int p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, SCOPE);
        if (p >= x || p < 0) return x;
        x = p;
    }
}

// links the trees of a and b: the larger root under the smaller.  max(a, b) strictly decreases from one round to the next.
template <int SCOPE>
__device__ __forceinline__ void uf_union(int *L, int a, int b) {
    for (;;) {
        a = uf_find<SCOPE>(L, a);
        b = uf_find<SCOPE>(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old >= a || old < 0) return;  // a was a root and now hangs under b
        a = old;                           // a had been linked under old < a meanwhile: go on with (old, b)
    }
}

template <int CONN, int MODE>
__global__ __launch_bounds__(256) void cc_local_kernel(const int32_t *__restrict__ labels, long pixel_stride, long channel_stride,
                                                      int H, int W, int tiles_x, long HW, int32_t *__restrict__ roots) {
    __shared__ int32_t val[CC_T * CC_T];
    __shared__ int par[CC_T * CC_T];
    const int c = blockIdx.y, tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * CC_T, x0 = tx * CC_T, tid = threadIdx.x;
    const int32_t *in = labels + (long) c * channel_stride;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + 256 * k, y = y0 + (i >> CC_SHIFT), x = x0 + (i & (CC_T - 1));
        const int32_t v = y < H && x < W ? cc_value<MODE>(in[((long) y * W + x) * pixel_stride]) : 0;
        val[i] = v;
        par[i] = v > 0 ? i : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + 256 * k, ly = i >> CC_SHIFT, lx = i & (CC_T - 1);
        const int32_t v = val[i];
        if (v <= 0) continue;
        // links that other pixels make are left out: with N equal, NW - N and N - NE are W links of N and NE; with W equal,
        // NW - W is the N link of W
        const bool w_eq = lx > 0 && val[i - 1] == v, n_eq = ly > 0 && val[i - CC_T] == v;
        if (w_eq) uf_union<SCOPE_WG>(par, i, i - 1);
        if (n_eq) uf_union<SCOPE_WG>(par, i, i - CC_T);
        if (CONN == 8 && ly > 0 && !n_eq) {
            if (lx > 0 && !w_eq && val[i - CC_T - 1] == v) uf_union<SCOPE_WG>(par, i, i - CC_T - 1);
            if (lx < CC_T - 1 && val[i - CC_T + 1] == v) uf_union<SCOPE_WG>(par, i, i - CC_T + 1);
        }
    }
    __syncthreads();
    int32_t *out = roots + (long) c * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + 256 * k, y = y0 + (i >> CC_SHIFT), x = x0 + (i & (CC_T - 1));
        if (y < H && x < W) {
            int r = -1;
            if (val[i] > 0) {
                const int l = uf_find<SCOPE_WG>(par, i);
                r = (y0 + (l >> CC_SHIFT)) * W + x0 + (l & (CC_T - 1));
            }
            out[(long) y * W + x] = r;
        }
    }
}

// seam pixels: first the (tiles_x - 1) * H pixels of the tiles' first columns, then the (tiles_y - 1) * W of their first rows
template <int CONN, int MODE>
__global__ __launch_bounds__(256) void cc_seam_kernel(const int32_t *__restrict__ labels, long pixel_stride, long channel_stride,
                                                     int H, int W, int tiles_x, long n_col, long n_seam, long HW, int32_t *roots) {
    const long i = (long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n_seam) return;
    const int c = blockIdx.y;
    int x, y, dxs, dys;  // the neighbours: (x - 1, y + k) for a column pixel, (x + k, y - 1) for a row pixel; k = -1, 0, 1 (CONN 4: 0)
    if (i < n_col) {
        x = (int) (i / H + 1) * CC_T;
        y = (int) (i % H);
        dxs = 0; dys = 1;
    } else {
        const long j = i - n_col;
        y = (int) (j / W + 1) * CC_T;
        x = (int) (j % W);
        dxs = 1; dys = 0;
    }
    const int32_t *in = labels + (long) c * channel_stride;
    const int32_t v = cc_value<MODE>(in[((long) y * W + x) * pixel_stride]);
    if (v <= 0) return;
    int *L = roots + (long) c * HW;
    constexpr int K = CONN == 8 ? 1 : 0;
    for (int k = -K; k <= K; ++k) {
        const int xx = dys ? x - 1 : x + k * dxs, yy = dys ? y + k : y - 1;
        if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
        if (cc_value<MODE>(in[((long) yy * W + xx) * pixel_stride]) == v) uf_union<SCOPE_AGENT>(L, y * W + x, yy * W + xx);
    }
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(long HW, int32_t *roots, cc_u64 *__restrict__ counters) {
    const long p = (long) blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    int *L = roots + (long) blockIdx.y * HW;
    const int first = __hip_atomic_load(L + p, __ATOMIC_RELAXED, SCOPE_AGENT);
    if (first < 0) return;
    if (first == (int) p) {
        atomicAdd(&counters[0], (cc_u64) 1);  // (one add per wave: the compiler merges the lanes)
        return;
    }
    const int r = uf_find<SCOPE_AGENT>(L, first);
    if (r != first) __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, SCOPE_AGENT);
}

// The three launches on `st`.  channels <= 65535 and 0 < H * W <= 2^31 - 1 are the caller's checks; counters[0] (zeroed by the
// caller) receives the number of roots.
template <int CONN, int MODE>
inline hipError_t cc_components_pass(const int32_t *labels, long pixel_stride, long channel_stride, int channels, int H, int W,
                                     int32_t *roots, cc_u64 *counters, hipStream_t st) {
    const long HW = (long) H * W;
    const int tiles_x = (W + CC_T - 1) >> CC_SHIFT, tiles_y = (H + CC_T - 1) >> CC_SHIFT;
    const long tiles = (long) tiles_x * tiles_y;
    hipLaunchKernelGGL((cc_local_kernel<CONN, MODE>), dim3((unsigned) tiles, (unsigned) channels), dim3(256), 0, st, labels,
                       pixel_stride, channel_stride, H, W, tiles_x, HW, roots);
    const long n_col = (long) (tiles_x - 1) * H, n_seam = n_col + (long) (tiles_y - 1) * W;
    if (n_seam > 0)
        hipLaunchKernelGGL((cc_seam_kernel<CONN, MODE>), dim3((unsigned) ((n_seam + 255) / 256), (unsigned) channels), dim3(256), 0,
                           st, labels, pixel_stride, channel_stride, H, W, tiles_x, n_col, n_seam, HW, roots);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned) ((HW + 255) / 256), (unsigned) channels), dim3(256), 0, st, HW, roots,
                       counters);
    return hipGetLastError();
}

}  // namespace
