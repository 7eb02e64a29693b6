// Component labelling on the GPU (gfx950): the kernels behind celldetection_amd.label_components / relabel_ / stack_labels /
// masks2labels (the reference's cd.data.relabel_, stack_labels, celldetection/data/segmentation.py:106-150, and cd.data.masks2labels,
// data/cpn.py:147-176).  The rule is the "Component labelling" section of include/cpn_hip.h.
//
// Components: the shared pass of csrc/components.h (tile union-find in LDS, seams with agent-scope atomicMin, flattening) in the
// instantiation for the call's connectivity and mode.  It leaves roots = int32 [C][H][W]: -1 where the pixel takes no part,
// otherwise the index y * W + x of the raster-first pixel of the pixel's component.  A ROOT is a pixel whose word is its own
// index.  The linear order of the roots image is channel ascending, then raster index: the numbering order.
//
// Numbering (no scan over a per-pixel flag array; a BLOCK is 256 consecutive pixels of one channel, csrc/component_rank.h):
//   cn_count_kernel:  the roots of every block: one ballot per wave, popcounts summed.  8 B per 256 pixels.
//   rocprim:          one exclusive scan over the block counts, 64-bit sums; the entry after the last block is the total.
//   cn_rank_kernel:   the same ballots again; a root's rank = its block's base + the roots before it in the block, stored in the
//                     root's own word as -2 - rank.  Only the thread of a root reads or writes a root word in this launch.
//   cn_counts_kernel: components per channel = the difference of two block bases.
//   cn_label_kernel:  every element of the output, in the image's own layout: a pixel that takes no part keeps its value (copied
//                     when out is another buffer, not touched in place); every other pixel reads its root's word (its own when
//                     it is the root) and gets first + rank.  Each input pixel is read at most once.
// The total is read back between the scan and the ranks (the one synchronisation): above 2^31 - 1, or with first + total - 1 above
// it, the call fails and no label is written.  Integers only, no value-carrying atomics (the atomicMin of the seams carries
// indices whose minimum does not depend on the order; the root counter of the flattening pass is a cross-check only): results
// are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <rocprim/device/device_scan.hpp>

#include "../../include/cpn_hip.h"
#include "component_rank.h"
#include "components.h"
#include "cpn_error.h"

namespace {

typedef unsigned long long u64;
static_assert(sizeof(u64) == sizeof(uint64_t), "ballots are 64 bits");

constexpr int CN_COUNTERS = 8;  // u64 each: [0] roots (flattening pass)

__device__ __forceinline__ bool cn_ballots(const int32_t *__restrict__ L, long p, long HW, uint64_t *ballots) {
    const bool root = p < HW && L[p] == (int32_t) p;
    const uint64_t m = __ballot(root);
    if ((threadIdx.x & 63) == 0) ballots[threadIdx.x >> 6] = m;
    __syncthreads();
    return root;
}

__global__ __launch_bounds__(CR_BLOCK) void cn_count_kernel(long HW, const int32_t *__restrict__ roots, long blocks_per_channel,
                                                           u64 *__restrict__ block_counts) {
    __shared__ uint64_t ballots[CR_WAVES];
    const long p = (long) blockIdx.x * CR_BLOCK + threadIdx.x;
    cn_ballots(roots + (long) blockIdx.y * HW, p, HW, ballots);
    if (threadIdx.x == 0) block_counts[(long) blockIdx.y * blocks_per_channel + blockIdx.x] = (u64) cr_block_count(ballots);
}

__global__ __launch_bounds__(CR_BLOCK) void cn_rank_kernel(long HW, int32_t *roots, long blocks_per_channel,
                                                          const u64 *__restrict__ block_base) {
    __shared__ uint64_t ballots[CR_WAVES];
    const long p = (long) blockIdx.x * CR_BLOCK + threadIdx.x;
    int32_t *L = roots + (long) blockIdx.y * HW;
    if (!cn_ballots(L, p, HW, ballots)) return;  // (after the barrier)
    const u64 base = block_base[(long) blockIdx.y * blocks_per_channel + blockIdx.x];
    L[p] = cr_encode((int64_t) base + cr_block_rank(ballots, (int) threadIdx.x));
}

__global__ __launch_bounds__(256) void cn_counts_kernel(const u64 *__restrict__ block_base, long blocks_per_channel, int C,
                                                       int32_t *__restrict__ counts) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    counts[c] = (int32_t) (block_base[(long) (c + 1) * blocks_per_channel] - block_base[(long) c * blocks_per_channel]);
}

// PLANAR: one thread per pixel of a channel plane (the fastest axis of a [N][H][W] stack); otherwise one thread per element of
// the channel-interleaved image.  in and out may be the same buffer (then with the same strides).
template <bool PLANAR>
__global__ __launch_bounds__(256) void cn_label_kernel(const int32_t *in, long pixel_stride, long channel_stride, int32_t *out,
                                                      long out_pixel_stride, long out_channel_stride, int C, long HW,
                                                      const int32_t *__restrict__ roots, int32_t first) {
    long p;
    int c;
    if (PLANAR) {
        p = (long) blockIdx.x * 256 + threadIdx.x;
        c = blockIdx.y;
        if (p >= HW) return;
    } else {
        const long e = (long) blockIdx.x * 256 + threadIdx.x;
        if (e >= HW * C) return;
        p = e / C;
        c = (int) (e - p * C);
    }
    const int32_t *L = roots + (long) c * HW;
    const int32_t *src = in + p * pixel_stride + (long) c * channel_stride;
    int32_t *dst = out + p * out_pixel_stride + (long) c * out_channel_stride;
    int32_t r = L[p];
    if (r == -1) {
        if (dst != src) *dst = *src;
        return;
    }
    if (r >= 0) r = L[r];  // the root's word: -2 - rank
    *dst = (int32_t) ((int64_t) first + cr_decode(r));
}

inline size_t cn_align(size_t n) { return (n + 255) & ~(size_t) 255; }

struct Layout {
    size_t counters, roots, block_counts, block_base, tmp, tmp_bytes, total;
    long blocks_per_channel, blocks;
};

// 0 < channels <= 65535, H, W >= 0, H * W <= 2^31 - 1 and channels * ceil(H * W / 256) <= 2^31 - 2 are checked by the caller
Layout cn_layout(int32_t C, int32_t H, int32_t W) {
    Layout l{};
    const long HW = (long) H * W;
    l.blocks_per_channel = (HW + CR_BLOCK - 1) / CR_BLOCK;
    l.blocks = l.blocks_per_channel * C;
    const size_t n = (size_t) l.blocks + 1;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = cn_align(o + bytes); return at; };
    l.counters = take(CN_COUNTERS * 8);
    l.roots = take((size_t) HW * C * 4);
    l.block_counts = take(n * 8);
    l.block_base = take(n * 8);
    (void) rocprim::exclusive_scan(nullptr, l.tmp_bytes, (u64 *) nullptr, (u64 *) nullptr, (u64) 0, n, rocprim::plus<u64>(),
                                   (hipStream_t) 0);
    l.tmp = take(l.tmp_bytes);
    l.total = o;
    return l;
}

// 0, or the error code with its message recorded
int cn_check_image(const char *who, int32_t C, int32_t H, int32_t W) {
    if (C < 1 || C > 65535 || H < 0 || W < 0) return cpn::fail(CPN_E_INVALID, who);
    const int64_t HW = (int64_t) H * W;
    if (HW > 0x7fffffff) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_components: more than 2^31 - 1 pixels");
    if ((HW + CR_BLOCK - 1) / CR_BLOCK * C > 0x7ffffffe)
        return cpn::fail(CPN_E_UNSUPPORTED, "cpn_components: more than 2^31 - 2 blocks of 256 pixels");
    return 0;
}

// the layouts the kernels index without overlap: channel-interleaved (channel_stride 1, pixel_stride >= channels) or planar
// (pixel_stride 1, channel_stride >= H * W)
bool cn_strides_ok(int64_t ps, int64_t cs, int32_t C, int64_t HW) {
    return (cs == 1 && ps >= C) || (ps == 1 && cs >= HW);
}

template <int CONN>
hipError_t cn_pass(int32_t mode, const int32_t *in, long ps, long cs, int C, int H, int W, int32_t *roots, u64 *counters,
                   hipStream_t st) {
    return mode == CPN_COMPONENTS_NONZERO ? cc_components_pass<CONN, CC_NONZERO>(in, ps, cs, C, H, W, roots, counters, st)
                                          : cc_components_pass<CONN, CC_EQUAL>(in, ps, cs, C, H, W, roots, counters, st);
}

}  // namespace

extern "C" {

int64_t cpn_components_workspace_bytes(int32_t channels, int32_t H, int32_t W) {
    if (channels < 1 || channels > 65535 || H < 0 || W < 0 || (int64_t) H * W > 0x7fffffff) return 0;
    if (((int64_t) H * W + CR_BLOCK - 1) / CR_BLOCK * channels > 0x7ffffffe) return 0;
    return (int64_t) cn_layout(channels, H, W).total;
}

int cpn_components_label(const int32_t *in, int64_t pixel_stride, int64_t channel_stride, int32_t channels, int32_t H, int32_t W,
                         int32_t connectivity, int32_t mode, int32_t first, int32_t *out, int64_t out_pixel_stride,
                         int64_t out_channel_stride, int32_t *counts, void *workspace, void *stream) {
    if (const int rc = cn_check_image("cpn_components_label: bad arguments", channels, H, W)) return rc;
    if (connectivity != 4 && connectivity != 8) return cpn::fail(CPN_E_INVALID, "cpn_components_label: connectivity must be 4 or 8");
    if (mode != CPN_COMPONENTS_EQUAL && mode != CPN_COMPONENTS_NONZERO)
        return cpn::fail(CPN_E_INVALID, "cpn_components_label: mode must be CPN_COMPONENTS_EQUAL or CPN_COMPONENTS_NONZERO");
    if (first < 1) return cpn::fail(CPN_E_INVALID, "cpn_components_label: first must be at least 1");
    const long HW = (long) H * W;
    if (!cn_strides_ok(pixel_stride, channel_stride, channels, HW) || !cn_strides_ok(out_pixel_stride, out_channel_stride, channels, HW))
        return cpn::fail(CPN_E_INVALID, "cpn_components_label: strides must be channel-interleaved (channel stride 1, pixel stride "
                                        ">= channels) or planar (pixel stride 1, channel stride >= H * W)");
    if (!counts || !workspace) return cpn::fail(CPN_E_INVALID, "cpn_components_label: null pointer");
    hipStream_t st = (hipStream_t) stream;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t) channels * 4, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_components_label: memset");
    if (HW == 0) return 0;
    if (!in || !out) return cpn::fail(CPN_E_INVALID, "cpn_components_label: no image");
    if (in == out && (pixel_stride != out_pixel_stride || channel_stride != out_channel_stride))
        return cpn::fail(CPN_E_INVALID, "cpn_components_label: in place needs the same strides for in and out");
    const Layout l = cn_layout(channels, H, W);
    char *ws = (char *) workspace;
    u64 *counters = (u64 *) (ws + l.counters);
    int32_t *roots = (int32_t *) (ws + l.roots);
    u64 *block_counts = (u64 *) (ws + l.block_counts), *block_base = (u64 *) (ws + l.block_base);
    e = hipMemsetAsync(counters, 0, CN_COUNTERS * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(block_counts + l.blocks, 0, 8, st);  // the entry after the last block
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_components_label: memset");
    e = connectivity == 8 ? cn_pass<8>(mode, in, pixel_stride, channel_stride, channels, H, W, roots, counters, st)
                          : cn_pass<4>(mode, in, pixel_stride, channel_stride, channels, H, W, roots, counters, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_components_label: components");
    const dim3 planes((unsigned) l.blocks_per_channel, (unsigned) channels);
    hipLaunchKernelGGL(cn_count_kernel, planes, dim3(CR_BLOCK), 0, st, HW, roots, l.blocks_per_channel, block_counts);
    size_t tmp = l.tmp_bytes;
    e = rocprim::exclusive_scan(ws + l.tmp, tmp, block_counts, block_base, (u64) 0, (size_t) l.blocks + 1, rocprim::plus<u64>(), st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_components_label: scan");
    u64 host[CN_COUNTERS], total = 0;
    e = hipMemcpyAsync(&total, block_base + l.blocks, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(host, counters, CN_COUNTERS * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_components_label: status");
    if (total != host[0]) return cpn::fail(CPN_E_INTERNAL, "cpn_components_label: the block counts do not add up to the root count");
    if (total > 0x7fffffffull) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_components_label: more than 2^31 - 1 components");
    if ((int64_t) first + (int64_t) total - 1 > 0x7fffffffll)
        return cpn::fail(CPN_E_UNSUPPORTED, "cpn_components_label: first + components - 1 does not fit int32");
    hipLaunchKernelGGL(cn_rank_kernel, planes, dim3(CR_BLOCK), 0, st, HW, roots, l.blocks_per_channel, block_base);
    hipLaunchKernelGGL(cn_counts_kernel, dim3((unsigned) ((channels + 255) / 256)), dim3(256), 0, st, block_base,
                       l.blocks_per_channel, channels, counts);
    if (pixel_stride == 1)
        hipLaunchKernelGGL(cn_label_kernel<true>, planes, dim3(256), 0, st, in, (long) pixel_stride, (long) channel_stride, out,
                           (long) out_pixel_stride, (long) out_channel_stride, channels, HW, roots, first);
    else
        hipLaunchKernelGGL(cn_label_kernel<false>, dim3((unsigned) ((HW * channels + 255) / 256)), dim3(256), 0, st, in,
                           (long) pixel_stride, (long) channel_stride, out, (long) out_pixel_stride, (long) out_channel_stride,
                           channels, HW, roots, first);
    return cpn::check_hip(hipGetLastError(), "cpn_components_label");
}

}  // extern "C"
