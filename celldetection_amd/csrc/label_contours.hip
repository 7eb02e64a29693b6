// Contours of label images on the GPU (gfx950): the kernels behind celldetection_amd.labels2contours / resample_contours (the
// reference's cd.data.labels2contours, celldetection/data/cpn.py:93-144, and cd.data.resample_contours, data/misc.py:371-405).
//
// Rule.  An OBJECT is a pair (channel, value v > 0) of the int32 [H][W][C] image; values <= 0 take no part.  Its COMPONENTS are
// the 8-connected sets of pixels of that channel that hold v.  An object with exactly one component yields one contour, the
// outer border of that component followed by the rule of csrc/contour_trace.h from its raster-first pixel, as (x, y) in image
// coordinates.  An object with more than one component is FRAGMENTED and yields nothing.  A component that lies in a hole of
// another component of the same value counts as a component (cv2.findContours(RETR_EXTERNAL) would not see it).  Contours are
// returned by ascending value; of a value that is unfragmented in several channels the highest channel is returned.
//
// Components (csrc/components.h, shared with csrc/components.hip; three launches, all channels at once; roots = int32 [C][H][W],
// 4 B per pixel and channel): the 8-connected equal-value instantiation of the tile union-find, the seam merge with agent-scope
// atomicMin and the flattening pass.  parent <= self everywhere and the root of a component is its smallest image index: its
// raster-first pixel, where the border following has to start.
//
// Object table (cpn_contours_table).  lc_compact_kernel gives every root a slot (key = value << 32 | channel, root) and replaces
// the root's own word by -2 - slot; lc_count_kernel counts the pixels per slot (one atomic per wave and slot); rocprim sorts the
// slots by key; runs of equal keys are the fragmented objects; of the unfragmented entries of one value (adjacent in the order,
// found by a binary search for the end of the value) the last one, the highest channel, is selected; two exclusive scans compact.
//
// Trace (lc_trace_kernel<WRITE>, two passes over the same code): pass one counts the points per contour, an inclusive scan gives
// the offsets, pass two writes the points.  It reads the contiguous root image of the object's channel: pixel q belongs to the
// component of root r iff q == r or roots[q] == r.  ONE LANE PER OBJECT: a very long contour runs on one lane (a known limit,
// profiles/label_contours.txt).  A trace is capped at 8 x the component's pixel count; reaching the cap (impossible for a
// component) is counted and reported as CPN_E_INTERNAL.  The write pass also checks every index against the contour's length.
//
// Resample (lc_resample_kernel): one wave per contour, fp64, the reference's order, no contraction: dt = sqrt(dx^2 + dy^2) +
// epsilon; the running sum of dt sequentially in index order by one lane (numpy's cumsum rounding); then, parallel over the
// samples, t_j = j * (total / num), the first i with t_j <= cumsum[i] (binary search: cumsum does not decrease), alpha =
// (t_j - cumsum0[i]) / dt[i], p_i * (1 - alpha) + p_{i+1} * alpha.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/cpn_hip.h"
#include "components.h"
#include "contour_trace.h"
#include "cpn_error.h"

namespace {

typedef unsigned long long u64;

constexpr int LC_COUNTERS = 8;  // u64 each: [0] roots, [1] slots given, [2] fragmented entries, [3] traces that reached the cap

__global__ __launch_bounds__(256) void lc_compact_kernel(const int32_t *__restrict__ labels, int C, long HW, int32_t *roots, long n,
                                                        u64 *__restrict__ keys, uint32_t *__restrict__ vals,
                                                        int32_t *__restrict__ slot_root, u64 *__restrict__ counters) {
    const long p = (long) blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int c = blockIdx.y;
    int32_t *L = roots + (long) c * HW;
    if (L[p] != (int) p) return;  // only the thread of a root reads or writes the root's word in this launch
    const u64 slot = atomicAdd(&counters[1], (u64) 1);
    if (slot >= (u64) n) return;
    keys[slot] = (u64) (uint32_t) labels[p * C + c] << 32 | (u64) (uint32_t) c;
    vals[slot] = (uint32_t) slot;
    slot_root[slot] = (int32_t) p;
    L[p] = -2 - (int32_t) slot;
}

__global__ __launch_bounds__(256) void lc_count_kernel(long HW, const int32_t *__restrict__ roots, long n, uint32_t *__restrict__ npix) {
    const long p = (long) blockIdx.x * 256 + threadIdx.x;
    const int32_t *L = roots + (long) blockIdx.y * HW;
    int s = -1;
    if (p < HW) {
        int32_t r = L[p];
        if (r >= 0) r = L[r];  // the root's word: -2 - slot
        if (r <= -2 && -2 - (long) r < n) s = (int) (-2 - (long) r);
    }
    const int lane = __lane_id();
    u64 active = __ballot(s >= 0);
    while (active) {  // one round per distinct slot of the wave: at most 64
        const int leader = __ffsll((long long) active) - 1;
        const int ls = __shfl(s, leader, 64);
        const u64 m = __ballot(s == ls);
        if (lane == leader) atomicAdd(&npix[ls], (uint32_t) __popcll(m));
        active &= ~m;
    }
}

__global__ __launch_bounds__(256) void lc_mark_kernel(const u64 *__restrict__ keys, long n, uint32_t *__restrict__ unfrag,
                                                     int32_t *__restrict__ frag_values, u64 *__restrict__ counters) {
    const long i = (long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = keys[i];
    const bool frag = (i > 0 && keys[i - 1] == k) || (i + 1 < n && keys[i + 1] == k);
    unfrag[i] = !frag;
    frag_values[i] = frag ? (int32_t) (k >> 32) : 0;
    if (frag) atomicAdd(&counters[2], (u64) 1);
}

// unfrag_pos = exclusive scan of unfrag.  Entry i is selected when it is the last unfragmented entry of its value.
__global__ __launch_bounds__(256) void lc_select_kernel(const u64 *__restrict__ keys, long n, const uint32_t *__restrict__ unfrag,
                                                       const uint32_t *__restrict__ unfrag_pos, uint32_t *__restrict__ sel) {
    const long i = (long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t s = 0;
    if (unfrag[i]) {
        const u64 top = keys[i] | 0xffffffffull;
        long lo = i + 1, hi = n;  // the first entry with a key > top: halves a range of at most n, so at most 64 rounds
        while (lo < hi) {
            const long mid = lo + (hi - lo) / 2;
            if (keys[mid] > top) hi = mid; else lo = mid + 1;
        }
        const uint32_t before_end = lo < n ? unfrag_pos[lo] : unfrag_pos[n - 1] + unfrag[n - 1];
        s = before_end == unfrag_pos[i] + 1;
    }
    sel[i] = s;
}

// table = int32 [4][n]: rows value, channel, root, pixel count of the selected entries, in key order
__global__ __launch_bounds__(256) void lc_gather_kernel(const u64 *__restrict__ keys, const uint32_t *__restrict__ vals, long n,
                                                       const uint32_t *__restrict__ sel, const uint32_t *__restrict__ sel_pos,
                                                       const int32_t *__restrict__ slot_root, const uint32_t *__restrict__ npix,
                                                       int32_t *__restrict__ table) {
    const long i = (long) blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !sel[i]) return;
    const long o = sel_pos[i];
    const uint32_t slot = vals[i];
    table[o] = (int32_t) (keys[i] >> 32);
    table[n + o] = (int32_t) (keys[i] & 0xffffffffull);
    table[2 * n + o] = slot_root[slot];
    table[3 * n + o] = (int32_t) npix[slot];
}

template <bool WRITE>
__global__ __launch_bounds__(64) void lc_trace_kernel(const int32_t *__restrict__ roots, long HW, int H, int W, int C, long K,
                                                     const int32_t *__restrict__ chan, const int32_t *__restrict__ root,
                                                     const int32_t *__restrict__ npix, int64_t *__restrict__ lengths,
                                                     const int64_t *__restrict__ offsets, int32_t *__restrict__ points,
                                                     u64 *__restrict__ counters) {
    const long k = (long) blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    const int c = chan[k], r = root[k];
    bool ok = c >= 0 && c < C && r >= 0 && (long) r < HW && npix[k] > 0;
    long n = -1;
    if (ok) {
        const int32_t *L = roots + (long) c * HW;
        auto inside = [=](int x, int y) {
            if (x < 0 || x >= W || y < 0 || y >= H) return false;
            const int q = y * W + x;
            return q == r || L[q] == r;
        };
        const long cap = 8 * (long) npix[k];
        if constexpr (WRITE) {
            const int64_t base = offsets[k], len = offsets[k + 1] - base;
            int32_t *out = points + 2 * base;
            n = ct_trace(r % W, r / W, cap, inside, [=](long i, int x, int y) {
                if (i < len) { out[2 * i] = x; out[2 * i + 1] = y; }
            });
            if (n != len) n = -1;
        } else {
            n = ct_trace(r % W, r / W, cap, inside, [](long, int, int) {});
        }
    }
    if (n < 0) atomicAdd(&counters[3], (u64) 1);
    if constexpr (!WRITE) lengths[k] = n < 0 ? 0 : n;
}

// One wave per contour.  cum = double [offsets[K] + K] scratch: contour k owns cum[offsets[k] + k ..], one word per segment.
__global__ __launch_bounds__(64) void lc_resample_kernel(const double *__restrict__ points, const int64_t *__restrict__ offsets,
                                                        int num, int close, double epsilon, double *__restrict__ cum,
                                                        double *__restrict__ out) {
    const long k = blockIdx.x;
    const int64_t base = offsets[k], n = offsets[k + 1] - base;
    const int64_t segs = close ? n : n - 1;
    if (segs < 1) return;  // (the caller rejects such contours)
    const double *p = points + 2 * base;
    double *cs = cum + base + k;
    auto dt = [=](int64_t i) {
        const int64_t j = i + 1 == n ? 0 : i + 1;
        const double dx = p[2 * j] - p[2 * i], dy = p[2 * j + 1] - p[2 * i + 1];
        return sqrt(dx * dx + dy * dy) + epsilon;
    };
    if (threadIdx.x == 0) {
        double s = 0.;
        for (int64_t i = 0; i < segs; ++i) {  // numpy's cumsum: sequentially, in index order
            s = i == 0 ? dt(0) : s + dt(i);
            cs[i] = s;
        }
    }
    __syncthreads();  // one wave: makes lane 0's stores visible to the others
    const double total = cs[segs - 1];
    const double step = total / (double) num;
    for (int j = threadIdx.x; j < num; j += 64) {
        const double t = (double) j * step;
        int64_t lo = 0, hi = segs - 1;  // the first i with t <= cs[i]; without one (never, for t < total) the last segment
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (t <= cs[mid]) hi = mid; else lo = mid + 1;
        }
        const int64_t i = lo, i1 = i + 1 == n ? 0 : i + 1;
        const double c0 = i == 0 ? 0. : cs[i - 1];
        const double alpha = (t - c0) / dt(i);
        double *o = out + ((long) k * num + j) * 2;
        o[0] = p[2 * i] * (1. - alpha) + p[2 * i1] * alpha;
        o[1] = p[2 * i + 1] * (1. - alpha) + p[2 * i1 + 1] * alpha;
    }
}

inline size_t lc_align(size_t n) { return (n + 255) & ~(size_t) 255; }

struct TableLayout {
    size_t counters, keys_in, keys_out, vals_in, vals_out, slot_root, npix, unfrag, unfrag_pos, sel, sel_pos, tmp, tmp_bytes, total;
};

TableLayout lc_table_layout(int64_t n_in) {
    TableLayout l{};
    const size_t n = n_in > 0 ? (size_t) n_in : 1;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = lc_align(o + bytes); return at; };
    l.counters = take(LC_COUNTERS * 8);
    l.keys_in = take(n * 8); l.keys_out = take(n * 8); l.vals_in = take(n * 4); l.vals_out = take(n * 4);
    l.slot_root = take(n * 4); l.npix = take(n * 4);
    l.unfrag = take(n * 4); l.unfrag_pos = take(n * 4); l.sel = take(n * 4); l.sel_pos = take(n * 4);
    size_t t1 = 0, t2 = 0, t3 = 0;
    (void) rocprim::radix_sort_pairs(nullptr, t1, (u64 *) nullptr, (u64 *) nullptr, (uint32_t *) nullptr, (uint32_t *) nullptr, n, 0,
                                     64, (hipStream_t) 0);
    (void) rocprim::exclusive_scan(nullptr, t2, (uint32_t *) nullptr, (uint32_t *) nullptr, (uint32_t) 0, n,
                                   rocprim::plus<uint32_t>(), (hipStream_t) 0);
    (void) rocprim::inclusive_scan(nullptr, t3, (int64_t *) nullptr, (int64_t *) nullptr, n, rocprim::plus<int64_t>(),
                                   (hipStream_t) 0);
    l.tmp_bytes = t1 > t2 ? t1 : t2;
    if (t3 > l.tmp_bytes) l.tmp_bytes = t3;
    l.tmp = take(l.tmp_bytes);
    l.total = o;
    return l;
}

int lc_check_image(const char *what, int32_t C, int32_t H, int32_t W) {
    if (C < 1 || C > 65535 || H < 0 || W < 0) return cpn::fail(CPN_E_INVALID, what);
    if ((int64_t) H * W > 0x7fffffff) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_contours: more than 2^31 - 1 pixels");
    return 0;
}

int lc_read_counters(const u64 *dev, u64 *host, hipStream_t st, const char *what) {
    hipError_t e = hipMemcpyAsync(host, dev, LC_COUNTERS * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return cpn::check_hip(e, what);
}

}  // namespace

extern "C" {

int64_t cpn_contours_workspace_bytes(int64_t entries) {
    if (entries < 0) return 0;
    return (int64_t) lc_table_layout(entries).total;
}

int cpn_contours_components(const int32_t *labels, int32_t channels, int32_t H, int32_t W, int32_t *roots, void *workspace,
                            int64_t workspace_bytes, int64_t *status_host, void *stream) {
    if (const int rc = lc_check_image("cpn_contours_components: bad arguments", channels, H, W)) return rc;
    if (!workspace || !status_host) return cpn::fail(CPN_E_INVALID, "cpn_contours_components: bad arguments");
    if (workspace_bytes < LC_COUNTERS * 8) return cpn::fail(CPN_E_WORKSPACE, "cpn_contours_components: workspace too small");
    status_host[0] = 0;
    const long HW = (long) H * W;
    if (HW == 0) return 0;
    if (!labels || !roots) return cpn::fail(CPN_E_INVALID, "cpn_contours_components: no image");
    hipStream_t st = (hipStream_t) stream;
    u64 *counters = (u64 *) workspace;
    hipError_t e = hipMemsetAsync(counters, 0, LC_COUNTERS * 8, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_components: memset");
    e = cc_components_pass<8, CC_EQUAL>(labels, channels, 1, channels, H, W, roots, counters, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_components");
    u64 host[LC_COUNTERS];
    if (const int rc = lc_read_counters(counters, host, st, "cpn_contours_components: status")) return rc;
    status_host[0] = (int64_t) host[0];
    return 0;
}

int cpn_contours_table(const int32_t *labels, int32_t channels, int32_t H, int32_t W, int32_t *roots, int64_t entries,
                       int32_t *table, int32_t *frag_values, void *workspace, int64_t workspace_bytes, int64_t *status_host,
                       void *stream) {
    if (const int rc = lc_check_image("cpn_contours_table: bad arguments", channels, H, W)) return rc;
    if (entries < 0 || entries > 0x7fffffff || !workspace || !status_host)
        return cpn::fail(CPN_E_INVALID, "cpn_contours_table: bad arguments");
    status_host[0] = status_host[1] = 0;
    if (entries == 0) return 0;
    if (!labels || !roots || !table || !frag_values) return cpn::fail(CPN_E_INVALID, "cpn_contours_table: null pointer");
    const TableLayout l = lc_table_layout(entries);
    if (workspace_bytes < (int64_t) l.total) return cpn::fail(CPN_E_WORKSPACE, "cpn_contours_table: workspace too small");
    hipStream_t st = (hipStream_t) stream;
    char *ws = (char *) workspace;
    u64 *counters = (u64 *) (ws + l.counters);
    u64 *keys_in = (u64 *) (ws + l.keys_in), *keys = (u64 *) (ws + l.keys_out);
    uint32_t *vals_in = (uint32_t *) (ws + l.vals_in), *vals = (uint32_t *) (ws + l.vals_out);
    int32_t *slot_root = (int32_t *) (ws + l.slot_root);
    uint32_t *npix = (uint32_t *) (ws + l.npix);
    uint32_t *unfrag = (uint32_t *) (ws + l.unfrag), *unfrag_pos = (uint32_t *) (ws + l.unfrag_pos);
    uint32_t *sel = (uint32_t *) (ws + l.sel), *sel_pos = (uint32_t *) (ws + l.sel_pos);
    const long HW = (long) H * W, n = entries;
    hipError_t e = hipMemsetAsync(counters, 0, LC_COUNTERS * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(npix, 0, (size_t) n * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(keys_in, 0xff, (size_t) n * 8, st);  // a slot nobody fills sorts last (never happens)
    if (e == hipSuccess) e = hipMemsetAsync(vals_in, 0, (size_t) n * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(slot_root, 0, (size_t) n * 4, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_table: memset");
    const dim3 pix((unsigned) ((HW + 255) / 256), (unsigned) channels), ent((unsigned) ((n + 255) / 256));
    hipLaunchKernelGGL(lc_compact_kernel, pix, dim3(256), 0, st, labels, channels, HW, roots, n, keys_in, vals_in, slot_root, counters);
    hipLaunchKernelGGL(lc_count_kernel, pix, dim3(256), 0, st, HW, roots, n, npix);
    size_t tmp = l.tmp_bytes;
    e = rocprim::radix_sort_pairs(ws + l.tmp, tmp, keys_in, keys, vals_in, vals, (size_t) n, 0, 64, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_table: sort");
    hipLaunchKernelGGL(lc_mark_kernel, ent, dim3(256), 0, st, keys, n, unfrag, frag_values, counters);
    tmp = l.tmp_bytes;
    e = rocprim::exclusive_scan(ws + l.tmp, tmp, unfrag, unfrag_pos, (uint32_t) 0, (size_t) n, rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_table: scan");
    hipLaunchKernelGGL(lc_select_kernel, ent, dim3(256), 0, st, keys, n, unfrag, unfrag_pos, sel);
    tmp = l.tmp_bytes;
    e = rocprim::exclusive_scan(ws + l.tmp, tmp, sel, sel_pos, (uint32_t) 0, (size_t) n, rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_table: scan");
    hipLaunchKernelGGL(lc_gather_kernel, ent, dim3(256), 0, st, keys, vals, n, sel, sel_pos, slot_root, npix, table);
    e = hipGetLastError();
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_table");
    uint32_t last[2] = {0, 0};
    u64 host[LC_COUNTERS];
    e = hipMemcpyAsync(&last[0], sel_pos + (n - 1), 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&last[1], sel + (n - 1), 4, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_table: status");
    if (const int rc = lc_read_counters(counters, host, st, "cpn_contours_table: status")) return rc;
    if (host[1] != (u64) n) return cpn::fail(CPN_E_INVALID, "cpn_contours_table: entries is not the root count of cpn_contours_components");
    status_host[0] = (int64_t) last[0] + last[1];
    status_host[1] = (int64_t) host[2];
    return 0;
}

int cpn_contours_count(const int32_t *roots, int32_t channels, int32_t H, int32_t W, int64_t K, const int32_t *chan,
                       const int32_t *root, const int32_t *npix, int64_t *lengths, int64_t *offsets, void *workspace,
                       int64_t workspace_bytes, int64_t *status_host, void *stream) {
    if (const int rc = lc_check_image("cpn_contours_count: bad arguments", channels, H, W)) return rc;
    if (K < 0 || K > 0x7fffffff || !offsets || !status_host || !workspace)
        return cpn::fail(CPN_E_INVALID, "cpn_contours_count: bad arguments");
    hipStream_t st = (hipStream_t) stream;
    status_host[0] = 0;
    hipError_t e = hipMemsetAsync(offsets, 0, 8, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_count: memset");
    if (K == 0) return 0;
    if (!roots || !chan || !root || !npix || !lengths) return cpn::fail(CPN_E_INVALID, "cpn_contours_count: null pointer");
    const TableLayout l = lc_table_layout(K);
    if (workspace_bytes < (int64_t) l.total) return cpn::fail(CPN_E_WORKSPACE, "cpn_contours_count: workspace too small");
    char *ws = (char *) workspace;
    u64 *counters = (u64 *) (ws + l.counters);
    e = hipMemsetAsync(counters, 0, LC_COUNTERS * 8, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_count: memset");
    hipLaunchKernelGGL(lc_trace_kernel<false>, dim3((unsigned) ((K + 63) / 64)), dim3(64), 0, st, roots, (long) H * W, H, W,
                       channels, (long) K, chan, root, npix, lengths, (const int64_t *) nullptr, (int32_t *) nullptr, counters);
    size_t tmp = l.tmp_bytes;
    e = rocprim::inclusive_scan(ws + l.tmp, tmp, lengths, offsets + 1, (size_t) K, rocprim::plus<int64_t>(), st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_count: scan");
    int64_t total = 0;
    u64 host[LC_COUNTERS];
    e = hipMemcpyAsync(&total, offsets + K, 8, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_count: status");
    if (const int rc = lc_read_counters(counters, host, st, "cpn_contours_count: status")) return rc;
    if (host[3]) return cpn::fail(CPN_E_INTERNAL, "cpn_contours_count: a trace reached 8 x the pixel count of its component");
    status_host[0] = total;
    return 0;
}

int cpn_contours_write(const int32_t *roots, int32_t channels, int32_t H, int32_t W, int64_t K, const int32_t *chan,
                       const int32_t *root, const int32_t *npix, const int64_t *offsets, int32_t *points, void *workspace,
                       int64_t workspace_bytes, void *stream) {
    if (const int rc = lc_check_image("cpn_contours_write: bad arguments", channels, H, W)) return rc;
    if (K < 0 || K > 0x7fffffff || !workspace) return cpn::fail(CPN_E_INVALID, "cpn_contours_write: bad arguments");
    if (K == 0) return 0;
    if (!roots || !chan || !root || !npix || !offsets || !points) return cpn::fail(CPN_E_INVALID, "cpn_contours_write: null pointer");
    if (workspace_bytes < LC_COUNTERS * 8) return cpn::fail(CPN_E_WORKSPACE, "cpn_contours_write: workspace too small");
    hipStream_t st = (hipStream_t) stream;
    u64 *counters = (u64 *) workspace;
    hipError_t e = hipMemsetAsync(counters, 0, LC_COUNTERS * 8, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_write: memset");
    hipLaunchKernelGGL(lc_trace_kernel<true>, dim3((unsigned) ((K + 63) / 64)), dim3(64), 0, st, roots, (long) H * W, H, W,
                       channels, (long) K, chan, root, npix, (int64_t *) nullptr, offsets, points, counters);
    e = hipGetLastError();
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_contours_write");
    u64 host[LC_COUNTERS];
    if (const int rc = lc_read_counters(counters, host, st, "cpn_contours_write: status")) return rc;
    if (host[3]) return cpn::fail(CPN_E_INTERNAL, "cpn_contours_write: a trace does not have the length that was counted");
    return 0;
}

int cpn_resample_contours(const double *points, const int64_t *offsets, int64_t K, int64_t total_points, int32_t num,
                          int32_t close, double epsilon, double *cumsum, double *out, void *stream) {
    if (K < 0 || K > 0x7fffffff || total_points < 0 || num < 1) return cpn::fail(CPN_E_INVALID, "cpn_resample_contours: bad arguments");
    if (K == 0) return 0;
    if (!points || !offsets || !cumsum || !out) return cpn::fail(CPN_E_INVALID, "cpn_resample_contours: null pointer");
    hipLaunchKernelGGL(lc_resample_kernel, dim3((unsigned) K), dim3(64), 0, (hipStream_t) stream, points, offsets, num, close != 0,
                       epsilon, cumsum, out);
    return cpn::check_hip(hipGetLastError(), "cpn_resample_contours");
}

}  // extern "C"
