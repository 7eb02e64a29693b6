// Instance evaluation of label images on the GPU (gfx950): the pixel pass, the pair table and the greedy matching behind
// celldetection_amd.LabelMatcher (the reference's cd.data.LabelMatcher, celldetection/data/instance_eval.py).
//
// Pixel pass.  Both label images are int32 [pixels][C] (channel-interleaved, as contours2labels writes them).  A pixel
// contributes
//   * one count per ELEMENT > 0 to the area of that label (a value in two channels of a pixel counts twice, like
//     np.unique(..., return_counts=True) over the whole array), and
//   * one count per DISTINCT pair (input label > 0, target label > 0) at that pixel.
// All three kinds of counter live in ONE open-addressing hash table (csrc/label_table.h) in global memory on a 64-bit key:
//   input area  (l << 32) | 0      target area  (0 << 32) | l      pair  (input << 32) | target
// (labels are > 0, so the three ranges cannot collide and key 0 means "empty").  A slot is claimed with a 64-bit
// compare-and-swap and counted with 64-bit integer adds: order-independent, hence reproducible run to run.
// Up to 15 slots (a slot = a channel or a channel pair, e.g. 3 x 3 channels) a thread owns 8 consecutive pixels and reads
// them with dwordx4 loads; per slot it run-lengths its pixels in registers (background in between does not end a run),
// the wave then merges runs of equal keys in neighbouring lanes (segmented suffix sum over shuffles), and one add per
// run reaches the table.  Inside an object that is one add per wave (512 pixels of a row) and slot instead of one per
// pixel; only where two different labels follow each other within a thread's pixels is the first one added directly.
// With more slots (or more than 4 channels a side) a lane owns one pixel and every slot goes through the wave merge at
// once: fewer registers, more waves in flight to hide the table's latency.  An insert that finds no slot within its
// probe limit counts an overflow; the host retries with a table twice the size, nothing is dropped silently.
//
// Matching.  Greedy selection under a strict total order (larger IoU first, compared exactly as i1 * u2 vs i2 * u1; among
// equal IoU the smaller (input, target) pair = the smaller index of the sorted pair list) equals rounds of: every live
// pair bids for both its labels (per-label compare-and-swap maximum), a pair that holds both its labels is taken, pairs
// sharing a label with a taken pair die.  The best live pair is always taken, so every round makes progress.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "label_table.h"

namespace {

constexpr int EV_MAX_C = 8;          // channels supported per side
constexpr int EV_VEC_C = 4;          // up to this many channels per side: kernels for the exact channel counts
constexpr int EV_VEC_SLOTS = 15;     // up to this many slots (CA + CB + CA * CB): vector loads + register run-lengths
constexpr int EV_PPT = 8;            // consecutive pixels per thread in the vector kernels
constexpr int64_t EV_MAX_CAPACITY = (int64_t) 1 << 40;

struct Table {
    u64 *keys, *counts;
    u64 cap;        // a power of two
    u64 *overflow;  // inserts that found no slot
};

__device__ __noinline__ void ev_insert(const Table t, u64 key, u64 n) {
    const i64 h = lt_claim(t.keys, t.cap, key);
    if (h >= 0) atomicAdd(&t.counts[h], n);
    else atomicAdd(t.overflow, 1ull);
}

// All 64 lanes call this together.  Lanes hold (key, n); runs of equal keys in consecutive lanes are summed into the
// run's first lane, which adds them to the table (key 0 = nothing).
__device__ __forceinline__ void ev_wave_flush(const Table &t, u64 key, unsigned n) {
    if (__ballot(key != 0) == 0) return;
    const int lane = __lane_id();
    const u64 prev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || prev != key;
    n = lt_segment_sum(head, n);
    if (head && key != 0 && n != 0) ev_insert(t, key, n);
}

template <int C, int PPT, bool VEC>
__device__ __forceinline__ void ev_load(const int32_t *__restrict__ x, int c_rt, long p0, long n, int32_t (&v)[PPT * C]) {
    if (VEC && p0 + PPT <= n) {
        const int4 *q = reinterpret_cast<const int4 *>(x + p0 * C);  // 32 * C bytes per thread: 16-byte aligned
#pragma unroll
        for (int i = 0; i < PPT * C / 4; ++i) {
            const int4 w = q[i];
            v[4 * i] = w.x; v[4 * i + 1] = w.y; v[4 * i + 2] = w.z; v[4 * i + 3] = w.w;
        }
    } else {
#pragma unroll
        for (int p = 0; p < PPT; ++p)
#pragma unroll
            for (int c = 0; c < C; ++c) v[p * C + c] = (p0 + p < n && c < c_rt) ? x[(p0 + p) * c_rt + c] : 0;
    }
}

// VEC: ca == CA, cb == CB, EV_PPT pixels per thread with run-lengths in registers.  Otherwise CA / CB are upper limits
// (ca <= CA, cb <= CB), one pixel per thread and every slot goes through the wave merge directly.
template <int CA, int CB, bool VEC>
__global__ __launch_bounds__(256) void ev_pixel_kernel(const int32_t *__restrict__ a, int ca, const int32_t *__restrict__ b,
                                                      int cb, long n, Table t) {
    constexpr int PPT = VEC ? EV_PPT : 1;
    constexpr int NS = CA + CB + CA * CB;
    const long p0 = ((long) blockIdx.x * 256 + threadIdx.x) * PPT;  // no early exit: the wave merge needs every lane
    int32_t va[PPT * CA], vb[PPT * CB];
    ev_load<CA, PPT, VEC>(a, ca, p0, n, va);
    ev_load<CB, PPT, VEC>(b, cb, p0, n, vb);
    u64 keys[VEC ? NS : 1];
    unsigned cnts[VEC ? NS : 1];
    if constexpr (VEC) {
#pragma unroll
        for (int s = 0; s < NS; ++s) { keys[s] = 0; cnts[s] = 0; }
    }
    auto upd = [&](int s, u64 k) {
        if constexpr (VEC) {
            if (k == 0) return;  // background keeps the pending key: equal keys merge whether or not their pixels touch
            if (k == keys[s]) {
                ++cnts[s];
            } else {
                if (keys[s] != 0) ev_insert(t, keys[s], cnts[s]);
                keys[s] = k;
                cnts[s] = 1;
            }
        } else {
            ev_wave_flush(t, k, 1);
        }
    };
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
        bool da[CA], db[CB];  // positive and not seen in an earlier channel of this pixel
#pragma unroll
        for (int i = 0; i < CA; ++i) {
            da[i] = va[p * CA + i] > 0;
#pragma unroll
            for (int j = 0; j < i; ++j) da[i] = da[i] && va[p * CA + j] != va[p * CA + i];
        }
#pragma unroll
        for (int i = 0; i < CB; ++i) {
            db[i] = vb[p * CB + i] > 0;
#pragma unroll
            for (int j = 0; j < i; ++j) db[i] = db[i] && vb[p * CB + j] != vb[p * CB + i];
        }
#pragma unroll
        for (int i = 0; i < CA; ++i) upd(i, va[p * CA + i] > 0 ? (u64) (uint32_t) va[p * CA + i] << 32 : 0);
#pragma unroll
        for (int j = 0; j < CB; ++j) upd(CA + j, vb[p * CB + j] > 0 ? (u64) (uint32_t) vb[p * CB + j] : 0);
#pragma unroll
        for (int i = 0; i < CA; ++i)
#pragma unroll
            for (int j = 0; j < CB; ++j)
                upd(CA + CB + i * CB + j,
                    da[i] && db[j] ? ((u64) (uint32_t) va[p * CA + i] << 32) | (uint32_t) vb[p * CB + j] : 0);
    }
    if constexpr (VEC) {
#pragma unroll
        for (int s = 0; s < NS; ++s) ev_wave_flush(t, keys[s], cnts[s]);
    }
}

// table -> compact arrays --------------------------------------------------------------------------------------------
struct KeyCountEmit {  // what lt_compact_kernel writes per occupied slot
    const u64 *__restrict__ counts;
    int64_t *__restrict__ keys_out, *__restrict__ counts_out;
    __device__ void operator()(long pos, long slot, u64 k) const {
        keys_out[pos] = (int64_t) k;
        counts_out[pos] = (int64_t) counts[slot];
    }
};

// pairs -> label positions and unions ---------------------------------------------------------------------------------
__device__ __forceinline__ int ev_find(const int64_t *__restrict__ v, int n, int64_t x) {  // position of x in sorted v, or -1
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < n && v[lo] == x ? lo : -1;
}

__global__ __launch_bounds__(256) void ev_unions_kernel(const int64_t *__restrict__ pair_keys, const int64_t *__restrict__ inter,
                                                       long P, const int64_t *__restrict__ in_labels,
                                                       const int64_t *__restrict__ in_counts, int n_in,
                                                       const int64_t *__restrict__ t_labels,
                                                       const int64_t *__restrict__ t_counts, int n_t,
                                                       int64_t *__restrict__ unions, int32_t *__restrict__ in_idx,
                                                       int32_t *__restrict__ t_idx, u64 *__restrict__ missing) {
    const long p = (long) blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const u64 k = (u64) pair_keys[p];
    const int i = ev_find(in_labels, n_in, (int64_t) (k >> 32)), j = ev_find(t_labels, n_t, (int64_t) (k & 0xffffffffull));
    if (i < 0 || j < 0) {  // cannot happen with a table of this file (every pair's labels have an area entry)
        atomicAdd(missing, 1ull);
        in_idx[p] = 0; t_idx[p] = 0; unions[p] = 0;
        return;
    }
    in_idx[p] = i;
    t_idx[p] = j;
    unions[p] = in_counts[i] + t_counts[j] - inter[p];
}

// greedy selection in rounds ------------------------------------------------------------------------------------------
struct Sel {
    const int64_t *inter, *unions;
    const int32_t *in_idx, *t_idx;
    long P;
    uint8_t *alive, *taken_in, *taken_t, *sel;
    int32_t *best_in, *best_t;
    u64 *counters;  // [0] taken in total, [1] live after the round
};

// strict total order: p before q
__device__ __forceinline__ bool ev_before(const Sel &s, int p, int q) {
    const u64 ip = (u64) s.inter[p], up = (u64) s.unions[p], iq = (u64) s.inter[q], uq = (u64) s.unions[q];
    const u64 l_lo = ip * uq, l_hi = __umul64hi(ip, uq), r_lo = iq * up, r_hi = __umul64hi(iq, up);  // ip / up vs iq / uq
    if (l_hi != r_hi) return l_hi > r_hi;
    if (l_lo != r_lo) return l_lo > r_lo;
    return p < q;
}

__device__ __forceinline__ void ev_bid(const Sel &s, int32_t *slot, int p) {
    int cur = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (cur < 0 || ev_before(s, p, cur)) {  // every failed swap means the slot improved: bounded by the label's pairs
        const int prev = atomicCAS(slot, cur, p);
        if (prev == cur) break;
        cur = prev;
    }
}

__global__ __launch_bounds__(256) void ev_sel_init_kernel(Sel s, double thresh) {
    const long p = (long) blockIdx.x * 256 + threadIdx.x;
    if (p >= s.P) return;
    const double iou = (double) s.inter[p] / (double) s.unions[p];  // int64 / int64 as numpy divides them
    const bool live = s.unions[p] > 0 && iou >= thresh;
    s.alive[p] = live;
    s.sel[p] = 0;
    if (live) atomicAdd(&s.counters[1], 1ull);
}

__global__ __launch_bounds__(256) void ev_sel_bid_kernel(Sel s) {
    const long p = (long) blockIdx.x * 256 + threadIdx.x;
    if (p >= s.P || !s.alive[p]) return;
    ev_bid(s, &s.best_in[s.in_idx[p]], (int) p);
    ev_bid(s, &s.best_t[s.t_idx[p]], (int) p);
}

__global__ __launch_bounds__(256) void ev_sel_take_kernel(Sel s) {
    const long p = (long) blockIdx.x * 256 + threadIdx.x;
    if (p >= s.P || !s.alive[p]) return;
    const int i = s.in_idx[p], j = s.t_idx[p];
    if (s.best_in[i] == (int) p && s.best_t[j] == (int) p) {
        s.sel[p] = 1;
        s.alive[p] = 0;
        s.taken_in[i] = 1;
        s.taken_t[j] = 1;
        atomicAdd(&s.counters[0], 1ull);
    }
}

__global__ __launch_bounds__(256) void ev_sel_prune_kernel(Sel s) {
    const long p = (long) blockIdx.x * 256 + threadIdx.x;
    if (p >= s.P || !s.alive[p]) return;
    const int i = s.in_idx[p], j = s.t_idx[p];
    if (s.taken_in[i] || s.taken_t[j]) {
        s.alive[p] = 0;
    } else {
        s.best_in[i] = -1;  // same value from every writer
        s.best_t[j] = -1;
        atomicAdd(&s.counters[1], 1ull);
    }
}

inline int64_t ev_align(int64_t n) { return (n + 63) & ~(int64_t) 63; }

// Register run-lengths pay while a thread's slots are few: measured on 16384^2 images of 10^5 objects, 2 x 2 channels
// 1.98 ms against 2.89 ms for one pixel per lane, 3 x 3 3.18 against 3.56, but 4 x 4 (24 slots) 5.82 against 4.69.
template <int CA, int CB>
void ev_launch(hipStream_t st, const int32_t *a, const int32_t *b, long n, Table t) {
    if constexpr (CA + CB + CA * CB <= EV_VEC_SLOTS) {
        const unsigned blocks = (unsigned) ((n + 256 * EV_PPT - 1) / (256 * EV_PPT));
        hipLaunchKernelGGL((ev_pixel_kernel<CA, CB, true>), dim3(blocks), dim3(256), 0, st, a, CA, b, CB, n, t);
    } else {
        hipLaunchKernelGGL((ev_pixel_kernel<CA, CB, false>), dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, a, CA, b, CB,
                           n, t);
    }
}

template <int CA>
void ev_launch_cb(int cb, hipStream_t st, const int32_t *a, const int32_t *b, long n, Table t) {
    switch (cb) {
        case 1: ev_launch<CA, 1>(st, a, b, n, t); break;
        case 2: ev_launch<CA, 2>(st, a, b, n, t); break;
        case 3: ev_launch<CA, 3>(st, a, b, n, t); break;
        default: ev_launch<CA, 4>(st, a, b, n, t); break;
    }
}

}  // namespace

extern "C" {

int64_t cpn_eval_workspace_bytes(int64_t table_capacity, int64_t pairs, int64_t labels) {
    if (table_capacity < 0 || pairs < 0 || labels < 0) return 0;
    // table: keys + counts; selection: alive + sel-side flags per pair, best (int32) + taken (u8) per label and side
    return LT_HEAD_BYTES + table_capacity * 16 + ev_align(pairs) + 2 * ev_align(labels * 4) + 2 * ev_align(labels);
}

int cpn_eval_pairs(const int32_t *inputs, int32_t c_in, const int32_t *targets, int32_t c_t, int64_t pixels,
                   int64_t table_capacity, void *workspace, int64_t workspace_bytes, void *stream) {
    if (c_in < 1 || c_t < 1 || pixels < 0 || lt_bad_capacity(table_capacity, EV_MAX_CAPACITY) || !workspace)
        return cpn::fail(CPN_E_INVALID, "cpn_eval_pairs: bad arguments (table_capacity must be a power of two)");
    if (c_in > EV_MAX_C || c_t > EV_MAX_C)
        return cpn::fail(CPN_E_UNSUPPORTED, "cpn_eval_pairs: more than 8 channels per label image");
    if (pixels > 0 && (!inputs || !targets || ((uintptr_t) inputs & 15) || ((uintptr_t) targets & 15)))
        return cpn::fail(CPN_E_INVALID, "cpn_eval_pairs: label images must be 16-byte aligned");
    if (workspace_bytes < cpn_eval_workspace_bytes(table_capacity, 0, 0))
        return cpn::fail(CPN_E_WORKSPACE, "cpn_eval_pairs: workspace too small");
    hipStream_t st = (hipStream_t) stream;
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t) (LT_HEAD_BYTES + table_capacity * 16), st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_eval_pairs: memset");
    if (pixels == 0) return 0;
    u64 *head = (u64 *) workspace;
    Table t{lt_keys(workspace), lt_keys(workspace) + table_capacity, (u64) table_capacity, head};
    if (pixels > (int64_t) 0x7fffffff * 256) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_eval_pairs: image too large");
    if (c_in <= EV_VEC_C && c_t <= EV_VEC_C) {
        switch (c_in) {
            case 1: ev_launch_cb<1>(c_t, st, inputs, targets, (long) pixels, t); break;
            case 2: ev_launch_cb<2>(c_t, st, inputs, targets, (long) pixels, t); break;
            case 3: ev_launch_cb<3>(c_t, st, inputs, targets, (long) pixels, t); break;
            default: ev_launch_cb<4>(c_t, st, inputs, targets, (long) pixels, t); break;
        }
    } else {
        hipLaunchKernelGGL((ev_pixel_kernel<EV_MAX_C, EV_MAX_C, false>), dim3((unsigned) ((pixels + 255) / 256)), dim3(256), 0,
                           st, inputs, c_in, targets, c_t, (long) pixels, t);
    }
    return cpn::check_hip(hipGetLastError(), "cpn_eval_pairs");
}

int cpn_eval_table_status(void *workspace, int64_t table_capacity, int64_t *status_host, void *stream) {
    if (!workspace || !status_host || lt_bad_capacity(table_capacity, EV_MAX_CAPACITY))
        return cpn::fail(CPN_E_INVALID, "cpn_eval_table_status: bad arguments");
    return cpn::check_hip(lt_status(workspace, table_capacity, status_host, (hipStream_t) stream), "cpn_eval_table_status");
}

int cpn_eval_compact(void *workspace, int64_t table_capacity, int64_t *keys, int64_t *counts, int64_t entries, void *stream) {
    if (!workspace || table_capacity < 2 || entries < 0 || (entries > 0 && (!keys || !counts)))
        return cpn::fail(CPN_E_INVALID, "cpn_eval_compact: bad arguments");
    if (entries == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    u64 *head = (u64 *) workspace;
    hipError_t e = hipMemsetAsync(head + 2, 0, 8, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_eval_compact: memset");
    hipLaunchKernelGGL(lt_compact_kernel<KeyCountEmit>, dim3(lt_scan_blocks(table_capacity)), dim3(256), 0, st, lt_keys(workspace),
                       (long) table_capacity, head + 2, KeyCountEmit{lt_keys(workspace) + table_capacity, keys, counts},
                       (long) entries);
    return cpn::check_hip(hipGetLastError(), "cpn_eval_compact");
}

int cpn_eval_unions(const int64_t *pair_keys, const int64_t *intersections, int64_t pairs, const int64_t *input_labels,
                    const int64_t *input_counts, int64_t n_inputs, const int64_t *target_labels, const int64_t *target_counts,
                    int64_t n_targets, int64_t *unions, int32_t *input_index, int32_t *target_index, void *workspace,
                    void *stream) {
    if (pairs < 0 || n_inputs < 0 || n_targets < 0 || pairs > 0x7fffffff || n_inputs > 0x7fffffff || n_targets > 0x7fffffff ||
        !workspace)
        return cpn::fail(CPN_E_INVALID, "cpn_eval_unions: bad arguments");
    if (pairs == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    u64 *head = (u64 *) workspace;
    hipError_t e = hipMemsetAsync(head + 3, 0, 8, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_eval_unions: memset");
    hipLaunchKernelGGL(ev_unions_kernel, dim3((unsigned) ((pairs + 255) / 256)), dim3(256), 0, st, pair_keys, intersections,
                       (long) pairs, input_labels, input_counts, (int) n_inputs, target_labels, target_counts, (int) n_targets,
                       unions, input_index, target_index, head + 3);
    e = hipGetLastError();
    u64 missing = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&missing, head + 3, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_eval_unions");
    if (missing) return cpn::fail(CPN_E_INVALID, "cpn_eval_unions: a pair names a label without an area entry");
    return 0;
}

int cpn_eval_select(const int64_t *intersections, const int64_t *unions, const int32_t *input_index, const int32_t *target_index,
                    int64_t pairs, int64_t n_inputs, int64_t n_targets, double iou_thresh, uint8_t *selected, void *workspace,
                    int64_t workspace_bytes, int64_t *result_host, void *stream) {
    if (pairs < 0 || pairs > 0x7fffffff || n_inputs < 0 || n_targets < 0 || !result_host || !workspace)
        return cpn::fail(CPN_E_INVALID, "cpn_eval_select: bad arguments");
    result_host[0] = result_host[1] = 0;
    if (pairs == 0) return 0;
    const int64_t labels = n_inputs > n_targets ? n_inputs : n_targets;
    if (workspace_bytes < cpn_eval_workspace_bytes(0, pairs, labels))
        return cpn::fail(CPN_E_WORKSPACE, "cpn_eval_select: workspace too small");
    hipStream_t st = (hipStream_t) stream;
    char *w = (char *) workspace;
    Sel s;
    s.inter = intersections; s.unions = unions; s.in_idx = input_index; s.t_idx = target_index; s.P = (long) pairs;
    s.sel = selected;
    s.counters = (u64 *) w;
    w += LT_HEAD_BYTES;
    s.alive = (uint8_t *) w;     w += ev_align(pairs);
    s.best_in = (int32_t *) w;   w += ev_align(labels * 4);
    s.best_t = (int32_t *) w;    w += ev_align(labels * 4);
    s.taken_in = (uint8_t *) w;  w += ev_align(labels);
    s.taken_t = (uint8_t *) w;
    hipError_t e = hipMemsetAsync(s.counters, 0, LT_HEAD_BYTES, st);
    if (e == hipSuccess) e = hipMemsetAsync(s.best_in, 0xff, (size_t) (2 * ev_align(labels * 4)), st);
    if (e == hipSuccess) e = hipMemsetAsync(s.taken_in, 0, (size_t) (2 * ev_align(labels)), st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_eval_select: memset");
    const dim3 grid((unsigned) ((pairs + 255) / 256)), block(256);
    hipLaunchKernelGGL(ev_sel_init_kernel, grid, block, 0, st, s, iou_thresh);
    u64 host[2] = {0, 0};
    e = hipMemcpyAsync(host, s.counters, 16, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_eval_select: init");
    int64_t rounds = 0;
    while (host[1] > 0) {
        const u64 live_before = host[1];
        e = hipMemsetAsync(s.counters + 1, 0, 8, st);
        if (e != hipSuccess) return cpn::check_hip(e, "cpn_eval_select: memset");
        hipLaunchKernelGGL(ev_sel_bid_kernel, grid, block, 0, st, s);
        hipLaunchKernelGGL(ev_sel_take_kernel, grid, block, 0, st, s);
        hipLaunchKernelGGL(ev_sel_prune_kernel, grid, block, 0, st, s);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(host, s.counters, 16, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return cpn::check_hip(e, "cpn_eval_select: round");
        ++rounds;
        if (host[1] >= live_before) return cpn::fail(CPN_E_INVALID, "cpn_eval_select: no progress (internal error)");
    }
    result_host[0] = (int64_t) host[0];
    result_host[1] = rounds;
    return 0;
}

}  // extern "C"
