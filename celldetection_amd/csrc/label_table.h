// The open-addressing table on a 64-bit key that instance evaluation (csrc/instance_eval.hip) and the region / shape properties
// (csrc/props_table.h, csrc/region_props.hip, csrc/shape_props.hip) share: hash, slot claim in global memory and in LDS,
// read-only lookup, the segmented wave sum that merges equal keys of neighbouring lanes before they reach the table, and the
// passes over a finished table (count, compact, status).  Key 0 means "empty", so a zeroed table is a valid empty table; the
// capacity is a power of two; probing is linear.  What a slot carries next to its key is the caller's.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr u64 LT_MAX_PROBE = 4096;  // probes before a claim gives up (a table of fewer slots: every slot once)
// 64-bit counters in front of a workspace: [0] overflow = claims that found no slot, [1] entries = occupied slots (lt_status),
// [2] cursor of lt_compact_kernel, [3] missing (instance evaluation: pairs that name a label without an area entry)
constexpr int64_t LT_HEAD_BYTES = 64;

__device__ __forceinline__ u64 lt_hash(u64 k) {  // splitmix64 finaliser
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    return k ^ (k >> 31);
}

// The slot of `key` in a table in global memory, claimed if no thread had it yet, or -1 when there is none within the probe
// limit (the caller counts the overflow).
__device__ __forceinline__ i64 lt_claim(u64 *keys, u64 cap, u64 key) {
    const u64 mask = cap - 1;
    u64 h = lt_hash(key) & mask;
    const u64 limit = cap < LT_MAX_PROBE ? cap : LT_MAX_PROBE;
    for (u64 i = 0; i < limit; ++i, h = (h + 1) & mask) {
        u64 cur = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(&keys[h], 0ull, key);
            if (cur == 0) cur = key;
        }
        if (cur == key) return (i64) h;
    }
    return -1;
}

// The same in a table of SLOTS keys in LDS, at most PROBE probes.
template <int SLOTS, int PROBE>
__device__ __forceinline__ int lt_claim_lds(u64 *keys, u64 key) {
    unsigned h = (unsigned) lt_hash(key) & (SLOTS - 1);
    for (int i = 0; i < PROBE; ++i, h = (h + 1) & (SLOTS - 1)) {
        u64 cur = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == 0) {
            cur = atomicCAS(&keys[h], 0ull, key);
            if (cur == 0) cur = key;
        }
        if (cur == key) return (int) h;
    }
    return -1;
}

// The slot of `key`, or -1: read only, for a table that no thread changes any more.
__device__ __forceinline__ i64 lt_lookup(const u64 *__restrict__ keys, u64 cap, u64 key) {
    const u64 mask = cap - 1;
    u64 h = lt_hash(key) & mask;
    const u64 limit = cap < LT_MAX_PROBE ? cap : LT_MAX_PROBE;
    for (u64 i = 0; i < limit; ++i, h = (h + 1) & mask) {
        const u64 cur = keys[h];
        if (cur == key) return (i64) h;
        if (cur == 0) return -1;
    }
    return -1;
}

// All 64 lanes call this together.  `head` marks the first lane of every run of lanes (lane 0 always is one); the head lane
// of a run gets the sum of n over its run, the other lanes a partial sum.
__device__ __forceinline__ unsigned lt_segment_sum(bool head, unsigned n) {
    const int lane = __lane_id();
    const u64 heads = __ballot(head);
    const int seg = __popcll(heads & (~0ull >> (63 - lane)));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned on = __shfl_down(n, d, 64);
        const int oseg = __shfl_down(seg, d, 64);
        if (lane + d < 64 && oseg == seg) n += on;
    }
    return n;
}

// table passes --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lt_count_kernel(const u64 *__restrict__ keys, long cap, u64 *__restrict__ entries) {
    unsigned n = 0;
    for (long i = (long) blockIdx.x * 256 + threadIdx.x; i < cap; i += (long) gridDim.x * 256) n += keys[i] != 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(entries, (u64) n);
}

// Every occupied slot gets a position 0 .. entries - 1 (in no particular order); emit(position, slot, key) writes the caller's
// output for the positions below n_out.
template <class Emit>
__global__ __launch_bounds__(256) void lt_compact_kernel(const u64 *__restrict__ keys, long cap, u64 *__restrict__ cursor, Emit emit,
                                                        long n_out) {
    const int lane = threadIdx.x & 63;
    const long rounds = (cap + (long) gridDim.x * 256 - 1) / ((long) gridDim.x * 256);  // uniform trip count: ballots inside
    for (long r = 0; r < rounds; ++r) {
        const long i = (r * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        const u64 k = i < cap ? keys[i] : 0;
        const u64 m = __ballot(k != 0);
        if (m == 0) continue;
        u64 base = 0;
        if (lane == 0) base = atomicAdd(cursor, (u64) __popcll(m));
        base = __shfl(base, 0, 64);
        if (k != 0) {
            const long pos = (long) base + __popcll(m & ((1ull << lane) - 1));
            if (pos < n_out) emit(pos, i, k);
        }
    }
}

// host side -----------------------------------------------------------------------------------------------------------
inline bool lt_bad_capacity(int64_t cap, int64_t max_cap) { return cap < 2 || cap > max_cap || (cap & (cap - 1)); }

inline unsigned lt_scan_blocks(int64_t cap) { return (unsigned) ((cap + 255) / 256 < 4096 ? (cap + 255) / 256 : 4096); }

inline u64 *lt_keys(void *workspace) { return (u64 *) ((char *) workspace + LT_HEAD_BYTES); }

// status_host[0] = overflow, [1] = occupied slots, counted afresh by every call.  Synchronises the stream.
inline hipError_t lt_status(void *workspace, int64_t cap, int64_t *status_host, hipStream_t st) {
    u64 *head = (u64 *) workspace;
    hipError_t e = hipMemsetAsync(head + 1, 0, 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lt_count_kernel, dim3(lt_scan_blocks(cap)), dim3(256), 0, st, lt_keys(workspace), (long) cap, head + 1);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(status_host, head, 16, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

}  // namespace
