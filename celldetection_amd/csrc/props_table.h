// Layout of the region property workspace (csrc/region_props.hip writes it, csrc/shape_props.hip reads it): the counters and
// the table of csrc/label_table.h keyed by (channel << 32 | label), its rows, and the sort buffer of
// (channel << 59 | label << 28 | slot).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "label_table.h"

namespace {

constexpr int RP_MAX_K = 4;          // intensity channels
constexpr int64_t RP_MAX_CAPACITY = (int64_t) 1 << 28;  // slot numbers take 28 bits of a sort key

struct Table {
    u64 *keys, *n, *sums;      // [cap], [cap], [5][cap]
    uint32_t *box;             // [4][cap]: 65536 - rmin, 65536 - cmin, rmax + 1, cmax + 1
    i64 *isum;                 // [K][cap]
    uint32_t *imin, *imax;     // [K][cap], mirrored / biased
    u64 cap;
    u64 *overflow;
};

inline int64_t rp_row_bytes(int K) { return 8 + 8 + 40 + 16 + (int64_t) K * 16; }

inline Table rp_table(void *workspace, int64_t cap, int K) {
    Table t;
    char *w = (char *) workspace;
    t.overflow = (u64 *) w;
    w += LT_HEAD_BYTES;
    t.keys = (u64 *) w;      w += cap * 8;
    t.n = (u64 *) w;         w += cap * 8;
    t.sums = (u64 *) w;      w += cap * 40;
    t.isum = (i64 *) w;      w += cap * 8 * K;
    t.box = (uint32_t *) w;  w += cap * 16;
    t.imin = (uint32_t *) w; w += cap * 4 * K;
    t.imax = (uint32_t *) w;
    t.cap = (u64) cap;
    return t;
}

inline u64 *rp_sort_buffer(void *workspace, int64_t cap, int K) {
    return (u64 *) ((char *) workspace + LT_HEAD_BYTES + cap * rp_row_bytes(K));
}

__device__ __forceinline__ int64_t rp_bits(double d) { return (int64_t) __double_as_longlong(d); }

inline bool rp_bad_capacity(int64_t cap) { return lt_bad_capacity(cap, RP_MAX_CAPACITY); }

}  // namespace
