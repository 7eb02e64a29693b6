// Shape properties of label images on the GPU (gfx950): perimeter, perimeter_crofton, euler_number, area_convex and solidity
// behind celldetection_amd.shape_properties / labels2property_table (scikit-image's perimeter(image, 4),
// perimeter_crofton(image, 4), euler_number and convex_hull_image, restated in include/cpn_hip.h, "Shape property tables").
//
// The pass runs after cpn_props_accumulate / table_status / compact_sort (csrc/region_props.hip): keys, slots, bounding boxes
// and the sorted order exist.  It only LOOKS UP the slot of a key (read-only probing of the table's keys) and adds to a
// workspace of its own, indexed by slot.
//
// Shape pass.  A workgroup owns a tile of 32 rows x 64 columns of the (H + 1) x (W + 1) grid of pixels and 2 x 2 windows (the
// window whose bottom right pixel is (r, c) belongs to the owner of (r, c); row H and column W hold no pixel, only windows).
// Per channel it stages the tile with a halo of 2 into LDS (values <= 0 and everything outside the image as 0), computes the
// border flag B on tile + 1 (B(p) = label(p) > 0 and an edge neighbour holds another value; for the object l this is the B
// of the definition wherever label == l), and then every thread handles 8 pixels: the perimeter class of the pixel, its four
// Crofton transitions, the bit-quad term of its window for each of the up to four labels in it, and the ends of row runs for
// the hull.  Pixels whose eight neighbours hold their own label add nothing and touch no table.
// Counts go to a table of 64 keys in LDS (the seven counts packed 16 bits each into two 64-bit words: a tile has 2048
// pixels; the Euler term as a signed word; with the hull the first and last column per tile row) and are flushed once per
// (tile, key) with integer global atomics; a key that finds no LDS slot goes to the global workspace itself.  Everything is
// integer arithmetic, so the result is bit-identical from run to run.
//
// Hull.  Per object the column extent of every row of its bounding box (atomicMax on mirrored values, zero = no pixel), at
// offsets that are the exclusive scan of the box heights in sorted order (the caller scans); then one lane per object runs
// csrc/hull_count.h.  Known limit: one lane per object, so one object as tall as the image serialises.
//
// Finalise computes the requested columns in fp64 in the order of operations include/cpn_hip.h states (this file is
// compiled with -ffp-contract=off).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "hull_count.h"
#include "props_table.h"

namespace {

constexpr int SP_MAX_C = 11;
constexpr int SP_TILE_H = 32, SP_TILE_W = 64, SP_HALO = 2;
constexpr int SP_LH = SP_TILE_H + 2 * SP_HALO, SP_LW = SP_TILE_W + 2 * SP_HALO;  // staged labels
constexpr int SP_BH = SP_TILE_H + 2, SP_BW = SP_TILE_W + 2;                      // border flags: tile + 1
constexpr int SP_LDS_SLOTS = 64, SP_LDS_PROBE = 16;
constexpr int SP_MAX_PROPS = 64;
constexpr int SP_COUNTS = 7;  // n1, n2, n3, Nv | Nh, Nd, Na

struct Shape {  // the shape workspace, indexed by the slot of the property table
    i64 *euler;        // [cap]: Q1 - Q3 - 2 QD
    i64 *row_begin;    // [cap]: first entry of the object's rows in the extents (hull only)
    uint32_t *counts;  // [7][cap]
    u64 cap;
};

Shape sp_shape(void *workspace, int64_t cap) {
    Shape s;
    char *w = (char *) workspace + LT_HEAD_BYTES;
    s.euler = (i64 *) w;      w += cap * 8;
    s.row_begin = (i64 *) w;  w += cap * 8;
    s.counts = (uint32_t *) w;
    s.cap = (u64) cap;
    return s;
}

int64_t sp_bytes(int64_t cap) { return LT_HEAD_BYTES + cap * (8 + 8 + 4 * SP_COUNTS); }

struct Extents {  // lo[i] = 65536 - first column (0: no pixel), hi[i] = last column + 1
    uint32_t *lo, *hi;
    i64 total;
};

struct LdsShape {
    u64 keys[SP_LDS_SLOTS];
    u64 a[SP_LDS_SLOTS], b[SP_LDS_SLOTS];  // n1 | n2 << 16 | n3 << 32 | Nv << 48;  Nh | Nd << 16 | Na << 32
    int euler[SP_LDS_SLOTS];
    i64 slot[SP_LDS_SLOTS];
};

struct LdsRows {  // hull only: per key and tile row, 65536 - first column (0: none) and last column + 1
    uint32_t lo[SP_LDS_SLOTS][SP_TILE_H], hi[SP_LDS_SLOTS][SP_TILE_H];
};

__device__ __forceinline__ void sp_global_counts(const Shape &s, i64 slot, u64 a, u64 b, int euler) {
    const uint32_t v[SP_COUNTS] = {(uint32_t) (a & 0xffff),         (uint32_t) ((a >> 16) & 0xffff), (uint32_t) ((a >> 32) & 0xffff),
                                   (uint32_t) (a >> 48),            (uint32_t) (b & 0xffff),         (uint32_t) ((b >> 16) & 0xffff),
                                   (uint32_t) ((b >> 32) & 0xffff)};
#pragma unroll
    for (int q = 0; q < SP_COUNTS; ++q)
        if (v[q]) atomicAdd(&s.counts[(u64) q * s.cap + (u64) slot], v[q]);
    if (euler) atomicAdd((u64 *) &s.euler[slot], (u64) (i64) euler);
}

// one column of row r of the object in `slot` (first: a run begins there, last: a run ends there)
__device__ __forceinline__ void sp_global_extent(const Shape &s, const Table &t, const Extents &x, i64 slot, int r, uint32_t lo,
                                                 uint32_t hi) {
    const i64 r0 = 65536 - (i64) t.box[slot];
    const i64 i = s.row_begin[slot] + (r - r0);
    if (r < r0 || i < 0 || i >= x.total) return;  // cannot happen on the image the table was built from
    if (lo) atomicMax(&x.lo[i], lo);
    if (hi) atomicMax(&x.hi[i], hi);
}

template <bool HULL>
__device__ __forceinline__ void sp_add(LdsShape &L, LdsRows *R, const Shape &s, const Table &t, const Extents &x, u64 key, u64 a, u64 b, int euler,
                                       int row_local, int r, uint32_t lo, uint32_t hi) {
    const int h = lt_claim_lds<SP_LDS_SLOTS, SP_LDS_PROBE>(L.keys, key);
    if (h >= 0) {
        if (a) atomicAdd(&L.a[h], a);
        if (b) atomicAdd(&L.b[h], b);
        if (euler) atomicAdd(&L.euler[h], euler);
        if (HULL) {
            if (lo) atomicMax(&R->lo[h][row_local], lo);
            if (hi) atomicMax(&R->hi[h][row_local], hi);
        }
        return;
    }
    // the tile holds more keys than the LDS table takes; the accumulate pass of region_props.hip inserted every key
    const i64 slot = lt_lookup(t.keys, t.cap, key);
    if (slot < 0) return;
    sp_global_counts(s, slot, a, b, euler);
    if (HULL && (lo | hi)) sp_global_extent(s, t, x, slot, r, lo, hi);
}

template <bool HULL>
__global__ __launch_bounds__(256) void sp_accumulate_kernel(const int32_t *__restrict__ img, int H, int W, int C, Table t, Shape s,
                                                           Extents x) {
    __shared__ LdsShape L;
    __shared__ uint32_t rows[HULL ? sizeof(LdsRows) / 4 : 1];
    LdsRows *R = (LdsRows *) rows;  // touched with the hull only
    __shared__ int32_t lab[SP_LH][SP_LW];
    __shared__ uint8_t bor[SP_BH][SP_BW + 2];
    const int tid = threadIdx.x;
    for (int i = tid; i < (int) (sizeof(LdsShape) / 4); i += 256) ((uint32_t *) &L)[i] = 0;
    if (HULL)
        for (int i = tid; i < (int) (sizeof(LdsRows) / 4); i += 256) ((uint32_t *) R)[i] = 0;
    const int r_tile = blockIdx.y * SP_TILE_H, c_tile = blockIdx.x * SP_TILE_W;
    for (int ch = 0; ch < C; ++ch) {
        __syncthreads();  // the table is zero (first round) or flushed (later rounds); lab and bor are free
        int any = 0;
        for (int i = tid; i < SP_LH * SP_LW; i += 256) {
            const int lr = i / SP_LW, lc = i - lr * SP_LW;
            const int r = r_tile + lr - SP_HALO, c = c_tile + lc - SP_HALO;
            int32_t v = 0;
            if (r >= 0 && r < H && c >= 0 && c < W) v = img[((long) r * W + c) * C + ch];
            lab[lr][lc] = v > 0 ? v : 0;
            any |= v > 0;
        }
        if (!__syncthreads_or(any)) continue;  // no object in the tile and its halo (the same answer in every thread)
        for (int i = tid; i < SP_BH * SP_BW; i += 256) {
            const int br = i / SP_BW, bc = i - br * SP_BW;
            const int lr = br + 1, lc = bc + 1;
            const int32_t v = lab[lr][lc];
            bor[br][bc] = v > 0 && (lab[lr - 1][lc] != v || lab[lr + 1][lc] != v || lab[lr][lc - 1] != v || lab[lr][lc + 1] != v);
        }
        __syncthreads();
#pragma unroll 2
        for (int k = 0; k < SP_TILE_H * SP_TILE_W / 256; ++k) {
            const int p = k * 256 + tid;
            const int pr = p / SP_TILE_W, pc = p - pr * SP_TILE_W;
            const int lr = pr + SP_HALO, lc = pc + SP_HALO;
            const int32_t d = lab[lr][lc];
            const int32_t nw = lab[lr - 1][lc - 1], nn = lab[lr - 1][lc], ne = lab[lr - 1][lc + 1], ww = lab[lr][lc - 1],
                          ee = lab[lr][lc + 1], sw = lab[lr + 1][lc - 1], ss = lab[lr + 1][lc], se = lab[lr + 1][lc + 1];
            if (nw == d && nn == d && ne == d && ww == d && ee == d && sw == d && ss == d && se == d) continue;  // inside, or empty
            const int r = r_tile + pr, c = c_tile + pc;
            if (d > 0) {
                u64 a = 0, b = 0;
                const int br = pr + 1, bc = pc + 1;
                if (bor[br][bc]) {
                    const int o = (nn == d && bor[br - 1][bc]) + (ss == d && bor[br + 1][bc]) + (ww == d && bor[br][bc - 1]) +
                                  (ee == d && bor[br][bc + 1]);
                    const int g = (nw == d && bor[br - 1][bc - 1]) + (ne == d && bor[br - 1][bc + 1]) + (sw == d && bor[br + 1][bc - 1]) +
                                  (se == d && bor[br + 1][bc + 1]);
                    const int code = 1 + 2 * o + 10 * g;
                    if (code == 5 || code == 7 || code == 15 || code == 17 || code == 25 || code == 27) a = 1ull;
                    else if (code == 21 || code == 33) a = 1ull << 16;
                    else if (code == 13 || code == 23) a = 1ull << 32;
                }
                a |= (u64) (nn != d) << 48;
                b = (u64) (ee != d) | (u64) (nw != d) << 16 | (u64) (sw != d) << 32;
                const int cnt = 1 + (nw == d) + (nn == d) + (ww == d);
                const int e = cnt == 1 ? 1 : cnt == 3 ? -1 : (cnt == 2 && nw == d) ? -2 : 0;
                const uint32_t lo = (HULL && ww != d) ? 65536u - (uint32_t) c : 0u, hi = (HULL && ee != d) ? (uint32_t) c + 1u : 0u;
                sp_add<HULL>(L, R, s, t, x, ((u64) ch << 32) | (uint32_t) d, a, b, e, pr, r, lo, hi);
            }
            // the other labels of the window nw nn / ww d
            if (nw > 0 && nw != d) {
                const int cnt = 1 + (nn == nw) + (ww == nw);
                const int e = cnt == 1 ? 1 : cnt == 3 ? -1 : 0;  // two of them: nw with nn or ww, an edge pair
                if (e) sp_add<HULL>(L, R, s, t, x, ((u64) ch << 32) | (uint32_t) nw, 0, 0, e, pr, r, 0, 0);
            }
            if (nn > 0 && nn != d && nn != nw)
                sp_add<HULL>(L, R, s, t, x, ((u64) ch << 32) | (uint32_t) nn, 0, 0, ww == nn ? -2 : 1, pr, r, 0, 0);  // nn with ww: the diagonal
            if (ww > 0 && ww != d && ww != nw && ww != nn) sp_add<HULL>(L, R, s, t, x, ((u64) ch << 32) | (uint32_t) ww, 0, 0, 1, pr, r, 0, 0);
        }
        __syncthreads();
        // flush: the slot of every key once, then its counts and its rows; the table is left zeroed for the next channel
        for (int h = tid; h < SP_LDS_SLOTS; h += 256) {
            const u64 key = L.keys[h];
            i64 slot = -1;
            if (key != 0) {
                slot = lt_lookup(t.keys, t.cap, key);
                if (slot >= 0) sp_global_counts(s, slot, L.a[h], L.b[h], L.euler[h]);
                L.keys[h] = 0; L.a[h] = 0; L.b[h] = 0; L.euler[h] = 0;
            }
            L.slot[h] = slot;
        }
        if (HULL) {
            __syncthreads();
            for (int i = tid; i < SP_LDS_SLOTS * SP_TILE_H; i += 256) {
                const int h = i / SP_TILE_H, pr = i - h * SP_TILE_H;
                const uint32_t lo = R->lo[h][pr], hi = R->hi[h][pr];
                if ((lo | hi) == 0) continue;
                R->lo[h][pr] = 0; R->hi[h][pr] = 0;
                if (L.slot[h] >= 0) sp_global_extent(s, t, x, L.slot[h], r_tile + pr, lo, hi);
            }
        }
    }
}

// heights of the bounding boxes in sorted order
__global__ __launch_bounds__(256) void sp_heights_kernel(const u64 *__restrict__ sorted, long N, Table t, i64 *__restrict__ out) {
    const long i = (long) blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const u64 slot = sorted[i] & (((u64) 1 << 28) - 1);
    out[i] = slot < t.cap ? (i64) t.box[2 * t.cap + slot] - (65536 - (i64) t.box[slot]) : 0;
}

__global__ __launch_bounds__(256) void sp_scatter_kernel(const u64 *__restrict__ sorted, long N, Shape s, const i64 *__restrict__ row_begin) {
    const long i = (long) blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const u64 slot = sorted[i] & (((u64) 1 << 28) - 1);
    if (slot < s.cap) s.row_begin[slot] = row_begin[i];
}

__global__ __launch_bounds__(64) void sp_hull_kernel(long N, const i64 *__restrict__ row_begin, Extents x, int32_t *__restrict__ scratch,
                                                    i64 *__restrict__ counts) {
    const long i = (long) blockIdx.x * 64 + threadIdx.x;
    if (i >= N) return;
    const i64 b = row_begin[i], rows = row_begin[i + 1] - b;
    i64 n = 0;
    if (b >= 0 && rows > 0 && b + rows <= x.total) n = hull_count(x.lo + b, x.hi + b, rows, scratch + 2 * (2 * b + i));
    counts[i] = n;
}

struct Props {
    int32_t code[SP_MAX_PROPS];
    int32_t n;
};

__global__ __launch_bounds__(256) void sp_finalise_kernel(const u64 *__restrict__ sorted, long N, Table t, Shape s,
                                                         const i64 *__restrict__ hull, Props props, double sp, double px,
                                                         int64_t *__restrict__ out) {
    const long i = (long) blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const u64 sk = sorted[i];
    const u64 slot = sk & (((u64) 1 << 28) - 1);
    if (slot >= t.cap) return;  // padding of the sort buffer
    const int64_t label = (int64_t) ((sk >> 28) & 0x7fffffffull), channel = (int64_t) (sk >> 59);
    const i64 n = (i64) t.n[slot];
    uint32_t v[SP_COUNTS];
#pragma unroll
    for (int q = 0; q < SP_COUNTS; ++q) v[q] = s.counts[(u64) q * s.cap + slot];
    const double perimeter = ((double) v[0] + (double) v[1] * sqrt(2.0) + (double) v[2] * ((1.0 + sqrt(2.0)) / 2.0)) * sp;
    const double pi = 3.14159265358979323846;
    const double crofton = (((double) ((i64) v[3] + (i64) v[4]) + (double) ((i64) v[5] + (i64) v[6]) / sqrt(2.0)) * (pi / 4.0)) * sp;
    const double area_convex = hull ? (double) hull[i] * px : 0.;
    int col = 0;
    auto put = [&](int64_t w) { out[(long) col * N + i] = w; ++col; };
    for (int q = 0; q < props.n; ++q) {
        switch (props.code[q]) {
            case CPN_SHAPE_LABEL: put(label); break;
            case CPN_SHAPE_NUM_PIXELS: put(n); break;
            case CPN_SHAPE_PERIMETER: put(rp_bits(perimeter)); break;
            case CPN_SHAPE_PERIMETER_CROFTON: put(rp_bits(crofton)); break;
            case CPN_SHAPE_EULER_NUMBER: put(s.euler[slot] / 4); break;
            case CPN_SHAPE_AREA_CONVEX: put(rp_bits(area_convex)); break;
            case CPN_SHAPE_SOLIDITY: put(rp_bits(((double) n * px) / area_convex)); break;
            default: break;
        }
    }
    out[(long) col * N + i] = channel;
}

bool sp_bad_table(const void *props_workspace, int64_t cap, int32_t K, int64_t entries) {
    return !props_workspace || rp_bad_capacity(cap) || K < 0 || K > RP_MAX_K || entries < 0 || entries > cap;
}

bool sp_needs_hull(const int32_t *properties, int32_t n) {
    for (int i = 0; i < n; ++i)
        if (properties[i] == CPN_SHAPE_AREA_CONVEX || properties[i] == CPN_SHAPE_SOLIDITY) return true;
    return false;
}

}  // namespace

extern "C" {

int64_t cpn_shape_workspace_bytes(int64_t table_capacity) { return rp_bad_capacity(table_capacity) ? 0 : sp_bytes(table_capacity); }

int32_t cpn_shape_columns(const int32_t *properties, int32_t n_properties) {
    if (!properties || n_properties < 0 || n_properties > SP_MAX_PROPS) return -1;
    for (int i = 0; i < n_properties; ++i)
        if (properties[i] < 0 || properties[i] >= CPN_SHAPE_COUNT) return -1;
    return n_properties;
}

int64_t cpn_shape_hull_scratch_bytes(int64_t entries, int64_t total_rows) {
    if (entries < 0 || total_rows < 0) return 0;
    return 8 * (2 * total_rows + entries) + 8;
}

int cpn_shape_heights(void *props_workspace, int64_t table_capacity, int32_t intensity_channels, int64_t entries, int64_t *heights,
                      void *stream) {
    if (sp_bad_table(props_workspace, table_capacity, intensity_channels, entries))
        return cpn::fail(CPN_E_INVALID, "cpn_shape_heights: bad arguments");
    if (entries == 0) return 0;
    if (!heights) return cpn::fail(CPN_E_INVALID, "cpn_shape_heights: heights is NULL");
    hipLaunchKernelGGL(sp_heights_kernel, dim3((unsigned) ((entries + 255) / 256)), dim3(256), 0, (hipStream_t) stream,
                       rp_sort_buffer(props_workspace, table_capacity, intensity_channels), (long) entries,
                       rp_table(props_workspace, table_capacity, intensity_channels), (i64 *) heights);
    return cpn::check_hip(hipGetLastError(), "cpn_shape_heights");
}

int cpn_shape_accumulate(const int32_t *labels, int32_t H, int32_t W, int32_t channels, void *props_workspace, int64_t table_capacity,
                         int32_t intensity_channels, int64_t entries, void *workspace, int64_t workspace_bytes,
                         const int64_t *row_begin, uint32_t *extents, int64_t total_rows, void *stream) {
    if (H < 0 || W < 0 || channels < 1 || !workspace || sp_bad_table(props_workspace, table_capacity, intensity_channels, entries) ||
        total_rows < 0 || (row_begin && total_rows > 0 && !extents))
        return cpn::fail(CPN_E_INVALID, "cpn_shape_accumulate: bad arguments (table_capacity must be a power of two <= 2^28)");
    if (channels > SP_MAX_C) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_shape_accumulate: more than 11 label channels");
    if ((int64_t) H * W > 0x7fffffff || H > 65536 || W > 65536)
        return cpn::fail(CPN_E_UNSUPPORTED, "cpn_shape_accumulate: image larger than 2^31 - 1 pixels or 65536 a side");
    if (workspace_bytes < sp_bytes(table_capacity)) return cpn::fail(CPN_E_WORKSPACE, "cpn_shape_accumulate: workspace too small");
    if ((int64_t) H * W > 0 && !labels) return cpn::fail(CPN_E_INVALID, "cpn_shape_accumulate: labels is NULL");
    hipStream_t st = (hipStream_t) stream;
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t) sp_bytes(table_capacity), st);
    if (e == hipSuccess && row_begin && total_rows > 0) e = hipMemsetAsync(extents, 0, (size_t) total_rows * 8, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_shape_accumulate: memset");
    if ((int64_t) H * W == 0 || entries == 0) return 0;
    const Table t = rp_table(props_workspace, table_capacity, intensity_channels);
    const Shape s = sp_shape(workspace, table_capacity);
    Extents x;
    x.lo = extents;
    x.hi = extents ? extents + total_rows : nullptr;
    x.total = row_begin ? total_rows : 0;
    const dim3 grid((unsigned) (W / SP_TILE_W + 1), (unsigned) (H / SP_TILE_H + 1));  // ceil((W + 1) / tile): the windows of row H, column W
    if (row_begin) {
        hipLaunchKernelGGL(sp_scatter_kernel, dim3((unsigned) ((entries + 255) / 256)), dim3(256), 0, st,
                           rp_sort_buffer(props_workspace, table_capacity, intensity_channels), (long) entries, s, (const i64 *) row_begin);
        hipLaunchKernelGGL(sp_accumulate_kernel<true>, grid, dim3(256), 0, st, labels, H, W, channels, t, s, x);
    } else {
        hipLaunchKernelGGL(sp_accumulate_kernel<false>, grid, dim3(256), 0, st, labels, H, W, channels, t, s, x);
    }
    return cpn::check_hip(hipGetLastError(), "cpn_shape_accumulate");
}

int cpn_shape_hull(int64_t entries, const int64_t *row_begin, const uint32_t *extents, int64_t total_rows, void *scratch,
                   int64_t scratch_bytes, int64_t *counts, void *stream) {
    if (entries < 0 || total_rows < 0) return cpn::fail(CPN_E_INVALID, "cpn_shape_hull: bad arguments");
    if (scratch_bytes < cpn_shape_hull_scratch_bytes(entries, total_rows))
        return cpn::fail(CPN_E_WORKSPACE, "cpn_shape_hull: scratch too small");
    if (entries == 0) return 0;
    if (!row_begin || !counts || !scratch || (total_rows > 0 && !extents)) return cpn::fail(CPN_E_INVALID, "cpn_shape_hull: null pointer");
    Extents x;
    x.lo = (uint32_t *) extents;
    x.hi = (uint32_t *) extents + total_rows;
    x.total = total_rows;
    hipLaunchKernelGGL(sp_hull_kernel, dim3((unsigned) ((entries + 63) / 64)), dim3(64), 0, (hipStream_t) stream, (long) entries,
                       (const i64 *) row_begin, x, (int32_t *) scratch, (i64 *) counts);
    return cpn::check_hip(hipGetLastError(), "cpn_shape_hull");
}

int cpn_shape_finalise(void *props_workspace, int64_t table_capacity, int32_t intensity_channels, int64_t entries, void *workspace,
                       const int64_t *hull_counts, const int32_t *properties, int32_t n_properties, double spacing_row,
                       double spacing_col, int64_t *out, int64_t out_columns, void *stream) {
    if (!workspace || sp_bad_table(props_workspace, table_capacity, intensity_channels, entries))
        return cpn::fail(CPN_E_INVALID, "cpn_shape_finalise: bad arguments");
    const int cols = cpn_shape_columns(properties, n_properties);
    if (cols < 0) return cpn::fail(CPN_E_INVALID, "cpn_shape_finalise: bad property list (unknown code or more than 64 properties)");
    if (out_columns != cols + 1) return cpn::fail(CPN_E_INVALID, "cpn_shape_finalise: out must hold one row per column plus one");
    bool lengths = false;
    for (int i = 0; i < n_properties; ++i) lengths |= properties[i] == CPN_SHAPE_PERIMETER || properties[i] == CPN_SHAPE_PERIMETER_CROFTON;
    if (lengths && spacing_row != spacing_col)
        return cpn::fail(CPN_E_UNSUPPORTED, "cpn_shape_finalise: perimeter and perimeter_crofton take isotropic spacings only");
    if (entries == 0) return 0;
    if (!out) return cpn::fail(CPN_E_INVALID, "cpn_shape_finalise: out is NULL");
    if (sp_needs_hull(properties, n_properties) && !hull_counts)
        return cpn::fail(CPN_E_INVALID, "cpn_shape_finalise: area_convex / solidity need the counts of cpn_shape_hull");
    Props p;
    p.n = n_properties;
    for (int i = 0; i < n_properties; ++i) p.code[i] = properties[i];
    hipLaunchKernelGGL(sp_finalise_kernel, dim3((unsigned) ((entries + 255) / 256)), dim3(256), 0, (hipStream_t) stream,
                       rp_sort_buffer(props_workspace, table_capacity, intensity_channels), (long) entries,
                       rp_table(props_workspace, table_capacity, intensity_channels), sp_shape(workspace, table_capacity),
                       (const i64 *) hull_counts, p, spacing_row, spacing_row * spacing_col, out);
    return cpn::check_hip(hipGetLastError(), "cpn_shape_finalise");
}

}  // extern "C"
