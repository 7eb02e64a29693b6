// Region property tables of label images on the GPU (gfx950): the accumulate pass, the table passes and the finalisation
// behind celldetection_amd.region_properties / labels2property_table (the reference's labels2property_table,
// celldetection/data/misc.py:320-347, which calls skimage.measure.regionprops_table per channel).
//
// Accumulate pass.  The label image is int32 [H][W][C], channel-interleaved.  Every element v > 0 adds to the row of key
// (channel << 32 | v): the pixel count, the sums of r, c, r^2, r*c, c^2 of the GLOBAL pixel coordinates (64-bit integers), the
// bounding box, and per intensity channel the sum (int64), minimum and maximum.  Everything is integer arithmetic: the
// result does not depend on the order of the adds, hence it is bit-identical from run to run.
//
// A workgroup owns a tile of 32 rows x 64 columns; a thread owns a strip of 8 consecutive pixels in FLAT pixel order whose
// first pixel lies in its tile row (a strip starts at a multiple of 8 pixels = 32 * C bytes, so its 2 * C loads are 16-byte
// loads for every C and every W; a strip may run past the tile or wrap into the next row, its pixels carry their own
// coordinates).  Runs of equal labels within a strip are merged in registers; a run needs no per-pixel sums: sum c,
// sum c^2, ... of columns a .. a + n - 1 are closed forms.  Per channel the thread first marks where runs begin (bit masks),
// then handles them in one loop.  Without an intensity image the runs that reach the end of a strip and continue in the
// next lane's strip are joined over wave shuffles first.
// A finished run is added to a table of 128 keys in LDS (64-bit LDS atomics); after the tile is done each occupied LDS
// slot goes to the global table once: one set of global integer atomics per (tile, key).  A run that finds no LDS slot
// goes to the global table directly.  The global table is an open-addressing table (64-bit compare-and-swap on the key);
// an insert without a slot within the probe limit counts an overflow and the host repeats with twice the capacity.
//
// Minima are kept as maxima of a mirrored value, so that a zeroed table is a valid empty table:
//   rows / columns: 65536 - r (min), r + 1 (max, the half-open end);  intensities: ~(i ^ 0x80000000) (min), i ^ 0x80000000 (max).
//
// Table passes: count the occupied slots; compact them (both csrc/label_table.h) as (channel << 59 | label << 28 | slot) and
// sort these ascending with a bitonic network (1024 elements per workgroup in LDS, global steps above); finalise computes the
// requested columns in fp64 in the order of operations include/cpn_hip.h states (this file is compiled with
// -ffp-contract=off).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "props_table.h"

namespace {

constexpr int RP_MAX_C = 11;         // label channels
constexpr int RP_TILE_H = 32, RP_TILE_W = 64, RP_PPT = 8;
constexpr int RP_LDS_SLOTS = 128, RP_LDS_PROBE = 16;
constexpr int RP_MAX_PROPS = 64;

struct Run {  // what one run or one LDS slot adds to a row
    unsigned n;
    uint32_t box[4];
    u64 sums[5];
    i64 isum[RP_MAX_K];
    uint32_t imin[RP_MAX_K], imax[RP_MAX_K];
};

__device__ __noinline__ void rp_global_add(const Table &t, u64 key, const Run &a, int K) {
    const i64 h = lt_claim(t.keys, t.cap, key);
    if (h < 0) {
        atomicAdd(t.overflow, 1ull);
        return;
    }
    atomicAdd(&t.n[h], (u64) a.n);
#pragma unroll
    for (int q = 0; q < 5; ++q) atomicAdd(&t.sums[q * t.cap + h], a.sums[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) atomicMax(&t.box[q * t.cap + h], a.box[q]);
#pragma unroll
    for (int k = 0; k < RP_MAX_K; ++k)
        if (k < K) {
            atomicAdd((u64 *) &t.isum[k * t.cap + h], (u64) a.isum[k]);
            atomicMax(&t.imin[k * t.cap + h], a.imin[k]);
            atomicMax(&t.imax[k * t.cap + h], a.imax[k]);
        }
}

struct LdsTable {
    u64 keys[RP_LDS_SLOTS];
    u64 sums[5][RP_LDS_SLOTS];
    unsigned n[RP_LDS_SLOTS];
    uint32_t box[4][RP_LDS_SLOTS];
    // used with an intensity image only
    i64 isum[RP_MAX_K][RP_LDS_SLOTS];
    uint32_t imin[RP_MAX_K][RP_LDS_SLOTS], imax[RP_MAX_K][RP_LDS_SLOTS];
};

// sum of x^2 over x = 0 .. m (m >= -1)
__device__ __forceinline__ i64 rp_sq_sum(i64 m) { return m * (m + 1) * (2 * m + 1) / 6; }

// One run: `n` pixels of row r from column a on, in channel / label `key`.
__device__ __forceinline__ void rp_run_add(LdsTable &L, const Table &t, u64 key, int r, int a, unsigned n, const i64 *isum,
                                           const uint32_t *imin, const uint32_t *imax, int K) {
    const u64 sc = (u64) n * (u64) (2 * (i64) a + n - 1) / 2;
    const i64 b = (i64) a + n - 1;
    u64 sums[5] = {(u64) n * (u64) r, sc, (u64) n * (u64) r * (u64) r, (u64) r * sc, (u64) (rp_sq_sum(b) - rp_sq_sum((i64) a - 1))};
    uint32_t box[4] = {65536u - (uint32_t) r, 65536u - (uint32_t) a, (uint32_t) r + 1u, (uint32_t) b + 1u};
    const int h = lt_claim_lds<RP_LDS_SLOTS, RP_LDS_PROBE>(L.keys, key);
    if (h >= 0) {
        atomicAdd(&L.n[h], n);
#pragma unroll
        for (int q = 0; q < 5; ++q) atomicAdd(&L.sums[q][h], sums[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) atomicMax(&L.box[q][h], box[q]);
#pragma unroll
        for (int k = 0; k < RP_MAX_K; ++k)
            if (k < K) {
                atomicAdd((u64 *) &L.isum[k][h], (u64) isum[k]);
                atomicMax(&L.imin[k][h], imin[k]);
                atomicMax(&L.imax[k][h], imax[k]);
            }
        return;
    }
    Run x;  // the tile holds more keys than the LDS table: this run goes to the global table itself
    x.n = n;
#pragma unroll
    for (int q = 0; q < 5; ++q) x.sums[q] = sums[q];
#pragma unroll
    for (int q = 0; q < 4; ++q) x.box[q] = box[q];
#pragma unroll
    for (int k = 0; k < RP_MAX_K; ++k) { x.isum[k] = isum[k]; x.imin[k] = imin[k]; x.imax[k] = imax[k]; }
    rp_global_add(t, key, x, K);
}

__device__ __forceinline__ int rp_intensity(const void *img, int dtype, long idx) {
    switch (dtype) {
        case CPN_PROPS_U8: return ((const uint8_t *) img)[idx];
        case CPN_PROPS_I16: return ((const int16_t *) img)[idx];
        default: return ((const int32_t *) img)[idx];
    }
}

template <int C>
__global__ __launch_bounds__(256) void rp_accumulate_kernel(const int32_t *__restrict__ x, int H, int W, const void *__restrict__ img,
                                                           int K, int dtype, Table t) {
    __shared__ LdsTable L;
    const int lds_words = (int) ((K > 0 ? sizeof(LdsTable) : offsetof(LdsTable, isum)) / 4);
    for (int i = threadIdx.x; i < lds_words; i += 256) ((uint32_t *) &L)[i] = 0;
    __syncthreads();
    const long total = (long) H * W;
    const int row = blockIdx.y * RP_TILE_H + (threadIdx.x >> 3);
    const long row0 = (long) row * W, lo = row0 + (long) blockIdx.x * RP_TILE_W;
    const long hi = lo + RP_TILE_W < row0 + W ? lo + RP_TILE_W : row0 + W;
    const long p0 = (((lo + RP_PPT - 1) / RP_PPT) + (threadIdx.x & 7)) * RP_PPT;  // first pixel of this thread's strip
    const bool valid = row < H && p0 < hi;  // no early exit: the wave merge and the barrier need every lane
    int32_t v[RP_PPT * C];
    if (valid && p0 + RP_PPT <= total) {
        const int4 *q = reinterpret_cast<const int4 *>(x + p0 * C);  // 32 * C bytes per strip: 16-byte aligned
#pragma unroll
        for (int i = 0; i < RP_PPT * C / 4; ++i) {
            const int4 w = q[i];
            v[4 * i] = w.x; v[4 * i + 1] = w.y; v[4 * i + 2] = w.z; v[4 * i + 3] = w.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < RP_PPT * C; ++i) v[i] = (valid && p0 * C + i < total * C) ? x[p0 * C + i] : 0;
    }
    const int c_first = (int) (p0 - row0);
    const int lane = __lane_id();
    unsigned wrap = 0;  // bit p: pixel p of the strip is the first of a row (p > 0)
    {
        int c = c_first;
#pragma unroll
        for (int p = 0; p < RP_PPT; ++p) {
            if (p > 0 && c == 0) wrap |= 1u << p;
            if (++c == W) c = 0;
        }
    }
    // coordinates of pixel s of the strip
    auto coords = [&](int s, int &r, int &c) {
        r = row;
        c = c_first + s;
        while (c >= W) { c -= W; ++r; }
    };
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        // bit p of pos: pixel p belongs to an object; of start: a run begins there (a run: equal labels side by side in a row)
        unsigned pos = 0, start = 0;
#pragma unroll
        for (int p = 0; p < RP_PPT; ++p) {
            const int32_t val = v[p * C + ch];
            if (val > 0) {
                pos |= 1u << p;
                if (p == 0 || val != v[(p > 0 ? p - 1 : 0) * C + ch] || ((wrap >> p) & 1)) start |= 1u << p;
            }
        }
        auto label_at = [&](int s) {
            int32_t lab = v[ch];
#pragma unroll
            for (int p = 1; p < RP_PPT; ++p) lab = s == p ? v[p * C + ch] : lab;
            return lab;
        };
        // the run that reaches the end of the strip may go on in the next lane's strip
        const int ps = (pos & 0x80u) ? 31 - __clz((int) start) : -1;
        unsigned pn = ps >= 0 ? (unsigned) (RP_PPT - ps) : 0u;
        if (K == 0 && __ballot(pn > 0) != 0) {
            // join the pending runs of consecutive lanes that continue each other (same label, same row, adjacent columns)
            int32_t cur = 0;
            int rr = 0, ra = 0;
            if (ps >= 0) { cur = label_at(ps); coords(ps, rr, ra); }
            const int32_t pcur = __shfl_up(cur, 1, 64);
            const int prr = __shfl_up(rr, 1, 64), pend = __shfl_up(ra + (int) pn, 1, 64);
            const unsigned ppn = __shfl_up(pn, 1, 64);
            const bool head = lane == 0 || pn == 0 || ppn == 0 || pcur != cur || prr != rr || pend != ra;
            const unsigned n = lt_segment_sum(head, pn);
            if (head) pn = n;
            else start &= ~(1u << ps);  // counted by the lane at the head of the joined run
        }
        const unsigned stops = (start | ~pos) & 0xffu;
        while (start) {
            const int s = __ffs((int) start) - 1;
            start &= start - 1;
            const int e = __ffs((int) ((stops >> (s + 1)) | (1u << (RP_PPT - 1 - s)))) + s;  // first pixel after the run
            const unsigned n = s == ps ? pn : (unsigned) (e - s);
            int r, c;
            coords(s, r, c);
            i64 isum[RP_MAX_K] = {0, 0, 0, 0};
            uint32_t imin[RP_MAX_K] = {0, 0, 0, 0}, imax[RP_MAX_K] = {0, 0, 0, 0};
            if (K > 0) {
                for (int p = s; p < e; ++p)
#pragma unroll
                    for (int k = 0; k < RP_MAX_K; ++k)
                        if (k < K) {
                            const int iv = rp_intensity(img, dtype, (p0 + p) * K + k);
                            const uint32_t en = (uint32_t) iv ^ 0x80000000u;
                            isum[k] += iv;
                            imin[k] = imin[k] > ~en ? imin[k] : ~en;
                            imax[k] = imax[k] > en ? imax[k] : en;
                        }
            }
            rp_run_add(L, t, ((u64) ch << 32) | (uint32_t) label_at(s), r, c, n, isum, imin, imax, K);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < RP_LDS_SLOTS; s += 256) {
        const u64 key = L.keys[s];
        if (key == 0) continue;
        Run a;
        a.n = L.n[s];
#pragma unroll
        for (int q = 0; q < 5; ++q) a.sums[q] = L.sums[q][s];
#pragma unroll
        for (int q = 0; q < 4; ++q) a.box[q] = L.box[q][s];
#pragma unroll
        for (int k = 0; k < RP_MAX_K; ++k)
            if (k < K) { a.isum[k] = L.isum[k][s]; a.imin[k] = L.imin[k][s]; a.imax[k] = L.imax[k][s]; }
        rp_global_add(t, key, a, K);
    }
}

// table -> sorted slot list -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rp_fill_kernel(u64 *__restrict__ a, long n) {
    const long i = (long) blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = ~0ull;
}

// lt_compact_kernel writes the sort key: channel << 59 | label << 28 | slot (label < 2^31, slot < 2^28)
struct SortKeyEmit {
    u64 *__restrict__ out;
    __device__ void operator()(long pos, long slot, u64 k) const {
        out[pos] = ((k >> 32) << 59) | ((k & 0xffffffffull) << 28) | (u64) slot;
    }
};

// Bitonic network, ascending.  FULL: sorts every block of 1024 (k = 2 .. 1024); otherwise the steps j = 512 .. 1 of stage k.
template <bool FULL>
__global__ __launch_bounds__(512) void rp_bitonic_local_kernel(u64 *__restrict__ a, u64 k_stage) {
    __shared__ u64 s[1024];
    const u64 base = (u64) blockIdx.x * 1024;
    const unsigned tid = threadIdx.x;
    s[tid] = a[base + tid];
    s[tid + 512] = a[base + tid + 512];
    __syncthreads();
    for (u64 k = FULL ? 2 : k_stage; k <= (FULL ? 1024 : k_stage); k <<= 1) {
        for (unsigned j = k >> 1 < 512 ? (unsigned) (k >> 1) : 512u; j >= 1; j >>= 1) {
            const unsigned i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), l = i + j;
            const bool up = ((base + i) & k) == 0;
            const u64 p = s[i], q = s[l];
            if ((p > q) == up) { s[i] = q; s[l] = p; }
            __syncthreads();
        }
    }
    a[base + tid] = s[tid];
    a[base + tid + 512] = s[tid + 512];
}

__global__ __launch_bounds__(256) void rp_bitonic_global_kernel(u64 *__restrict__ a, u64 half, u64 k, u64 j) {
    const u64 t = (u64) blockIdx.x * 256 + threadIdx.x;
    if (t >= half) return;
    const u64 i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
    const bool up = (i & k) == 0;
    const u64 p = a[i], q = a[l];
    if ((p > q) == up) { a[i] = q; a[l] = p; }
}

// finalisation --------------------------------------------------------------------------------------------------------
struct Props {
    int32_t code[RP_MAX_PROPS];
    int32_t n;
};

__host__ __device__ inline int rp_prop_columns(int code, int K) {
    switch (code) {
        case CPN_PROP_BBOX: case CPN_PROP_INERTIA_TENSOR: return 4;
        case CPN_PROP_CENTROID: case CPN_PROP_CENTROID_LOCAL: case CPN_PROP_INERTIA_TENSOR_EIGVALS: return 2;
        case CPN_PROP_INTENSITY_MEAN: case CPN_PROP_INTENSITY_MIN: case CPN_PROP_INTENSITY_MAX: return K;
        default: return 1;
    }
}

__global__ __launch_bounds__(256) void rp_finalise_kernel(const u64 *__restrict__ sorted, long N, Table t, int K, Props props,
                                                         double sy, double sx, int64_t *__restrict__ out) {
    const long i = (long) blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const u64 sk = sorted[i];
    const u64 slot = sk & (((u64) 1 << 28) - 1);
    if (slot >= t.cap) return;  // padding of the sort buffer: `entries` exceeds the occupied slots
    const int64_t label = (int64_t) ((sk >> 28) & 0x7fffffffull), channel = (int64_t) (sk >> 59);
    const i64 n = (i64) t.n[slot];
    const i64 Sr = (i64) t.sums[0 * t.cap + slot], Sc = (i64) t.sums[1 * t.cap + slot], Srr = (i64) t.sums[2 * t.cap + slot],
              Src = (i64) t.sums[3 * t.cap + slot], Scc = (i64) t.sums[4 * t.cap + slot];
    const i64 r0 = 65536 - (i64) t.box[0 * t.cap + slot], c0 = 65536 - (i64) t.box[1 * t.cap + slot];
    const i64 r1 = (i64) t.box[2 * t.cap + slot], c1 = (i64) t.box[3 * t.cap + slot];
    // sums relative to the corner of the bounding box, in integers (two's complement keeps the intermediate steps exact)
    const u64 un = (u64) n, ur0 = (u64) r0, uc0 = (u64) c0;
    const i64 sr = (i64) ((u64) Sr - un * ur0), sc = (i64) ((u64) Sc - un * uc0);
    const i64 srr = (i64) ((u64) Srr - 2 * ur0 * (u64) Sr + un * ur0 * ur0);
    const i64 src = (i64) ((u64) Src - ur0 * (u64) Sc - uc0 * (u64) Sr + un * ur0 * uc0);
    const i64 scc = (i64) ((u64) Scc - 2 * uc0 * (u64) Sc + un * uc0 * uc0);
    const double nd = (double) n, px = sy * sx;
    const double dsr = (double) sr, dsc = (double) sc;
    const double area = nd * px;
    const double area_bbox = (double) ((r1 - r0) * (c1 - c0)) * px;
    const double mu20 = ((double) srr - dsr * dsr / nd) * (sy * sy);
    const double mu02 = ((double) scc - dsc * dsc / nd) * (sx * sx);
    const double mu11 = ((double) src - dsr * dsc / nd) * (sy * sx);
    const double a = mu02 / nd, b = -mu11 / nd, c = mu20 / nd;
    const double m = (a + c) / 2, d = (a - c) / 2, s = sqrt(d * d + b * b);
    const double l1 = m + s, l2 = fmax(m - s, 0.);
    const double pi = 3.14159265358979323846;
    int col = 0;
    auto put = [&](int64_t v) { out[(long) col * N + i] = v; ++col; };
    for (int q = 0; q < props.n; ++q) {
        switch (props.code[q]) {
            case CPN_PROP_LABEL: put(label); break;
            case CPN_PROP_BBOX: put(r0); put(c0); put(r1); put(c1); break;
            case CPN_PROP_NUM_PIXELS: put(n); break;
            case CPN_PROP_AREA: put(rp_bits(area)); break;
            case CPN_PROP_AREA_BBOX: put(rp_bits(area_bbox)); break;
            case CPN_PROP_EXTENT: put(rp_bits(area / area_bbox)); break;
            case CPN_PROP_EQUIVALENT_DIAMETER_AREA: put(rp_bits(sqrt(4 * area / pi))); break;
            case CPN_PROP_CENTROID: put(rp_bits((double) Sr / nd * sy)); put(rp_bits((double) Sc / nd * sx)); break;
            case CPN_PROP_CENTROID_LOCAL: put(rp_bits(dsr / nd * sy)); put(rp_bits(dsc / nd * sx)); break;
            case CPN_PROP_INERTIA_TENSOR: put(rp_bits(a)); put(rp_bits(b)); put(rp_bits(b)); put(rp_bits(c)); break;
            case CPN_PROP_INERTIA_TENSOR_EIGVALS: put(rp_bits(l1)); put(rp_bits(l2)); break;
            case CPN_PROP_AXIS_MAJOR_LENGTH: put(rp_bits(4 * sqrt(l1))); break;
            case CPN_PROP_AXIS_MINOR_LENGTH: put(rp_bits(4 * sqrt(l2))); break;
            case CPN_PROP_ECCENTRICITY: put(rp_bits(l1 == 0 ? 0. : sqrt(1 - l2 / l1))); break;
            case CPN_PROP_ORIENTATION:
                put(rp_bits(a - c == 0 ? (b < 0 ? pi / 4 : -pi / 4) : 0.5 * atan2(-2 * b, c - a)));
                break;
            case CPN_PROP_INTENSITY_MEAN:
                for (int k = 0; k < K; ++k) put(rp_bits((double) t.isum[k * t.cap + slot] / nd));
                break;
            case CPN_PROP_INTENSITY_MIN:
                for (int k = 0; k < K; ++k) put((int64_t) (int32_t) (~t.imin[k * t.cap + slot] ^ 0x80000000u));
                break;
            case CPN_PROP_INTENSITY_MAX:
                for (int k = 0; k < K; ++k) put((int64_t) (int32_t) (t.imax[k * t.cap + slot] ^ 0x80000000u));
                break;
            default: break;
        }
    }
    out[(long) col * N + i] = channel;  // one more row after the requested columns
}

int64_t rp_sort_length(int64_t entries) {
    int64_t m = 1024;
    while (m < entries) m <<= 1;
    return m;
}

template <int C>
void rp_launch(hipStream_t st, dim3 grid, const int32_t *x, int H, int W, const void *img, int K, int dtype, const Table &t) {
    hipLaunchKernelGGL((rp_accumulate_kernel<C>), grid, dim3(256), 0, st, x, H, W, img, K, dtype, t);
}

}  // namespace

extern "C" {

int64_t cpn_props_workspace_bytes(int64_t table_capacity, int32_t intensity_channels) {
    if (rp_bad_capacity(table_capacity) || intensity_channels < 0 || intensity_channels > RP_MAX_K) return 0;
    const int64_t sort = table_capacity > 1024 ? table_capacity : 1024;
    return LT_HEAD_BYTES + table_capacity * rp_row_bytes(intensity_channels) + sort * 8;
}

int32_t cpn_props_columns(const int32_t *properties, int32_t n_properties, int32_t intensity_channels) {
    if (!properties || n_properties < 0 || n_properties > RP_MAX_PROPS || intensity_channels < 0 || intensity_channels > RP_MAX_K)
        return -1;
    int cols = 0;
    for (int i = 0; i < n_properties; ++i) {
        if (properties[i] < 0 || properties[i] >= CPN_PROP_COUNT) return -1;
        if (properties[i] >= CPN_PROP_INTENSITY_MEAN && intensity_channels == 0) return -1;
        cols += rp_prop_columns(properties[i], intensity_channels);
    }
    return cols;
}

int cpn_props_accumulate(const int32_t *labels, int32_t H, int32_t W, int32_t channels, const void *intensity,
                         int32_t intensity_channels, int32_t intensity_dtype, int64_t table_capacity, void *workspace,
                         int64_t workspace_bytes, void *stream) {
    if (H < 0 || W < 0 || channels < 1 || rp_bad_capacity(table_capacity) || !workspace || intensity_channels < 0 ||
        (intensity_channels > 0 && (!intensity || intensity_dtype < CPN_PROPS_U8 || intensity_dtype > CPN_PROPS_I32)))
        return cpn::fail(CPN_E_INVALID, "cpn_props_accumulate: bad arguments (table_capacity must be a power of two <= 2^28)");
    if (channels > RP_MAX_C) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_props_accumulate: more than 11 label channels");
    if (intensity_channels > RP_MAX_K) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_props_accumulate: more than 4 intensity channels");
    if ((int64_t) H * W > 0x7fffffff || H > 65536 || W > 65536)
        return cpn::fail(CPN_E_UNSUPPORTED, "cpn_props_accumulate: image larger than 2^31 - 1 pixels or 65536 a side");
    if (workspace_bytes < cpn_props_workspace_bytes(table_capacity, intensity_channels))
        return cpn::fail(CPN_E_WORKSPACE, "cpn_props_accumulate: workspace too small");
    if ((int64_t) H * W > 0 && (!labels || ((uintptr_t) labels & 15)))
        return cpn::fail(CPN_E_INVALID, "cpn_props_accumulate: the label image must be 16-byte aligned");
    hipStream_t st = (hipStream_t) stream;
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t) (LT_HEAD_BYTES + table_capacity * rp_row_bytes(intensity_channels)), st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_props_accumulate: memset");
    if ((int64_t) H * W == 0) return 0;
    const Table t = rp_table(workspace, table_capacity, intensity_channels);
    const dim3 grid((unsigned) ((W + RP_TILE_W - 1) / RP_TILE_W), (unsigned) ((H + RP_TILE_H - 1) / RP_TILE_H));
    const int K = intensity_channels, dt = intensity_dtype;
    switch (channels) {
        case 1: rp_launch<1>(st, grid, labels, H, W, intensity, K, dt, t); break;
        case 2: rp_launch<2>(st, grid, labels, H, W, intensity, K, dt, t); break;
        case 3: rp_launch<3>(st, grid, labels, H, W, intensity, K, dt, t); break;
        case 4: rp_launch<4>(st, grid, labels, H, W, intensity, K, dt, t); break;
        case 5: rp_launch<5>(st, grid, labels, H, W, intensity, K, dt, t); break;
        case 6: rp_launch<6>(st, grid, labels, H, W, intensity, K, dt, t); break;
        case 7: rp_launch<7>(st, grid, labels, H, W, intensity, K, dt, t); break;
        case 8: rp_launch<8>(st, grid, labels, H, W, intensity, K, dt, t); break;
        case 9: rp_launch<9>(st, grid, labels, H, W, intensity, K, dt, t); break;
        case 10: rp_launch<10>(st, grid, labels, H, W, intensity, K, dt, t); break;
        default: rp_launch<11>(st, grid, labels, H, W, intensity, K, dt, t); break;
    }
    return cpn::check_hip(hipGetLastError(), "cpn_props_accumulate");
}

int cpn_props_table_status(void *workspace, int64_t table_capacity, int64_t *status_host, void *stream) {
    if (!workspace || !status_host || rp_bad_capacity(table_capacity))
        return cpn::fail(CPN_E_INVALID, "cpn_props_table_status: bad arguments");
    return cpn::check_hip(lt_status(workspace, table_capacity, status_host, (hipStream_t) stream), "cpn_props_table_status");
}

int cpn_props_compact_sort(void *workspace, int64_t table_capacity, int32_t intensity_channels, int64_t entries, void *stream) {
    if (!workspace || rp_bad_capacity(table_capacity) || intensity_channels < 0 || intensity_channels > RP_MAX_K || entries < 0 ||
        entries > table_capacity)
        return cpn::fail(CPN_E_INVALID, "cpn_props_compact_sort: bad arguments");
    if (entries == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    u64 *head = (u64 *) workspace;
    u64 *buf = rp_sort_buffer(workspace, table_capacity, intensity_channels);
    const int64_t M = rp_sort_length(entries);
    hipError_t e = hipMemsetAsync(head + 2, 0, 8, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_props_compact_sort: memset");
    hipLaunchKernelGGL(rp_fill_kernel, dim3((unsigned) ((M + 255) / 256)), dim3(256), 0, st, buf, (long) M);
    hipLaunchKernelGGL(lt_compact_kernel<SortKeyEmit>, dim3(lt_scan_blocks(table_capacity)), dim3(256), 0, st, lt_keys(workspace),
                       (long) table_capacity, head + 2, SortKeyEmit{buf}, (long) entries);
    hipLaunchKernelGGL((rp_bitonic_local_kernel<true>), dim3((unsigned) (M / 1024)), dim3(512), 0, st, buf, (u64) 0);
    for (int64_t k = 2048; k <= M; k <<= 1) {
        for (int64_t j = k >> 1; j >= 1024; j >>= 1)
            hipLaunchKernelGGL(rp_bitonic_global_kernel, dim3((unsigned) ((M / 2 + 255) / 256)), dim3(256), 0, st, buf, (u64) (M / 2),
                               (u64) k, (u64) j);
        hipLaunchKernelGGL((rp_bitonic_local_kernel<false>), dim3((unsigned) (M / 1024)), dim3(512), 0, st, buf, (u64) k);
    }
    return cpn::check_hip(hipGetLastError(), "cpn_props_compact_sort");
}

int cpn_props_finalise(void *workspace, int64_t table_capacity, int32_t intensity_channels, int64_t entries,
                       const int32_t *properties, int32_t n_properties, double spacing_row, double spacing_col, int64_t *out,
                       int64_t out_columns, void *stream) {
    if (!workspace || rp_bad_capacity(table_capacity) || entries < 0 || entries > table_capacity)
        return cpn::fail(CPN_E_INVALID, "cpn_props_finalise: bad arguments");
    const int cols = cpn_props_columns(properties, n_properties, intensity_channels);
    if (cols < 0)
        return cpn::fail(CPN_E_INVALID, "cpn_props_finalise: bad property list (unknown code, more than 64 properties, or an "
                                        "intensity property without an intensity image)");
    if (out_columns != cols + 1) return cpn::fail(CPN_E_INVALID, "cpn_props_finalise: out must hold one row per column plus one");
    if (entries == 0) return 0;
    if (!out) return cpn::fail(CPN_E_INVALID, "cpn_props_finalise: out is NULL");
    Props p;
    p.n = n_properties;
    for (int i = 0; i < n_properties; ++i) p.code[i] = properties[i];
    hipStream_t st = (hipStream_t) stream;
    hipLaunchKernelGGL(rp_finalise_kernel, dim3((unsigned) ((entries + 255) / 256)), dim3(256), 0, st,
                       rp_sort_buffer(workspace, table_capacity, intensity_channels), (long) entries,
                       rp_table(workspace, table_capacity, intensity_channels), (int) intensity_channels, p, spacing_row,
                       spacing_col, out);
    return cpn::check_hip(hipGetLastError(), "cpn_props_finalise");
}

}  // extern "C"
