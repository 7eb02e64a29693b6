// Overlay images on the GPU (gfx950): the kernels behind celldetection_amd.contours2overlay and celldetection_amd.label_cmap
// (the reference's cd.data.contours2overlay, celldetection/data/cpn.py:647-662,699-723,811-855, and cd.label_cmap(ubyte=True),
// celldetection/visualization/cmaps.py:21-77; both called from celldetection_scripts/cpn_inference.py:839-848).
//
// contours2overlay.  Rule: with n(p) = number of contours whose filled polygon (csrc/polygon_fill.h, the rule of
// contours2labels) contains pixel p and S(p) = per-channel sum of their uint8 colours, out(p) = (floor(Sr / n), floor(Sg / n),
// floor(Sb / n), 255) where n >= 1 and (0, 0, 0, 0) elsewhere.  The reference keeps S and n as full-image arrays (10 B per
// pixel at uint16); here NO full-image intermediate exists: an OV_TILE x OV_TILE pixel tile belongs to one workgroup, which
// keeps S and n of its pixels in LDS (two 64-bit words per pixel: Sr | Sg << 32 and Sb | n << 32, 16 KiB), walks the contours
// whose bounding box meets the tile and writes every pixel of the tile exactly once, zeros included: no memset and no global
// atomic on the image.  All arithmetic is integer, so the result does not depend on the order of the contours in a list.
//
// Binning (one thread per contour, looping over the tiles of its box: sized for cell contours of a few tiles each; a contour
// that spans a whole 16384 x 16384 image issues its 2.6 * 10^5 atomics from one lane, twice, which is correct but serial).
// ov_count_kernel adds, per contour, one to the counter of every tile its box (of cpn_labels_prepare) meets; the
// caller turns the counters into list offsets (an exclusive scan); ov_fill_kernel writes the contour index into the list of
// each of its tiles through a per-tile cursor.  A contour may span any number of tiles and a tile may hold any number of
// contours: the paint kernel walks its list in chunks of OV_CHUNK contours, and nothing in LDS is sized by the list.
//
// Paint.  A work item is (contour of the chunk, row of the tile): one thread walks the contour's edges ONCE for that row
// (lb_filled_row32: boundary pixels by on_line, scanline crossings as parity toggles) and gets the 32 pixels of the row as a bit
// mask, then adds the colour to the LDS sums of the set pixels with ds_add_u64.  The per-pixel form (lb_filled) would walk all
// edges for every pixel.  The points are read from global memory: the 32 lanes of a contour read the same address.  The
// largest n of the image goes to one device word (a wave maximum, then one atomicMax per wave), which the host reads once:
// beyond iinfo(intermediate_dtype).max / 255 overlapping contours the reference's sums wrap.
//
// label_cmap.  One streaming kernel: int32 labels [pixels][C], channel-interleaved, one thread per pixel; the uint8 RGBA table
// (row 0 = the zero label) sits in LDS (up to OV_LDS_ROWS rows, else it is read through the cache); label v -> row v % n + 1,
// 0 -> row 0.  Without reduction the pixel is its table row.  With it (cmaps.py:70-75) the channels are averaged with their
// alpha as weight, in float32 and in exactly the reference's order: den = float(sum_c a_c) + 1e-12f; for c = 0 .. C-1:
// w = a_c / den (correctly rounded), acc_j = acc_j + w * col_cj (separate multiply and add: the unit is compiled with
// -ffp-contract=off); the result is acc_j truncated.  Negative labels are flagged (one atomicOr per wave that saw one).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "polygon_fill.h"

namespace {

typedef unsigned long long u64;

constexpr int OV_TILE = CPN_OVERLAY_TILE, OV_SHIFT = 5;
static_assert(OV_TILE == 32 && (1 << OV_SHIFT) == OV_TILE, "a row of a tile is one 32-bit mask");
constexpr int OV_CHUNK = 256 / OV_TILE;  // contours per pass of the paint kernel: one thread per (contour, row)
constexpr int OV_MAX_S = 512;            // points per contour (the limit of cpn_labels_prepare)
constexpr int OV_LDS_ROWS = 10240;       // colour-table rows kept in LDS (40 KiB): 'rand' draws at most 9999 + the zero row
constexpr int64_t OV_CMAP_GRID = 2048;   // workgroups of the colour-map kernel, walking the image; each loads the table once:
                                         // 8 per CU with a small table, 4 resident at a time with the 40 KiB of a 'rand' table

// the tiles a box meets, clamped to the grid: x in [tx0, tx1], y in [ty0, ty1]; false: none
__device__ __forceinline__ bool ov_tile_range(const int32_t *b, int H, int W, int &tx0, int &ty0, int &tx1, int &ty1) {
    const int x0 = max(b[0], 0), y0 = max(b[1], 0), x1 = min(b[2], W - 1), y1 = min(b[3], H - 1);
    if (x1 < x0 || y1 < y0) return false;
    tx0 = x0 >> OV_SHIFT; ty0 = y0 >> OV_SHIFT; tx1 = x1 >> OV_SHIFT; ty1 = y1 >> OV_SHIFT;
    return true;
}

__global__ __launch_bounds__(256) void ov_count_kernel(const int32_t *__restrict__ boxes, long K, int H, int W, int tiles_x,
                                                      int32_t *__restrict__ tile_count) {
    const long k = blockIdx.x * 256l + threadIdx.x;
    if (k >= K) return;
    int tx0, ty0, tx1, ty1;
    if (!ov_tile_range(boxes + k * 4, H, W, tx0, ty0, tx1, ty1)) return;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(&tile_count[(long) ty * tiles_x + tx], 1);
}

__global__ __launch_bounds__(256) void ov_fill_kernel(const int32_t *__restrict__ boxes, long K, int H, int W, int tiles_x,
                                                     const int32_t *__restrict__ tile_begin, int32_t *__restrict__ cursor,
                                                     int32_t *__restrict__ list, long pairs) {
    const long k = blockIdx.x * 256l + threadIdx.x;
    if (k >= K) return;
    int tx0, ty0, tx1, ty1;
    if (!ov_tile_range(boxes + k * 4, H, W, tx0, ty0, tx1, ty1)) return;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const long t = (long) ty * tiles_x + tx;
            const long pos = (long) tile_begin[t] + atomicAdd(&cursor[t], 1);
            if (pos < pairs) list[pos] = (int32_t) k;  // always, when the counters came from ov_count_kernel on the same boxes
        }
}

__global__ __launch_bounds__(256) void ov_paint_kernel(const int32_t *__restrict__ pts, const int32_t *__restrict__ boxes,
                                                      const uint8_t *__restrict__ colors, long K, int S, int H, int W,
                                                      int tiles_x, const int32_t *__restrict__ tile_begin,
                                                      const int32_t *__restrict__ list, uint32_t *__restrict__ out,
                                                      uint32_t *__restrict__ max_overlap) {
    __shared__ u64 acc_rg[OV_TILE * OV_TILE], acc_bn[OV_TILE * OV_TILE];  // Sr | Sg << 32 and Sb | n << 32 per pixel
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int px0 = tx << OV_SHIFT, py0 = ty << OV_SHIFT;
    for (int i = tid; i < OV_TILE * OV_TILE; i += 256) { acc_rg[i] = 0; acc_bn[i] = 0; }
    __syncthreads();
    const int begin = tile_begin[blockIdx.x], end = tile_begin[blockIdx.x + 1];
    const int row = tid & (OV_TILE - 1), yy = py0 + row;
    for (int base = begin; base < end; base += OV_CHUNK) {  // the same trip count for the whole workgroup
        const int i = base + (tid >> OV_SHIFT);
        if (i >= end) continue;
        const long k = list[i];
        if (k < 0 || k >= K) continue;
        const int32_t *b = boxes + k * 4;
        if (yy < b[1] || yy > b[3] || yy >= H) continue;
        unsigned int m = lb_filled_row32(px0, yy, reinterpret_cast<const int2 *>(pts) + k * S, S);
        if (!m) continue;
        const u64 rg = (u64) colors[k * 3] | (u64) colors[k * 3 + 1] << 32, bn = (u64) colors[k * 3 + 2] | 1ull << 32;
        while (m) {
            const int c = __ffs(m) - 1;
            m &= m - 1;
            atomicAdd(&acc_rg[row * OV_TILE + c], rg);
            atomicAdd(&acc_bn[row * OV_TILE + c], bn);
        }
    }
    __syncthreads();
    unsigned int n_max = 0;
    for (int i = tid; i < OV_TILE * OV_TILE; i += 256) {  // consecutive lanes: consecutive pixels of a row
        const int y = py0 + (i >> OV_SHIFT), x = px0 + (i & (OV_TILE - 1));
        if (y >= H || x >= W) continue;
        const u64 rg = acc_rg[i], bn = acc_bn[i];
        const unsigned int n = (unsigned int) (bn >> 32);
        uint32_t v = 0;
        if (n) {
            const unsigned int r = (unsigned int) rg / n, g = (unsigned int) (rg >> 32) / n, bl = (unsigned int) bn / n;
            v = (r & 255u) | (g & 255u) << 8 | (bl & 255u) << 16 | 255u << 24;  // bytes r, g, b, a in memory order
        }
        out[(size_t) y * W + x] = v;
        n_max = max(n_max, n);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n_max = max(n_max, (unsigned int) __shfl_xor((int) n_max, d, 64));
    if ((tid & 63) == 0 && n_max) atomicMax(max_overlap, n_max);
}

// REDUCE: weighted average over the channels; otherwise (C == 1) the table row itself
template <bool REDUCE>
__global__ __launch_bounds__(256) void ov_cmap_kernel(const int32_t *__restrict__ labels, long n_pix, int C,
                                                     const uint32_t *__restrict__ table, int rows, int lds_rows,
                                                     uint32_t *__restrict__ out, int32_t *__restrict__ flag) {
    extern __shared__ uint32_t ov_table[];
    for (int i = threadIdx.x; i < lds_rows; i += 256) ov_table[i] = table[i];
    __syncthreads();
    const uint32_t *tab = lds_rows ? ov_table : table;
    const int n = rows - 1;  // colours; row 0 is the zero label
    bool neg = false;
    for (long p = blockIdx.x * 256l + threadIdx.x; p < n_pix; p += (long) gridDim.x * 256l) {
        const int32_t *x = labels + p * C;
        uint32_t res;
        if constexpr (!REDUCE) {
            const int32_t v = x[0];
            neg |= v < 0;
            res = tab[v > 0 ? v % n + 1 : 0];
        } else {
            int asum = 0;
            for (int c = 0; c < C; ++c) {
                const int32_t v = x[c];
                neg |= v < 0;
                asum += (int) (tab[v > 0 ? v % n + 1 : 0] >> 24);
            }
            const float den = (float) asum + 1e-12f;
            float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
            for (int c = 0; c < C; ++c) {
                const int32_t v = x[c];
                const uint32_t col = tab[v > 0 ? v % n + 1 : 0];
                const float w = (float) (col >> 24) / den;
                acc0 = acc0 + w * (float) (col & 255u);
                acc1 = acc1 + w * (float) (col >> 8 & 255u);
                acc2 = acc2 + w * (float) (col >> 16 & 255u);
                acc3 = acc3 + w * (float) (col >> 24);
            }
            res = ((uint32_t) (int) acc0 & 255u) | ((uint32_t) (int) acc1 & 255u) << 8 | ((uint32_t) (int) acc2 & 255u) << 16 |
                  ((uint32_t) (int) acc3 & 255u) << 24;
        }
        out[p] = res;
    }
    if (__ballot(neg) && __lane_id() == 0) atomicOr(flag, 1);
}

int ov_check_image(const char *what, int32_t H, int32_t W) {
    if (H < 1 || W < 1) return cpn::fail(CPN_E_INVALID, what);
    if ((int64_t) H * W > 0x7fffffff) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_overlay: more than 2^31 - 1 pixels");
    return 0;
}

}  // namespace

extern "C" {

int cpn_overlay_bin_count(const int32_t *boxes, int64_t K, int32_t H, int32_t W, int32_t *tile_count, void *stream) {
    if (K < 0 || (K > 0 && (!boxes || !tile_count))) return cpn::fail(CPN_E_INVALID, "cpn_overlay_bin_count: bad arguments");
    if (const int rc = ov_check_image("cpn_overlay_bin_count: bad image size", H, W)) return rc;
    if (K == 0) return 0;
    hipLaunchKernelGGL(ov_count_kernel, dim3((unsigned) ((K + 255) / 256)), dim3(256), 0, (hipStream_t) stream, boxes, (long) K,
                       H, W, (W + OV_TILE - 1) >> OV_SHIFT, tile_count);
    return cpn::check_hip(hipGetLastError(), "cpn_overlay_bin_count");
}

int cpn_overlay_bin_fill(const int32_t *boxes, int64_t K, int32_t H, int32_t W, const int32_t *tile_begin, int32_t *cursor,
                         int32_t *list, int64_t pairs, void *stream) {
    if (K < 0 || pairs < 0 || pairs > 0x7fffffff || (K > 0 && (!boxes || !tile_begin || !cursor || (pairs > 0 && !list))))
        return cpn::fail(CPN_E_INVALID, "cpn_overlay_bin_fill: bad arguments");
    if (const int rc = ov_check_image("cpn_overlay_bin_fill: bad image size", H, W)) return rc;
    if (K == 0) return 0;
    hipLaunchKernelGGL(ov_fill_kernel, dim3((unsigned) ((K + 255) / 256)), dim3(256), 0, (hipStream_t) stream, boxes, (long) K,
                       H, W, (W + OV_TILE - 1) >> OV_SHIFT, tile_begin, cursor, list, (long) pairs);
    return cpn::check_hip(hipGetLastError(), "cpn_overlay_bin_fill");
}

int cpn_overlay_paint(const int32_t *points, const int32_t *boxes, const uint8_t *colors, int64_t K, int32_t S, int32_t H,
                      int32_t W, const int32_t *tile_begin, const int32_t *list, uint8_t *out, uint32_t *max_overlap,
                      uint32_t *max_overlap_host, void *stream) {
    if (K < 0 || S < 1 || S > OV_MAX_S || !tile_begin || !out || !max_overlap || (K > 0 && (!points || !boxes || !colors)))
        return cpn::fail(CPN_E_INVALID, "cpn_overlay_paint: bad arguments (1 <= points per contour <= 512)");
    if (const int rc = ov_check_image("cpn_overlay_paint: bad image size", H, W)) return rc;
    if (((uintptr_t) out & 3) || ((uintptr_t) points & 7))
        return cpn::fail(CPN_E_INVALID, "cpn_overlay_paint: out must be 4-byte and points 8-byte aligned");
    hipStream_t st = (hipStream_t) stream;
    const int tiles_x = (W + OV_TILE - 1) >> OV_SHIFT, tiles_y = (H + OV_TILE - 1) >> OV_SHIFT;
    hipLaunchKernelGGL(ov_paint_kernel, dim3((unsigned) (tiles_x * tiles_y)), dim3(256), 0, st, points, boxes, colors, (long) K,
                       S, H, W, tiles_x, tile_begin, list, reinterpret_cast<uint32_t *>(out), max_overlap);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_overlay_paint");
    if (!max_overlap_host) return 0;
    e = hipMemcpyAsync(max_overlap_host, max_overlap, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return cpn::check_hip(e, "cpn_overlay_paint: largest overlap");
}

int cpn_label_cmap(const int32_t *labels, int64_t pixels, int32_t channels, int32_t reduce, const uint8_t *table, int32_t rows,
                   uint8_t *out, int32_t *flag, int32_t *flag_host, void *stream) {
    if (pixels < 0 || channels < 1 || rows < 2 || !table || !flag || (pixels > 0 && (!labels || !out)))
        return cpn::fail(CPN_E_INVALID, "cpn_label_cmap: bad arguments (the table holds the zero row and at least one colour)");
    if (!reduce && channels != 1)
        return cpn::fail(CPN_E_INVALID, "cpn_label_cmap: more than one channel needs the reduction");
    if (pixels > 0x7fffffff) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_label_cmap: more than 2^31 - 1 pixels");
    if (((uintptr_t) out & 3) || ((uintptr_t) table & 3))
        return cpn::fail(CPN_E_INVALID, "cpn_label_cmap: out and table must be 4-byte aligned");
    hipStream_t st = (hipStream_t) stream;
    if (pixels > 0) {
        const int64_t blocks = (pixels + 255) / 256;
        const unsigned grid = (unsigned) (blocks < OV_CMAP_GRID ? blocks : OV_CMAP_GRID);
        const int lds_rows = rows <= OV_LDS_ROWS ? rows : 0;
        const uint32_t *tab = reinterpret_cast<const uint32_t *>(table);
        uint32_t *o = reinterpret_cast<uint32_t *>(out);
        if (reduce)
            hipLaunchKernelGGL((ov_cmap_kernel<true>), dim3(grid), dim3(256), (size_t) lds_rows * 4, st, labels, (long) pixels,
                               channels, tab, rows, lds_rows, o, flag);
        else
            hipLaunchKernelGGL((ov_cmap_kernel<false>), dim3(grid), dim3(256), (size_t) lds_rows * 4, st, labels, (long) pixels,
                               channels, tab, rows, lds_rows, o, flag);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return cpn::check_hip(e, "cpn_label_cmap");
    }
    if (!flag_host) return 0;
    hipError_t e = hipMemcpyAsync(flag_host, flag, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return cpn::check_hip(e, "cpn_label_cmap: flag");
}

}  // extern "C"
