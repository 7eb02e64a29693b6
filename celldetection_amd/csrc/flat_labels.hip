// Flat label images on the GPU (gfx950): the kernels behind celldetection_amd.resolve_label_channels (the reference's
// cd.data.resolve_label_channels, celldetection/data/cpn.py:361-399).  Integer only.
//
// Rule.  A pixel of the int32 [H][W][C] image is an OVERLAP pixel when more than one channel is > 0 and a CORE pixel when
// exactly one is.  Without any overlap pixel the result is the plain channel maximum.  Otherwise lbl = channel maximum at
// core pixels, 0 elsewhere, and in synchronous steps every overlap pixel that still holds 0 takes the maximum of lbl over
// its footprint neighbours (default: the 4-neighbourhood; neighbours outside the image take no part), all pixels at once
// from the values of the previous step, until nothing is unresolved, a step changes nothing or max_iter steps are done.
//
// Encoding.  lbl holds > 0 = label, 0 = background (never changes) and FL_UNRES = -1 = overlap pixel without a label yet.
// Every neighbour value <= 0 loses against the floor 0 of the maximum, so -1 needs no special case in the inner loop, a
// pixel changes exactly once (-1 -> label), and "unresolved pixels" = overlap pixels - pixels changed so far.
//
// Classify pass (fl_classify_kernel).  One read of the channel-interleaved image: a thread owns 4 consecutive pixels =
// C dwordx4 loads (any C up to 8; more channels take one pixel per thread), computes positive count and maximum per pixel,
// writes one dwordx4 of lbl, marks the tiles that hold overlap pixels and counts overlap pixels and pixels whose maximum is
// negative.  A fixed grid walks the image and keeps the counts in registers (two atomics per wave in all), and lanes that
// share a tile mark it once.  With plain != 0 it writes the plain maximum instead (the no-overlap result; only needed again
// when negative maxima exist, since lbl and the plain maximum agree everywhere else).
//
// Propagation (fl_step_kernel), blocked in space and time.  A workgroup owns a TS x TS tile, loads it with a halo of T
// pixels into LDS and runs up to T synchronous steps there; after k steps a pixel depends only on values within distance k
// (L-infinity, which covers every 3 x 3 footprint), so whatever the missing surroundings spoil stays inside the halo and the
// tile interior is exact.  A step is synchronous by construction: every thread first reads the neighbours of its
// unresolved pixels into registers, a barrier, then the pixels that received a label are written, a barrier.  The interior
// goes to a SECOND global image (neighbouring workgroups read their halos from the first one during the same launch), and
// fl_commit_kernel copies the tiles that changed back.  Only tiles that hold unresolved pixels AND whose 3 x 3 tile
// neighbourhood changed in the previous launch run (a tile plus halo that did not change gives the same interior again):
// fl_list_kernel compacts them into a worklist on the device, and fixed grids of workgroups walk that list, so a launch
// costs what its active tiles cost, whatever the image size.  A workgroup leaves a tile early when a step changes nothing
// in its region.  The host reads 16 bytes per launch: pixels changed and tiles run.
//
// Tile size: TS = 32, T = 8.  LDS per workgroup = one image of (TS + 2 T + 2)^2 int32 = 50^2 * 4 = 10 000 B (one more ring
// of zeros saves every bounds check); a thread owns K = (TS + 2 T)^2 / 256 = 9 region pixels with one register each for the
// step's new values: 68 VGPRs, 7 waves per SIMD, 7 workgroups per CU; 44 % of the region is interior.  The measurements
// behind the choice (a 64 / 16 shape was built as well) are in profiles/flat_labels.txt.  Row-major LDS image with lanes
// on consecutive pixels: the four neighbour reads of a step (+-1, +-row) and the write are conflict-free for ds_read_b32 /
// ds_write_b32 (32 consecutive dwords per half wave) wherever all lanes take part.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"

namespace {

typedef unsigned long long u64;

constexpr int FL_UNRES = -1;
constexpr int FL_PPT = 4;              // pixels per thread of the classify pass
constexpr int FL_VEC_C = 8;            // up to this many channels: kernels for the exact channel count
constexpr int64_t FL_GRID = 4096;      // workgroups of the classify pass and of the worklist kernels (16 per CU)
constexpr int64_t FL_HEAD_BYTES = 64;  // counters in front of the workspace: [0] overlap pixels, [1] pixels with a negative
                                       // maximum, [2] pixels changed by the last launch, [3] tiles run by the last launch = length of its worklist
constexpr int FL_TS = 32, FL_SHIFT = 5;  // side of a propagation tile
constexpr int FL_T = CPN_FLAT_MAX_STEPS;  // halo = steps per launch
static_assert(FL_T == 8 && (1 << FL_SHIFT) == FL_TS, "tile geometry");
constexpr unsigned FL_CROSS = 0272;    // footprint bits, bit 3 * row + column: 010 / 111 / 010

inline int64_t fl_align(int64_t n) { return (n + 63) & ~(int64_t) 63; }

struct Layout {  // the workspace behind the counters
    int tiles_x, tiles_y;
    int64_t tiles;
    int64_t scratch, unres, chg, act, list, bytes;  // byte offsets
};

inline Layout fl_layout(int64_t H, int64_t W) {
    Layout l;
    l.tiles_x = (int) ((W + FL_TS - 1) >> FL_SHIFT);
    l.tiles_y = (int) ((H + FL_TS - 1) >> FL_SHIFT);
    l.tiles = (int64_t) l.tiles_x * l.tiles_y;
    l.scratch = FL_HEAD_BYTES;
    l.unres = l.scratch + fl_align(H * W * 4);
    l.chg = l.unres + fl_align(l.tiles);
    l.act = l.chg + fl_align(l.tiles);
    l.list = l.act + 2 * fl_align(l.tiles);
    l.bytes = l.list + fl_align(l.tiles * 4);
    return l;
}

__device__ __forceinline__ void fl_wave_add(u64 *counter, unsigned n) {  // all 64 lanes call this together
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    if (__lane_id() == 0 && n) atomicAdd(counter, (u64) n);
}

// C > 0: exactly C channels, FL_PPT pixels per thread and round with dwordx4 loads.  C == 0: c_rt channels, one pixel per
// thread and round.  A fixed grid walks the image in `rounds` rounds (the same for every thread: the wave merges need all
// lanes) and keeps its counts in registers: two atomics per wave at the end, and one tile mark per run of lanes that share
// a tile (same-address atomics and stores per overlap pixel cost several times the memory traffic).
template <int C>
__global__ __launch_bounds__(256) void fl_classify_kernel(const int32_t *__restrict__ x, int c_rt, long n, int W, int plain,
                                                         int32_t *__restrict__ lbl, int shift, int tiles_x, int rounds,
                                                         uint8_t *__restrict__ unres, u64 *__restrict__ counters) {
    constexpr int PPT = C > 0 ? FL_PPT : 1;
    const int lane = __lane_id();
    unsigned n_over = 0, n_neg = 0;
    for (int rd = 0; rd < rounds; ++rd) {
        const long p0 = (((long) rd * gridDim.x + blockIdx.x) * 256 + threadIdx.x) * PPT;
        int32_t out[PPT];
        int row = 0, col = 0, mark = -1;  // mark: the tile of this thread's overlap pixels (a second one is marked directly)
        if (p0 < n) {
            row = (int) (p0 / W);
            col = (int) (p0 - (long) row * W);
        }
        if constexpr (C > 0) {
            int32_t v[PPT * C];
            if (p0 + PPT <= n) {
                const int4 *q = reinterpret_cast<const int4 *>(x + p0 * C);  // 16 * C bytes per thread: 16-byte aligned
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    const int4 w = q[i];
                    v[4 * i] = w.x; v[4 * i + 1] = w.y; v[4 * i + 2] = w.z; v[4 * i + 3] = w.w;
                }
            } else {
#pragma unroll
                for (int p = 0; p < PPT; ++p)
#pragma unroll
                    for (int c = 0; c < C; ++c) v[p * C + c] = p0 + p < n ? x[(p0 + p) * C + c] : 0;
            }
#pragma unroll
            for (int p = 0; p < PPT; ++p) {
                int cnt = 0, mx = v[p * C];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    cnt += v[p * C + c] > 0;
                    mx = max(mx, v[p * C + c]);
                }
                const bool in = p0 + p < n, over = in && cnt > 1;
                n_over += over;
                n_neg += in && mx < 0;
                out[p] = plain ? mx : (cnt > 1 ? FL_UNRES : (cnt == 1 ? mx : 0));
                if (over) {
                    const int tl = (row >> shift) * tiles_x + (col >> shift);
                    if (mark < 0) mark = tl;
                    else if (tl != mark) unres[tl] = 1;  // the thread's pixels span two tiles (a row end inside them)
                }
                if (++col == W) { col = 0; ++row; }
            }
            if (p0 + PPT <= n) {
                *reinterpret_cast<int4 *>(lbl + p0) = make_int4(out[0], out[1], out[2], out[3]);  // p0 is a multiple of 4
            } else {
#pragma unroll
                for (int p = 0; p < PPT; ++p)
                    if (p0 + p < n) lbl[p0 + p] = out[p];
            }
        } else {
            if (p0 < n) {
                int cnt = 0, mx = x[p0 * c_rt];
                for (int c = 0; c < c_rt; ++c) {
                    const int32_t v = x[p0 * c_rt + c];
                    cnt += v > 0;
                    mx = max(mx, v);
                }
                n_over += cnt > 1;
                n_neg += mx < 0;
                lbl[p0] = plain ? mx : (cnt > 1 ? FL_UNRES : (cnt == 1 ? mx : 0));
                if (cnt > 1) mark = (row >> shift) * tiles_x + (col >> shift);
            }
        }
        const int prev = __shfl_up(mark, 1, 64);
        if (mark >= 0 && (lane == 0 || prev != mark)) unres[mark] = 1;  // the same value from every writer
    }
    fl_wave_add(&counters[0], n_over);
    fl_wave_add(&counters[1], n_neg);
}

// The worklist of a launch: every tile with unresolved pixels that is active (first launch: all of them), in no
// particular order (the result does not depend on it).  *count must be 0 before.
__global__ __launch_bounds__(256) void fl_list_kernel(const uint8_t *__restrict__ unres, const uint8_t *__restrict__ act_cur,
                                                     int first, int tiles, int32_t *__restrict__ list, u64 *__restrict__ count) {
    const int t = blockIdx.x * 256 + threadIdx.x, lane = __lane_id();
    const bool on = t < tiles && unres[t] && (first || act_cur[t]);
    const u64 m = __ballot(on);
    if (m == 0) return;
    u64 base = 0;
    if (lane == 0) base = atomicAdd(count, (u64) __popcll(m));
    base = __shfl(base, 0, 64);
    if (on) list[base + __popcll(m & ((1ull << lane) - 1))] = t;
}

// One launch = up to T synchronous steps on every tile of the worklist.  src is read (tile + halo), dst receives the interior
// of the tiles that changed.  LDS: ONE image of RP x RP int32, RP = TS + 2 T + 2; the outermost ring stays 0.  A thread owns K =
// R * R / 256 pixels of the region and keeps, in a register bit mask, which of them are unresolved: a step reads the
// footprint neighbours of those only, into registers; after a barrier the pixels that received a label are written (a pixel
// changes once) and leave the mask.  Resolved and background pixels, the bulk of every tile, cost nothing per step.
template <int TS, int T, bool CROSS>
__global__ __launch_bounds__(256) void fl_step_kernel(const int32_t *__restrict__ src, int32_t *__restrict__ dst, int H, int W,
                                                     int tiles_x, int tiles_y, int steps, unsigned fp,
                                                     const int32_t *__restrict__ list, const u64 *__restrict__ count,
                                                     uint8_t *__restrict__ unres, uint8_t *__restrict__ act_next,
                                                     uint8_t *__restrict__ chg, u64 *__restrict__ counters) {
    constexpr int R = TS + 2 * T, RP = R + 2, K = R * R / 256;
    static_assert(R * R % 256 == 0 && K <= 64, "a thread owns K pixels, one mask bit each");
    extern __shared__ __attribute__((aligned(16))) int32_t fl_lds[];
    __shared__ int totals[2];  // interior pixels changed, interior pixels still unresolved
    const int n_work = (int) *count;
    for (int work = blockIdx.x; work < n_work; work += gridDim.x) {  // the same trip count for the whole workgroup
    const int tile = list[work];
    const int tid = threadIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * TS - T, x0 = tx * TS - T;  // image position of region pixel (0, 0)
    int32_t *a = fl_lds;
    if (tid < 2) totals[tid] = 0;
    for (int i = tid; i < RP * RP; i += 256) {  // the ring
        const int r = i / RP, c = i % RP;
        if (r == 0 || r == RP - 1 || c == 0 || c == RP - 1) a[i] = 0;
    }
    u64 mask = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = tid + 256 * k, r = i / R, c = i % R;
        const int y = y0 + r, x = x0 + c;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        const int32_t v = in ? src[(long) y * W + x] : 0;  // outside the image: 0 never wins a maximum and never changes
        a[(r + 1) * RP + c + 1] = v;
        mask |= (u64) (v == FL_UNRES) << k;
    }
    const u64 mask0 = mask;
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        int32_t nv[K];
        int changed = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            nv[k] = 0;
            if (mask >> k & 1) {
                const int i = tid + 256 * k, idx = (i / R + 1) * RP + i % R + 1;
                int32_t m = 0;
                if constexpr (CROSS) {
                    m = max(max(a[idx - 1], a[idx + 1]), max(a[idx - RP], a[idx + RP]));
                } else {
#pragma unroll
                    for (int j = 0; j < 9; ++j)
                        if (fp >> j & 1) m = max(m, a[idx + (j / 3 - 1) * RP + (j % 3 - 1)]);
                }
                nv[k] = m;
                changed |= m > 0;
            }
        }
        if (!__syncthreads_or(changed)) break;  // a fixed point of the whole region (every read is done: safe to write below)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (nv[k] > 0) {
                const int i = tid + 256 * k;
                a[(i / R + 1) * RP + i % R + 1] = nv[k];
                mask &= ~((u64) 1 << k);
            }
        }
        __syncthreads();
    }
    // interior: what received a label in this launch, what is left
    const int h_in = min(TS, H - ty * TS), w_in = min(TS, W - tx * TS);
    int n_chg = 0, n_left = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = tid + 256 * k, r = i / R - T, c = i % R - T;
        if (r >= 0 && r < h_in && c >= 0 && c < w_in) {
            n_chg += (int) ((mask0 & ~mask) >> k & 1);
            n_left += (int) (mask >> k & 1);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        n_chg += __shfl_xor(n_chg, d, 64);
        n_left += __shfl_xor(n_left, d, 64);
    }
    if ((tid & 63) == 0) {
        if (n_chg) atomicAdd(&totals[0], n_chg);
        if (n_left) atomicAdd(&totals[1], n_left);
    }
    __syncthreads();
    const int t_chg = totals[0], t_left = totals[1];
    if (t_chg) {
        for (int i = tid; i < TS * TS; i += 256) {
            const int r = i / TS, c = i % TS;
            if (r < h_in && c < w_in) dst[(long) (ty * TS + r) * W + tx * TS + c] = a[(r + T + 1) * RP + c + T + 1];
        }
    }
    if (tid == 0) {
        if (t_left == 0) unres[tile] = 0;  // only this workgroup reads or writes the flag of its tile during a launch
        if (t_chg) {
            atomicAdd(&counters[2], (u64) t_chg);
            chg[tile] = 1;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int yy = ty + dy, xx = tx + dx;
                    if (yy >= 0 && yy < tiles_y && xx >= 0 && xx < tiles_x) act_next[yy * tiles_x + xx] = 1;
                }
        }
    }
    __syncthreads();  // the LDS image and the totals are free for the next tile
    }
}

// FINISH == false: the interior of every tile of the worklist that changed, dst (second image) -> lbl.
// FINISH == true:  what is still unresolved in lbl becomes 0, over all `tiles` tiles (list == nullptr).
template <int TS, bool FINISH>
__global__ __launch_bounds__(256) void fl_commit_kernel(int32_t *__restrict__ lbl, const int32_t *__restrict__ dst, int H, int W,
                                                       int tiles_x, const uint8_t *__restrict__ flag,
                                                       const int32_t *__restrict__ list, const u64 *__restrict__ count, int tiles) {
    const int n_work = FINISH ? tiles : (int) *count;
    for (int work = blockIdx.x; work < n_work; work += gridDim.x) {
        const int tile = FINISH ? work : list[work];
        if (!flag[tile]) continue;
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int h_in = min(TS, H - ty * TS), w_in = min(TS, W - tx * TS);
        for (int i = threadIdx.x; i < TS * TS; i += 256) {
            const int r = i / TS, c = i % TS;
            if (r < h_in && c < w_in) {
                const long g = (long) (ty * TS + r) * W + tx * TS + c;
                if constexpr (FINISH) {
                    if (lbl[g] == FL_UNRES) lbl[g] = 0;
                } else {
                    lbl[g] = dst[g];
                }
            }
        }
    }
}

template <bool CROSS>
int fl_launch_step(hipStream_t st, int32_t *lbl, int32_t *scratch, int H, int W, const Layout &l, int steps, unsigned fp,
                   int first, uint8_t *unres, uint8_t *act_cur, uint8_t *act_next, uint8_t *chg, int32_t *list, u64 *counters) {
    constexpr int RP = FL_TS + 2 * FL_T + 2;
    constexpr int lds = RP * RP * 4;
    const unsigned grid = (unsigned) (l.tiles < FL_GRID ? l.tiles : FL_GRID);
    hipLaunchKernelGGL(fl_list_kernel, dim3((unsigned) ((l.tiles + 255) / 256)), dim3(256), 0, st, unres, act_cur, first,
                       (int) l.tiles, list, counters + 3);
    hipLaunchKernelGGL((fl_step_kernel<FL_TS, FL_T, CROSS>), dim3(grid), dim3(256), lds, st, lbl, scratch, H, W, l.tiles_x,
                       l.tiles_y, steps, fp, list, counters + 3, unres, act_next, chg, counters);
    hipLaunchKernelGGL((fl_commit_kernel<FL_TS, false>), dim3(grid), dim3(256), 0, st, lbl, scratch, H, W, l.tiles_x, chg, list,
                       counters + 3, (int) l.tiles);
    return cpn::check_hip(hipGetLastError(), "cpn_flat_step");
}

}  // namespace

extern "C" {

int64_t cpn_flat_workspace_bytes(int32_t H, int32_t W) {
    if (H < 0 || W < 0) return 0;
    return fl_layout(H, W).bytes;
}

int cpn_flat_classify(const int32_t *labels, int32_t channels, int32_t H, int32_t W, int32_t plain_max, int32_t *lbl,
                      void *workspace, int64_t workspace_bytes, int64_t *status_host, void *stream) {
    if (channels < 1 || H < 0 || W < 0 || !workspace) return cpn::fail(CPN_E_INVALID, "cpn_flat_classify: bad arguments");
    const int64_t n = (int64_t) H * W;
    if (n > 0x7fffffff) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_flat_classify: more than 2^31 - 1 pixels");
    const Layout l = fl_layout(H, W);
    if (workspace_bytes < l.bytes) return cpn::fail(CPN_E_WORKSPACE, "cpn_flat_classify: workspace too small");
    if (n > 0 && (!labels || !lbl || ((uintptr_t) labels & 15) || ((uintptr_t) lbl & 15)))
        return cpn::fail(CPN_E_INVALID, "cpn_flat_classify: images must be 16-byte aligned");
    hipStream_t st = (hipStream_t) stream;
    char *w = (char *) workspace;
    u64 *counters = (u64 *) w;
    uint8_t *unres = (uint8_t *) (w + l.unres);
    hipError_t e = hipMemsetAsync(counters, 0, FL_HEAD_BYTES, st);
    if (e == hipSuccess) e = hipMemsetAsync(unres, 0, (size_t) (l.bytes - l.unres), st);  // every tile flag
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_flat_classify: memset");
    if (n > 0) {
        // a fixed grid (16 workgroups for each of the 256 CUs) that walks the image in rounds
        int64_t blocks = (n + 256 * FL_PPT - 1) / (256 * FL_PPT);
        const unsigned vec_blocks = (unsigned) (blocks < FL_GRID ? blocks : FL_GRID);
        const int vec_rounds = (int) ((blocks + vec_blocks - 1) / vec_blocks);
#define FL_CASE(C)                                                                                                       \
    case C:                                                                                                              \
        hipLaunchKernelGGL((fl_classify_kernel<C>), dim3(vec_blocks), dim3(256), 0, st, labels, C, (long) n, W, plain_max, \
                           lbl, FL_SHIFT, l.tiles_x, vec_rounds, unres, counters);                                       \
        break;
        switch (channels <= FL_VEC_C ? channels : 0) {
            FL_CASE(1) FL_CASE(2) FL_CASE(3) FL_CASE(4) FL_CASE(5) FL_CASE(6) FL_CASE(7) FL_CASE(8)
            default: {
                blocks = (n + 255) / 256;
                const unsigned grid = (unsigned) (blocks < FL_GRID ? blocks : FL_GRID);
                hipLaunchKernelGGL((fl_classify_kernel<0>), dim3(grid), dim3(256), 0, st, labels, channels, (long) n, W,
                                   plain_max, lbl, FL_SHIFT, l.tiles_x, (int) ((blocks + grid - 1) / grid), unres, counters);
            }
        }
#undef FL_CASE
        e = hipGetLastError();
        if (e != hipSuccess) return cpn::check_hip(e, "cpn_flat_classify");
    }
    if (!status_host) return 0;
    u64 host[2] = {0, 0};
    e = hipMemcpyAsync(host, counters, 16, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_flat_classify: status");
    status_host[0] = (int64_t) host[0];
    status_host[1] = (int64_t) host[1];
    return 0;
}

int cpn_flat_step(int32_t *lbl, int32_t H, int32_t W, int32_t steps, int32_t footprint, int32_t launch, void *workspace,
                  int64_t workspace_bytes, int64_t *status_host, void *stream) {
    if (H < 0 || W < 0 || !workspace || launch < 0 || footprint < 0 || footprint > 0777)
        return cpn::fail(CPN_E_INVALID, "cpn_flat_step: bad arguments");
    if (steps < 1 || steps > CPN_FLAT_MAX_STEPS)
        return cpn::fail(CPN_E_INVALID, "cpn_flat_step: steps must be in 1 .. CPN_FLAT_MAX_STEPS");
    const int64_t n = (int64_t) H * W;
    if (n > 0x7fffffff) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_flat_step: more than 2^31 - 1 pixels");
    const Layout l = fl_layout(H, W);
    if (workspace_bytes < l.bytes) return cpn::fail(CPN_E_WORKSPACE, "cpn_flat_step: workspace too small");
    if (status_host) status_host[0] = status_host[1] = 0;
    if (n == 0) return 0;
    if (!lbl) return cpn::fail(CPN_E_INVALID, "cpn_flat_step: no image");
    hipStream_t st = (hipStream_t) stream;
    char *w = (char *) workspace;
    u64 *counters = (u64 *) w;
    int32_t *scratch = (int32_t *) (w + l.scratch);
    uint8_t *unres = (uint8_t *) (w + l.unres), *chg = (uint8_t *) (w + l.chg);
    uint8_t *act_cur = (uint8_t *) (w + l.act) + (launch & 1) * fl_align(l.tiles);
    uint8_t *act_next = (uint8_t *) (w + l.act) + ((launch & 1) ^ 1) * fl_align(l.tiles);
    int32_t *list = (int32_t *) (w + l.list);
    hipError_t e = hipMemsetAsync(counters + 2, 0, 16, st);
    if (e == hipSuccess) e = hipMemsetAsync(chg, 0, (size_t) l.tiles, st);
    if (e == hipSuccess) e = hipMemsetAsync(act_next, 0, (size_t) l.tiles, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_flat_step: memset");
    const unsigned fp = (unsigned) footprint;
    const int first = launch == 0;
    const int rc = fp == FL_CROSS
        ? fl_launch_step<true>(st, lbl, scratch, H, W, l, steps, fp, first, unres, act_cur, act_next, chg, list, counters)
        : fl_launch_step<false>(st, lbl, scratch, H, W, l, steps, fp, first, unres, act_cur, act_next, chg, list, counters);
    if (rc) return rc;
    if (!status_host) return 0;
    u64 host[2] = {0, 0};
    e = hipMemcpyAsync(host, counters + 2, 16, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_flat_step: status");
    status_host[0] = (int64_t) host[0];
    status_host[1] = (int64_t) host[1];
    return 0;
}

int cpn_flat_finish(int32_t *lbl, int32_t H, int32_t W, void *workspace, int64_t workspace_bytes, void *stream) {
    if (H < 0 || W < 0 || !workspace) return cpn::fail(CPN_E_INVALID, "cpn_flat_finish: bad arguments");
    const int64_t n = (int64_t) H * W;
    if (n > 0x7fffffff) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_flat_finish: more than 2^31 - 1 pixels");
    const Layout l = fl_layout(H, W);
    if (workspace_bytes < l.bytes) return cpn::fail(CPN_E_WORKSPACE, "cpn_flat_finish: workspace too small");
    if (n == 0) return 0;
    if (!lbl) return cpn::fail(CPN_E_INVALID, "cpn_flat_finish: no image");
    hipLaunchKernelGGL((fl_commit_kernel<FL_TS, true>), dim3((unsigned) (l.tiles < FL_GRID ? l.tiles : FL_GRID)), dim3(256), 0,
                       (hipStream_t) stream, lbl, (const int32_t *) nullptr, H, W, l.tiles_x,
                       (const uint8_t *) workspace + l.unres, (const int32_t *) nullptr, (const u64 *) nullptr, (int) l.tiles);
    return cpn::check_hip(hipGetLastError(), "cpn_flat_finish");
}

}  // extern "C"
