// CPN training targets on the GPU (gfx950): the kernels behind celldetection_amd.labels2distances, mask_labels_by_distance_ and
// filter_instances_ (the reference's cd.data.labels2distances, celldetection/data/cpn.py:424-497, and filter_instances_,
// celldetection/data/segmentation.py:67-103).  Integer only until the finalise pass; no floating-point atomics.
//
// Rule.  owner(p) of the int32 [H][W][C] image is the one positive value at p when exactly one channel is > 0, and 0 otherwise
// (background, negatives, overlap).  The reference runs cv2.distanceTransform(mask, type, 3) per object: OpenCV's 3 x 3 chamfer
// transform in 16-bit fixed point, t(p) = min over zero pixels q of DIAG * min(|dx|, |dy|) + HV * (max - min) in uint32, result
// float32(t) * 2^-16.  That value is the fixed point of
//     seed:   t(p) = the cheapest step (HV straight, DIAG diagonal) to an 8-neighbour that is a zero pixel for p, no such: none
//     relax:  t(p) = min(t(p), t(n) + w(n)) over the 8-neighbours n that are no zero pixel for p
// and integer minima have no order dependence: any schedule reaches the same bits.  INSTANCE mode (per_instance): a zero pixel
// for p is every pixel whose owner differs from owner(p), pixels outside the image included (the reference pads every object
// by a ring of zeros); so all objects relax at once in one image.  FG mode: a zero pixel is a pixel with owner 0 inside the
// image; outside takes no part.  Sums saturate below 2^32 - 1 (= none); with H, W <= 32768 every true value is smaller.
// Per label v over its owner pixels: n = count, tmax = max t.  d = float32(t) * 2^-16; instance mode: n > protected_size and
// tmax > 0: d = d / (float32(tmax) * 2^-16) (IEEE division); fg mode: d = d / max(float32(tmax) * 2^-16, 1e-6f); then d is clipped
// to [0, 1].  Label copy: every channel of an overlap pixel becomes -1.
//
// Classify pass (ld_classify_kernel): one read of the channel-interleaved image, writes owner and counts owner-0 pixels.
// Seed pass (ld_seed_kernel): reads the 3 x 3 owners (cached), writes t and marks the tiles that hold owner pixels.
//
// Relaxation (ld_step_kernel), blocked in space and time, the scheme and geometry of flat_labels.hip: a workgroup owns a
// TS x TS tile, loads owner and t with a halo of T pixels into LDS and runs up to T synchronous steps there.  Everything a
// workgroup computes is the length of a real path, so an upper bound of the result, whatever the missing surroundings are; the
// first step sees global values only, so a launch that changes no interior pixel anywhere has reached the fixed point, which
// is unique among upper bounds.  The interior goes to a SECOND global image (neighbours read their halos from the first one
// during the same launch) and ld_commit_kernel copies the tiles that changed back.  Only tiles that hold owner pixels AND whose
// 3 x 3 tile neighbourhood changed in the previous launch run; ld_list_kernel compacts them into a worklist and fixed grids
// walk it.  A workgroup leaves a tile when a step changes nothing.  The host reads 16 bytes per launch: pixels changed, tiles run.
// A pixel is ACTIVE when it has an owner and t >= 2 * min(HV, DIAG): a seeded border pixel can never get smaller.  Which of its
// neighbours take part is fixed, so a thread keeps it as 8 bits per pixel in registers and a step reads t only.
//
// Tile shape: TS = 32, T = 8.  LDS per workgroup = owner and t, (TS + 2 T + 2)^2 words each = 2 * 50^2 * 4 = 20 000 B (the outer
// ring holds owner 0 / t none and saves every bounds check): 7 workgroups per CU by LDS.  A thread owns K = 48^2 / 256 = 9
// region pixels with their t, new t and neighbour bits in registers.  VGPRs (hipcc --save-temps, gfx950): ld_step_kernel 123
// (4 waves per SIMD = 4 workgroups per CU: the registers bound the occupancy, not the LDS), ld_reduce_kernel 28 (24 576 B of LDS),
// ld_seed_kernel 24, ld_finalise_kernel 16, ld_classify_kernel 14, the others 12 or fewer; no scratch anywhere.  Row-major LDS
// images with lanes on consecutive pixels: the neighbour reads of a step (+-1, +-row, the diagonals) are conflict-free.
//
// Keyed reduction (ld_reduce_kernel): labels are arbitrary sparse int32, so (n, tmax) live in an open-addressing hash table
// (key, n, tmax; key 0 = empty; linear probing, LD_PROBES at most).  A workgroup first accumulates its tile in an LDS table of
// 2048 slots (a tile has at most 1024 labels) with LDS atomics, then issues one insert + atomicAdd + atomicMax per tile and
// label.  Inserts that find no slot are counted; the host repeats with a larger table.  Integer atomics only: bit-identical.
//
// Remap (ld_remap_kernel, filter_instances_): every element is looked up in a sorted key table by binary search and replaced
// by the value of its key; elements without a key stay.  One pass whatever the number of labels.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"

namespace {

typedef unsigned long long u64;
typedef uint32_t u32;

constexpr u32 LD_NONE = 0xffffffffu;
constexpr int LD_TS = 32, LD_SHIFT = 5;
constexpr int LD_T = CPN_LABEL_DISTANCES_MAX_STEPS;
static_assert(LD_T == 8 && (1 << LD_SHIFT) == LD_TS, "tile geometry");
constexpr int64_t LD_GRID = 4096;
constexpr int64_t LD_HEAD_BYTES = 64;  // u64 counters: [0] owner-0 pixels, [1] owner pixels, [2] pixels changed by the last launch,
                                       // [3] tiles run by the last launch, [4] inserts without a slot
constexpr int LD_PROBES = 256;
constexpr int LD_LOCAL = 2048;         // slots of the LDS table of the reduction

inline int64_t ld_align(int64_t n) { return (n + 63) & ~(int64_t) 63; }

struct Layout {
    int tiles_x, tiles_y;
    int64_t tiles;
    int64_t owner, t, scratch, has, chg, act, list, bytes;  // byte offsets
};

inline Layout ld_layout(int64_t H, int64_t W) {
    Layout l;
    l.tiles_x = (int) ((W + LD_TS - 1) >> LD_SHIFT);
    l.tiles_y = (int) ((H + LD_TS - 1) >> LD_SHIFT);
    l.tiles = (int64_t) l.tiles_x * l.tiles_y;
    l.owner = LD_HEAD_BYTES;
    l.t = l.owner + ld_align(H * W * 4);
    l.scratch = l.t + ld_align(H * W * 4);
    l.has = l.scratch + ld_align(H * W * 4);
    l.chg = l.has + ld_align(l.tiles);
    l.act = l.chg + ld_align(l.tiles);
    l.list = l.act + 2 * ld_align(l.tiles);
    l.bytes = l.list + ld_align(l.tiles * 4);
    return l;
}

__device__ __forceinline__ void ld_wave_add(u64 *counter, unsigned n) {  // all 64 lanes call this together
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    if (__lane_id() == 0 && n) atomicAdd(counter, (u64) n);
}

__device__ __forceinline__ u32 ld_sat_add(u32 a, u32 w) {  // a + w, saturating at none
    const u32 s = a + w;
    return s < a ? LD_NONE : s;
}

__device__ __forceinline__ u32 ld_hash(int32_t key, int shift) { return ((u32) key * 0x9E3779B1u) >> shift; }

__global__ __launch_bounds__(256) void ld_classify_kernel(const int32_t *__restrict__ x, int C, long n, int rounds,
                                                         int32_t *__restrict__ owner, u64 *__restrict__ counters) {
    unsigned n_zero = 0;
    for (int rd = 0; rd < rounds; ++rd) {
        const long p = ((long) rd * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        if (p < n) {
            int cnt = 0, mx = 0;
            for (int c = 0; c < C; ++c) {
                const int32_t v = x[p * C + c];
                cnt += v > 0;
                mx = max(mx, v);
            }
            const int32_t o = cnt == 1 ? mx : 0;
            owner[p] = o;
            n_zero += o == 0;
        }
    }
    ld_wave_add(&counters[0], n_zero);
}

template <bool FG>
__global__ __launch_bounds__(256) void ld_seed_kernel(const int32_t *__restrict__ owner, int H, int W, long n, int rounds, u32 hv,
                                                     u32 diag, int tiles_x, u32 *__restrict__ t, uint8_t *__restrict__ has) {
    for (int rd = 0; rd < rounds; ++rd) {
        const long p = ((long) rd * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        if (p >= n) continue;
        const int y = (int) (p / W), x = (int) (p - (long) y * W);
        const int32_t o = owner[p];
        u32 v = 0;
        if (o != 0) {
            v = LD_NONE;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                if (j == 4) continue;
                const int dy = j / 3 - 1, dx = j % 3 - 1, yy = y + dy, xx = x + dx;
                const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
                const int32_t on = in ? owner[(long) yy * W + xx] : 0;
                const bool zero = FG ? (in && on == 0) : (!in || on != o);
                if (zero) v = min(v, (dy != 0 && dx != 0) ? diag : hv);
            }
            has[(y >> LD_SHIFT) * tiles_x + (x >> LD_SHIFT)] = 1;  // the same value from every writer
        }
        t[p] = v;
    }
}

// The worklist of a launch: every tile with owner pixels that is active (first launch: all of them).  *count must be 0 before.
__global__ __launch_bounds__(256) void ld_list_kernel(const uint8_t *__restrict__ has, const uint8_t *__restrict__ act_cur, int first,
                                                     int tiles, int32_t *__restrict__ list, u64 *__restrict__ count) {
    const int t = blockIdx.x * 256 + threadIdx.x, lane = __lane_id();
    const bool on = t < tiles && has[t] && (first || act_cur[t]);
    const u64 m = __ballot(on);
    if (m == 0) return;
    u64 base = 0;
    if (lane == 0) base = atomicAdd(count, (u64) __popcll(m));
    base = __shfl(base, 0, 64);
    if (on) list[base + __popcll(m & ((1ull << lane) - 1))] = t;
}

template <bool FG>
__global__ __launch_bounds__(256) void ld_step_kernel(const int32_t *__restrict__ owner, const u32 *__restrict__ src,
                                                     u32 *__restrict__ dst, int H, int W, int tiles_x, int tiles_y, int steps,
                                                     u32 hv, u32 diag, const int32_t *__restrict__ list,
                                                     const u64 *__restrict__ count, uint8_t *__restrict__ act_next,
                                                     uint8_t *__restrict__ chg, u64 *__restrict__ counters) {
    constexpr int TS = LD_TS, T = LD_T, R = TS + 2 * T, RP = R + 2, K = R * R / 256;
    static_assert(R * R % 256 == 0 && K <= 32, "a thread owns K pixels, one mask bit each");
    __shared__ int32_t own[RP * RP];
    __shared__ u32 a[RP * RP];
    __shared__ int total;
    const int n_work = (int) *count;
    const u32 floor2 = 2 * min(hv, diag);
    const int tid = threadIdx.x;
    for (int work = blockIdx.x; work < n_work; work += gridDim.x) {  // the same trip count for the whole workgroup
        const int tile = list[work];
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int y0 = ty * TS - T, x0 = tx * TS - T;  // image position of region pixel (0, 0)
        if (tid == 0) total = 0;
        for (int i = tid; i < RP * RP; i += 256) {  // the ring
            const int r = i / RP, c = i % RP;
            if (r == 0 || r == RP - 1 || c == 0 || c == RP - 1) {
                own[i] = 0;
                a[i] = LD_NONE;
            }
        }
        u32 cur[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = tid + 256 * k, r = i / R, c = i % R;
            const int y = y0 + r, x = x0 + c;
            const bool in = y >= 0 && y < H && x >= 0 && x < W;
            const long g = (long) y * W + x;
            own[(r + 1) * RP + c + 1] = in ? owner[g] : 0;
            cur[k] = in ? src[g] : LD_NONE;
            a[(r + 1) * RP + c + 1] = cur[k];
        }
        __syncthreads();
        uint8_t nb[K];  // bit j: neighbour j (3 * row + column without the centre, see below) takes part
        unsigned active = 0, touched = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = tid + 256 * k, idx = (i / R + 1) * RP + i % R + 1;
            const int32_t o = own[idx];
            unsigned m = 0;
            if (o != 0 && cur[k] >= floor2) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int q = j < 4 ? j : j + 1;
                    const int32_t on = own[idx + (q / 3 - 1) * RP + (q % 3 - 1)];
                    m |= (unsigned) (FG ? on != 0 : on == o) << j;
                }
            }
            nb[k] = (uint8_t) m;
            active |= (unsigned) (m != 0) << k;
        }
        for (int s = 0; s < steps; ++s) {
            u32 nv[K];
            int changed = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                nv[k] = cur[k];
                if (active >> k & 1) {
                    const int i = tid + 256 * k, idx = (i / R + 1) * RP + i % R + 1;
                    u32 m = cur[k];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int q = j < 4 ? j : j + 1;
                        const int dy = q / 3 - 1, dx = q % 3 - 1;
                        if (nb[k] >> j & 1) m = min(m, ld_sat_add(a[idx + dy * RP + dx], (dy != 0 && dx != 0) ? diag : hv));
                    }
                    nv[k] = m;
                    changed |= m < cur[k];
                }
            }
            if (!__syncthreads_or(changed)) break;  // a fixed point of the whole region (every read is done)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (nv[k] < cur[k]) {
                    const int i = tid + 256 * k;
                    a[(i / R + 1) * RP + i % R + 1] = nv[k];
                    cur[k] = nv[k];
                    touched |= 1u << k;
                }
            }
            __syncthreads();
        }
        const int h_in = min(TS, H - ty * TS), w_in = min(TS, W - tx * TS);
        int n_chg = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = tid + 256 * k, r = i / R - T, c = i % R - T;
            if (r >= 0 && r < h_in && c >= 0 && c < w_in) n_chg += (int) (touched >> k & 1);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n_chg += __shfl_xor(n_chg, d, 64);
        if ((tid & 63) == 0 && n_chg) atomicAdd(&total, n_chg);
        __syncthreads();
        const int t_chg = total;
        if (t_chg) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int i = tid + 256 * k, r = i / R - T, c = i % R - T;
                if (r >= 0 && r < h_in && c >= 0 && c < w_in) dst[(long) (ty * TS + r) * W + tx * TS + c] = cur[k];
            }
            if (tid == 0) {
                atomicAdd(&counters[2], (u64) t_chg);
                chg[tile] = 1;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int yy = ty + dy, xx = tx + dx;
                        if (yy >= 0 && yy < tiles_y && xx >= 0 && xx < tiles_x) act_next[yy * tiles_x + xx] = 1;
                    }
            }
        }
        __syncthreads();  // the LDS images and the total are free for the next tile
    }
}

// The interior of every tile of the worklist that changed, dst (second image) -> t.
__global__ __launch_bounds__(256) void ld_commit_kernel(u32 *__restrict__ t, const u32 *__restrict__ dst, int H, int W, int tiles_x,
                                                       const uint8_t *__restrict__ chg, const int32_t *__restrict__ list,
                                                       const u64 *__restrict__ count) {
    constexpr int TS = LD_TS;
    const int n_work = (int) *count;
    for (int work = blockIdx.x; work < n_work; work += gridDim.x) {
        const int tile = list[work];
        if (!chg[tile]) continue;
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int h_in = min(TS, H - ty * TS), w_in = min(TS, W - tx * TS);
        for (int i = threadIdx.x; i < TS * TS; i += 256) {
            const int r = i / TS, c = i % TS;
            if (r < h_in && c < w_in) {
                const long g = (long) (ty * TS + r) * W + tx * TS + c;
                t[g] = dst[g];
            }
        }
    }
}

// table: int32 keys [cap], u32 n [cap], u32 tmax [cap].  One workgroup per tile of the walk.
__global__ __launch_bounds__(256) void ld_reduce_kernel(const int32_t *__restrict__ owner, const u32 *__restrict__ t, int H, int W,
                                                       int tiles_x, int tiles, const uint8_t *__restrict__ has,
                                                       int32_t *__restrict__ keys, u32 *__restrict__ cnt, u32 *__restrict__ tmax,
                                                       int shift, u32 cap_mask, u64 *__restrict__ counters) {
    constexpr int TS = LD_TS;
    __shared__ int32_t lk[LD_LOCAL];
    __shared__ u32 ln[LD_LOCAL], lm[LD_LOCAL];
    unsigned n_fail = 0, n_own = 0;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        if (!has[tile]) continue;  // the same for the whole workgroup
        for (int i = threadIdx.x; i < LD_LOCAL; i += 256) {
            lk[i] = 0;
            ln[i] = 0;
            lm[i] = 0;
        }
        __syncthreads();
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int h_in = min(TS, H - ty * TS), w_in = min(TS, W - tx * TS);
        for (int i = threadIdx.x; i < TS * TS; i += 256) {
            const int r = i / TS, c = i % TS;
            if (r < h_in && c < w_in) {
                const long g = (long) (ty * TS + r) * W + tx * TS + c;
                const int32_t o = owner[g];
                if (o != 0) {
                    ++n_own;
                    u32 s = ld_hash(o, 32 - 11);
                    for (;;) {  // ends: at most 1024 keys in 2048 slots
                        const int32_t was = atomicCAS(&lk[s], 0, o);
                        if (was == 0 || was == o) break;
                        s = (s + 1) & (LD_LOCAL - 1);
                    }
                    atomicAdd(&ln[s], 1u);
                    atomicMax(&lm[s], t[g]);
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < LD_LOCAL; i += 256) {
            const int32_t o = lk[i];
            if (o == 0) continue;
            u32 s = ld_hash(o, shift);
            int probe = 0;
            for (; probe < LD_PROBES; ++probe) {
                const int32_t was = atomicCAS(&keys[s], 0, o);
                if (was == 0 || was == o) break;
                s = (s + 1) & cap_mask;
            }
            if (probe == LD_PROBES) {
                ++n_fail;
            } else {
                atomicAdd(&cnt[s], ln[i]);
                atomicMax(&tmax[s], lm[i]);
            }
        }
        __syncthreads();
    }
    ld_wave_add(&counters[4], n_fail);
    ld_wave_add(&counters[1], n_own);
}

template <bool FG>
__global__ __launch_bounds__(256) void ld_finalise_kernel(const int32_t *__restrict__ x, int C, long n, int rounds,
                                                         const int32_t *__restrict__ owner, const u32 *__restrict__ t,
                                                         const int32_t *__restrict__ keys, const u32 *__restrict__ cnt,
                                                         const u32 *__restrict__ tmax, int shift, u32 cap_mask, u32 protected_size,
                                                         float *__restrict__ dist, int32_t *__restrict__ out) {
    constexpr float SCALE = 1.f / 65536.f;
    for (int rd = 0; rd < rounds; ++rd) {
        const long p = ((long) rd * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        if (p >= n) continue;
        int pos = 0;
        for (int c = 0; c < C; ++c) pos += x[p * C + c] > 0;
        for (int c = 0; c < C; ++c) out[p * C + c] = pos > 1 ? -1 : x[p * C + c];
        const int32_t o = owner[p];
        float d = 0.f;
        if (o != 0) {
            u32 s = ld_hash(o, shift);
            for (int probe = 0; probe < LD_PROBES && keys[s] != o; ++probe) s = (s + 1) & cap_mask;  // the insert succeeded: found
            const u32 m = tmax[s];
            d = (float) t[p] * SCALE;
            if (FG) {
                d = d / fmaxf((float) m * SCALE, 1e-6f);
            } else if (cnt[s] > protected_size && m > 0) {
                d = d / ((float) m * SCALE);
            }
            d = fminf(fmaxf(d, 0.f), 1.f);
        }
        dist[p] = d;
    }
}

__global__ __launch_bounds__(256) void ld_mask_kernel(int32_t *__restrict__ x, int C, long n, int rounds, const float *__restrict__ dist,
                                                     float max_bg, float min_fg, int32_t *__restrict__ reduced) {
    for (int rd = 0; rd < rounds; ++rd) {
        const long p = ((long) rd * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        if (p >= n) continue;
        const float d = dist[p];
        bool any = false;
        int32_t mx = x[p * C];
        for (int c = 0; c < C; ++c) {
            const int32_t v = x[p * C + c];
            any |= v > 0;
            mx = max(mx, v);
        }
        const bool zero = any && d <= max_bg, flag = d > max_bg && d < min_fg;
        if (zero || flag) {
            mx = flag ? -1 : 0;
            for (int c = 0; c < C; ++c) x[p * C + c] = mx;
        }
        if (reduced) reduced[p] = mx;
    }
}

__global__ __launch_bounds__(256) void ld_remap_kernel(int32_t *__restrict__ x, long n, int rounds, const int32_t *__restrict__ keys,
                                                      const int32_t *__restrict__ values, int m) {
    for (int rd = 0; rd < rounds; ++rd) {
        const long p = ((long) rd * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        if (p >= n) continue;
        const int32_t v = x[p];
        int lo = 0, hi = m;  // the first key >= v
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        if (lo < m && keys[lo] == v) {
            const int32_t w = values[lo];
            if (w != v) x[p] = w;
        }
    }
}

struct Walk {
    unsigned grid;
    int rounds;
};

inline Walk ld_walk(int64_t n) {
    const int64_t blocks = (n + 255) / 256;
    Walk w;
    w.grid = (unsigned) (blocks < LD_GRID ? blocks : LD_GRID);
    w.rounds = (int) ((blocks + w.grid - 1) / w.grid);
    return w;
}

inline int ld_check_image(const char *who, int32_t H, int32_t W, const void *workspace, int64_t workspace_bytes, Layout *l) {
    const std::string name(who);
    if (H < 0 || W < 0 || !workspace) return cpn::fail(CPN_E_INVALID, (name + ": bad arguments").c_str());
    if (H > 32768 || W > 32768) return cpn::fail(CPN_E_UNSUPPORTED, (name + ": H and W are at most 32768").c_str());
    *l = ld_layout(H, W);
    if (workspace_bytes < l->bytes) return cpn::fail(CPN_E_WORKSPACE, (name + ": workspace too small").c_str());
    return 0;
}

inline int ld_weights(int32_t distance_type, u32 *hv, u32 *diag) {
    switch (distance_type) {
        case CPN_DIST_L1: *hv = 65536; *diag = 131072; return 0;
        case CPN_DIST_L2: *hv = 62587; *diag = 89738; return 0;  // round(0.955 * 2^16), round(1.3693 * 2^16)
        case CPN_DIST_C: *hv = 65536; *diag = 65536; return 0;
    }
    return -1;
}

inline int ld_table(int64_t capacity, int *shift) {
    if (capacity < 64 || capacity > ((int64_t) 1 << 28) || (capacity & (capacity - 1))) return -1;
    int lg = 0;
    while (((int64_t) 1 << lg) < capacity) ++lg;
    *shift = 32 - lg;
    return 0;
}

}  // namespace

extern "C" {

int64_t cpn_label_distances_workspace_bytes(int32_t H, int32_t W) {
    if (H < 0 || W < 0 || H > 32768 || W > 32768) return 0;
    return ld_layout(H, W).bytes;
}

int64_t cpn_label_distances_table_bytes(int64_t table_capacity) {
    int shift;
    if (ld_table(table_capacity, &shift)) return 0;
    return table_capacity * 12;
}

int cpn_label_distances_classify(const int32_t *labels, int32_t channels, int32_t H, int32_t W, int32_t distance_type,
                                 int32_t per_instance, void *workspace, int64_t workspace_bytes, int64_t *status_host,
                                 void *stream) {
    Layout l;
    if (channels < 1) return cpn::fail(CPN_E_INVALID, "cpn_label_distances_classify: bad arguments");
    if (int rc = ld_check_image("cpn_label_distances_classify", H, W, workspace, workspace_bytes, &l)) return rc;
    u32 hv, diag;
    if (ld_weights(distance_type, &hv, &diag))
        return cpn::fail(CPN_E_INVALID, "cpn_label_distances_classify: distance_type must be CPN_DIST_L1, CPN_DIST_L2 or CPN_DIST_C");
    const int64_t n = (int64_t) H * W;
    if (n > 0 && !labels) return cpn::fail(CPN_E_INVALID, "cpn_label_distances_classify: no image");
    hipStream_t st = (hipStream_t) stream;
    char *w = (char *) workspace;
    u64 *counters = (u64 *) w;
    hipError_t e = hipMemsetAsync(counters, 0, LD_HEAD_BYTES, st);
    if (e == hipSuccess) e = hipMemsetAsync(w + l.has, 0, (size_t) (l.bytes - l.has), st);  // every tile flag
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_label_distances_classify: memset");
    if (n > 0) {
        const Walk k = ld_walk(n);
        int32_t *owner = (int32_t *) (w + l.owner);
        u32 *t = (u32 *) (w + l.t);
        uint8_t *has = (uint8_t *) (w + l.has);
        hipLaunchKernelGGL(ld_classify_kernel, dim3(k.grid), dim3(256), 0, st, labels, channels, (long) n, k.rounds, owner, counters);
        if (per_instance)
            hipLaunchKernelGGL(ld_seed_kernel<false>, dim3(k.grid), dim3(256), 0, st, owner, H, W, (long) n, k.rounds, hv, diag,
                               l.tiles_x, t, has);
        else
            hipLaunchKernelGGL(ld_seed_kernel<true>, dim3(k.grid), dim3(256), 0, st, owner, H, W, (long) n, k.rounds, hv, diag,
                               l.tiles_x, t, has);
        e = hipGetLastError();
        if (e != hipSuccess) return cpn::check_hip(e, "cpn_label_distances_classify");
    }
    if (!status_host) return 0;
    u64 host = 0;
    e = hipMemcpyAsync(&host, counters, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_label_distances_classify: status");
    status_host[0] = (int64_t) host;
    return 0;
}

int cpn_label_distances_step(int32_t H, int32_t W, int32_t steps, int32_t distance_type, int32_t per_instance, int32_t launch,
                             void *workspace, int64_t workspace_bytes, int64_t *status_host, void *stream) {
    Layout l;
    if (launch < 0) return cpn::fail(CPN_E_INVALID, "cpn_label_distances_step: bad arguments");
    if (int rc = ld_check_image("cpn_label_distances_step", H, W, workspace, workspace_bytes, &l)) return rc;
    if (steps < 1 || steps > CPN_LABEL_DISTANCES_MAX_STEPS)
        return cpn::fail(CPN_E_INVALID, "cpn_label_distances_step: steps must be in 1 .. CPN_LABEL_DISTANCES_MAX_STEPS");
    u32 hv, diag;
    if (ld_weights(distance_type, &hv, &diag))
        return cpn::fail(CPN_E_INVALID, "cpn_label_distances_step: distance_type must be CPN_DIST_L1, CPN_DIST_L2 or CPN_DIST_C");
    if (status_host) status_host[0] = status_host[1] = 0;
    if ((int64_t) H * W == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    char *w = (char *) workspace;
    u64 *counters = (u64 *) w;
    const int32_t *owner = (const int32_t *) (w + l.owner);
    u32 *t = (u32 *) (w + l.t), *scratch = (u32 *) (w + l.scratch);
    uint8_t *has = (uint8_t *) (w + l.has), *chg = (uint8_t *) (w + l.chg);
    uint8_t *act_cur = (uint8_t *) (w + l.act) + (launch & 1) * ld_align(l.tiles);
    uint8_t *act_next = (uint8_t *) (w + l.act) + ((launch & 1) ^ 1) * ld_align(l.tiles);
    int32_t *list = (int32_t *) (w + l.list);
    hipError_t e = hipMemsetAsync(counters + 2, 0, 16, st);
    if (e == hipSuccess) e = hipMemsetAsync(chg, 0, (size_t) l.tiles, st);
    if (e == hipSuccess) e = hipMemsetAsync(act_next, 0, (size_t) l.tiles, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_label_distances_step: memset");
    const unsigned grid = (unsigned) (l.tiles < LD_GRID ? l.tiles : LD_GRID);
    hipLaunchKernelGGL(ld_list_kernel, dim3((unsigned) ((l.tiles + 255) / 256)), dim3(256), 0, st, has, act_cur, launch == 0,
                       (int) l.tiles, list, counters + 3);
    if (per_instance)
        hipLaunchKernelGGL(ld_step_kernel<false>, dim3(grid), dim3(256), 0, st, owner, t, scratch, H, W, l.tiles_x, l.tiles_y, steps,
                           hv, diag, list, counters + 3, act_next, chg, counters);
    else
        hipLaunchKernelGGL(ld_step_kernel<true>, dim3(grid), dim3(256), 0, st, owner, t, scratch, H, W, l.tiles_x, l.tiles_y, steps,
                           hv, diag, list, counters + 3, act_next, chg, counters);
    hipLaunchKernelGGL(ld_commit_kernel, dim3(grid), dim3(256), 0, st, t, scratch, H, W, l.tiles_x, chg, list, counters + 3);
    e = hipGetLastError();
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_label_distances_step");
    if (!status_host) return 0;
    u64 host[2] = {0, 0};
    e = hipMemcpyAsync(host, counters + 2, 16, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_label_distances_step: status");
    status_host[0] = (int64_t) host[0];
    status_host[1] = (int64_t) host[1];
    return 0;
}

int cpn_label_distances_reduce(int32_t H, int32_t W, void *workspace, int64_t workspace_bytes, void *table,
                               int64_t table_capacity, int64_t *status_host, void *stream) {
    Layout l;
    int shift;
    if (int rc = ld_check_image("cpn_label_distances_reduce", H, W, workspace, workspace_bytes, &l)) return rc;
    if (!table || ld_table(table_capacity, &shift))
        return cpn::fail(CPN_E_INVALID, "cpn_label_distances_reduce: table_capacity must be a power of two from 64 to 2^28");
    hipStream_t st = (hipStream_t) stream;
    char *w = (char *) workspace;
    u64 *counters = (u64 *) w;
    int32_t *keys = (int32_t *) table;
    u32 *cnt = (u32 *) table + table_capacity, *tmax = (u32 *) table + 2 * table_capacity;
    hipError_t e = hipMemsetAsync(table, 0, (size_t) table_capacity * 12, st);
    if (e == hipSuccess) e = hipMemsetAsync(counters + 4, 0, 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(counters + 1, 0, 8, st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_label_distances_reduce: memset");
    if (l.tiles > 0) {
        const unsigned grid = (unsigned) (l.tiles < LD_GRID ? l.tiles : LD_GRID);
        hipLaunchKernelGGL(ld_reduce_kernel, dim3(grid), dim3(256), 0, st, (const int32_t *) (w + l.owner), (const u32 *) (w + l.t), H, W,
                           l.tiles_x, (int) l.tiles, (const uint8_t *) (w + l.has), keys, cnt, tmax, shift, (u32) (table_capacity - 1),
                           counters);
        e = hipGetLastError();
        if (e != hipSuccess) return cpn::check_hip(e, "cpn_label_distances_reduce");
    }
    if (!status_host) return 0;
    u64 host = 0;
    e = hipMemcpyAsync(&host, counters + 4, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return cpn::check_hip(e, "cpn_label_distances_reduce: status");
    status_host[0] = (int64_t) host;
    return 0;
}

int cpn_label_distances_finalise(const int32_t *labels, int32_t channels, int32_t H, int32_t W, int32_t per_instance,
                                 int32_t protected_size, void *workspace, int64_t workspace_bytes, const void *table,
                                 int64_t table_capacity, float *distances, int32_t *labels_out, void *stream) {
    Layout l;
    int shift;
    if (channels < 1 || protected_size < 0) return cpn::fail(CPN_E_INVALID, "cpn_label_distances_finalise: bad arguments");
    if (int rc = ld_check_image("cpn_label_distances_finalise", H, W, workspace, workspace_bytes, &l)) return rc;
    if (!table || ld_table(table_capacity, &shift))
        return cpn::fail(CPN_E_INVALID, "cpn_label_distances_finalise: table_capacity must be a power of two from 64 to 2^28");
    const int64_t n = (int64_t) H * W;
    if (n == 0) return 0;
    if (!labels || !distances || !labels_out) return cpn::fail(CPN_E_INVALID, "cpn_label_distances_finalise: no image");
    char *w = (char *) workspace;
    const int32_t *keys = (const int32_t *) table;
    const u32 *cnt = (const u32 *) table + table_capacity, *tmax = (const u32 *) table + 2 * table_capacity;
    const Walk k = ld_walk(n);
    if (per_instance)
        hipLaunchKernelGGL(ld_finalise_kernel<false>, dim3(k.grid), dim3(256), 0, (hipStream_t) stream, labels, channels, (long) n,
                           k.rounds, (const int32_t *) (w + l.owner), (const u32 *) (w + l.t), keys, cnt, tmax, shift,
                           (u32) (table_capacity - 1), (u32) protected_size, distances, labels_out);
    else
        hipLaunchKernelGGL(ld_finalise_kernel<true>, dim3(k.grid), dim3(256), 0, (hipStream_t) stream, labels, channels, (long) n,
                           k.rounds, (const int32_t *) (w + l.owner), (const u32 *) (w + l.t), keys, cnt, tmax, shift,
                           (u32) (table_capacity - 1), (u32) protected_size, distances, labels_out);
    return cpn::check_hip(hipGetLastError(), "cpn_label_distances_finalise");
}

int cpn_label_distances_mask(int32_t *labels, int32_t channels, int64_t pixels, const float *distances, float max_bg_dist,
                             float min_fg_dist, int32_t *reduced, void *stream) {
    if (channels < 1 || pixels < 0) return cpn::fail(CPN_E_INVALID, "cpn_label_distances_mask: bad arguments");
    if (pixels > 0x7fffffff) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_label_distances_mask: more than 2^31 - 1 pixels");
    if (pixels == 0) return 0;
    if (!labels || !distances) return cpn::fail(CPN_E_INVALID, "cpn_label_distances_mask: no image");
    const Walk k = ld_walk(pixels);
    hipLaunchKernelGGL(ld_mask_kernel, dim3(k.grid), dim3(256), 0, (hipStream_t) stream, labels, channels, (long) pixels, k.rounds,
                       distances, max_bg_dist, min_fg_dist, reduced);
    return cpn::check_hip(hipGetLastError(), "cpn_label_distances_mask");
}

int cpn_label_remap(int32_t *labels, int64_t elements, const int32_t *keys, const int32_t *values, int32_t entries, void *stream) {
    if (elements < 0 || entries < 0) return cpn::fail(CPN_E_INVALID, "cpn_label_remap: bad arguments");
    if (elements == 0 || entries == 0) return 0;
    if (!labels || !keys || !values) return cpn::fail(CPN_E_INVALID, "cpn_label_remap: no image or no table");
    const Walk k = ld_walk(elements);
    hipLaunchKernelGGL(ld_remap_kernel, dim3(k.grid), dim3(256), 0, (hipStream_t) stream, labels, (long) elements, k.rounds, keys,
                       values, entries);
    return cpn::check_hip(hipGetLastError(), "cpn_label_remap");
}

}  // extern "C"
