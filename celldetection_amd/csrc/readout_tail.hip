// Trainable ReadOut tail on the GPU (gfx950): Dropout2d fused into a 1x1 conv to at most 32 output channels, the kernels behind
// celldetection_amd.nn.dropout_conv1x1.  The rule is the "Trainable ReadOut tail" section of include/cpn_hip.h.
//
// x is [N][HW][Cin] bf16 as it lies (a channels-last tensor), y and dy are [N][Cout][HW] planes, keep is [N][Cin] bytes.  The dropout
// never touches x: the WEIGHT operand is masked per image (a dropped channel contributes an exact zero), the factor s = 1 / (1 - p)
// is applied to the fp32 sum.  All three products run on v_mfma_f32_32x32x16_bf16 (D[i][j] = sum_k A[i][k] B[k][j]; lane l holds
// A[l % 32][8 (l / 32) + e] and B[8 (l / 32) + e][l % 32], e = 0 ... 7; D: j = l % 32, i = mf_row(reg, l / 32); csrc/mfma_frag.h):
//   rt_forward_kernel:   D[o][pixel] = W[o][c] x^T[c][pixel].  The pixel is on the lanes: a lane's B operand is 16 bytes of x as they
//                        lie, every accumulator register is one output channel of 32 consecutive pixels (a coalesced store into an
//                        NCHW plane).  The masked W of the workgroup's image sits in LDS as [step][lane half][o] x 16 bytes (64 B x
//                        Cin; rows o >= Cout are zeros).  A workgroup takes consecutive 32-pixel tiles of ONE image, so a tile never
//                        straddles two masks; the lanes behind the image's last pixel read that pixel again and store nothing.
//   rt_backward_kernel:  one workgroup per slab (csrc/tail_slabs.h; a slab never crosses an image), chunks of PT pixels.  dy is
//                        rounded to bf16 into the LDS image G[o][pixel] (rows o >= Cout and pixels behind the slab are zeros), x is
//                        staged as it lies in 32-channel rows of 64 bytes.
//                          dx:  D[c][pixel] = W^T[c][o] G[o][pixel], K = Cout padded to 16 or 32 (one or two steps).  B is read from G
//                               with the transposed LDS read; row i of the masked W^T image is channel 16 ((i / 4) % 2) + 4 (i / 8) +
//                               i % 4 of the 32-channel tile, so that a lane's 16 registers are 16 CONSECUTIVE channels of its
//                               pixel: 32 bytes of dx, two 16-byte stores.
//                          dW:  D[o][c] = G[o][pixel] x[pixel][c], K = the slab's pixels, 16 per step; A is 16 bytes of a G row, B the
//                               staged x through the transposed LDS read (ds_read_b64_tr_b16), as csrc/wgrad_dense.h does.  Wave w
//                               owns the channel tiles w, w + 4, ...: one fp32 accumulator per element for the whole slab, written
//                               to workspace[slab][o][c].
//                          db:  eight interleaved chains per channel over G, added in order, to workspace[slabs ...][slab][o].
//                        Padded, never masked: EXEC is all ones around every transposed read (branches are workgroup- or
//                        wave-uniform), zeros stand for what is not there.
//   rt_reduce_kernel:    adds the slabs in ascending (image, slab) order, the slabs of images that dropped the channel as + 0,
//                        multiplies by s once and rounds once to the parameter dtype; the bias sums likewise, unmasked, without s.
// No floating-point atomics: results are bit-identical from run to run.  Vector stores only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "mfma_frag.h"
#include "tail_slabs.h"

namespace {

constexpr int RT_F32 = 0, RT_BF16 = 1;
constexpr int RT_ROW = 64;        // bytes of a staged x row: 32 channels
constexpr int RT_MAX_CIN = 1024, RT_MAX_COUT = 32;
constexpr int RT_SLABS = 512;     // auto partition of the backward: two workgroups per CU
constexpr int RT_GROUPS = 1024;   // ... and of the forward: four
constexpr int64_t RT_MAX_SLABS = (1 << 24) - 1;

__device__ __forceinline__ uint16_t rt_bf16_rne(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t) ((u >> 16) | 0x40);  // NaN stays NaN
    return (uint16_t) ((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float rt_bf16_value(uint16_t b) { return __uint_as_float((uint32_t) b << 16); }

// element i of an fp32 | bf16 array as bf16 (RNE)
__device__ __forceinline__ uint16_t rt_load_bf16(const void *p, int dtype, int64_t i) {
    return dtype == RT_BF16 ? ((const uint16_t *) p)[i] : rt_bf16_rne(((const float *) p)[i]);
}
__device__ __forceinline__ float rt_load_f32(const void *p, int dtype, int64_t i) {
    return dtype == RT_BF16 ? rt_bf16_value(((const uint16_t *) p)[i]) : ((const float *) p)[i];
}
__device__ __forceinline__ u32x4 rt_pack8(const uint16_t e[8]) {
    return u32x4{(uint32_t) e[0] | ((uint32_t) e[1] << 16), (uint32_t) e[2] | ((uint32_t) e[3] << 16),
                 (uint32_t) e[4] | ((uint32_t) e[5] << 16), (uint32_t) e[6] | ((uint32_t) e[7] << 16)};
}

__global__ __launch_bounds__(256) void rt_forward_kernel(const uint16_t *__restrict__ x, const void *__restrict__ w, int w_dtype,
                                                          const void *__restrict__ bias, int bias_dtype,
                                                          const uint8_t *__restrict__ keep, float s, void *__restrict__ y, int y_dtype,
                                                          TailTiles tiles, int64_t HW, int Cin, int Cout) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [Cin / 16 steps][2 lane halves][32 o] x 16 bytes
    const int tid = threadIdx.x;
    int n;
    int64_t t0, t1;
    tls_tile_range(tiles, blockIdx.x, &n, &t0, &t1);
    for (int i = tid; i < Cin * 4; i += 256) {  // item i: o = i % 32, channels 8 (i / 32) ... + 8
        const int o = i & 31, c0 = (i >> 5) * 8;
        u32x4 v = {0, 0, 0, 0};
        if (o < Cout) {
            uint16_t e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool kept = !keep || keep[(int64_t) n * Cin + c0 + j] != 0;
                e[j] = kept ? rt_load_bf16(w, w_dtype, (int64_t) o * Cin + c0 + j) : (uint16_t) 0;
            }
            v = rt_pack8(e);
        }
        *(u32x4 *) (smem + i * 16) = v;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    float b[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int o = mf_row(reg, h);
        b[reg] = bias && o < Cout ? rt_load_f32(bias, bias_dtype, o) : 0.f;
    }
    const int steps = Cin / 16;
    for (int64_t t = t0 + wave; t < t1; t += 4) {
        const int64_t q = t * TLS_TILE + r;
        const bool ok = q < HW;
        const uint16_t *xp = x + ((int64_t) n * HW + (ok ? q : HW - 1)) * Cin + 8 * h;
        const char *ap = smem + (h * 32 + r) * 16;
        f32x16 acc;
        mf_zero(acc);
        for (int st = 0; st < steps; st += 2) {  // (Cin is a multiple of 32: two steps per round, in ascending channel order)
            const bf16x8 B0 = *(const bf16x8 *) (xp + 16 * st), B1 = *(const bf16x8 *) (xp + 16 * st + 16);
            const bf16x8 A0 = *(const bf16x8 *) (ap + st * 1024), A1 = *(const bf16x8 *) (ap + st * 1024 + 1024);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, B0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1, B1, acc, 0, 0, 0);
        }
        if (ok) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int o = mf_row(reg, h);
                if (o < Cout) {
                    const float v = fmaf(acc[reg], s, b[reg]);
                    const int64_t at = ((int64_t) n * Cout + o) * HW + q;
                    if (y_dtype == RT_BF16) ((uint16_t *) y)[at] = rt_bf16_rne(v);
                    else ((float *) y)[at] = v;
                }
            }
        }
    }
}

// LDS image of the backward kernel: the masked W^T [Cin / 32 tiles][ks steps][2 lane halves][32 rows] x 16 bytes, G [32 o][PT pixels]
// bf16 in rows of PT * 2 + 16 bytes, x [Cin / 32 tiles][PT pixels] rows of 64 bytes, the bias chains [8][32] fp32.  Every offset is
// a multiple of 16.
template <int PT>
struct RtLds {
    static constexpr int GS_ROW = PT * 2 + 16;
    __host__ __device__ static constexpr int wt(int cin, int ks) { return cin * 32 * ks; }
    __host__ __device__ static constexpr int total(int cin, int ks) { return wt(cin, ks) + 32 * GS_ROW + cin / 32 * PT * RT_ROW + 8 * 32 * 4; }
};

template <int CT, int PT>
__global__ __launch_bounds__(256) void rt_backward_kernel(const uint16_t *__restrict__ x, const void *__restrict__ g, int g_dtype,
                                                           const void *__restrict__ w, int w_dtype, const uint8_t *__restrict__ keep,
                                                           float s, uint16_t *__restrict__ dx, float *__restrict__ ws,
                                                           float *__restrict__ wsb, TailSlabs part, int Cin, int Cout) {
    typedef RtLds<PT> L;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, ks = Cout > 16 ? 2 : 1, ctiles = Cin / 32;
    char *WT = smem, *GS = WT + L::wt(Cin, ks), *XS = GS + 32 * L::GS_ROW;
    float *BS = (float *) (XS + ctiles * PT * RT_ROW);
    const int64_t slab = blockIdx.x, HW = part.HW;
    int n;
    int64_t q0, q1;
    tls_range(part, slab, &n, &q0, &q1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int r = lane & 31, h = lane >> 5, wq = (lane >> 2) & 3;
    const int cb = mf_lane_bytes(lane);

    if (dx) {  // item i = ((tile * ks + step) * 2 + lane half) * 32 + row: W[16 step + 8 half + j][channel of the row], j = 0 ... 7
        for (int i = tid; i < Cin * 2 * ks; i += 256) {
            const int row = i & 31, hh = (i >> 5) & 1, st = (i >> 6) % ks, ct = (i >> 6) / ks;
            const int c = ct * 32 + 16 * ((row >> 2) & 1) + 4 * (row >> 3) + (row & 3);
            const bool kept = !keep || keep[(int64_t) n * Cin + c] != 0;
            uint16_t e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int o = 16 * st + 8 * hh + j;
                e[j] = kept && o < Cout ? rt_load_bf16(w, w_dtype, (int64_t) o * Cin + c) : (uint16_t) 0;
            }
            *(u32x4 *) (WT + i * 16) = rt_pack8(e);
        }
    }
    for (int i = tid; i < 32 * L::GS_ROW / 16; i += 256) *(u32x4 *) (GS + i * 16) = u32x4{0, 0, 0, 0};  // rows >= Cout stay zeros
    __syncthreads();

    f32x16 acc[CT];
#pragma unroll
    for (int m = 0; m < CT; ++m) mf_zero(acc[m]);
    float bsum = 0.f;
    const int bo = tid & 31, bchain = tid >> 5;

    for (int64_t c0 = q0; c0 < q1; c0 += PT) {
        const int left = (int) (q1 - c0 < PT ? q1 - c0 : PT);
        // ---- stage: dy -> bf16 (RNE), coalesced along the pixels of a plane; x in 16-byte items as it lies
        for (int i = tid; i < Cout * PT; i += 256) {
            const int o = i / PT, t = i % PT;
            const uint16_t v = t < left ? rt_load_bf16(g, g_dtype, ((int64_t) n * Cout + o) * HW + c0 + t) : (uint16_t) 0;
            *(uint16_t *) (GS + o * L::GS_ROW + t * 2) = v;
        }
        if (ws) {
            const int per = Cin / 8;
            for (int i = tid; i < PT * per; i += 256) {
                const int t = i / per, qq = i % per;
                u32x4 v = {0, 0, 0, 0};
                if (t < left) v = *(const u32x4 *) (x + ((int64_t) n * HW + c0 + t) * Cin + qq * 8);
                *(u32x4 *) (XS + ((qq >> 2) * PT + t) * RT_ROW + (qq & 3) * 16) = v;
            }
        }
        __syncthreads();
        // ---- bias: chain bchain takes the pixels bchain, bchain + 8, ... of the slab (c0 - q0 is a multiple of 8)
        if (wsb)
            for (int t = bchain; t < left; t += TLS_BIAS_LANES) bsum += rt_bf16_value(*(const uint16_t *) (GS + bo * L::GS_ROW + t * 2));
        // ---- dx: tiles of 32 channels x 32 pixels, dealt to the waves
        if (dx) {
            const int ptiles = (left + 31) / 32;
            for (int t = wave; t < ctiles * (PT / 32); t += 4) {
                const int ct = t / (PT / 32), pt = t % (PT / 32);
                if (pt >= ptiles) continue;  // (wave-uniform)
                f32x16 d;
                mf_zero(d);
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    if (st < ks) {
                        const bf16x8 A = *(const bf16x8 *) (WT + (((ct * ks + st) * 2 + h) * 32 + r) * 16);
                        const int g_at = (int) (GS - smem) + (16 * st + 8 * h + wq) * L::GS_ROW + pt * 64 + cb;
                        const bf16x8 B = mf_operand(smem, g_at, g_at + 4 * L::GS_ROW);
                        d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, d, 0, 0, 0);
                    }
                }
                if (pt * 32 + r < left) {  // the lane's registers are the channels 32 ct + 16 h + reg of its pixel
                    uint16_t e[16];
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) e[reg] = rt_bf16_rne(d[reg] * s);
                    uint16_t *out = dx + ((int64_t) n * HW + c0 + pt * 32 + r) * Cin + ct * 32 + 16 * h;
                    *(u32x4 *) out = rt_pack8(e);
                    *(u32x4 *) (out + 8) = rt_pack8(e + 8);
                }
            }
        }
        // ---- dW: wave w owns the channel tiles w, w + 4, ...; steps behind the slab's end are not run (their rows are zeros anyway)
        if (ws) {
            const int steps = (int) tls_steps(left);
            const int x_at = (int) (XS - smem) + (8 * h + wq) * RT_ROW + cb;
            for (int st = 0; st < steps; ++st) {
                const bf16x8 A = *(const bf16x8 *) (GS + r * L::GS_ROW + (16 * st + 8 * h) * 2);
#pragma unroll
                for (int m = 0; m < CT; ++m) {
                    const int ct = wave + 4 * m;
                    if (ct < ctiles) {  // (wave-uniform)
                        const int at = x_at + (ct * PT + 16 * st) * RT_ROW;
                        const bf16x8 B = mf_operand(smem, at, at + 4 * RT_ROW);
                        acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, acc[m], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }
    // ---- partial sums: D[i = o][j = c]
    if (ws) {
#pragma unroll
        for (int m = 0; m < CT; ++m) {
            const int ct = wave + 4 * m;
            if (ct < ctiles) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int o = mf_row(reg, h);
                    if (o < Cout) ws[((int64_t) slab * Cout + o) * Cin + ct * 32 + r] = acc[m][reg];
                }
            }
        }
    }
    if (wsb) {
        BS[bchain * 32 + bo] = bsum;
        __syncthreads();
        if (tid < Cout) {
            float sum = BS[tid];
            for (int i = 1; i < TLS_BIAS_LANES; ++i) sum += BS[i * 32 + tid];
            wsb[slab * Cout + tid] = sum;
        }
    }
}

// workspace [slab][o][c] -> dw [o][c]; bias sums [slab][o] -> db [o].  Element e < Cout Cin is a weight gradient (masked per image,
// multiplied by s), the Cout behind them are the bias gradients.  A workgroup owns 32 consecutive elements: its 256 lanes fetch 128
// slabs at a time into LDS (16 independent loads per lane, a dropped channel's slab as +0), then one lane per element adds them in
// ascending slab order -- one thread per element reading slab by slab waited for memory 512 times in a row (0.16 ms for 512 slabs).
constexpr int RT_RED = 128;
__global__ __launch_bounds__(256) void rt_reduce_kernel(const float *__restrict__ ws, const float *__restrict__ wsb,
                                                         const uint8_t *__restrict__ keep, float s, int slabs, int per_image, int Cin,
                                                         int Cout, void *dw, int dw_dtype, void *db, int db_dtype) {
    __shared__ float buf[RT_RED][32];
    const int lane = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int per = Cout * Cin, e = blockIdx.x * 32 + lane;
    const bool is_w = e < per;
    const bool live = is_w ? dw != nullptr : (db != nullptr && e < per + Cout);
    const float *src = !live ? nullptr : is_w ? ws + e : wsb + (e - per);
    const int64_t stride = is_w ? per : Cout;
    const uint8_t *kp = live && is_w && keep ? keep + e % Cin : nullptr;
    float sum = 0.f;
    for (int s0 = 0; s0 < slabs; s0 += RT_RED) {
#pragma unroll
        for (int k = 0; k < RT_RED / 8; ++k) {
            const int j = sl + 8 * k, slab = s0 + j;
            float v = 0.f;
            if (live && slab < slabs) {
                v = src[(int64_t) slab * stride];
                if (kp && kp[(int64_t) (slab / per_image) * Cin] == 0) v = 0.f;  // the slab of an image that dropped the channel: + 0
            }
            buf[j][lane] = v;
        }
        __syncthreads();
        if (sl == 0) {
            const int cnt = slabs - s0 < RT_RED ? slabs - s0 : RT_RED;
            for (int j = 0; j < cnt; ++j) sum += buf[j][lane];
        }
        __syncthreads();
    }
    if (sl == 0 && live) {
        if (is_w) {
            sum *= s;
            if (dw_dtype == RT_BF16) ((uint16_t *) dw)[e] = rt_bf16_rne(sum);
            else ((float *) dw)[e] = sum;
        } else {
            if (db_dtype == RT_BF16) ((uint16_t *) db)[e - per] = rt_bf16_rne(sum);
            else ((float *) db)[e - per] = sum;
        }
    }
}

// 0, or the error code with its message recorded; the partition of an accepted call
int rt_check(const char *who, int64_t N, int64_t HW, int cin, int cout, int64_t slab_pixels, TailSlabs *part) {
    static thread_local char msg[200];
    const char *bad = nullptr;
    if (N < 1 || HW < 1) bad = "N and HW must be at least 1";
    else if (cin < 32 || cin % 32 || cin > RT_MAX_CIN) bad = "cin must be a positive multiple of 32, at most 1024";
    else if (cout < 1 || cout > RT_MAX_COUT) bad = "cout must be 1 ... 32";
    else if (slab_pixels < 0) bad = "slab_pixels must be 0 (auto) or positive";
    if (bad) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return cpn::fail(CPN_E_INVALID, msg);
    }
    if (N > 0x7fffffffll || HW > 0x7fffffffll || N * HW > 0x7fffffffll) {
        snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 pixels", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    const TailSlabs s = tls_partition((int32_t) N, HW, slab_pixels, RT_SLABS);
    if (s.slabs > RT_MAX_SLABS) {
        snprintf(msg, sizeof msg, "%s: more than 2^24 - 1 slabs (raise slab_pixels)", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    if (part) *part = s;
    return 0;
}

int rt_bad(const char *who, const char *what) {
    static thread_local char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return cpn::fail(CPN_E_INVALID, msg);
}

bool rt_dtype(int d) { return d == RT_F32 || d == RT_BF16; }
bool rt_aligned(const void *p, uintptr_t a) { return ((uintptr_t) p & (a - 1)) == 0; }
bool rt_scale(float s) { return s >= 0.f && isfinite(s); }

// the dynamic-LDS limit is a per-device function attribute
int rt_allow_lds(const void *kern, std::atomic<bool> *set) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return cpn::check_hip(hipErrorInvalidDevice, "cpn_tail");
    if (!set[dev].load(std::memory_order_acquire)) {
        if (const int rc = cpn::check_hip(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), "cpn_tail"))
            return rc;
        set[dev].store(true, std::memory_order_release);
    }
    return 0;
}

template <int CT, int PT>
int rt_launch_backward(const TailSlabs &part, const void *x, const void *dy, int dy_dtype, const void *w, int w_dtype,
                       const uint8_t *keep, float s, void *dx, float *ws, float *wsb, int cin, int cout, hipStream_t st) {
    static std::atomic<bool> set[64];
    auto kern = rt_backward_kernel<CT, PT>;
    if (const int rc = rt_allow_lds((const void *) kern, set)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned) part.slabs), dim3(256), (size_t) RtLds<PT>::total(cin, cout > 16 ? 2 : 1), st,
                       (const uint16_t *) x, dy, dy_dtype, w, w_dtype, keep, s, (uint16_t *) dx, ws, wsb, part, cin, cout);
    return 0;
}

}  // namespace

extern "C" {

int cpn_tail_info(int64_t N, int64_t HW, int32_t cin, int32_t cout, int64_t slab_pixels, int64_t info[8]) {
    TailSlabs part;
    if (const int rc = rt_check("cpn_tail_info", N, HW, cin, cout, slab_pixels, &part)) return rc;
    if (!info) return rt_bad("cpn_tail_info", "null pointer");
    info[0] = part.slabs;
    info[1] = part.slab_pixels;
    info[2] = part.steps;
    info[3] = tls_reduce_chain(part);
    info[4] = tls_bias_chain(part);
    info[5] = tls_forward_chain(cin);
    info[6] = part.per_image;
    info[7] = cout > 16 ? 2 : 1;
    return 0;
}

int64_t cpn_tail_workspace_bytes(int64_t N, int64_t HW, int32_t cin, int32_t cout, int64_t slab_pixels) {
    TailSlabs part;
    if (rt_check("cpn_tail_workspace_bytes", N, HW, cin, cout, slab_pixels, &part)) return 0;
    return part.slabs * ((int64_t) cin * cout + cout) * 4;
}

int cpn_tail_forward(const void *x, const void *weight, int32_t weight_dtype, const void *bias, int32_t bias_dtype,
                     const uint8_t *keep, float scale, int64_t N, int64_t HW, int32_t cin, int32_t cout, void *y, int32_t y_dtype,
                     void *stream) {
    const char *who = "cpn_tail_forward";
    if (const int rc = rt_check(who, N, HW, cin, cout, 0, nullptr)) return rc;
    if (!x || !weight || !y) return rt_bad(who, "null pointer");
    if (!rt_dtype(weight_dtype) || (bias && !rt_dtype(bias_dtype)) || !rt_dtype(y_dtype)) return rt_bad(who, "a dtype must be 0 (fp32) or 1 (bf16)");
    if (!rt_scale(scale)) return rt_bad(who, "scale must be finite and not negative");
    if (!rt_aligned(x, 16)) return rt_bad(who, "x must start at a 16-byte aligned address");
    if (!rt_aligned(y, y_dtype == RT_BF16 ? 2 : 4)) return rt_bad(who, "y must be aligned to its element size");
    static std::atomic<bool> set[64];
    if (const int rc = rt_allow_lds((const void *) rt_forward_kernel, set)) return rc;
    const TailTiles tiles = tls_tiles((int32_t) N, HW, RT_GROUPS);
    hipLaunchKernelGGL(rt_forward_kernel, dim3((unsigned) (N * tiles.groups)), dim3(256), (size_t) cin * 64, (hipStream_t) stream,
                       (const uint16_t *) x, weight, weight_dtype, bias, bias_dtype, keep, scale, y, y_dtype, tiles, HW, cin, cout);
    return cpn::check_hip(hipGetLastError(), who);
}

int cpn_tail_backward(const void *x, const void *dy, int32_t dy_dtype, const void *weight, int32_t weight_dtype, const uint8_t *keep,
                      float scale, int64_t N, int64_t HW, int32_t cin, int32_t cout, int64_t slab_pixels, void *dx, void *dw,
                      int32_t dw_dtype, void *db, int32_t db_dtype, void *workspace, int64_t workspace_bytes, void *stream) {
    const char *who = "cpn_tail_backward";
    TailSlabs part;
    if (const int rc = rt_check(who, N, HW, cin, cout, slab_pixels, &part)) return rc;
    if (!dy || (!dx && !dw && !db) || (dx && !weight) || (dw && !x) || ((dw || db) && !workspace)) return rt_bad(who, "null pointer");
    if (!rt_dtype(dy_dtype) || (dx && !rt_dtype(weight_dtype)) || (dw && !rt_dtype(dw_dtype)) || (db && !rt_dtype(db_dtype)))
        return rt_bad(who, "a dtype must be 0 (fp32) or 1 (bf16)");
    if (!rt_scale(scale)) return rt_bad(who, "scale must be finite and not negative");
    if (!rt_aligned(x, 16) || !rt_aligned(dx, 16) || !rt_aligned(workspace, 16))
        return rt_bad(who, "x, dx and the workspace must start at a 16-byte aligned address");
    if (!rt_aligned(dy, dy_dtype == RT_BF16 ? 2 : 4)) return rt_bad(who, "dy must be aligned to its element size");
    const int64_t per = (int64_t) cin * cout;
    if ((dw || db) && workspace_bytes < part.slabs * (per + cout) * 4)
        return cpn::fail(CPN_E_WORKSPACE, "cpn_tail_backward: workspace smaller than cpn_tail_workspace_bytes");
    hipStream_t st = (hipStream_t) stream;
    float *ws = dw ? (float *) workspace : nullptr, *wsb = db ? (float *) workspace + part.slabs * per : nullptr;
    int rc;
    if (cin <= 128) rc = rt_launch_backward<1, 64>(part, x, dy, dy_dtype, weight, weight_dtype, keep, scale, dx, ws, wsb, cin, cout, st);
    else if (cin <= 256) rc = rt_launch_backward<2, 64>(part, x, dy, dy_dtype, weight, weight_dtype, keep, scale, dx, ws, wsb, cin, cout, st);
    else if (cin <= 512) rc = rt_launch_backward<4, 64>(part, x, dy, dy_dtype, weight, weight_dtype, keep, scale, dx, ws, wsb, cin, cout, st);
    else rc = rt_launch_backward<8, 32>(part, x, dy, dy_dtype, weight, weight_dtype, keep, scale, dx, ws, wsb, cin, cout, st);
    if (rc) return rc;
    if (dw || db)
        hipLaunchKernelGGL(rt_reduce_kernel, dim3((unsigned) ((per + cout + 31) / 32)), dim3(256), 0, st, ws, wsb, keep, scale,
                           (int) part.slabs, (int) part.per_image, cin, cout, dw, dw_dtype, db, db_dtype);
    return cpn::check_hip(hipGetLastError(), who);
}

}  // extern "C"
