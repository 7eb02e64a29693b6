// The optimizer step on the GPU (gfx950): the kernels behind celldetection_amd.optim (AdamW, clip_grad_norm_, grad_norm).  The rule
// is the "Optimizer step" section of include/cpn_hip.h; the chunk partition, the lane mapping and the alignment rule are
// csrc/optim_chunks.h.  Compiled with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt: every operation below is one IEEE
// operation, the division and the square root included.
//
// All kernels are multi-tensor: they read the table of CpnOptimTensor records (one per tensor, uploaded once per step by
// cpn_optim_upload) and the chunk map (one record per chunk of OPT_CHUNK elements, uploaded once per set of sizes).  A workgroup of
// 256 lanes works on one chunk at a time, 16 bytes of the parameter's dtype per lane and item; at most OPT_MAX_GRID workgroups,
// which walk more chunks with that stride.
//   optim_sumsq_kernel:  per chunk one fp64 partial: each lane adds the squares of its elements (exact in fp64) in ascending order,
//                        the wave adds its lanes by halving (32, 16, ... 1), lane 0 adds the four waves in ascending order.
//   optim_norm_kernel:   one workgroup: lane l adds its run of partials in ascending order, lane 0 adds the lanes in ascending
//                        order; sqrt in fp64 -> the fp32 norm and the fp32 clip coefficient.
//   optim_adamw_kernel:  the update of p, m, v; all loads of an item are issued before its first use.  <NT>: m and v are stored
//                        with the non-temporal hint.
//   optim_scale_kernel:  g = g * coef rounded once to g's dtype.
// No floating-point atomics: results are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "optim_chunks.h"

static_assert(sizeof(CpnOptimTensor) == 80, "the table record is 80 bytes (celldetection_amd/optim.py lays it out by hand)");
static_assert(OPT_CHUNK == CPN_OPTIM_CHUNK && OPT_F32 == 0 && OPT_BF16 == 1, "include/cpn_hip.h states the chunk and the dtype codes");

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ uint16_t opt_bf16_rne(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t) ((u >> 16) | 0x40);  // NaN stays NaN
    return (uint16_t) ((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float opt_bf16_value(uint32_t b) { return __uint_as_float(b << 16); }
// fp64 -> fp32 rounded to odd: a later rounding to bf16 (to nearest even) is then the one rounding of the fp64 value
__device__ __forceinline__ float opt_f64_to_f32_odd(double v) {
    float f = (float) v;
    if ((double) f != v && !(v != v)) {
        uint32_t u = __float_as_uint(f);
        if (!(u & 1u)) u = fabs((double) f) < fabs(v) ? u + 1 : u - 1;
        f = __uint_as_float(u);
    }
    return f;
}

// one 16-byte vector of T <-> VEC floats (bf16 widens exactly and narrows to nearest even); float runs of 4 or 8
template <typename T>
struct Vec;
template <>
struct Vec<float> {
    static constexpr int N = 4;
    static __device__ __forceinline__ void load(const float *q, float v[4]) {
        const f32x4 a = *(const f32x4 *) q;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = a[i];
    }
    static __device__ __forceinline__ void store(float *q, const float v[4]) { *(f32x4 *) q = f32x4{v[0], v[1], v[2], v[3]}; }
    static __device__ __forceinline__ float load1(const float *q) { return *q; }
    static __device__ __forceinline__ void store1(float *q, float v) { *q = v; }
    static __device__ __forceinline__ void store1_rounded(float *q, double v) { *q = (float) v; }
};
template <>
struct Vec<uint16_t> {
    static constexpr int N = 8;
    static __device__ __forceinline__ void load(const uint16_t *q, float v[8]) {
        const u32x4 r = *(const u32x4 *) q;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = opt_bf16_value(r[i] & 0xffffu);
            v[2 * i + 1] = opt_bf16_value(r[i] >> 16);
        }
    }
    static __device__ __forceinline__ void store(uint16_t *q, const float v[8]) {
        u32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = (uint32_t) opt_bf16_rne(v[2 * i]) | ((uint32_t) opt_bf16_rne(v[2 * i + 1]) << 16);
        *(u32x4 *) q = r;
    }
    static __device__ __forceinline__ float load1(const uint16_t *q) { return opt_bf16_value(*q); }
    static __device__ __forceinline__ void store1(uint16_t *q, float v) { *q = opt_bf16_rne(v); }
    static __device__ __forceinline__ void store1_rounded(uint16_t *q, double v) { *q = opt_bf16_rne(opt_f64_to_f32_odd(v)); }
};

template <int N>
__device__ __forceinline__ void opt_load_f32(const float *q, float v[N]) {
#pragma unroll
    for (int i = 0; i < N; i += 4) {
        const f32x4 a = *(const f32x4 *) (q + i);
        v[i] = a[0], v[i + 1] = a[1], v[i + 2] = a[2], v[i + 3] = a[3];
    }
}
template <int N, bool NT>
__device__ __forceinline__ void opt_store_f32(float *q, const float v[N]) {
#pragma unroll
    for (int i = 0; i < N; i += 4) {
        const f32x4 a = f32x4{v[i], v[i + 1], v[i + 2], v[i + 3]};
        if (NT) __builtin_nontemporal_store(a, (f32x4 *) (q + i));
        else *(f32x4 *) (q + i) = a;
    }
}

// the rule of include/cpn_hip.h, operation by operation
__device__ __forceinline__ void opt_adamw(float &p, float g, float &m, float &v, const CpnOptimTensor &s, float coef) {
    g = g * coef;
    p = p * s.decay;
    m = m + (g - m) * s.w1;
    v = v * s.beta2 + (g * g) * s.w2;
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = p - s.step_size * (m / denom);
}

// the chunk a workgroup is at: false (and count 0) for a record that names no tensor of the table or no element of it
__device__ __forceinline__ bool opt_chunk(const CpnOptimTensor *table, int n, const int32_t *map, int64_t c, CpnOptimTensor *t,
                                          int64_t *base, int *count) {
    const int32_t ti = map[2 * c], k = map[2 * c + 1];
    *count = 0;
    if ((uint32_t) ti >= (uint32_t) n || k < 0) return false;
    *t = table[ti];
    *base = (int64_t) k * OPT_CHUNK;
    *count = opt_chunk_count(t->numel, k);
    return *count > 0;
}

template <typename T>
__device__ __forceinline__ double opt_sumsq_chunk(const CpnOptimTensor &t, int64_t base, int count, int lane) {
    constexpr int VEC = Vec<T>::N;
    const T *g = (const T *) t.g + base;
    const bool whole = !(t.flags & OPT_FLAG_SCALAR);
    double acc = 0.;
    for (int item = 0, items = opt_items(count, VEC); item < items; ++item) {
        const int e0 = opt_item_first(item, lane, VEC), ne = opt_item_elements(count, item, lane, VEC);
        if (ne == VEC && whole) {
            float gv[VEC];
            Vec<T>::load(g + e0, gv);
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc = acc + (double) gv[j] * (double) gv[j];
        } else {
            for (int j = 0; j < ne; ++j) {
                const double x = (double) Vec<T>::load1(g + e0 + j);
                acc = acc + x * x;
            }
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void optim_sumsq_kernel(const CpnOptimTensor *__restrict__ table, int n, const int32_t *__restrict__ map,
                                                          int64_t chunks, double *__restrict__ partials) {
    __shared__ double waves[OPT_LANES / 64];
    const int lane = threadIdx.x;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        CpnOptimTensor t;
        int64_t base;
        int count;
        double acc = 0.;
        if (opt_chunk(table, n, map, c, &t, &base, &count))
            acc = t.dtype == OPT_BF16 ? opt_sumsq_chunk<uint16_t>(t, base, count, lane) : opt_sumsq_chunk<float>(t, base, count, lane);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_down(acc, off, 64);
        if ((lane & 63) == 0) waves[lane >> 6] = acc;
        __syncthreads();
        if (lane == 0) partials[c] = ((waves[0] + waves[1]) + waves[2]) + waves[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void optim_norm_kernel(const double *__restrict__ partials, int64_t chunks, double max_norm,
                                                         float *__restrict__ out) {
    __shared__ double lanes[OPT_LANES];
    const int lane = threadIdx.x;
    const int64_t per = opt_final_per(chunks);
    int64_t end = (lane + 1) * per;
    if (end > chunks) end = chunks;
    double acc = 0.;
    for (int64_t i = lane * per; i < end; ++i) acc = acc + partials[i];
    lanes[lane] = acc;
    __syncthreads();
    if (lane == 0) {
        double sum = 0.;
        for (int l = 0; l < OPT_LANES; ++l) sum = sum + lanes[l];
        const float norm = (float) sqrt(sum);
        const double c = max_norm / ((double) norm + 1e-6);
        out[0] = norm;
        out[1] = (float) (c > 1. ? 1. : c);  // (a NaN stays a NaN)
    }
}

template <typename T, bool NT>
__device__ __forceinline__ void opt_adamw_chunk(const CpnOptimTensor &t, int64_t base, int count, float coef, int lane) {
    constexpr int VEC = Vec<T>::N;
    T *p = (T *) t.p + base;
    const T *g = (const T *) t.g + base;
    float *m = t.m + base, *v = t.v + base;
    const bool whole = !(t.flags & OPT_FLAG_SCALAR);
    for (int item = 0, items = opt_items(count, VEC); item < items; ++item) {
        const int e0 = opt_item_first(item, lane, VEC), ne = opt_item_elements(count, item, lane, VEC);
        if (ne == VEC && whole) {
            float pv[VEC], gv[VEC], mv[VEC], vv[VEC];
            Vec<T>::load(p + e0, pv);
            Vec<T>::load(g + e0, gv);
            opt_load_f32<VEC>(m + e0, mv);
            opt_load_f32<VEC>(v + e0, vv);
#pragma unroll
            for (int j = 0; j < VEC; ++j) opt_adamw(pv[j], gv[j], mv[j], vv[j], t, coef);
            Vec<T>::store(p + e0, pv);
            opt_store_f32<VEC, NT>(m + e0, mv);
            opt_store_f32<VEC, NT>(v + e0, vv);
        } else {
            for (int j = 0; j < ne; ++j) {
                const int e = e0 + j;
                float pe = Vec<T>::load1(p + e), me = m[e], ve = v[e];
                opt_adamw(pe, Vec<T>::load1(g + e), me, ve, t, coef);
                Vec<T>::store1(p + e, pe);
                m[e] = me;
                v[e] = ve;
            }
        }
    }
}

template <bool NT>
__global__ __launch_bounds__(256) void optim_adamw_kernel(const CpnOptimTensor *__restrict__ table, int n, const int32_t *__restrict__ map,
                                                          int64_t chunks, const float *__restrict__ coef_word) {
    const int lane = threadIdx.x;
    const float coef = coef_word ? *coef_word : 1.f;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        CpnOptimTensor t;
        int64_t base;
        int count;
        if (!opt_chunk(table, n, map, c, &t, &base, &count)) continue;
        if (!t.p || !t.m || !t.v) continue;  // a table uploaded without state (the norm's): nothing to update
        if (t.dtype == OPT_BF16) opt_adamw_chunk<uint16_t, NT>(t, base, count, coef, lane);
        else opt_adamw_chunk<float, NT>(t, base, count, coef, lane);
    }
}

template <typename T>
__device__ __forceinline__ void opt_scale_chunk(const CpnOptimTensor &t, int64_t base, int count, float coef, int lane) {
    constexpr int VEC = Vec<T>::N;
    T *g = (T *) t.g + base;
    const bool whole = !(t.flags & OPT_FLAG_SCALAR);
    for (int item = 0, items = opt_items(count, VEC); item < items; ++item) {
        const int e0 = opt_item_first(item, lane, VEC), ne = opt_item_elements(count, item, lane, VEC);
        if (ne == VEC && whole) {
            float gv[VEC];
            Vec<T>::load(g + e0, gv);
            if (sizeof(T) == 2) {  // the fp64 product of a bf16 and an fp32 is exact: one rounding to bf16
#pragma unroll
                for (int j = 0; j < VEC; ++j) gv[j] = opt_f64_to_f32_odd((double) gv[j] * (double) coef);
            } else {
#pragma unroll
                for (int j = 0; j < VEC; ++j) gv[j] = gv[j] * coef;
            }
            Vec<T>::store(g + e0, gv);
        } else {
            for (int j = 0; j < ne; ++j) Vec<T>::store1_rounded(g + e0 + j, (double) Vec<T>::load1(g + e0 + j) * (double) coef);
        }
    }
}

__global__ __launch_bounds__(256) void optim_scale_kernel(const CpnOptimTensor *__restrict__ table, int n, const int32_t *__restrict__ map,
                                                          int64_t chunks, const float *__restrict__ coef_word) {
    const int lane = threadIdx.x;
    const float coef = *coef_word;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        CpnOptimTensor t;
        int64_t base;
        int count;
        if (!opt_chunk(table, n, map, c, &t, &base, &count)) continue;
        if (t.dtype == OPT_BF16) opt_scale_chunk<uint16_t>(t, base, count, coef, lane);
        else opt_scale_chunk<float>(t, base, count, coef, lane);
    }
}

// the checks every launch over a device table shares; *launch: whether there is anything to do
int opt_check_launch(const char *who, const void *table, int32_t n, const int32_t *map, int64_t chunks, bool *launch) {
    static thread_local char msg[160];
    const char *what = nullptr;
    if (n < 0 || chunks < 0) what = "n and chunks must not be negative";
    else if (chunks > OPT_MAX_CHUNKS) what = "more than 2^31 - 1 chunks";
    else if (chunks > 0 && (!table || !map || n < 1)) what = "null table or map";
    else if (((uintptr_t) table & 7u) || ((uintptr_t) map & 3u)) what = "table (8 bytes) or map (4 bytes) unaligned";
    if (what) {
        snprintf(msg, sizeof msg, "%s: %s", who, what);
        return cpn::fail(chunks > OPT_MAX_CHUNKS ? CPN_E_UNSUPPORTED : CPN_E_INVALID, msg);
    }
    *launch = chunks > 0;
    return 0;
}

}  // namespace

extern "C" {

int cpn_optim_info(const int64_t *numel, int32_t n, int64_t info[3], int64_t *per_tensor) {
    if (n < 0 || (n > 0 && !numel) || !info) return cpn::fail(CPN_E_INVALID, "cpn_optim_info: null pointer or negative n");
    const int64_t chunks = opt_total_chunks(numel, n);
    if (chunks < 0) {
        for (int32_t t = 0; t < n; ++t)
            if (numel[t] < 0) return cpn::fail(CPN_E_INVALID, "cpn_optim_info: a negative size");
        return cpn::fail(CPN_E_UNSUPPORTED, "cpn_optim_info: more than 2^31 - 1 chunks");
    }
    info[0] = OPT_CHUNK;
    info[1] = chunks;
    info[2] = chunks;  // one fp64 partial per chunk
    if (per_tensor) {
        int64_t first = 0;
        for (int32_t t = 0; t < n; ++t) {
            per_tensor[3 * t] = first;
            per_tensor[3 * t + 1] = opt_chunks(numel[t]);
            per_tensor[3 * t + 2] = opt_tail(numel[t]);
            first += opt_chunks(numel[t]);
        }
    }
    return 0;
}

int cpn_optim_chunk_map(const int64_t *numel, int32_t n, int32_t *map, int64_t chunks) {
    if (n < 0 || (n > 0 && !numel)) return cpn::fail(CPN_E_INVALID, "cpn_optim_chunk_map: null pointer or negative n");
    const int64_t total = opt_total_chunks(numel, n);
    if (total < 0) return cpn::fail(CPN_E_INVALID, "cpn_optim_chunk_map: a negative size or more than 2^31 - 1 chunks");
    if (total != chunks) return cpn::fail(CPN_E_INVALID, "cpn_optim_chunk_map: chunks is not the count cpn_optim_info gives");
    if (total > 0 && !map) return cpn::fail(CPN_E_INVALID, "cpn_optim_chunk_map: null map");
    opt_fill_map(numel, n, map);
    return 0;
}

int cpn_optim_upload(CpnOptimTensor *host, int32_t n, int32_t with_state, void *device, void *stream) {
    if (n < 0 || (n > 0 && (!host || !device))) return cpn::fail(CPN_E_INVALID, "cpn_optim_upload: null pointer or negative n");
    if (((uintptr_t) host & 7u) || ((uintptr_t) device & 7u)) return cpn::fail(CPN_E_INVALID, "cpn_optim_upload: tables must be 8-byte aligned");
    for (int32_t i = 0; i < n; ++i) {
        CpnOptimTensor &t = host[i];
        if (t.numel < 0) return cpn::fail(CPN_E_INVALID, "cpn_optim_upload: a negative size");
        if (t.dtype != OPT_F32 && t.dtype != OPT_BF16) return cpn::fail(CPN_E_INVALID, "cpn_optim_upload: dtype must be 0 (fp32) or 1 (bf16)");
        if (!with_state) t.p = t.m = t.v = nullptr;
        t.flags = 0;
        if (t.numel == 0) continue;
        if (!t.g || (with_state && (!t.p || !t.m || !t.v))) return cpn::fail(CPN_E_INVALID, "cpn_optim_upload: null tensor pointer");
        const uintptr_t elem = t.dtype == OPT_BF16 ? 1u : 3u;
        if (((uintptr_t) t.g & elem) || ((uintptr_t) t.p & elem) || ((uintptr_t) t.m & 3u) || ((uintptr_t) t.v & 3u))
            return cpn::fail(CPN_E_INVALID, "cpn_optim_upload: a tensor pointer is not aligned to its element");
        t.flags = opt_flags((uint64_t) (uintptr_t) t.p, (uint64_t) (uintptr_t) t.g, (uint64_t) (uintptr_t) t.m, (uint64_t) (uintptr_t) t.v);
    }
    if (n == 0) return 0;
    return cpn::check_hip(hipMemcpyAsync(device, host, (size_t) n * sizeof(CpnOptimTensor), hipMemcpyHostToDevice, (hipStream_t) stream),
                          "cpn_optim_upload");
}

int cpn_optim_sumsq(const void *table, int32_t n, const int32_t *map, int64_t chunks, double *partials, void *stream) {
    bool launch;
    if (const int rc = opt_check_launch("cpn_optim_sumsq", table, n, map, chunks, &launch)) return rc;
    if (!launch) return 0;
    if (!partials || ((uintptr_t) partials & 7u)) return cpn::fail(CPN_E_INVALID, "cpn_optim_sumsq: null or unaligned partials");
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3((unsigned) opt_grid(chunks)), dim3(OPT_LANES), 0, (hipStream_t) stream,
                       (const CpnOptimTensor *) table, (int) n, map, chunks, partials);
    return cpn::check_hip(hipGetLastError(), "cpn_optim_sumsq");
}

int cpn_optim_norm(const double *partials, int64_t chunks, double max_norm, float *norm_coef, void *stream) {
    if (chunks < 0 || chunks > OPT_MAX_CHUNKS || (chunks > 0 && !partials) || !norm_coef)
        return cpn::fail(CPN_E_INVALID, "cpn_optim_norm: null pointer or chunks outside 0 ... 2^31 - 1");
    if (((uintptr_t) partials & 7u) || ((uintptr_t) norm_coef & 3u)) return cpn::fail(CPN_E_INVALID, "cpn_optim_norm: unaligned pointer");
    if (!(max_norm >= 0.)) return cpn::fail(CPN_E_INVALID, "cpn_optim_norm: max_norm must be >= 0 (+inf: no clipping)");
    hipLaunchKernelGGL(optim_norm_kernel, dim3(1), dim3(OPT_LANES), 0, (hipStream_t) stream, partials, chunks, max_norm, norm_coef);
    return cpn::check_hip(hipGetLastError(), "cpn_optim_norm");
}

int cpn_optim_adamw(const void *table, int32_t n, const int32_t *map, int64_t chunks, const float *coef, int32_t nontemporal,
                    void *stream) {
    bool launch;
    if (const int rc = opt_check_launch("cpn_optim_adamw", table, n, map, chunks, &launch)) return rc;
    if ((uintptr_t) coef & 3u) return cpn::fail(CPN_E_INVALID, "cpn_optim_adamw: unaligned coef");
    if (nontemporal != 0 && nontemporal != 1) return cpn::fail(CPN_E_INVALID, "cpn_optim_adamw: nontemporal must be 0 or 1");
    if (!launch) return 0;
    if (nontemporal)
        hipLaunchKernelGGL(optim_adamw_kernel<true>, dim3((unsigned) opt_grid(chunks)), dim3(OPT_LANES), 0, (hipStream_t) stream,
                           (const CpnOptimTensor *) table, (int) n, map, chunks, coef);
    else
        hipLaunchKernelGGL(optim_adamw_kernel<false>, dim3((unsigned) opt_grid(chunks)), dim3(OPT_LANES), 0, (hipStream_t) stream,
                           (const CpnOptimTensor *) table, (int) n, map, chunks, coef);
    return cpn::check_hip(hipGetLastError(), "cpn_optim_adamw");
}

int cpn_optim_scale(const void *table, int32_t n, const int32_t *map, int64_t chunks, const float *coef, void *stream) {
    bool launch;
    if (const int rc = opt_check_launch("cpn_optim_scale", table, n, map, chunks, &launch)) return rc;
    if (!coef || ((uintptr_t) coef & 3u)) return cpn::fail(CPN_E_INVALID, "cpn_optim_scale: null or unaligned coef");
    if (!launch) return 0;
    hipLaunchKernelGGL(optim_scale_kernel, dim3((unsigned) opt_grid(chunks)), dim3(OPT_LANES), 0, (hipStream_t) stream,
                       (const CpnOptimTensor *) table, (int) n, map, chunks, coef);
    return cpn::check_hip(hipGetLastError(), "cpn_optim_scale");
}

}  // extern "C"
