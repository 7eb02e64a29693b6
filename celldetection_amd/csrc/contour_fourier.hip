// Elliptic Fourier descriptors of contours on the GPU (gfx950): the kernels behind celldetection_amd.efd / contours2fourier /
// labels2fourier (the reference's cd.data.cpn.efd and contours2fourier, celldetection/data/cpn.py:23-90, 213-227).
//
// The rule (csrc/efd_chunks.h has it with the arithmetic; include/cpn_hip.h and celldetection_amd/fourier.py restate it).  A
// contour is n >= 1 points (x, y).  It is closed if |first - last| <= 1e-8 + 1e-5 |last| holds for both coordinates; depending
// on close_mode the first point is appended (N = n segments) or not (N = n - 1).  dt_i = sqrt(dx_i^2 + dy_i^2) + epsilon,
// t_0 = 0, t_(i+1) = t_i + dt_i, T = t_N; phi_(k,i) = k * (2 pi t_i / T), C_k = T / (2 k^2 pi^2);
// coeff[k-1] = C_k * (sum dx_i/dt_i dcos, sum dx_i/dt_i dsin, sum dy_i/dt_i dcos, sum dy_i/dt_i dsin), dcos = cos phi_(k,i+1) -
// cos phi_(k,i); location = first point + (1/T) sum [d_i/(2 dt_i) (t_(i+1)^2 - t_i^2) + (D_i - d_i/dt_i t_(i+1)) dt_i] with
// D_i = sum_(j<=i) d_j, for d = dx and d = dy.  N = 0 gives coefficients 0 and location NaN; the doubled point (N = 1, T =
// epsilon) gives coefficients 0 and exactly that point.  float64 throughout, no contraction (build.py).
//
// Passes (one wave of 64 lanes works on one chunk of up to CPN_EFD_CHUNK segments, efd_chunks.h):
//   prepare   one thread per contour: checks its offsets, decides the closing, N_k, and the number of chunks of a contour of
//             more than one chunk (0 for the others); an exclusive scan of those counts is the work list: work item w belongs
//             to the contour k with chunk_begin[k] <= w < chunk_begin[k + 1], chunk c = w - chunk_begin[k];
//   single    contours of at most one chunk (nearly all contours of a cell image), one wave each, everything in registers:
//             the scan of dt, sincos once per (k, segment end) with the start value taken from the neighbouring lane, the sums,
//             the constants, the result.  No workspace traffic;
//   sums      per work item: the chunk's sum of dt;          bases: per contour, the chunk bases and T in chunk order;
//   partials  per work item: 4 order + 2 partial sums into the workspace;
//   finish    per contour: the partials added in chunk order, constants, result.
// The k loop is the outer loop and keeps four accumulators: register use does not grow with the order.  No floating-point
// atomic anywhere; every sum has a fixed order that depends on the contour alone (efd_chunks.h), so results are bit-identical
// from run to run and wherever the contour lies in the packed array.  Every index is derived from `offsets`, which prepare
// checks before any other kernel is launched.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <rocprim/device/device_scan.hpp>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "efd_chunks.h"

namespace {

using u64 = unsigned long long;

constexpr int EF_R = EFD_ROUNDS;
constexpr int EF_COUNTERS = 4;  // invalid contours, open contours
static_assert(CPN_EFD_CHUNK % EFD_WAVE == 0 && EF_R >= 1 && EF_R <= 8, "a chunk is a whole number of rounds of one wave");

struct EfLane {
    double dxdt[EF_R], dydt[EF_R], t1[EF_R];
    double ax, ay;  // the lane's location sums
};

// Loads chunk c of a contour (p = its first point, n points, N segments) and scans t from `base`: efd_chunks.h, "t".  Returns
// the chunk's sum of dt.  All 64 lanes of the wave call it together.
template <class T>
__device__ __forceinline__ double ef_wave_load(const T *__restrict__ p, int64_t n, int64_t N, int64_t c, double epsilon, double base,
                                               int lane, EfLane &L) {
    const int len = efd_chunk_len(N, c);
    double carry = 0., t_before = base;
    L.ax = L.ay = 0.;
    double x0 = 0., y0 = 0.;
    if (len > 0) {
        x0 = (double) p[0];
        y0 = (double) p[1];
    }
#pragma unroll
    for (int r = 0; r < EF_R; ++r) {
        L.dxdt[r] = L.dydt[r] = 0.;
        L.t1[r] = t_before;
        if (r * EFD_WAVE < len) {  // the same for all lanes
            const int s = r * EFD_WAVE + lane;
            const bool has = s < len;
            EfdSeg sg = efd_no_segment();
            if (has) {
                const int64_t i = efd_chunk_begin(c) + s, j = i + 1 == n ? 0 : i + 1;  // i < N <= n, j < n
                sg = efd_segment((double) p[2 * i], (double) p[2 * i + 1], (double) p[2 * j], (double) p[2 * j + 1], x0, y0, epsilon);
            }
            double v = sg.dt;
#pragma unroll
            for (int d = 1; d < EFD_WAVE; d *= 2) {
                const double u = __shfl_up(v, d);
                if (lane >= d) v = v + u;
            }
            const double t = base + (carry + v);
            double t0 = __shfl_up(t, 1);
            if (lane == 0) t0 = t_before;
            if (has) {
                L.ax = L.ax + efd_location_term(sg.dx, sg.dxdt, sg.dt, sg.X, t0, t);
                L.ay = L.ay + efd_location_term(sg.dy, sg.dydt, sg.dt, sg.Y, t0, t);
            }
            carry = carry + __shfl(v, EFD_WAVE - 1);
            t_before = __shfl(t, EFD_WAVE - 1);
            L.dxdt[r] = sg.dxdt;
            L.dydt[r] = sg.dydt;
            L.t1[r] = t;
        }
    }
    return carry;
}

__device__ __forceinline__ double ef_butterfly(double v) {
#pragma unroll
    for (int d = EFD_WAVE / 2; d >= 1; d /= 2) v = v + __shfl_xor(v, d);
    return v;
}

// The sums of a loaded chunk (efd_chunks.h, "sums"): emit(j, value) receives sum j of 4 * order + 2 on every lane.
template <class Emit>
__device__ __forceinline__ void ef_wave_partials(EfLane &L, int len, double base, double T_, int order, int lane, Emit emit) {
    const int rounds = (len + EFD_WAVE - 1) / EFD_WAVE;
    emit(4 * order, ef_butterfly(L.ax));
    emit(4 * order + 1, ef_butterfly(L.ay));
    if (rounds == 0) {
        for (int j = 0; j < 4 * order; ++j) emit(j, 0.);
        return;
    }
#pragma unroll
    for (int r = 0; r < EF_R; ++r) L.t1[r] = efd_phi1(L.t1[r], T_);  // from here on phi_(1, segment end)
    const double phi_base = efd_phi1(base, T_);
    for (int k = 1; k <= order; ++k) {
        const double kk = (double) k;
        double c_before = 1., s_before = 0.;  // cos 0, sin 0: the first chunk starts at t = 0
        if (base != 0.) sincos(phi_base * kk, &s_before, &c_before);
        double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
#pragma unroll
        for (int r = 0; r < EF_R; ++r) {
            if (r < rounds) {  // the same for all lanes
                double s1, c1;
                sincos(L.t1[r] * kk, &s1, &c1);
                double c0 = __shfl_up(c1, 1), s0 = __shfl_up(s1, 1);
                if (lane == 0) {
                    c0 = c_before;
                    s0 = s_before;
                }
                const double dc = c1 - c0, ds = s1 - s0;
                a0 = a0 + L.dxdt[r] * dc;
                a1 = a1 + L.dxdt[r] * ds;
                a2 = a2 + L.dydt[r] * dc;
                a3 = a3 + L.dydt[r] * ds;
                c_before = __shfl(c1, EFD_WAVE - 1);
                s_before = __shfl(s1, EFD_WAVE - 1);
            }
        }
        emit(4 * (k - 1), ef_butterfly(a0));
        emit(4 * (k - 1) + 1, ef_butterfly(a1));
        emit(4 * (k - 1) + 2, ef_butterfly(a2));
        emit(4 * (k - 1) + 3, ef_butterfly(a3));
    }
}

// sum j of a contour -> its place in the result
__device__ __forceinline__ void ef_store(int j, double sum, double T_, int order, double x0, double y0, double *__restrict__ coeff_k,
                                         double *__restrict__ loc_k) {
    if (j < 4 * order) coeff_k[j] = efd_constant(T_, j / 4 + 1) * sum;
    else loc_k[j - 4 * order] = efd_location(j == 4 * order ? x0 : y0, sum, T_);
}

template <class T>
__global__ __launch_bounds__(256) void ef_prepare_kernel(const T *__restrict__ points, const int64_t *__restrict__ offsets, int64_t K,
                                                         int64_t P, int mode, int64_t *__restrict__ nseg, int64_t *__restrict__ nch,
                                                         u64 *__restrict__ counters) {
    const int64_t k = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k > K) return;
    if (k == K) {
        nch[K] = 0;
        if (!efd_ends_ok(offsets[0], offsets[K], P)) atomicAdd(&counters[0], (u64) 1);
        return;
    }
    const int64_t a = offsets[k], b = offsets[k + 1];
    nseg[k] = 0;
    nch[k] = 0;
    if (!efd_range_ok(a, b, P)) {
        atomicAdd(&counters[0], (u64) 1);
        return;
    }
    const int64_t n = b - a;
    const bool closed = efd_is_closed((double) points[2 * a], (double) points[2 * a + 1], (double) points[2 * (b - 1)],
                                      (double) points[2 * (b - 1) + 1]);
    if (!closed) atomicAdd(&counters[1], (u64) 1);
    const bool append = mode == CPN_EFD_CLOSE_ALL || (mode == CPN_EFD_CLOSE_EACH && !closed);
    const int64_t N = efd_num_segments(n, append);
    nseg[k] = N;
    nch[k] = N > CPN_EFD_CHUNK ? efd_num_chunks(N) : 0;
}

// contours of at most one chunk: one wave each, 4 waves per block
template <class T>
__global__ __launch_bounds__(256) void ef_single_kernel(const T *__restrict__ points, const int64_t *__restrict__ offsets,
                                                        const int64_t *__restrict__ nseg, int64_t K, int order, double epsilon,
                                                        double *__restrict__ coeff, double *__restrict__ loc) {
    const int lane = threadIdx.x & (EFD_WAVE - 1);
    const int64_t k = (int64_t) blockIdx.x * (blockDim.x / EFD_WAVE) + threadIdx.x / EFD_WAVE;
    if (k >= K) return;
    const int64_t N = nseg[k];
    if (N > CPN_EFD_CHUNK) return;
    const int64_t a = offsets[k], n = offsets[k + 1] - a;
    const T *p = points + 2 * a;
    EfLane L;
    const double T_ = ef_wave_load(p, n, N, 0, epsilon, 0., lane, L);
    const double x0 = (double) p[0], y0 = (double) p[1];
    double *ck = coeff + k * 4 * order, *lk = loc + k * 2;
    ef_wave_partials(L, (int) N, 0., T_, order, lane, [&](int j, double v) {
        if (lane == 0) ef_store(j, v, T_, order, x0, y0, ck, lk);
    });
}

// work item w -> the contour k with chunk_begin[k] <= w < chunk_begin[k + 1] (chunk_begin[K] = all work items > w)
__device__ __forceinline__ int64_t ef_find(const int64_t *__restrict__ chunk_begin, int64_t K, int64_t w) {
    int64_t lo = 0, hi = K;
    while (lo < hi) {  // the first index whose chunk_begin is > w
        const int64_t mid = lo + (hi - lo) / 2;
        if (chunk_begin[mid] > w) hi = mid; else lo = mid + 1;
    }
    return lo - 1;
}

// MODE 0: the chunk's sum of dt.  MODE 1: its partial sums.
template <class T, int MODE>
__global__ __launch_bounds__(256) void ef_chunk_kernel(const T *__restrict__ points, const int64_t *__restrict__ offsets,
                                                       const int64_t *__restrict__ nseg, const int64_t *__restrict__ chunk_begin,
                                                       int64_t K, int64_t M, int order, double epsilon, double *__restrict__ chunk_sum,
                                                       const double *__restrict__ chunk_base, const double *__restrict__ total,
                                                       double *__restrict__ part) {
    const int lane = threadIdx.x & (EFD_WAVE - 1);
    const int64_t w = (int64_t) blockIdx.x * (blockDim.x / EFD_WAVE) + threadIdx.x / EFD_WAVE;
    if (w >= M) return;
    const int64_t k = ef_find(chunk_begin, K, w);
    if (k < 0 || k >= K) return;
    const int64_t c = w - chunk_begin[k], N = nseg[k];
    if (c < 0 || c >= efd_num_chunks(N)) return;
    const int64_t a = offsets[k], n = offsets[k + 1] - a;
    const T *p = points + 2 * a;
    EfLane L;
    if constexpr (MODE == 0) {
        const double sum = ef_wave_load(p, n, N, c, epsilon, 0., lane, L);
        if (lane == 0) chunk_sum[w] = sum;
    } else {
        const double base = chunk_base[w];
        ef_wave_load(p, n, N, c, epsilon, base, lane, L);
        double *out = part + w * (int64_t) (4 * order + 2);
        ef_wave_partials(L, efd_chunk_len(N, c), base, total[k], order, lane, [&](int j, double v) {
            if (lane == 0) out[j] = v;
        });
    }
}

// one thread per work item; the thread of a contour's chunk 0 walks the contour's chunk sums in chunk order
__global__ __launch_bounds__(256) void ef_bases_kernel(const int64_t *__restrict__ nseg, const int64_t *__restrict__ chunk_begin,
                                                       int64_t K, int64_t M, const double *__restrict__ chunk_sum,
                                                       double *__restrict__ chunk_base, double *__restrict__ total) {
    const int64_t w = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= M) return;
    const int64_t k = ef_find(chunk_begin, K, w);
    if (k < 0 || k >= K || w != chunk_begin[k]) return;
    const int64_t chunks = chunk_begin[k + 1] - w;
    double b = 0.;
    for (int64_t c = 0; c < chunks; ++c) {
        chunk_base[w + c] = b;
        b = b + chunk_sum[w + c];
    }
    total[k] = b;
}

// one wave per work item; the wave of a contour's chunk 0 adds the contour's partials in chunk order, one sum per lane
template <class T>
__global__ __launch_bounds__(256) void ef_finish_kernel(const T *__restrict__ points, const int64_t *__restrict__ offsets,
                                                        const int64_t *__restrict__ chunk_begin, int64_t K, int64_t M, int order,
                                                        const double *__restrict__ total, const double *__restrict__ part,
                                                        double *__restrict__ coeff, double *__restrict__ loc) {
    const int lane = threadIdx.x & (EFD_WAVE - 1);
    const int64_t w = (int64_t) blockIdx.x * (blockDim.x / EFD_WAVE) + threadIdx.x / EFD_WAVE;
    if (w >= M) return;
    const int64_t k = ef_find(chunk_begin, K, w);
    if (k < 0 || k >= K || w != chunk_begin[k]) return;
    const int64_t chunks = chunk_begin[k + 1] - w;
    const int nv = 4 * order + 2;
    const T *p = points + 2 * offsets[k];
    const double x0 = (double) p[0], y0 = (double) p[1], T_ = total[k];
    for (int j = lane; j < nv; j += EFD_WAVE) {
        double s = part[w * nv + j];
        for (int64_t c = 1; c < chunks; ++c) s = s + part[(w + c) * nv + j];
        ef_store(j, s, T_, order, x0, y0, coeff + k * 4 * order, loc + k * 2);
    }
}

inline size_t ef_align(size_t n) { return (n + 255) & ~(size_t) 255; }

// an upper bound of the work items: a contour of more than one chunk has N >= CHUNK + 1 segments and at most N / CHUNK + 1
// chunks, and all contours together have at most P + K segments
inline int64_t ef_max_items(int64_t K, int64_t P) { return (P + K) / CPN_EFD_CHUNK + (P + K) / (CPN_EFD_CHUNK + 1) + 1; }

struct EfLayout {
    size_t counters, nseg, nch, chunk_begin, total, chunk_sum, chunk_base, part, tmp, tmp_bytes, bytes;
};

EfLayout ef_layout(int64_t K, int64_t P, int order) {
    EfLayout l{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = ef_align(o + bytes); return at; };
    const size_t k1 = (size_t) K + 1, m = (size_t) ef_max_items(K, P);
    l.counters = take(EF_COUNTERS * 8);
    l.nseg = take(k1 * 8); l.nch = take(k1 * 8); l.chunk_begin = take(k1 * 8); l.total = take(k1 * 8);
    l.chunk_sum = take(m * 8); l.chunk_base = take(m * 8);
    l.part = take(m * (size_t) (4 * order + 2) * 8);
    (void) rocprim::exclusive_scan(nullptr, l.tmp_bytes, (int64_t *) nullptr, (int64_t *) nullptr, (int64_t) 0, k1,
                                   rocprim::plus<int64_t>(), (hipStream_t) 0);
    l.tmp = take(l.tmp_bytes);
    l.bytes = o;
    return l;
}

bool ef_shape_ok(int64_t K, int64_t P, int32_t order) {
    return K >= 0 && K <= 0x7fffffff && P >= 0 && P <= ((int64_t) 1 << 40) && order >= 1 && order <= CPN_EFD_MAX_ORDER;
}

template <class T>
int ef_run(const T *points, const int64_t *offsets, int64_t K, int64_t P, int order, double epsilon, int mode, bool timed, char *ws,
           const EfLayout &l, double *coeff, double *loc, int64_t *status, hipStream_t st) {
    u64 *counters = (u64 *) (ws + l.counters);
    int64_t *nseg = (int64_t *) (ws + l.nseg), *nch = (int64_t *) (ws + l.nch), *chunk_begin = (int64_t *) (ws + l.chunk_begin);
    double *total = (double *) (ws + l.total), *chunk_sum = (double *) (ws + l.chunk_sum), *chunk_base = (double *) (ws + l.chunk_base);
    double *part = (double *) (ws + l.part);
    hipEvent_t ev[6] = {};
    int n_ev = 0;
    auto mark = [&]() {
        if (timed && n_ev < 6 && hipEventCreate(&ev[n_ev]) == hipSuccess) {
            (void) hipEventRecord(ev[n_ev], st);
            ++n_ev;
        }
    };
    auto done = [&](int rc) {
        for (int i = 0; i < n_ev; ++i) (void) hipEventDestroy(ev[i]);
        return rc;
    };
    mark();
    hipError_t e = hipMemsetAsync(counters, 0, EF_COUNTERS * 8, st);
    if (e != hipSuccess) return done(cpn::check_hip(e, "cpn_efd"));
    const unsigned kb = (unsigned) ((K + 1 + 255) / 256);
    hipLaunchKernelGGL(ef_prepare_kernel<T>, dim3(kb), dim3(256), 0, st, points, offsets, K, P, mode, nseg, nch, counters);
    size_t tmp_bytes = l.tmp_bytes;
    e = rocprim::exclusive_scan(ws + l.tmp, tmp_bytes, nch, chunk_begin, (int64_t) 0, (size_t) K + 1, rocprim::plus<int64_t>(), st);
    if (e != hipSuccess) return done(cpn::check_hip(e, "cpn_efd: scan"));
    u64 host[EF_COUNTERS];
    int64_t M = 0;
    e = hipMemcpyAsync(host, counters, sizeof(host), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&M, chunk_begin + K, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return done(cpn::check_hip(e, "cpn_efd: prepare"));
    if (host[0]) return done(cpn::fail(CPN_E_INVALID, "cpn_efd: offsets must start at 0, end at the number of points, and grow by at "
                                                       "least one point per contour"));
    status[0] = (int64_t) host[1];
    status[1] = M;
    if (mode == CPN_EFD_CLOSE_NONE && host[1]) return done(0);  // the caller raises: nothing is computed
    if (M < 0 || M > ef_max_items(K, P)) return done(cpn::fail(CPN_E_INTERNAL, "cpn_efd: more work items than the bound"));
    mark();
    hipLaunchKernelGGL(ef_single_kernel<T>, dim3((unsigned) ((K + 3) / 4)), dim3(256), 0, st, points, offsets, nseg, K, order, epsilon,
                       coeff, loc);
    mark();
    if (M > 0) {
        const unsigned wb = (unsigned) ((M + 3) / 4), tb = (unsigned) ((M + 255) / 256);
        hipLaunchKernelGGL((ef_chunk_kernel<T, 0>), dim3(wb), dim3(256), 0, st, points, offsets, nseg, chunk_begin, K, M, order, epsilon,
                           chunk_sum, (const double *) chunk_base, (const double *) total, part);
        hipLaunchKernelGGL(ef_bases_kernel, dim3(tb), dim3(256), 0, st, nseg, chunk_begin, K, M, chunk_sum, chunk_base, total);
        mark();
        hipLaunchKernelGGL((ef_chunk_kernel<T, 1>), dim3(wb), dim3(256), 0, st, points, offsets, nseg, chunk_begin, K, M, order, epsilon,
                           chunk_sum, (const double *) chunk_base, (const double *) total, part);
        mark();
        hipLaunchKernelGGL(ef_finish_kernel<T>, dim3(wb), dim3(256), 0, st, points, offsets, chunk_begin, K, M, order,
                           (const double *) total, (const double *) part, coeff, loc);
        mark();
    }
    e = hipGetLastError();
    if (e != hipSuccess) return done(cpn::check_hip(e, "cpn_efd"));
    if (timed) {
        e = hipStreamSynchronize(st);
        if (e != hipSuccess) return done(cpn::check_hip(e, "cpn_efd"));
        for (int i = 0; i + 1 < n_ev; ++i) {
            float ms = 0.f;
            (void) hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            status[2 + i] = (int64_t) ((double) ms * 1e6);
        }
    }
    return done(0);
}

}  // namespace

extern "C" {

int64_t cpn_efd_workspace_bytes(int64_t K, int64_t P, int32_t order) {
    if (!ef_shape_ok(K, P, order)) return 0;
    return (int64_t) ef_layout(K, P, order).bytes;
}

int cpn_efd(const void *points, int32_t points_dtype, const int64_t *offsets, int64_t K, int64_t P, int32_t order, double epsilon,
            int32_t close_mode, void *workspace, int64_t workspace_bytes, double *coefficients, double *locations, int64_t *status_host,
            void *stream) {
    const int mode = close_mode & ~CPN_EFD_TIMED;
    if (!ef_shape_ok(K, P, order))
        return cpn::fail(CPN_E_INVALID, "cpn_efd: bad arguments (need K >= 0, P >= 0, 1 <= order <= CPN_EFD_MAX_ORDER)");
    if (points_dtype != CPN_EFD_POINTS_I32 && points_dtype != CPN_EFD_POINTS_F64)
        return cpn::fail(CPN_E_INVALID, "cpn_efd: points_dtype must be CPN_EFD_POINTS_I32 or CPN_EFD_POINTS_F64");
    if (mode != CPN_EFD_CLOSE_NONE && mode != CPN_EFD_CLOSE_ALL && mode != CPN_EFD_CLOSE_EACH)
        return cpn::fail(CPN_E_INVALID, "cpn_efd: close_mode must be CPN_EFD_CLOSE_NONE, _ALL or _EACH");
    if (!(epsilon >= 0.)) return cpn::fail(CPN_E_INVALID, "cpn_efd: epsilon must be >= 0");
    if (!status_host) return cpn::fail(CPN_E_INVALID, "cpn_efd: null pointer");
    for (int i = 0; i < CPN_EFD_STATUS_WORDS; ++i) status_host[i] = 0;
    if (K == 0) {
        if (P != 0) return cpn::fail(CPN_E_INVALID, "cpn_efd: offsets must end at the number of points");
        return 0;
    }
    if (P < K) return cpn::fail(CPN_E_INVALID, "cpn_efd: every contour needs at least one point");
    if (!points || !offsets || !workspace || !coefficients || !locations) return cpn::fail(CPN_E_INVALID, "cpn_efd: null pointer");
    const EfLayout l = ef_layout(K, P, order);
    if (workspace_bytes < (int64_t) l.bytes) return cpn::fail(CPN_E_WORKSPACE, "cpn_efd: workspace too small");
    const bool timed = (close_mode & CPN_EFD_TIMED) != 0;
    if (points_dtype == CPN_EFD_POINTS_I32)
        return ef_run((const int32_t *) points, offsets, K, P, order, epsilon, mode, timed, (char *) workspace, l, coefficients,
                      locations, status_host, (hipStream_t) stream);
    return ef_run((const double *) points, offsets, K, P, order, epsilon, mode, timed, (char *) workspace, l, coefficients, locations,
                  status_host, (hipStream_t) stream);
}

}  // extern "C"
