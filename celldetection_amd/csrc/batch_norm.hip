// Trainable batch normalisation with an optional fused ReLU on the GPU (gfx950): the kernels behind celldetection_amd.nn.batch_norm.
// The rule is the "Trainable batch normalisation" section of include/cpn_hip.h; the slab partition and the lane mapping are
// csrc/bn_slabs.h.  Compiled with -ffp-contract=off: every fma below is written out.
//
// x is [M pixels][C channels] (a channels-last [N, C, H, W] tensor), bf16 or fp32, C = 8 V.  A workgroup of 256 lanes owns one
// channel block of vb <= 256 vectors and one slab of pixels; per step it moves R = 256 / vb consecutive pixels as one contiguous
// run, 16 B per lane and load (two loads for fp32).  A lane keeps its 8 channels: coefficients and accumulators stay in registers.
//   bn_sum_kernel<T, MODE>:   per (slab, channel) two fp64 sums -> workspace [slab][C][2].  MODE 0: sum x, sum x^2 (the
//                             products are exact: bf16^2 fits fp32, fp32^2 fits fp64).  MODE 1 / 2: sum g, sum g x with g = dy or
//                             dy [fmaf(x, scale, shift) > 0].  Each lane's chain over its pixels, then the lane partials per
//                             channel through LDS in ascending lane order.
//   bn_stats_finalise_kernel: adds the slabs in ascending order (8 channels per workgroup, bn_add_slabs); mean, var, invstd,
//                             scale, shift in fp64, each rounded once to fp32; the running statistics in fp64, rounded once to
//                             the buffers' dtype.
//   bn_eval_coeffs_kernel:    the same coefficients from the running statistics.
//   bn_apply_kernel<T, RELU>: y = fmaf(x, scale, shift), or its positive part.
//   bn_grad_finalise_kernel:  adds the slabs; dbeta, dgamma and the input kernel's per-channel a, b, c.
//   bn_input_kernel<T, RELU>: dx = fmaf(a, g, fmaf(b, x, c)) (training) or fmaf(a, g, 0) (eval).
// The tail of a residual block ("Trainable bottleneck block" of include/cpn_hip.h), kernels of their own beside the ones above:
//   bn_apply_residual_kernel<T, RELU>: y = fmaf(x, scale, shift) + r (an fp32 add), or its positive part.
//   bn_sum_residual_kernel<T>:         g = dy [y > 0] written once (the residual's gradient) and the sums of modes 1 / 2 on it.
// No floating-point atomics: results are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"
#include "bn_slabs.h"
#include "cpn_error.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int BN_F32 = 0, BN_BF16 = 1;
constexpr int BN_SLABS_WANTED = 2048;  // auto partition: about 8 workgroups per CU of the 256
constexpr int BN_MAX_SLABS = (1 << 24) - 1;  // a forced slab_pixels may not ask for more workgroups than one launch takes

__device__ __forceinline__ uint16_t bn_bf16_rne(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t) ((u >> 16) | 0x40);  // NaN stays NaN
    return (uint16_t) ((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float bn_bf16_value(uint32_t b) { return __uint_as_float(b << 16); }

// 8 channels of pixel p from vector offset c0 of a [M][C] tensor, widened exactly to fp32
template <typename T>
__device__ __forceinline__ void bn_load8(const T *base, int64_t p, int C, int c0, float v[8]);
template <>
__device__ __forceinline__ void bn_load8<uint16_t>(const uint16_t *base, int64_t p, int C, int c0, float v[8]) {
    const u32x4 r = *(const u32x4 *) (base + p * C + c0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = bn_bf16_value(r[i] & 0xffffu);
        v[2 * i + 1] = bn_bf16_value(r[i] >> 16);
    }
}
template <>
__device__ __forceinline__ void bn_load8<float>(const float *base, int64_t p, int C, int c0, float v[8]) {
    const f32x4 a = *(const f32x4 *) (base + p * C + c0), b = *(const f32x4 *) (base + p * C + c0 + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = a[i];
        v[4 + i] = b[i];
    }
}

template <typename T>
__device__ __forceinline__ void bn_store8(T *base, int64_t p, int C, int c0, const float v[8]);
template <>
__device__ __forceinline__ void bn_store8<uint16_t>(uint16_t *base, int64_t p, int C, int c0, const float v[8]) {
    u32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (uint32_t) bn_bf16_rne(v[2 * i]) | ((uint32_t) bn_bf16_rne(v[2 * i + 1]) << 16);
    *(u32x4 *) (base + p * C + c0) = r;
}
template <>
__device__ __forceinline__ void bn_store8<float>(float *base, int64_t p, int C, int c0, const float v[8]) {
    *(f32x4 *) (base + p * C + c0) = f32x4{v[0], v[1], v[2], v[3]};
    *(f32x4 *) (base + p * C + c0 + 4) = f32x4{v[4], v[5], v[6], v[7]};
}

__device__ __forceinline__ double bn_param(const void *p, int dtype, int c, double absent) {
    if (!p) return absent;
    return dtype == BN_BF16 ? (double) bn_bf16_value(((const uint16_t *) p)[c]) : (double) ((const float *) p)[c];
}
// one rounding from fp64 to bf16 (double -> float -> bf16 to nearest would round twice): round to odd into fp32 first (fp32 has more
// than 2 * 8 + 2 bits), then to nearest even
__device__ __forceinline__ float bn_f64_to_f32_odd(double v) {
    float f = (float) v;
    if ((double) f != v && !(v != v)) {
        uint32_t u = __float_as_uint(f);
        if (!(u & 1u)) {  // the neighbour on the other side of v is odd
            const bool away = fabs((double) f) < fabs(v);
            u = away ? u + 1 : u - 1;
        }
        f = __uint_as_float(u);
    }
    return f;
}
__device__ __forceinline__ void bn_store_rounded(void *p, int dtype, int c, double v) {
    if (dtype == BN_BF16) ((uint16_t *) p)[c] = bn_bf16_rne(bn_f64_to_f32_odd(v));
    else ((float *) p)[c] = (float) v;
}

// MODE 0: (x, x^2); 1: (g, g x), g = dy; 2: g = dy [fmaf(x, scale, shift) > 0]
template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_sum_kernel(const T *__restrict__ x, const T *__restrict__ dy,
                                                      const float *__restrict__ scale, const float *__restrict__ shift,
                                                      double *__restrict__ ws, BnSlabs part, int C) {
    __shared__ double lds[BNS_LANES * 16];  // [lane][channel of the lane][2]
    const int tid = threadIdx.x, block = blockIdx.y;
    const int vb = bns_block_vectors(part, block), R = bns_rows(vb);
    int row, vec;
    const bool active = bns_lane(vb, tid, &row, &vec);
    const int c0 = (block * BNS_LANES + vec) * BNS_VEC;
    int64_t p0, p1;
    bns_range(part, (int32_t) blockIdx.x, &p0, &p1);

    double s0[8], s1[8];
    float sc[8], sh[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        s0[i] = s1[i] = 0.;
        sc[i] = sh[i] = 0.f;
    }
    if (active) {
        if (MODE == 2) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                sc[i] = scale[c0 + i];
                sh[i] = shift[c0 + i];
            }
        }
        for (int64_t p = p0 + row; p < p1; p += R) {
            float xv[8], gv[8];
            bn_load8<T>(x, p, C, c0, xv);
            if (MODE != 0) bn_load8<T>(dy, p, C, c0, gv);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double xd = (double) xv[i];
                if (MODE == 0) {
                    s0[i] = s0[i] + xd;
                    s1[i] = s1[i] + xd * xd;
                } else {
                    float g = gv[i];
                    if (MODE == 2) g = __builtin_fmaf(xv[i], sc[i], sh[i]) > 0.f ? g : 0.f;
                    const double gd = (double) g;
                    s0[i] = s0[i] + gd;
                    s1[i] = s1[i] + gd * xd;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        lds[tid * 16 + 2 * i] = s0[i];
        lds[tid * 16 + 2 * i + 1] = s1[i];
    }
    __syncthreads();
    const int rows = bns_partials(p1 - p0, vb);
    double *out = ws + ((int64_t) blockIdx.x * C + (int64_t) block * BNS_LANES * BNS_VEC) * 2;
    for (int item = tid; item < vb * 16; item += BNS_LANES) {  // (vector, channel of it, which sum): consecutive in ws and in LDS
        const int v = item >> 4, j = item & 15;
        double sum = lds[v * 16 + j];
        for (int r = 1; r < rows; ++r) sum = sum + lds[(r * vb + v) * 16 + j];
        out[item] = sum;
    }
}

// The two sums of the workgroup's 8 consecutive channels (c0 ...), added over the slabs in ascending order: one chain per sum, held
// by lanes 0 ... 15 (lane j: channel c0 + j / 2, sum j % 2) -> total[16] in LDS, visible to the workgroup on return.  The slabs'
// 128-byte records are staged 256 at a time through LDS (one record per lane, the next 256 already on their way while a chain
// runs), so the chain waits for LDS and never for memory.
typedef __attribute__((ext_vector_type(2))) double f64x2;
__device__ __forceinline__ void bn_add_slabs(const double *__restrict__ ws, int slabs, int C, int c0, double *total) {
    __shared__ double stage[BNS_LANES * 16];
    const int tid = threadIdx.x;
    f64x2 rec[8] = {};
    auto fetch = [&](int slab) {
        if (slab < slabs) {
            const f64x2 *src = (const f64x2 *) (ws + ((int64_t) slab * C + c0) * 2);
#pragma unroll
            for (int i = 0; i < 8; ++i) rec[i] = src[i];
        }
    };
    fetch(tid);
    double acc = 0.;  // (0 + the first term is exact)
    for (int first = 0; first < slabs; first += BNS_LANES) {
#pragma unroll
        for (int i = 0; i < 8; ++i) ((f64x2 *) stage)[tid * 8 + i] = rec[i];
        __syncthreads();
        fetch(first + BNS_LANES + tid);
        if (tid < 16) {
            const int n = slabs - first < BNS_LANES ? slabs - first : BNS_LANES;
            for (int s = 0; s < n; ++s) acc = acc + stage[s * 16 + tid];
        }
        __syncthreads();
    }
    if (tid < 16) total[tid] = acc;
    __syncthreads();
}

__global__ __launch_bounds__(256) void bn_stats_finalise_kernel(const double *__restrict__ ws, int slabs, int C, int64_t M,
                                                                 const void *weight, int w_dtype, const void *bias, int b_dtype,
                                                                 void *running_mean, void *running_var, int r_dtype,
                                                                 double momentum, double eps, float *save_mean,
                                                                 float *save_invstd, float *scale, float *shift) {
    __shared__ double total[16];
    bn_add_slabs(ws, slabs, C, blockIdx.x * 8, total);
    if (threadIdx.x >= 8) return;
    const int c = blockIdx.x * 8 + threadIdx.x;
    const double sx = total[2 * threadIdx.x], sxx = total[2 * threadIdx.x + 1];
    const double m = (double) M;
    const double mean = sx / m;
    double var = sxx / m - mean * mean;
    var = var > 0. ? var : 0.;
    const double invstd = 1. / sqrt(var + eps);
    const double sc = bn_param(weight, w_dtype, c, 1.) * invstd;
    const double sh = bn_param(bias, b_dtype, c, 0.) - mean * sc;
    save_mean[c] = (float) mean;
    save_invstd[c] = (float) invstd;
    scale[c] = (float) sc;
    shift[c] = (float) sh;
    if (running_mean) bn_store_rounded(running_mean, r_dtype, c, (1. - momentum) * bn_param(running_mean, r_dtype, c, 0.) + momentum * mean);
    if (running_var)
        bn_store_rounded(running_var, r_dtype, c, (1. - momentum) * bn_param(running_var, r_dtype, c, 0.) + momentum * var * m / (m - 1.));
}

__global__ __launch_bounds__(256) void bn_eval_coeffs_kernel(int C, const void *weight, int w_dtype, const void *bias, int b_dtype,
                                                              const void *running_mean, const void *running_var, int r_dtype,
                                                              double eps, float *save_mean, float *save_invstd, float *scale,
                                                              float *shift) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double mean = bn_param(running_mean, r_dtype, c, 0.);
    const double invstd = 1. / sqrt(bn_param(running_var, r_dtype, c, 1.) + eps);
    const double sc = bn_param(weight, w_dtype, c, 1.) * invstd;
    const double sh = bn_param(bias, b_dtype, c, 0.) - mean * sc;
    save_mean[c] = (float) mean;
    save_invstd[c] = (float) invstd;
    scale[c] = (float) sc;
    shift[c] = (float) sh;
}

template <typename T, bool RELU>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T *__restrict__ x, T *__restrict__ y, const float *__restrict__ scale,
                                                        const float *__restrict__ shift, BnSlabs part, int C) {
    const int block = blockIdx.y;
    const int vb = bns_block_vectors(part, block), R = bns_rows(vb);
    int row, vec;
    if (!bns_lane(vb, threadIdx.x, &row, &vec)) return;
    const int c0 = (block * BNS_LANES + vec) * BNS_VEC;
    int64_t p0, p1;
    bns_range(part, (int32_t) blockIdx.x, &p0, &p1);
    float sc[8], sh[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sc[i] = scale[c0 + i];
        sh[i] = shift[c0 + i];
    }
    for (int64_t p = p0 + row; p < p1; p += R) {
        float v[8];
        bn_load8<T>(x, p, C, c0, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float t = __builtin_fmaf(v[i], sc[i], sh[i]);
            v[i] = RELU ? (t > 0.f ? t : 0.f) : t;
        }
        bn_store8<T>(y, p, C, c0, v);
    }
}

// coeffs: [3][C] fp32 (a, b, c of the input kernel) or NULL
__global__ __launch_bounds__(256) void bn_grad_finalise_kernel(const double *__restrict__ ws, int slabs, int C, int64_t M,
                                                                const float *save_mean, const float *save_invstd,
                                                                const void *weight, int w_dtype, void *dgamma, int dg_dtype,
                                                                void *dbeta, int db_dtype, float *coeffs) {
    __shared__ double total[16];
    bn_add_slabs(ws, slabs, C, blockIdx.x * 8, total);
    if (threadIdx.x >= 8) return;
    const int c = blockIdx.x * 8 + threadIdx.x;
    const double sg = total[2 * threadIdx.x], sgx = total[2 * threadIdx.x + 1];
    const double mean = (double) save_mean[c], invstd = (double) save_invstd[c], m = (double) M;
    const double dg = invstd * (sgx - mean * sg);
    if (dbeta) bn_store_rounded(dbeta, db_dtype, c, sg);
    if (dgamma) bn_store_rounded(dgamma, dg_dtype, c, dg);
    if (coeffs) {
        const double a = bn_param(weight, w_dtype, c, 1.) * invstd;
        const double b = -a * invstd * dg / m;
        const double cc = -a * sg / m - b * mean;
        coeffs[c] = (float) a;
        coeffs[C + c] = (float) b;
        coeffs[2 * C + c] = (float) cc;
    }
}

// b == NULL: eval mode, dx = fmaf(a, g, 0)
template <typename T, bool RELU>
__global__ __launch_bounds__(256) void bn_input_kernel(const T *__restrict__ x, const T *__restrict__ dy, T *__restrict__ dx,
                                                        const float *__restrict__ scale, const float *__restrict__ shift,
                                                        const float *__restrict__ a, const float *__restrict__ b,
                                                        const float *__restrict__ c, BnSlabs part, int C) {
    const int block = blockIdx.y;
    const int vb = bns_block_vectors(part, block), R = bns_rows(vb);
    int row, vec;
    if (!bns_lane(vb, threadIdx.x, &row, &vec)) return;
    const int c0 = (block * BNS_LANES + vec) * BNS_VEC;
    int64_t p0, p1;
    bns_range(part, (int32_t) blockIdx.x, &p0, &p1);
    float sc[8], sh[8], ca[8], cb[8], cc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sc[i] = RELU ? scale[c0 + i] : 0.f;
        sh[i] = RELU ? shift[c0 + i] : 0.f;
        ca[i] = a[c0 + i];
        cb[i] = b ? b[c0 + i] : 0.f;
        cc[i] = b ? c[c0 + i] : 0.f;
    }
    const bool affine_in_x = b != nullptr;
    for (int64_t p = p0 + row; p < p1; p += R) {
        float xv[8], gv[8];
        if (RELU || affine_in_x) bn_load8<T>(x, p, C, c0, xv);
        bn_load8<T>(dy, p, C, c0, gv);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float g = gv[i];
            if (RELU) g = __builtin_fmaf(xv[i], sc[i], sh[i]) > 0.f ? g : 0.f;
            const float inner = affine_in_x ? __builtin_fmaf(cb[i], xv[i], cc[i]) : 0.f;
            gv[i] = __builtin_fmaf(ca[i], g, inner);
        }
        bn_store8<T>(dx, p, C, c0, gv);
    }
}

// The tail of a residual block ("Trainable bottleneck block" of include/cpn_hip.h): y = t + r or its positive part,
// t = fmaf(x, scale, shift); the fp32 add is a rounding of its own, the store the only other one.
template <typename T, bool RELU>
__global__ __launch_bounds__(256) void bn_apply_residual_kernel(const T *__restrict__ x, const T *__restrict__ r, T *__restrict__ y,
                                                                 const float *__restrict__ scale, const float *__restrict__ shift,
                                                                 BnSlabs part, int C) {
    const int block = blockIdx.y;
    const int vb = bns_block_vectors(part, block), R = bns_rows(vb);
    int row, vec;
    if (!bns_lane(vb, threadIdx.x, &row, &vec)) return;
    const int c0 = (block * BNS_LANES + vec) * BNS_VEC;
    int64_t p0, p1;
    bns_range(part, (int32_t) blockIdx.x, &p0, &p1);
    float sc[8], sh[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sc[i] = scale[c0 + i];
        sh[i] = shift[c0 + i];
    }
    for (int64_t p = p0 + row; p < p1; p += R) {
        float v[8], rv[8];
        bn_load8<T>(x, p, C, c0, v);
        bn_load8<T>(r, p, C, c0, rv);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float s = __builtin_fmaf(v[i], sc[i], sh[i]) + rv[i];
            v[i] = RELU ? (s > 0.f ? s : 0.f) : s;
        }
        bn_store8<T>(y, p, C, c0, v);
    }
}

// bn_sum_kernel's modes 1 / 2 with the mask of the stored output: g = dy [y > 0], written once to `g` (the residual's gradient),
// and the same two fp64 sums (g, g x) in the same order into the same workspace layout.
template <typename T>
__global__ __launch_bounds__(256) void bn_sum_residual_kernel(const T *__restrict__ x, const T *__restrict__ dy,
                                                               const T *__restrict__ y, T *__restrict__ g,
                                                               double *__restrict__ ws, BnSlabs part, int C) {
    __shared__ double lds[BNS_LANES * 16];  // [lane][channel of the lane][2]
    const int tid = threadIdx.x, block = blockIdx.y;
    const int vb = bns_block_vectors(part, block), R = bns_rows(vb);
    int row, vec;
    const bool active = bns_lane(vb, tid, &row, &vec);
    const int c0 = (block * BNS_LANES + vec) * BNS_VEC;
    int64_t p0, p1;
    bns_range(part, (int32_t) blockIdx.x, &p0, &p1);

    double s0[8], s1[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s0[i] = s1[i] = 0.;
    if (active) {
        for (int64_t p = p0 + row; p < p1; p += R) {
            float xv[8], gv[8], yv[8];
            bn_load8<T>(x, p, C, c0, xv);
            bn_load8<T>(dy, p, C, c0, gv);
            bn_load8<T>(y, p, C, c0, yv);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                gv[i] = yv[i] > 0.f ? gv[i] : 0.f;
                const double xd = (double) xv[i], gd = (double) gv[i];
                s0[i] = s0[i] + gd;
                s1[i] = s1[i] + gd * xd;
            }
            bn_store8<T>(g, p, C, c0, gv);  // (values of the dtype already: the rounding is the identity)
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        lds[tid * 16 + 2 * i] = s0[i];
        lds[tid * 16 + 2 * i + 1] = s1[i];
    }
    __syncthreads();
    const int rows = bns_partials(p1 - p0, vb);
    double *out = ws + ((int64_t) blockIdx.x * C + (int64_t) block * BNS_LANES * BNS_VEC) * 2;
    for (int item = tid; item < vb * 16; item += BNS_LANES) {  // as in bn_sum_kernel
        const int v = item >> 4, j = item & 15;
        double sum = lds[v * 16 + j];
        for (int r = 1; r < rows; ++r) sum = sum + lds[(r * vb + v) * 16 + j];
        out[item] = sum;
    }
}

// 0, or the error code with its message recorded; the partition of an accepted call
int bn_check(const char *who, int64_t M, int64_t C, int64_t slab_pixels, BnSlabs *part) {
    static thread_local char msg[200];
    const char *bad = nullptr;
    if (M < 1) bad = "M must be at least 1";
    else if (C < 8 || C % 8) bad = "C must be a positive multiple of 8";
    else if (slab_pixels < 0) bad = "slab_pixels must be 0 (auto) or positive";
    if (bad) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return cpn::fail(CPN_E_INVALID, msg);
    }
    if (M > 0x7fffffffll || C > 65535 * 2048ll || slab_pixels > 0x7fffffffll) {
        snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 pixels (or pixels per slab), or more than 65535 blocks of 2048 channels", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    const int32_t V = (int32_t) (C / 8);
    const int32_t blocks = (V + BNS_LANES - 1) / BNS_LANES;
    const BnSlabs s = bns_partition(M, V, (int32_t) slab_pixels, BN_SLABS_WANTED / blocks);
    if (s.slabs > BN_MAX_SLABS) {  // grid.x = slabs: 256 * grid.x must stay below 2^32
        snprintf(msg, sizeof msg, "%s: more than 2^24 - 1 slabs (raise slab_pixels, or pass 0)", who);
        return cpn::fail(CPN_E_UNSUPPORTED, msg);
    }
    if (part) *part = s;
    return 0;
}

bool bn_dtype_ok(int d) { return d == BN_F32 || d == BN_BF16; }
// the tensors and the workspace are read and written 16 bytes at a time (NULL passes: an absent tensor)
bool bn_aligned(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr) {
    return (((uintptr_t) a | (uintptr_t) b | (uintptr_t) c | (uintptr_t) d) & 15) == 0;
}
int64_t bn_ws_bytes(const BnSlabs &s, int64_t C) { return (int64_t) s.slabs * C * 2 * (int64_t) sizeof(double); }
dim3 bn_grid(const BnSlabs &s) { return dim3((unsigned) s.slabs, (unsigned) s.blocks); }

}  // namespace

extern "C" {

int cpn_bn_info(int64_t M, int64_t C, int64_t slab_pixels, int64_t info[5]) {
    BnSlabs part;
    if (const int rc = bn_check("cpn_bn_info", M, C, slab_pixels, &part)) return rc;
    if (!info) return cpn::fail(CPN_E_INVALID, "cpn_bn_info: null pointer");
    info[0] = part.slabs;
    info[1] = part.slab_pixels;
    info[2] = bns_rows(bns_block_vectors(part, 0));
    info[3] = part.blocks;
    info[4] = bns_chain_max(part);
    return 0;
}

int64_t cpn_bn_workspace_bytes(int64_t M, int64_t C, int64_t slab_pixels) {
    BnSlabs part;
    if (bn_check("cpn_bn_workspace_bytes", M, C, slab_pixels, &part)) return 0;
    return bn_ws_bytes(part, C);
}

int cpn_bn_train_stats(const void *x, int32_t x_dtype, int64_t M, int64_t C, int64_t slab_pixels, const void *weight,
                       int32_t weight_dtype, const void *bias, int32_t bias_dtype, void *running_mean, void *running_var,
                       int32_t running_dtype, double momentum, double eps, float *save_mean, float *save_invstd, float *scale,
                       float *shift, void *workspace, int64_t workspace_bytes, void *stream) {
    BnSlabs part;
    if (const int rc = bn_check("cpn_bn_train_stats", M, C, slab_pixels, &part)) return rc;
    if (!x || !save_mean || !save_invstd || !scale || !shift || !workspace) return cpn::fail(CPN_E_INVALID, "cpn_bn_train_stats: null pointer");
    if (!bn_dtype_ok(x_dtype) || (weight && !bn_dtype_ok(weight_dtype)) || (bias && !bn_dtype_ok(bias_dtype)) ||
        ((running_mean || running_var) && !bn_dtype_ok(running_dtype)))
        return cpn::fail(CPN_E_INVALID, "cpn_bn_train_stats: a dtype must be 0 (fp32) or 1 (bf16)");
    if (running_var && M < 2) return cpn::fail(CPN_E_INVALID, "cpn_bn_train_stats: the unbiased running variance needs M >= 2");
    if (workspace_bytes < bn_ws_bytes(part, C)) return cpn::fail(CPN_E_WORKSPACE, "cpn_bn_train_stats: workspace smaller than cpn_bn_workspace_bytes");
    if (!bn_aligned(x, workspace)) return cpn::fail(CPN_E_INVALID, "cpn_bn_train_stats: x and workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t) stream;
    double *ws = (double *) workspace;
    if (x_dtype == BN_BF16)
        hipLaunchKernelGGL((bn_sum_kernel<uint16_t, 0>), bn_grid(part), dim3(256), 0, st, (const uint16_t *) x, (const uint16_t *) nullptr,
                           (const float *) nullptr, (const float *) nullptr, ws, part, (int) C);
    else
        hipLaunchKernelGGL((bn_sum_kernel<float, 0>), bn_grid(part), dim3(256), 0, st, (const float *) x, (const float *) nullptr,
                           (const float *) nullptr, (const float *) nullptr, ws, part, (int) C);
    if (const int rc = cpn::check_hip(hipGetLastError(), "cpn_bn_train_stats")) return rc;  // (no finalise on an unwritten workspace)
    hipLaunchKernelGGL(bn_stats_finalise_kernel, dim3((unsigned) (C / 8)), dim3(256), 0, st, ws, part.slabs, (int) C, M, weight,
                       weight_dtype, bias, bias_dtype, running_mean, running_var, running_dtype, momentum, eps, save_mean, save_invstd,
                       scale, shift);
    return cpn::check_hip(hipGetLastError(), "cpn_bn_train_stats");
}

int cpn_bn_eval_coeffs(int64_t C, const void *weight, int32_t weight_dtype, const void *bias, int32_t bias_dtype,
                       const void *running_mean, const void *running_var, int32_t running_dtype, double eps, float *save_mean,
                       float *save_invstd, float *scale, float *shift, void *stream) {
    if (const int rc = bn_check("cpn_bn_eval_coeffs", 1, C, 0, nullptr)) return rc;
    if (!running_mean || !running_var || !save_mean || !save_invstd || !scale || !shift)
        return cpn::fail(CPN_E_INVALID, "cpn_bn_eval_coeffs: null pointer");
    if (!bn_dtype_ok(running_dtype) || (weight && !bn_dtype_ok(weight_dtype)) || (bias && !bn_dtype_ok(bias_dtype)))
        return cpn::fail(CPN_E_INVALID, "cpn_bn_eval_coeffs: a dtype must be 0 (fp32) or 1 (bf16)");
    hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3((unsigned) ((C + 255) / 256)), dim3(256), 0, (hipStream_t) stream, (int) C, weight,
                       weight_dtype, bias, bias_dtype, running_mean, running_var, running_dtype, eps, save_mean, save_invstd, scale,
                       shift);
    return cpn::check_hip(hipGetLastError(), "cpn_bn_eval_coeffs");
}

int cpn_bn_apply(const void *x, void *y, int32_t dtype, int64_t M, int64_t C, int64_t slab_pixels, const float *scale,
                 const float *shift, int32_t relu, void *stream) {
    BnSlabs part;
    if (const int rc = bn_check("cpn_bn_apply", M, C, slab_pixels, &part)) return rc;
    if (!x || !y || !scale || !shift) return cpn::fail(CPN_E_INVALID, "cpn_bn_apply: null pointer");
    if (!bn_dtype_ok(dtype)) return cpn::fail(CPN_E_INVALID, "cpn_bn_apply: dtype must be 0 (fp32) or 1 (bf16)");
    if (!bn_aligned(x, y)) return cpn::fail(CPN_E_INVALID, "cpn_bn_apply: x and y must be 16-byte aligned");
    hipStream_t st = (hipStream_t) stream;
#define BN_APPLY(T, RELU) \
    hipLaunchKernelGGL((bn_apply_kernel<T, RELU>), bn_grid(part), dim3(256), 0, st, (const T *) x, (T *) y, scale, shift, part, (int) C)
    if (dtype == BN_BF16) {
        if (relu) BN_APPLY(uint16_t, true);
        else BN_APPLY(uint16_t, false);
    } else {
        if (relu) BN_APPLY(float, true);
        else BN_APPLY(float, false);
    }
#undef BN_APPLY
    return cpn::check_hip(hipGetLastError(), "cpn_bn_apply");
}

int cpn_bn_backward_reduce(const void *x, const void *dy, int32_t dtype, int64_t M, int64_t C, int64_t slab_pixels,
                           const float *scale, const float *shift, int32_t relu, const float *save_mean, const float *save_invstd,
                           const void *weight, int32_t weight_dtype, void *dgamma, int32_t dgamma_dtype, void *dbeta,
                           int32_t dbeta_dtype, float *coeffs, void *workspace, int64_t workspace_bytes, void *stream) {
    BnSlabs part;
    if (const int rc = bn_check("cpn_bn_backward_reduce", M, C, slab_pixels, &part)) return rc;
    if (!x || !dy || !save_mean || !save_invstd || !workspace || (relu && (!scale || !shift)) || (!dgamma && !dbeta && !coeffs))
        return cpn::fail(CPN_E_INVALID, "cpn_bn_backward_reduce: null pointer");
    if (!bn_dtype_ok(dtype) || (weight && !bn_dtype_ok(weight_dtype)) || (dgamma && !bn_dtype_ok(dgamma_dtype)) ||
        (dbeta && !bn_dtype_ok(dbeta_dtype)))
        return cpn::fail(CPN_E_INVALID, "cpn_bn_backward_reduce: a dtype must be 0 (fp32) or 1 (bf16)");
    if (workspace_bytes < bn_ws_bytes(part, C))
        return cpn::fail(CPN_E_WORKSPACE, "cpn_bn_backward_reduce: workspace smaller than cpn_bn_workspace_bytes");
    if (!bn_aligned(x, dy, workspace)) return cpn::fail(CPN_E_INVALID, "cpn_bn_backward_reduce: x, dy and workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t) stream;
    double *ws = (double *) workspace;
#define BN_SUM(T, MODE) \
    hipLaunchKernelGGL((bn_sum_kernel<T, MODE>), bn_grid(part), dim3(256), 0, st, (const T *) x, (const T *) dy, scale, shift, ws, part, (int) C)
    if (dtype == BN_BF16) {
        if (relu) BN_SUM(uint16_t, 2);
        else BN_SUM(uint16_t, 1);
    } else {
        if (relu) BN_SUM(float, 2);
        else BN_SUM(float, 1);
    }
#undef BN_SUM
    if (const int rc = cpn::check_hip(hipGetLastError(), "cpn_bn_backward_reduce")) return rc;  // (as in cpn_bn_train_stats)
    hipLaunchKernelGGL(bn_grad_finalise_kernel, dim3((unsigned) (C / 8)), dim3(256), 0, st, ws, part.slabs, (int) C, M, save_mean,
                       save_invstd, weight, weight_dtype, dgamma, dgamma_dtype, dbeta, dbeta_dtype, coeffs);
    return cpn::check_hip(hipGetLastError(), "cpn_bn_backward_reduce");
}

int cpn_residual_bn_apply(const void *x, const void *r, void *y, int32_t dtype, int64_t M, int64_t C, int64_t slab_pixels,
                          const float *scale, const float *shift, int32_t relu, void *stream) {
    BnSlabs part;
    if (const int rc = bn_check("cpn_residual_bn_apply", M, C, slab_pixels, &part)) return rc;
    if (!x || !r || !y || !scale || !shift) return cpn::fail(CPN_E_INVALID, "cpn_residual_bn_apply: null pointer");
    if (!bn_dtype_ok(dtype)) return cpn::fail(CPN_E_INVALID, "cpn_residual_bn_apply: dtype must be 0 (fp32) or 1 (bf16)");
    if (!bn_aligned(x, r, y)) return cpn::fail(CPN_E_INVALID, "cpn_residual_bn_apply: x, r and y must be 16-byte aligned");
    hipStream_t st = (hipStream_t) stream;
#define BN_APPLY_RES(T, RELU)                                                                                                      \
    hipLaunchKernelGGL((bn_apply_residual_kernel<T, RELU>), bn_grid(part), dim3(256), 0, st, (const T *) x, (const T *) r, (T *) y, \
                       scale, shift, part, (int) C)
    if (dtype == BN_BF16) {
        if (relu) BN_APPLY_RES(uint16_t, true);
        else BN_APPLY_RES(uint16_t, false);
    } else {
        if (relu) BN_APPLY_RES(float, true);
        else BN_APPLY_RES(float, false);
    }
#undef BN_APPLY_RES
    return cpn::check_hip(hipGetLastError(), "cpn_residual_bn_apply");
}

int cpn_residual_bn_backward_reduce(const void *x, const void *dy, const void *y, void *g, int32_t dtype, int64_t M, int64_t C,
                                    int64_t slab_pixels, const float *scale, const float *shift, int32_t relu,
                                    const float *save_mean, const float *save_invstd, const void *weight, int32_t weight_dtype,
                                    void *dgamma, int32_t dgamma_dtype, void *dbeta, int32_t dbeta_dtype, float *coeffs,
                                    void *workspace, int64_t workspace_bytes, void *stream) {
    if (!relu)  // g = dy: nothing to mask and nothing to write; y and g are not looked at
        return cpn_bn_backward_reduce(x, dy, dtype, M, C, slab_pixels, scale, shift, 0, save_mean, save_invstd, weight, weight_dtype,
                                      dgamma, dgamma_dtype, dbeta, dbeta_dtype, coeffs, workspace, workspace_bytes, stream);
    BnSlabs part;
    if (const int rc = bn_check("cpn_residual_bn_backward_reduce", M, C, slab_pixels, &part)) return rc;
    const bool sums = dgamma || dbeta || coeffs;  // without them g alone is written and the sums are dropped
    if (!x || !dy || !y || !g || !workspace || (sums && (!save_mean || !save_invstd)))
        return cpn::fail(CPN_E_INVALID, "cpn_residual_bn_backward_reduce: null pointer");
    if (!bn_dtype_ok(dtype) || (weight && !bn_dtype_ok(weight_dtype)) || (dgamma && !bn_dtype_ok(dgamma_dtype)) ||
        (dbeta && !bn_dtype_ok(dbeta_dtype)))
        return cpn::fail(CPN_E_INVALID, "cpn_residual_bn_backward_reduce: a dtype must be 0 (fp32) or 1 (bf16)");
    if (workspace_bytes < bn_ws_bytes(part, C))
        return cpn::fail(CPN_E_WORKSPACE, "cpn_residual_bn_backward_reduce: workspace smaller than cpn_bn_workspace_bytes");
    if (!bn_aligned(x, dy, y, g) || !bn_aligned(workspace))
        return cpn::fail(CPN_E_INVALID, "cpn_residual_bn_backward_reduce: x, dy, y, g and workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t) stream;
    double *ws = (double *) workspace;
    if (dtype == BN_BF16)
        hipLaunchKernelGGL((bn_sum_residual_kernel<uint16_t>), bn_grid(part), dim3(256), 0, st, (const uint16_t *) x, (const uint16_t *) dy,
                           (const uint16_t *) y, (uint16_t *) g, ws, part, (int) C);
    else
        hipLaunchKernelGGL((bn_sum_residual_kernel<float>), bn_grid(part), dim3(256), 0, st, (const float *) x, (const float *) dy,
                           (const float *) y, (float *) g, ws, part, (int) C);
    if (const int rc = cpn::check_hip(hipGetLastError(), "cpn_residual_bn_backward_reduce")) return rc;  // (as in cpn_bn_train_stats)
    if (!sums) return 0;
    hipLaunchKernelGGL(bn_grad_finalise_kernel, dim3((unsigned) (C / 8)), dim3(256), 0, st, ws, part.slabs, (int) C, M, save_mean,
                       save_invstd, weight, weight_dtype, dgamma, dgamma_dtype, dbeta, dbeta_dtype, coeffs);
    return cpn::check_hip(hipGetLastError(), "cpn_residual_bn_backward_reduce");
}

int cpn_bn_backward_input(const void *x, const void *dy, void *dx, int32_t dtype, int64_t M, int64_t C, int64_t slab_pixels,
                          const float *scale, const float *shift, int32_t relu, const float *a, const float *b, const float *c,
                          void *stream) {
    BnSlabs part;
    if (const int rc = bn_check("cpn_bn_backward_input", M, C, slab_pixels, &part)) return rc;
    if (!dy || !dx || !a || (!x && (relu || b)) || (relu && (!scale || !shift)) || ((b != nullptr) != (c != nullptr)))
        return cpn::fail(CPN_E_INVALID, "cpn_bn_backward_input: null pointer");
    if (!bn_dtype_ok(dtype)) return cpn::fail(CPN_E_INVALID, "cpn_bn_backward_input: dtype must be 0 (fp32) or 1 (bf16)");
    if (!bn_aligned(x, dy, dx)) return cpn::fail(CPN_E_INVALID, "cpn_bn_backward_input: x, dy and dx must be 16-byte aligned");
    hipStream_t st = (hipStream_t) stream;
#define BN_INPUT(T, RELU)                                                                                                       \
    hipLaunchKernelGGL((bn_input_kernel<T, RELU>), bn_grid(part), dim3(256), 0, st, (const T *) x, (const T *) dy, (T *) dx, scale, \
                       shift, a, b, c, part, (int) C)
    if (dtype == BN_BF16) {
        if (relu) BN_INPUT(uint16_t, true);
        else BN_INPUT(uint16_t, false);
    } else {
        if (relu) BN_INPUT(float, true);
        else BN_INPUT(float, false);
    }
#undef BN_INPUT
    return cpn::check_hip(hipGetLastError(), "cpn_bn_backward_input");
}

}  // extern "C"
