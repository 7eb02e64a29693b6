// The bias gradient of the trainable convs and the bf16 rounding they share (csrc/wgrad_dense.h, csrc/grouped_conv_train.hip):
//   ct_bias_slab_kernel / ct_bias_reduce_kernel: sum of dY per channel, eight interleaved chains per slab added in order, then the
//   slabs in ascending order; ct_launch_bias launches the two.  No floating-point atomics.  The partition is csrc/wgrad_slabs.h.
// Device code with internal linkage: every unit that includes this header gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "wgrad_slabs.h"

namespace {

constexpr int CT_F32 = 0, CT_BF16 = 1;

__device__ __forceinline__ uint16_t ct_bf16_rne(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t) ((u >> 16) | 0x40);  // NaN stays NaN
    return (uint16_t) ((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float ct_bf16_value(uint16_t b) { return __uint_as_float((uint32_t) b << 16); }

__global__ __launch_bounds__(256) void ct_bias_slab_kernel(const uint16_t *__restrict__ dy, float *__restrict__ wsb, WgSlabs part,
                                                            int Cout) {
    __shared__ float part_sum[WGS_BIAS_LANES][32];
    const int c = threadIdx.x & 31, chain = threadIdx.x >> 5, ch = blockIdx.y * 32 + c;
    int64_t p0, p1;
    wgs_range(part, blockIdx.x, &p0, &p1);
    float acc = 0.f;
    for (int64_t p = p0 + chain; p < p1; p += WGS_BIAS_LANES) acc += ct_bf16_value(dy[p * Cout + ch]);
    part_sum[chain][c] = acc;
    __syncthreads();
    if (chain == 0) {
        float s = part_sum[0][c];
        for (int i = 1; i < WGS_BIAS_LANES; ++i) s += part_sum[i][c];
        wsb[(int64_t) blockIdx.x * Cout + ch] = s;
    }
}

__global__ __launch_bounds__(256) void ct_bias_reduce_kernel(const float *__restrict__ wsb, int slabs, int Cout, void *db,
                                                              int db_dtype) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= Cout) return;
    float sum = wsb[ch];
    for (int s = 1; s < slabs; ++s) sum += wsb[(int64_t) s * Cout + ch];
    if (db_dtype == CT_BF16) ((uint16_t *) db)[ch] = ct_bf16_rne(sum);
    else ((float *) db)[ch] = sum;
}

// db [cout] from dY [pixel][cout] over the partition `part`: the slabs' sums into wsb [slab][cout], then the slabs in ascending order
inline void ct_launch_bias(const WgSlabs &part, const void *dy, float *wsb, int cout, void *db, int db_dtype, hipStream_t st) {
    hipLaunchKernelGGL(ct_bias_slab_kernel, dim3((unsigned) part.slabs, (unsigned) (cout / 32)), dim3(256), 0, st, (const uint16_t *) dy,
                       wsb, part, cout);
    hipLaunchKernelGGL(ct_bias_reduce_kernel, dim3((unsigned) ((cout + 255) / 256)), dim3(256), 0, st, wsb, part.slabs, cout, db, db_dtype);
}

}  // namespace
