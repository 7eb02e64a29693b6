// What the dense weight gradient (csrc/conv_train.hip) and the weight gradient over a virtual concat (csrc/cat_conv_train.hip) share
// besides the partition (csrc/wgrad_slabs.h) and the bias kernels (csrc/wgrad_bias.h): the kernel that adds the slabs' partial sums,
// and the choice of fragments per wave and of slabs per filter size.  Device code with internal linkage: every unit that includes
// this header gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "wgrad_bias.h"  // ct_bf16_rne, the dtype codes

namespace {

// workspace [slab][tap][co][ci] -> dw [co][ci][tap]: the slabs in ascending order (one fp32 chain per element), one rounding
__global__ __launch_bounds__(256) void ct_wgrad_reduce_kernel(const float *__restrict__ ws, int slabs, int KK, int Cout, int Cin,
                                                               void *dw, int dw_dtype) {
    const long per = (long) KK * Cout * Cin;
    const long e = (long) blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    float sum = ws[e];
    for (int s = 1; s < slabs; ++s) sum += ws[s * per + e];
    const long cc = e % ((long) Cout * Cin);
    const long o = cc * KK + e / ((long) Cout * Cin);
    if (dw_dtype == CT_BF16) ((uint16_t *) dw)[o] = ct_bf16_rne(sum);
    else ((float *) dw)[o] = sum;
}

// The kernel per filter size: MT fragments of 32 output channels per wave (a workgroup: 64 MT output x 64 input channels), and the
// slabs of the auto partition, both as measured on an MI355X (profiles/conv_train.txt).  k <= 3: two fragments share every X
// operand read (half the LDS traffic per MFMA; 84 / 204 registers, 50 KB of LDS: 3 / 2 workgroups per CU) and the slabs fill the
// 256 CUs once.  k >= 5: one fragment (two would leave one workgroup per CU with nothing to overlap its staging: 13.5 ms instead
// of 9.8 ms on 7x7 256 -> 256 at 8 x 256^2) and about 1024 workgroups (11.8 ms with the 448 that fill the CUs once).
constexpr int CT_CUS = 256, CT_GROUPS = 1024;
constexpr int ct_mt(int k) { return k <= 3 ? 2 : 1; }
constexpr int ct_resident(int k) { return k == 3 ? 2 : 3; }
inline int ct_tiles_co(int cout, int k) { return (cout + 64 * ct_mt(k) - 1) / (64 * ct_mt(k)); }
inline int ct_slabs_wanted(int cin, int cout, int k) {
    const int per_slab = ct_tiles_co(cout, k) * ((cin + 63) / 64) * k;
    const int want = k <= 3 ? CT_CUS * ct_resident(k) / per_slab : (CT_GROUPS + per_slab - 1) / per_slab;
    return want < 1 ? 1 : want;
}

}  // namespace
