// Trainable convolution on the GPU (gfx950): the kernels behind celldetection_amd.nn.conv2d that csrc/conv_igemm.hip does not
// already provide.  The rule is the "Trainable convolution" section of include/cpn_hip.h.
//
// Forward and input gradient are calls of cpn_conv2d; what they need per step is the weight tensor in that kernel's record layout:
//   ct_pack_kernel:        [Cout][Cin][k][k] fp32 | bf16 -> [item][out channel][32] bf16, forward (item = (chunk of Cin, tap)) or
//                          dgrad (item = (chunk of Cout, tap), tap flipped, channel roles swapped); one zero item behind an odd count.
// The weight gradient is csrc/wgrad_dense.h (ct_wgrad_slab_kernel, ct_wgrad_reduce_kernel, the host path around them) with the
// plainest Source (CtDense, defined there): a staged X row is the row of x as it lies.  The bias gradient is csrc/wgrad_bias.h.  No
// floating-point atomics: results are bit-identical from run to run.  The partition is csrc/wgrad_slabs.h.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "wgrad_dense.h"  // the dense weight gradient: slab kernel, reduce kernel, check, workspace, launches
#include "wgrad_slabs.h"

namespace {

__global__ __launch_bounds__(256) void ct_pack_kernel(const void *w, int w_dtype, int Cout, int Cin, int K, int dgrad,
                                                       uint16_t *packed, long total) {
    const long o = (long) blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int CO = dgrad ? Cin : Cout, CR = dgrad ? Cout : Cin, KK = K * K;
    const int c = (int) (o & 31), oc = (int) ((o >> 5) % CO), item = (int) ((o >> 5) / CO);
    uint16_t v = 0;
    if (item < CR / 32 * KK) {  // (the item behind an odd count is zeros)
        const int rc = item / KK * 32 + c, tap = item % KK;
        int ky = tap / K, kx = tap % K;
        long idx;
        if (dgrad) {
            ky = K - 1 - ky;
            kx = K - 1 - kx;
            idx = (((long) rc * Cin + oc) * K + ky) * K + kx;
        } else {
            idx = (((long) oc * Cin + rc) * K + ky) * K + kx;
        }
        v = w_dtype == CT_BF16 ? ((const uint16_t *) w)[idx] : ct_bf16_rne(((const float *) w)[idx]);
    }
    packed[o] = v;
}

// 0, or the error code with its message recorded; the partition of an accepted call
int ct_check(const char *who, int N, int H, int W, int cin, int cout, int k, int slab_rows, WgSlabs *part) {
    static thread_local char msg[160];
    const char *bad = nullptr;
    if (N < 1 || H < 1 || W < 1) bad = "N, H and W must be at least 1";
    else if (cin < 32 || cin % 32 || cout < 32 || cout % 32) bad = "cin and cout must be positive multiples of 32";
    else if (k != 1 && k != 3 && k != 5 && k != 7) bad = "k must be 1, 3, 5 or 7";
    else if (slab_rows < 0) bad = "slab_rows must be 0 (auto) or positive";
    if (bad) {
        snprintf(msg, sizeof msg, "%s: %s", who, bad);
        return cpn::fail(CPN_E_INVALID, msg);
    }
    return ct_check_partition(who, N, H, W, cin, cout, k, slab_rows, part);
}

}  // namespace

extern "C" {

int cpn_conv_train_pack(const void *w, int32_t w_dtype, int32_t cout, int32_t cin, int32_t k, int32_t mode, void *packed,
                        void *stream) {
    if (const int rc = ct_check("cpn_conv_train_pack", 1, 1, 1, cin, cout, k, 0, nullptr)) return rc;
    if (!w || !packed) return cpn::fail(CPN_E_INVALID, "cpn_conv_train_pack: null pointer");
    if (w_dtype != CT_F32 && w_dtype != CT_BF16) return cpn::fail(CPN_E_INVALID, "cpn_conv_train_pack: w_dtype must be 0 (fp32) or 1 (bf16)");
    if (mode != CPN_CONV_PACK_FORWARD && mode != CPN_CONV_PACK_DGRAD)
        return cpn::fail(CPN_E_INVALID, "cpn_conv_train_pack: mode must be CPN_CONV_PACK_FORWARD or CPN_CONV_PACK_DGRAD");
    const int reduced = mode == CPN_CONV_PACK_DGRAD ? cout : cin, outc = mode == CPN_CONV_PACK_DGRAD ? cin : cout;
    const long items = (long) reduced / 32 * k * k, total = (items + (items & 1)) * outc * 32;
    hipLaunchKernelGGL(ct_pack_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, (hipStream_t) stream, w, w_dtype, cout,
                       cin, k, mode == CPN_CONV_PACK_DGRAD ? 1 : 0, (uint16_t *) packed, total);
    return cpn::check_hip(hipGetLastError(), "cpn_conv_train_pack");
}

int64_t cpn_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t k, int32_t slab_rows) {
    WgSlabs part;
    if (ct_check("cpn_conv_wgrad_workspace_bytes", N, H, W, cin, cout, k, slab_rows, &part)) return 0;
    return ct_workspace_bytes(part.slabs, cin, cout, k);
}

int cpn_conv_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t k, int32_t slab_rows, int32_t info[5]) {
    WgSlabs part;
    if (const int rc = ct_check("cpn_conv_wgrad_info", N, H, W, cin, cout, k, slab_rows, &part)) return rc;
    if (!info) return cpn::fail(CPN_E_INVALID, "cpn_conv_wgrad_info: null pointer");
    wgs_info(part, info);
    return 0;
}

int cpn_conv_wgrad(const void *x, const void *dy, int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t k,
                   int32_t slab_rows, void *dw, int32_t dw_dtype, void *db, int32_t db_dtype, void *workspace,
                   int64_t workspace_bytes, void *stream) {
    WgSlabs part;
    if (const int rc = ct_check("cpn_conv_wgrad", N, H, W, cin, cout, k, slab_rows, &part)) return rc;
    if (!x || !dy || !workspace || (!dw && !db)) return cpn::fail(CPN_E_INVALID, "cpn_conv_wgrad: null pointer");
    if ((dw && dw_dtype != CT_F32 && dw_dtype != CT_BF16) || (db && db_dtype != CT_F32 && db_dtype != CT_BF16))
        return cpn::fail(CPN_E_INVALID, "cpn_conv_wgrad: an output dtype must be 0 (fp32) or 1 (bf16)");
    if (workspace_bytes < ct_workspace_bytes(part.slabs, cin, cout, k))
        return cpn::fail(CPN_E_WORKSPACE, "cpn_conv_wgrad: workspace smaller than cpn_conv_wgrad_workspace_bytes");
    ct_launch_wgrad(part, dy, CtDense{(const uint16_t *) x, cin}, H, cin, cout, k, dw, dw_dtype, db, db_dtype, workspace,
                    (hipStream_t) stream);
    return cpn::check_hip(hipGetLastError(), "cpn_conv_wgrad");
}

}  // extern "C"
