// What the trainable convs on the padded 4-channel image share: the weight pack, the kernel that adds the slabs' partial sums, the
// dY staging of the slab kernels, the argument checks and the host path around a unit's own kernels.  Two units include it and
// differ in their Geometry, their forward kernel and their slab kernel: csrc/stem_train.hip (7x7, stride 2) and
// csrc/image_conv_train.hip (3x3, stride 1).  The padded input is bf16 [N][H + PAD_ROWS][W + PAD_COLS][4], in which the K taps of a
// filter row are contiguous; a weight record is [K][Cout][REC] with REC = 4 * (taps rounded up to a power of two); the partial sums of
// a slab are workspace[slab][K][Cout][REC] fp32, the slabs' bias sums behind them.  The partition is csrc/wgrad_slabs.h, the bias
// kernels are csrc/wgrad_bias.h.  Device code with internal linkage: every unit that includes this header gets its own copy.
//
// A Geometry names
//   static constexpr int K, STRIDE                         filter rows (= columns), stride; the padding is K / 2
//   static constexpr int PAD_ROWS, PAD_COLS                rows and columns the padded input has more than the image
//   static constexpr int REC                               values per weight record: 32 | 16
//   static constexpr int COUTS[]                           the output channel counts its kernels are built for, ascending
//   static constexpr int SLABS                             slabs of the auto partition
//   static constexpr const char *X                         what its header section calls the padded input (in messages)
// A unit's extern "C" functions are one call each of it_pack, it_forward, it_wgrad_workspace_bytes, it_wgrad_info and it_wgrad; the
// two launches take a callable that launches the unit's own kernel for an accepted call.
#pragma once
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cpn_hip.h"  // the error codes
#include "cpn_error.h"
#include "mfma_frag.h"
#include "wgrad_bias.h"  // ct_launch_bias, ct_bf16_rne, the dtype codes
#include "wgrad_slabs.h"

namespace {

typedef u32x4 __attribute__((aligned(8))) u32x4_a8;  // a pixel of the padded input starts at a multiple of 8 bytes (odd W)

constexpr int IT_CH = 128;  // pixels per staged chunk (8 MFMA steps)
constexpr int IT_ROW = 64;  // bytes of an LDS row: 32 channels of dY, or 32 values (kx, c) of one pixel

template <class G>
constexpr int it_out(int size) { return (size - 1) / G::STRIDE + 1; }  // (padding K / 2)

// ---- weight pack: weight [Cout][C][K][K] (fp32 | bf16) -> [K][Cout][REC] bf16, zeros at kx >= K and c >= C ---------------------
template <int K, int REC>
__global__ __launch_bounds__(256) void it_pack_kernel(const void *__restrict__ w, int w_dtype, int Cout, int C, uint16_t *__restrict__ out) {
    constexpr int SHIFT = REC == 32 ? 5 : 4;
    static_assert(REC == 1 << SHIFT && 4 * K <= REC, "a record holds (kx, c) with four channels per tap");
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= K * Cout * REC) return;
    const int v = e & (REC - 1), co = (e >> SHIFT) % Cout, ky = (e >> SHIFT) / Cout;
    const int kx = v >> 2, c = v & 3;
    uint16_t r = 0;
    if (kx < K && c < C) {
        const int si = ((co * C + c) * K + ky) * K + kx;
        r = w_dtype == CT_BF16 ? ((const uint16_t *) w)[si] : ct_bf16_rne(((const float *) w)[si]);
    }
    out[e] = r;
}

// ---- workspace [slab][K][Cout][REC] -> dw [Cout][C][K][K]: the slabs in ascending order, one rounding; columns kx >= K and c >= C
// unread
template <int K, int REC>
__global__ __launch_bounds__(256) void it_wgrad_reduce_kernel(const float *__restrict__ ws, int slabs, int Cout, int C, void *dw,
                                                               int dw_dtype) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Cout * C * K * K) return;
    const int kx = e % K, ky = (e / K) % K, c = (e / (K * K)) % C, co = e / (K * K * C);
    const long per = (long) K * Cout * REC, at = ((long) ky * Cout + co) * REC + kx * 4 + c;
    float sum = ws[at];
#pragma unroll 16
    for (int s = 1; s < slabs; ++s) sum += ws[s * per + at];  // (the loads of 16 slabs in flight, the adds in order)
    if (dw_dtype == CT_BF16) ((uint16_t *) dw)[e] = ct_bf16_rne(sum);
    else ((float *) dw)[e] = sum;
}

// ---- the dY staging of a slab kernel of 256 threads: the rows of the chunk's IT_CH pixels from c0 go into LDS as [NF blocks][IT_CH
// rows] of IT_ROW bytes, 16 bytes = 8 channels per item, 4 NF items per pixel, IT_DY_ITEMS<NF> items per thread: item tid + 256 j is
// its j-th.  A kernel loads all its items into registers and stores them afterwards (or a chunk later).  A pixel behind the slab's end
// p1 reads the slab's last pixel and is zeroed in registers: no masks, no uninitialised LDS.
template <int NF>
constexpr int IT_DY_ITEMS = IT_CH * 4 * NF / 256;

template <int NF>
struct ItDyItem {
    int t, blk, q;  // chunk pixel, 32-channel block, quarter of the block
    __device__ __forceinline__ explicit ItDyItem(int i) : t(i / (4 * NF)), blk((i % (4 * NF)) >> 2), q(i & 3) {}
    __device__ __forceinline__ u32x4 load(const uint16_t *dy, int64_t c0, int64_t p1) const {
        const int64_t p = c0 + t;
        u32x4 v = *(const u32x4 *) (dy + (p < p1 ? p : p1 - 1) * (NF * 32) + blk * 32 + q * 8);
        if (p >= p1) v = u32x4{0, 0, 0, 0};
        return v;
    }
    __device__ __forceinline__ void store(char *lds, u32x4 v) const { *(u32x4 *) (lds + (blk * IT_CH + t) * IT_ROW + q * 16) = v; }
};

// ---- argument checks (0, or the error code with "<who>: <sentence>" recorded) ---------------------------------------------------
int it_fail(int code, const char *who, const char *format, ...) {
    static thread_local char msg[200];
    const int n = snprintf(msg, sizeof msg, "%s: ", who);
    va_list args;
    va_start(args, format);
    vsnprintf(msg + n, sizeof msg - n, format, args);
    va_end(args);
    return cpn::fail(code, msg);
}

template <class G>
int it_check_cout(const char *who, int cout) {
    constexpr int M = sizeof G::COUTS / sizeof *G::COUTS;
    char list[64];
    int n = 0;
    for (int i = 0; i < M; ++i) {
        if (G::COUTS[i] == cout) return 0;
        n += snprintf(list + n, sizeof list - n, "%s%d", i == 0 ? "" : i == M - 1 ? " or " : ", ", G::COUTS[i]);
    }
    return it_fail(CPN_E_INVALID, who, "cout must be %s", list);
}

// the geometry of a call, the 2^31 - 1 limits on the padded input and, where asked for, the partition of the output rows
template <class G>
int it_check(const char *who, int N, int H, int W, int cout, int slab_rows, WgSlabs *part) {
    if (N < 1 || H < 1 || W < 1) return it_fail(CPN_E_INVALID, who, "N, H and W must be at least 1");
    if (const int rc = it_check_cout<G>(who, cout)) return rc;
    if (slab_rows < 0) return it_fail(CPN_E_INVALID, who, "slab_rows must be 0 (auto) or positive");
    if ((int64_t) N * (H + G::PAD_ROWS) > 0x7fffffffll || (int64_t) N * (H + G::PAD_ROWS) * (W + G::PAD_COLS) > 0x7fffffffll)
        return it_fail(CPN_E_UNSUPPORTED, who, "more than 2^31 - 1 pixels in the padded input");
    if (part) *part = wgs_partition((int64_t) N * it_out<G>(H), it_out<G>(W), slab_rows, G::SLABS);
    return 0;
}

int it_check_cin(const char *who, int cin) { return cin < 1 || cin > 4 ? it_fail(CPN_E_INVALID, who, "cin must lie in 1 ... 4") : 0; }

// ---- the host path ----------------------------------------------------------------------------------------------------------------
template <class G>
int it_pack(const char *who, const void *weight, int weight_dtype, int cout, int cin, void *packed, void *stream) {
    if (const int rc = it_check_cout<G>(who, cout)) return rc;
    if (const int rc = it_check_cin(who, cin)) return rc;
    if (weight_dtype != CT_F32 && weight_dtype != CT_BF16) return it_fail(CPN_E_INVALID, who, "weight_dtype must be 0 (fp32) or 1 (bf16)");
    if (!weight || !packed) return it_fail(CPN_E_INVALID, who, "null pointer");
    hipLaunchKernelGGL((it_pack_kernel<G::K, G::REC>), dim3((unsigned) ((G::K * cout * G::REC + 255) / 256)), dim3(256), 0,
                       (hipStream_t) stream, weight, weight_dtype, cout, cin, (uint16_t *) packed);
    return cpn::check_hip(hipGetLastError(), who);
}

// launch(xp, packed, bias, y, N, H, W, cout, stream): the unit's forward kernel
template <class G, class Launch>
int it_forward(const char *who, const void *xp, const void *packed, const float *bias, int N, int H, int W, int cout, void *y,
               void *stream, const Launch &launch) {
    if (const int rc = it_check<G>(who, N, H, W, cout, 0, nullptr)) return rc;
    if (!xp || !packed || !y) return it_fail(CPN_E_INVALID, who, "null pointer");
    if (((uintptr_t) xp | (uintptr_t) packed | (uintptr_t) y) & 15)
        return it_fail(CPN_E_INVALID, who, "%s, packed and y must start at 16-byte aligned addresses", G::X);
    launch((const unsigned char *) xp, (const unsigned char *) packed, bias, (unsigned char *) y, N, H, W, cout, (hipStream_t) stream);
    return cpn::check_hip(hipGetLastError(), who);
}

template <class G>
constexpr int64_t it_slab_floats(int cout) { return (int64_t) G::K * cout * G::REC; }  // partial sums of dW per slab

template <class G>
int64_t it_wgrad_workspace_bytes(const char *who, int N, int H, int W, int cout, int slab_rows) {
    WgSlabs part;
    if (it_check<G>(who, N, H, W, cout, slab_rows, &part)) return 0;
    return (int64_t) part.slabs * (it_slab_floats<G>(cout) + cout) * 4;
}

template <class G>
int it_wgrad_info(const char *who, int N, int H, int W, int cout, int slab_rows, int32_t info[5]) {
    WgSlabs part;
    if (const int rc = it_check<G>(who, N, H, W, cout, slab_rows, &part)) return rc;
    if (!info) return it_fail(CPN_E_INVALID, who, "null pointer");
    wgs_info(part, info);
    return 0;
}

// launch_slabs(part, dy, xp, ws, H, W, cout, stream): the unit's slab kernel.  dW (slab kernel, then the reduce) and db (bias slab,
// bias reduce), whichever is asked for, on one stream
template <class G, class Launch>
int it_wgrad(const char *who, const void *xp, const void *dy, int N, int H, int W, int cin, int cout, int slab_rows, void *dw,
             int dw_dtype, void *db, int db_dtype, void *workspace, int64_t workspace_bytes, void *stream, const Launch &launch_slabs) {
    WgSlabs part;
    if (const int rc = it_check<G>(who, N, H, W, cout, slab_rows, &part)) return rc;
    if (const int rc = it_check_cin(who, cin)) return rc;
    if (!xp || !dy || !workspace || (!dw && !db)) return it_fail(CPN_E_INVALID, who, "null pointer");
    if (((uintptr_t) xp | (uintptr_t) dy | (uintptr_t) workspace) & 15)
        return it_fail(CPN_E_INVALID, who, "%s, dy and workspace must start at 16-byte aligned addresses", G::X);
    if ((dw && dw_dtype != CT_F32 && dw_dtype != CT_BF16) || (db && db_dtype != CT_F32 && db_dtype != CT_BF16))
        return it_fail(CPN_E_INVALID, who, "an output dtype must be 0 (fp32) or 1 (bf16)");
    const int64_t per = it_slab_floats<G>(cout);
    if (workspace_bytes < (int64_t) part.slabs * (per + cout) * 4)
        return it_fail(CPN_E_WORKSPACE, who, "workspace smaller than %s_workspace_bytes", who);
    hipStream_t st = (hipStream_t) stream;
    float *ws = (float *) workspace;
    if (dw) {
        launch_slabs(part, (const uint16_t *) dy, (const unsigned char *) xp, ws, H, W, cout, st);
        hipLaunchKernelGGL((it_wgrad_reduce_kernel<G::K, G::REC>), dim3((unsigned) ((cout * cin * G::K * G::K + 255) / 256)), dim3(256), 0,
                           st, ws, part.slabs, cout, cin, dw, dw_dtype);
    }
    if (db) ct_launch_bias(part, dy, ws + (int64_t) part.slabs * per, cout, db, db_dtype, st);
    return cpn::check_hip(hipGetLastError(), who);
}

}  // namespace
