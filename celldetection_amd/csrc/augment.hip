// Training augmentation on the GPU (gfx950): the kernel behind celldetection_amd.augment.warp.  One launch warps a batch of
// channels-last images and their [H, W, C] label stacks together, every sample by its own affine map: bilinear interpolation with
// the intensity transform folded in for the image, nearest sampling in integers for the labels.  The rule is the "Augmentation
// warp" section of include/cpn_hip.h; the index and weight arithmetic is csrc/warp_rule.h.  This unit is compiled with
// -ffp-contract=off: the fp64 position and the fp32 blend have one stated order of operations.
//
//   au_warp_kernel: a workgroup of 256 lanes owns one AU_TILE x AU_TILE tile of one sample's output.  Lane l takes row l / 8 of
//                   the tile and the AU_VEC = 4 consecutive columns from 4 * (l % 8): it computes the four positions once, blends
//                   the K channels of each and writes every image plane with one 16-byte store (8 bytes for bf16; element by
//                   element where the width or the address does not allow it).  The source pixel of the label of each position
//                   goes to an LDS table of the tile (-1: the fill); after a barrier the workgroup copies the tile's labels with
//                   one lane per (pixel, channel) in output order, so that consecutive lanes write consecutive words and read
//                   the C consecutive words of a source pixel.  The uint8 tables of the sample (K x 256 fp32) sit in LDS.
// No atomics, no reductions: every output element is written exactly once and the result is bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "warp_rule.h"

namespace {

constexpr int AU_TILE = CPN_AUGMENT_TILE, AU_VEC = 4, AU_MAX_K = 4;
static_assert(AU_TILE == 32 && AU_TILE * (AU_TILE / AU_VEC) == 256, "one lane per four columns of a tile row");
static_assert(WR_CONSTANT == CPN_AUGMENT_BORDER_CONSTANT && WR_REFLECT == CPN_AUGMENT_BORDER_REFLECT, "border codes");

typedef float au_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t au_u32x2 __attribute__((ext_vector_type(2)));

// the K mapped values of source pixel `pix` of the sample (pix < 0: the fill)
template <bool U8>
__device__ __forceinline__ void au_tap(const void *img, int pix, int K, bool word, const float *tab, const float (&scale)[AU_MAX_K],
                                       const float (&offset)[AU_MAX_K], float fill, float (&t)[AU_MAX_K]) {
    if (pix < 0) {
#pragma unroll
        for (int k = 0; k < AU_MAX_K; ++k) t[k] = fill;
        return;
    }
    if (U8) {
        const uint8_t *p = (const uint8_t *) img;
        if (word) {  // K = 4 and a 4-byte aligned sample: the pixel is one word
            const uint32_t v = *(const uint32_t *) (p + (int64_t) pix * 4);
#pragma unroll
            for (int k = 0; k < AU_MAX_K; ++k) t[k] = tab[k * 256 + ((v >> (8 * k)) & 255u)];
        } else {
#pragma unroll
            for (int k = 0; k < AU_MAX_K; ++k) t[k] = k < K ? tab[k * 256 + p[(int64_t) pix * K + k]] : 0.f;
        }
    } else {
        const float *p = (const float *) img + (int64_t) pix * K;
#pragma unroll
        for (int k = 0; k < AU_MAX_K; ++k) t[k] = k < K ? p[k] * scale[k] + offset[k] : 0.f;  // (product and sum each rounded)
    }
}

template <bool U8, bool BF16>
__global__ __launch_bounds__(256) void au_warp_kernel(const void *__restrict__ image, const int32_t *__restrict__ labels, int H, int W,
                                                       int K, int C, const double *__restrict__ maps, const float *__restrict__ tables,
                                                       int border, float image_fill, int label_fill, void *__restrict__ image_out,
                                                       int32_t *__restrict__ labels_out, int h, int w, int vector_ok) {
    __shared__ float tab[AU_MAX_K * 256];
    __shared__ int32_t src[AU_TILE * AU_TILE];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int x0 = blockIdx.x * AU_TILE, y0 = blockIdx.y * AU_TILE;
    const int ry = tid >> 3, rx = (tid & 7) * AU_VEC;
    const int y = y0 + ry, x = x0 + rx;
    const int64_t in_pixels = (int64_t) H * W, out_pixels = (int64_t) h * w;

    double m[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) m[q] = maps[(int64_t) b * 6 + q];
    float scale[AU_MAX_K] = {1.f, 1.f, 1.f, 1.f}, offset[AU_MAX_K] = {0.f, 0.f, 0.f, 0.f};
    if (image) {
        if (U8) {
            for (int q = tid; q < K * 256; q += 256) tab[q] = tables[(int64_t) b * K * 256 + q];
            __syncthreads();
        } else {
#pragma unroll
            for (int k = 0; k < AU_MAX_K; ++k)
                if (k < K) scale[k] = tables[((int64_t) b * K + k) * 2], offset[k] = tables[((int64_t) b * K + k) * 2 + 1];
        }
    }

    const void *img = nullptr;
    bool word = false;
    if (image) {
        img = (const char *) image + (int64_t) b * in_pixels * K * (U8 ? 1 : 4);
        word = U8 && K == 4 && ((uintptr_t) img & 3) == 0;
    }
    float val[AU_MAX_K][AU_VEC];
#pragma unroll
    for (int e = 0; e < AU_VEC; ++e) {
        int nearest = -1;
#pragma unroll
        for (int k = 0; k < AU_MAX_K; ++k) val[k][e] = 0.f;
        if (y < h && x + e < w) {
            double sx, sy;
            wr_position(m, y, x + e, &sx, &sy);
            if (labels) {
                const int nx = wr_index(wr_nearest(sx), W, border), ny = wr_index(wr_nearest(sy), H, border);
                nearest = nx >= 0 && ny >= 0 ? ny * W + nx : -1;
            }
            if (image) {
                float lx, ly;
                const double fx = wr_floor(sx, &lx), fy = wr_floor(sy, &ly);
                const int ix0 = wr_index(fx, W, border), ix1 = wr_index(fx + 1.0, W, border);
                const int iy0 = wr_index(fy, H, border), iy1 = wr_index(fy + 1.0, H, border);
                if ((iy0 < 0 && iy1 < 0) || (ix0 < 0 && ix1 < 0)) {  // all four taps outside: the fill itself, no blend
#pragma unroll
                    for (int k = 0; k < AU_MAX_K; ++k) val[k][e] = image_fill;
                    src[ry * AU_TILE + rx + e] = nearest;
                    continue;
                }
                float t00[AU_MAX_K], t01[AU_MAX_K], t10[AU_MAX_K], t11[AU_MAX_K];
                au_tap<U8>(img, iy0 >= 0 && ix0 >= 0 ? iy0 * W + ix0 : -1, K, word, tab, scale, offset, image_fill, t00);
                au_tap<U8>(img, iy0 >= 0 && ix1 >= 0 ? iy0 * W + ix1 : -1, K, word, tab, scale, offset, image_fill, t01);
                au_tap<U8>(img, iy1 >= 0 && ix0 >= 0 ? iy1 * W + ix0 : -1, K, word, tab, scale, offset, image_fill, t10);
                au_tap<U8>(img, iy1 >= 0 && ix1 >= 0 ? iy1 * W + ix1 : -1, K, word, tab, scale, offset, image_fill, t11);
#pragma unroll
                for (int k = 0; k < AU_MAX_K; ++k) val[k][e] = wr_blend(t00[k], t01[k], t10[k], t11[k], ly, lx);
            }
        }
        src[ry * AU_TILE + rx + e] = nearest;
    }

    if (image && y < h && x < w) {
        const bool whole = vector_ok && x + AU_VEC <= w;
#pragma unroll
        for (int k = 0; k < AU_MAX_K; ++k) {
            if (k >= K) break;
            const int64_t o = (((int64_t) b * K + k) * h + y) * (int64_t) w + x;
            if (BF16) {
                uint16_t *dst = (uint16_t *) image_out + o;
                if (whole) {
                    *(au_u32x2 *) dst = au_u32x2{(uint32_t) wr_bf16(val[k][0]) | ((uint32_t) wr_bf16(val[k][1]) << 16),
                                                 (uint32_t) wr_bf16(val[k][2]) | ((uint32_t) wr_bf16(val[k][3]) << 16)};
                } else {
#pragma unroll
                    for (int e = 0; e < AU_VEC; ++e)
                        if (x + e < w) dst[e] = wr_bf16(val[k][e]);
                }
            } else {
                float *dst = (float *) image_out + o;
                if (whole) {
                    *(au_f32x4 *) dst = au_f32x4{val[k][0], val[k][1], val[k][2], val[k][3]};
                } else {
#pragma unroll
                    for (int e = 0; e < AU_VEC; ++e)
                        if (x + e < w) dst[e] = val[k][e];
                }
            }
        }
    }

    if (!labels) return;  // (the same in every lane)
    __syncthreads();
    const unsigned tw = (unsigned) min(AU_TILE, w - x0), th = (unsigned) min(AU_TILE, h - y0);
    const unsigned row_items = tw * (unsigned) C, items = th * row_items;  // <= 1024 * 65535
    const int32_t *lab = labels + (int64_t) b * in_pixels * C;
    int32_t *out = labels_out + (int64_t) b * out_pixels * C;
    for (unsigned q = tid; q < items; q += 256) {
        const unsigned r = q / row_items, rem = q - r * row_items;
        const unsigned px = rem / (unsigned) C, c = rem - px * (unsigned) C;
        const int s = src[r * AU_TILE + px];
        out[((int64_t) (y0 + (int) r) * w + x0) * C + rem] = s < 0 ? label_fill : lab[(int64_t) s * C + c];
    }
}

}  // namespace

extern "C" {

int cpn_augment_warp(const void *image, int32_t image_dtype, const int32_t *labels, int64_t B, int64_t H, int64_t W, int32_t K,
                     int32_t C, const double *maps, const float *tables, int32_t border, float image_fill, int32_t label_fill,
                     void *image_out, int32_t out_dtype, int32_t *labels_out, int64_t h, int64_t w, void *stream) {
    if (!image && !labels) return cpn::fail(CPN_E_INVALID, "cpn_augment_warp: image and labels are both null");
    if (B < 1 || H < 1 || W < 1 || h < 1 || w < 1) return cpn::fail(CPN_E_INVALID, "cpn_augment_warp: a size below 1");
    if (H > 0x7fffffff || W > 0x7fffffff || h > 0x7fffffff || w > 0x7fffffff || H * W > 0x7fffffff || h * w > 0x7fffffff)
        return cpn::fail(CPN_E_UNSUPPORTED, "cpn_augment_warp: more than 2^31 - 1 pixels in a source or a destination");
    const int64_t tiles_x = (w + AU_TILE - 1) / AU_TILE, tiles_y = (h + AU_TILE - 1) / AU_TILE;
    if (B > 65535 || tiles_y > 65535) return cpn::fail(CPN_E_UNSUPPORTED, "cpn_augment_warp: more than 65535 samples or tile rows");
    if (border != CPN_AUGMENT_BORDER_CONSTANT && border != CPN_AUGMENT_BORDER_REFLECT)
        return cpn::fail(CPN_E_INVALID, "cpn_augment_warp: unknown border code");
    if (!maps || ((uintptr_t) maps & 7)) return cpn::fail(CPN_E_INVALID, "cpn_augment_warp: maps is null or not 8-byte aligned");
    int vector_ok = 0;
    if (image) {
        if (image_dtype != CPN_AUGMENT_IMAGE_U8 && image_dtype != CPN_AUGMENT_IMAGE_F32)
            return cpn::fail(CPN_E_INVALID, "cpn_augment_warp: unknown image dtype code");
        if (out_dtype != 0 && out_dtype != 1) return cpn::fail(CPN_E_INVALID, "cpn_augment_warp: unknown output dtype code");
        if (K < 1 || K > AU_MAX_K) return cpn::fail(CPN_E_INVALID, "cpn_augment_warp: K outside 1 ... 4");
        if (!(fabsf(image_fill) <= 3.402823466e38f)) return cpn::fail(CPN_E_INVALID, "cpn_augment_warp: image_fill is not finite");
        if (!tables || ((uintptr_t) tables & 3) || !image_out || ((uintptr_t) image_out & (out_dtype ? 1 : 3)) ||
            (image_dtype == CPN_AUGMENT_IMAGE_F32 && ((uintptr_t) image & 3)))
            return cpn::fail(CPN_E_INVALID, "cpn_augment_warp: tables or image_out is null, or a pointer is not aligned to its element");
        vector_ok = w % AU_VEC == 0 && ((uintptr_t) image_out & (out_dtype ? 7 : 15)) == 0;
    }
    if (labels) {
        if (C < 1 || C > CPN_AUGMENT_MAX_CHANNELS) return cpn::fail(CPN_E_INVALID, "cpn_augment_warp: C outside 1 ... 65535");
        if (!labels_out || ((uintptr_t) labels & 3) || ((uintptr_t) labels_out & 3))
            return cpn::fail(CPN_E_INVALID, "cpn_augment_warp: labels_out is null, or a label pointer is not 4-byte aligned");
    }
    const dim3 grid((unsigned) tiles_x, (unsigned) tiles_y, (unsigned) B);
    hipStream_t st = (hipStream_t) stream;
#define AU_LAUNCH(U8, BF16)                                                                                                       \
    hipLaunchKernelGGL((au_warp_kernel<U8, BF16>), grid, dim3(256), 0, st, image, labels, (int) H, (int) W, K, C, maps, tables, border, \
                       image_fill, label_fill, image_out, labels_out, (int) h, (int) w, vector_ok)
    const bool u8 = !image || image_dtype == CPN_AUGMENT_IMAGE_U8, bf16 = image && out_dtype == 1;
    if (u8 && bf16) AU_LAUNCH(true, true);
    else if (u8) AU_LAUNCH(true, false);
    else if (bf16) AU_LAUNCH(false, true);
    else AU_LAUNCH(false, false);
#undef AU_LAUNCH
    return cpn::check_hip(hipGetLastError(), "cpn_augment_warp");
}

}  // extern "C"
