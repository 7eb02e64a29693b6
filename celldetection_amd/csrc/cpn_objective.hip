// CPN training objective for gfx950 (wave64): the loss terms of the reference's CPN.forward(inputs, targets) in training mode
// (celldetection/models/cpn.py:441-692) and the gradients of the four head maps, computed in the forward call.
// The rule is stated in include/cpn_hip.h, section "Training objective".
//
// Compiled with -ffp-contract=off.  Everything that feeds a discontinuity (decode, scaling, round / clamp / gather / add,
// minimum and maximum, the >= 1 box filter, the differences of the L1 terms) is float32 in the reference's order and shares its
// device functions with decode_nms.hip (decode_device.h).  Loss elements of the score and iou terms, every sum and every
// gradient are float64; sums run in an order that depends on the shapes alone.  No floating-point atomics anywhere:
// the one scatter (gradient of the refinement map) is a list of contributions, sorted by target element with a stable radix
// sort and summed in an order that the sorted list fixes.
//
// Passes:  head   label pooling, class of every head pixel, counts            (obj_head_kernel, then cpn_compact)
//          score  BCE / CE element, its gradient, block sums                   (obj_score_kernel)
//          -- the host reads P and the checks --
//          values one wave per proposal: decode, refinement, L1 sums, box, iou (obj_proposal_kernel<false>)
//          reduce column sums -> the eight terms, the loss, the iou count      (obj_reduce_kernel)
//          grads  one wave per proposal: the same walk, gradients              (obj_proposal_kernel<true>)
//          sort + sum of the refinement contributions                          (rocprim, obj_segment_pieces / _sum_kernel)
#include <cstdio>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <stdint.h>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "decode_device.h"

namespace {

using cpn_dec::Buckets;
using cpn_dec::refine_step;
using cpn_dec::synth;

constexpr int WAVE = 64;
constexpr int PWAVES = 4;            // proposals per block
constexpr int MAX_COEF = 256;        // order * 4 <= 256
constexpr int HBLK = 256;            // head pixels per block
constexpr int RBLK = 1024;           // threads of the reduction
constexpr int FIXED_COLS = 5;        // columns of the per-proposal sums before the refinement iterations
constexpr int COL_FOURIER = 0, COL_LOCATION = 1, COL_CONTOUR = 2, COL_IOU = 3, COL_VALID = 4;
constexpr int META_BG = 0, META_FLAGS = 1;  // words of meta after the N + 1 compaction counts (P = counts[N])

struct Dev {  // what the kernels read of CpnObjectiveArgs, plus the buffers of this call
    CpnObjectiveArgs a;
    const int32_t *indices;   // [P] linear head pixel of proposal p
    const int32_t *headlab;   // [N][h][w] pooled labels
    int32_t P;
    double c_fourier, c_location, c_contour, c_refine;  // weight / element count of the L1 terms
    double *sums;             // [cols][P]: column c of proposal p at c * P + p
    double *reduced;          // [cols + 2]: column sums, then score fg / bg sums
    uint32_t *keys;           // [E] pair plane element (b * buckets + bucket) * H * W + pixel
    uint32_t *perm;           // [E] slot numbers
    double2 *vals;            // [E] contribution to the x and y channel
    int cols, nk;
};

__device__ __forceinline__ long read_label(const void *labels, int is64, size_t i) {
    return is64 ? (long) ((const int64_t *) labels)[i] : (long) ((const int32_t *) labels)[i];
}

// torch's nearest interpolation index (upsample_nearest: floor(dst * float(in) / float(out)), at most in - 1)
__device__ __forceinline__ int nearest_index(int dst, int out, int in) {
    if (out == in) return dst;
    if (out == 2 * in) return dst >> 1;
    const float scale = (float) in / (float) out;
    const int i = (int) floorf(__fmul_rn((float) dst, scale));
    return i < in - 1 ? i : in - 1;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ float wave_minf(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}
// smallest value of the wave and the lowest sample index that holds it (torch: min / max over a dim send the gradient to the first)
__device__ __forceinline__ void wave_argmin(float &v, int &i) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_xor(v, d, 64);
        const int oi = __shfl_xor(i, d, 64);
        if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}
__device__ __forceinline__ double sign_of(double d) { return (double) ((d > 0.) - (d < 0.)); }

// ---------------------------------------------------------------------------------------------------------
// head pass
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HBLK) void obj_head_kernel(const void *__restrict__ labels, int is64, int N, int H, int W, int h,
                                                       int w, int K, int32_t *__restrict__ headlab,
                                                       float *__restrict__ fgmap, int32_t *__restrict__ meta) {
    const long total = (long) N * h * w;
    const long i = (long) blockIdx.x * HBLK + threadIdx.x;
    bool bg = false;
    int flags = 0;
    if (i < total) {
        const int b = (int) (i / ((long) h * w));
        const int rem = (int) (i - (long) b * h * w);
        const int hy = rem / w, hx = rem - hy * w;
        long L;
        const size_t base = (size_t) b * H * W;
        if (H == h && W == w) {
            L = read_label(labels, is64, base + (size_t) hy * W + hx);
        } else {  // downsample_labels, ops/commons.py:51-78
            const int kh = H / h, kw = W / w;
            const int ph = H / kh, pw = W / kw;
            const int py = nearest_index(hy, h, ph), px = nearest_index(hx, w, pw);
            L = read_label(labels, is64, base + (size_t) (py * kh) * W + (size_t) px * kw);
            for (int dy = 0; dy < kh; ++dy)
                for (int dx = 0; dx < kw; ++dx) {
                    const long v = read_label(labels, is64, base + (size_t) (py * kh + dy) * W + (size_t) px * kw + dx);
                    L = v > L ? v : L;
                }
        }
        if (L > (1l << 24)) flags |= CPN_OBJECTIVE_FLAG_LABEL_RANGE;
        if (L > K) flags |= CPN_OBJECTIVE_FLAG_LABEL_ROWS;
        bg = L == 0;
        headlab[i] = (int32_t) (L > K ? K : (L < -1 ? -1 : L));
        fgmap[i] = L > 0 ? 1.f : 0.f;
    }
    const unsigned long long m = __ballot(bg);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&meta[META_BG], __popcll(m));
    if (flags) atomicOr(&meta[META_FLAGS], flags);
}

// ---------------------------------------------------------------------------------------------------------
// score pass (cpn.py:508-523): element and gradient in float64 from the float32 logits
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HBLK) void obj_score_kernel(const float *__restrict__ scores, const int32_t *__restrict__ headlab,
                                                        const int32_t *__restrict__ classes, int N, int C, int hw, int K,
                                                        double w_fg, double w_bg, const int32_t *__restrict__ counts_total,
                                                        int32_t *__restrict__ meta, float *__restrict__ g_scores,
                                                        double *__restrict__ block_sums) {
    const long total = (long) N * hw;
    const long i = (long) blockIdx.x * HBLK + threadIdx.x;
    const int n_fg = counts_total[0], n_bg = meta[META_BG];
    double e_fg = 0., e_bg = 0.;
    if (i < total) {
        const int b = (int) (i / hw);
        const int pos = (int) (i - (long) b * hw);
        const int L = headlab[i];
        const float *z = scores + (size_t) b * C * hw + pos;
        float *g = g_scores ? g_scores + (size_t) b * C * hw + pos : nullptr;
        if (L < 0) {
            if (g)
                for (int c = 0; c < C; ++c) g[(size_t) c * hw] = 0.f;
        } else {
            const bool fg = L > 0;
            const double scale = fg ? w_fg / (double) n_fg : w_bg / (double) n_bg;
            double e;
            if (C == 1) {  // BCEWithLogitsLoss
                const double v = (double) z[0], t = fg ? 1. : 0.;
                e = fmax(v, 0.) - v * t + log1p(exp(-fabs(v)));
                const double sig = v >= 0. ? 1. / (1. + exp(-v)) : exp(v) / (1. + exp(v));
                if (g) g[0] = (float) ((sig - t) * scale);
            } else {  // CrossEntropyLoss against targets['classes'] (or 1) and 0
                int cls = 0;
                if (fg) {
                    cls = classes ? classes[(size_t) b * K + (L - 1)] : 1;
                    if (cls < 0 || cls >= C) {
                        atomicOr(&meta[META_FLAGS], CPN_OBJECTIVE_FLAG_CLASS_RANGE);
                        cls = 0;
                    }
                }
                double zm = (double) z[0];
                for (int c = 1; c < C; ++c) zm = fmax(zm, (double) z[(size_t) c * hw]);
                double se = 0.;
                for (int c = 0; c < C; ++c) se += exp((double) z[(size_t) c * hw] - zm);
                e = zm + log(se) - (double) z[(size_t) cls * hw];
                if (g)
                    for (int c = 0; c < C; ++c)
                        g[(size_t) c * hw] = (float) ((exp((double) z[(size_t) c * hw] - zm) / se - (c == cls ? 1. : 0.)) * scale);
            }
            if (fg) e_fg = e; else e_bg = e;
        }
    }
    // block sums in a fixed order: lanes by shuffles, waves in sequence
    __shared__ double ws[2][HBLK / WAVE];
    e_fg = wave_sum(e_fg);
    e_bg = wave_sum(e_bg);
    if ((threadIdx.x & 63) == 0) {
        ws[0][threadIdx.x >> 6] = e_fg;
        ws[1][threadIdx.x >> 6] = e_bg;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double s = 0.;
        for (int k = 0; k < HBLK / WAVE; ++k) s += ws[threadIdx.x][k];
        block_sums[(size_t) blockIdx.x * 2 + threadIdx.x] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------
// 1 - GIoU of a box and its target and the gradient by the box (ops/boxes.py:101-126, ops/loss.py:90-110), float64.  torch's
// rules: maximum / minimum of equal values split the gradient evenly, clamp(min=0) passes it on >= 0.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double part_larger(double u, double v) { return u == v ? .5 : (u > v ? 1. : 0.); }
__device__ __forceinline__ double part_smaller(double u, double v) { return u == v ? .5 : (u < v ? 1. : 0.); }

__device__ void giou_loss(const float *box, const float *tbox, double &loss, double *grad) {
    double A[4], T[4];
    for (int j = 0; j < 4; ++j) { A[j] = (double) box[j]; T[j] = (double) tbox[j]; }
    const double a1 = (A[2] - A[0]) * (A[3] - A[1]), a2 = (T[2] - T[0]) * (T[3] - T[1]);
    double wh[2], dm[2], whi[2], dim[2];
    for (int c = 0; c < 2; ++c) {
        const double d = fmin(A[2 + c], T[2 + c]) - fmax(A[c], T[c]);
        wh[c] = d > 0. ? d : 0.;
        dm[c] = d >= 0. ? 1. : 0.;
        const double di = fmax(A[2 + c], T[2 + c]) - fmin(A[c], T[c]);
        whi[c] = di > 0. ? di : 0.;
        dim[c] = di >= 0. ? 1. : 0.;
    }
    const double inter = wh[0] * wh[1], uni = a1 + a2 - inter, enc = whi[0] * whi[1];
    loss = 1. - (inter / uni - (enc - uni) / enc);
    const double d_union = -inter / (uni * uni) + 1. / enc, d_inter = 1. / uni - d_union, d_enc = -uni / (enc * enc);
    for (int c = 0; c < 2; ++c) {
        const int o = 1 - c;
        const double side = A[2 + o] - A[o];
        const double lo = d_inter * wh[o] * dm[c] * -part_larger(A[c], T[c]) + d_enc * whi[o] * dim[c] * -part_smaller(A[c], T[c]) +
                          d_union * -side;
        const double hi = d_inter * wh[o] * dm[c] * part_smaller(A[2 + c], T[2 + c]) +
                          d_enc * whi[o] * dim[c] * part_larger(A[2 + c], T[2 + c]) + d_union * side;
        grad[c] = -lo;
        grad[2 + c] = -hi;
    }
}

// ---------------------------------------------------------------------------------------------------------
// proposal pass: one wave per proposal.  GRAD = false: the sums of the L1 elements, the box and its iou element, the detail
// buffers.  GRAD = true: the same walk again, now writing the gradients (the iou term needs the count of valid boxes first).
// ---------------------------------------------------------------------------------------------------------
template <bool GRAD>
__global__ __launch_bounds__(PWAVES *WAVE) void obj_proposal_kernel(const Dev d) {
    const CpnObjectiveArgs &a = d.a;
    __shared__ float coef_s[PWAVES][MAX_COEF];
    __shared__ double acc_s[PWAVES][MAX_COEF + 2];  // GRAD: gradient of every coefficient, then of the location (x, y)
    __shared__ double gp_s[PWAVES][2][WAVE];        // GRAD: gradient of the contour points of one chunk of 64 samples
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * PWAVES + wave;
    if (p >= d.P) return;  // waves of a block share no data and meet at no barrier
    float *coef = coef_s[wave];
    double *acc = acc_s[wave];
    const int hw = a.h * a.w, S = a.samples, nc = a.order * 4;
    const int lin = d.indices[p];
    const int b = lin / hw;
    const int pos = lin - b * hw;
    const int y = pos / a.w, x = pos - y * a.w;
    int row = d.headlab[lin] - 1;
    row = row < 0 ? 0 : (row >= a.K ? a.K - 1 : row);  // the host has refused labels above K before this launch
    for (int i = lane; i < nc; i += 64) coef[i] = a.fourier[((size_t) b * a.order_total * 4 + i) * hw + pos];
    if (GRAD)
        for (int i = lane; i < nc + 2; i += 64) acc[i] = 0.;
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    const float lx = __fadd_rn(a.locations[((size_t) b * 2 + 0) * hw + pos], (float) x);  // rel_location2abs_location
    const float ly = __fadd_rn(a.locations[((size_t) b * 2 + 1) * hw + pos], (float) y);
    const float sx = (float) a.W / (float) a.w, sy = (float) a.H / (float) a.h;              // get_scale
    const float hix = (float) (a.W - 1), hiy = (float) (a.H - 1);
    const float *cos_b = a.cos_table + (size_t) b * a.order * S, *sin_b = a.sin_table + (size_t) b * a.order * S;
    const bool refine = a.refinement != nullptr && a.iterations > 0;
    const int B = a.buckets < 1 ? 1 : a.buckets;
    const float *ref_b = refine ? a.refinement + (size_t) b * 2 * B * a.H * a.W : nullptr;
    const Buckets bk{B, B > 1 ? a.bucket_index + (size_t) b * 3 * S : nullptr, B > 1 ? a.bucket_weight + (size_t) b * 3 * S : nullptr, S};
    const float *tc = a.t_contours + ((size_t) b * a.K + row) * S * 2;
    const int iters = refine ? a.iterations : 0;
    double *sums = d.sums + p;  // column c at sums[c * P]
    const size_t PS = (size_t) d.P;

    // ---- walk 1: proposals, refined sets, box with the sample that gives each side, target box
    float mn[2] = {__builtin_inff(), __builtin_inff()}, mx[2] = {-__builtin_inff(), -__builtin_inff()};
    int amn[2] = {0x7fffffff, 0x7fffffff}, amx[2] = {0x7fffffff, 0x7fffffff};
    float tmn[2] = {__builtin_inff(), __builtin_inff()}, tmx[2] = {-__builtin_inff(), -__builtin_inff()};
    for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        const bool on = s < S;
        double e_contour = 0.;
        float cx = 0.f, cy = 0.f, tx = 0.f, ty = 0.f;
        if (on) {
            tx = tc[s * 2];
            ty = tc[s * 2 + 1];
            cx = __fmul_rn(synth(coef, a.order, S, s, 1, 0, cos_b, sin_b, lx), sx);  // fouriers2contours, scale_contours
            cy = __fmul_rn(synth(coef, a.order, S, s, 3, 2, cos_b, sin_b, ly), sy);
            if (!refine) {  // the proposals themselves are clamped in place (cpn.py:659-663)
                cx = fminf(fmaxf(cx, 0.f), hix);
                cy = fminf(fmaxf(cy, 0.f), hiy);
            }
            if (!GRAD) {
                e_contour = (double) fabsf(__fsub_rn(cx, tx)) + (double) fabsf(__fsub_rn(cy, ty));
                if (a.detail_proposals) {
                    a.detail_proposals[((size_t) p * S + s) * 2] = cx;
                    a.detail_proposals[((size_t) p * S + s) * 2 + 1] = cy;
                }
            }
            tmn[0] = fminf(tmn[0], tx); tmn[1] = fminf(tmn[1], ty);
            tmx[0] = fmaxf(tmx[0], tx); tmx[1] = fmaxf(tmx[1], ty);
        }
        if (!GRAD) {
            e_contour = wave_sum(e_contour);
            if (lane == 0) sums[(COL_CONTOUR) * PS] = (base ? sums[(COL_CONTOUR) * PS] : 0.) + e_contour;
        }
        float fx = cx, fy = cy;  // the last set, clamped
        for (int it = 0; it < iters; ++it) {
            double e_ref = 0.;
            if (on) {
                refine_step(cx, cy, ref_b, a.H, a.W, bk, s);
                fx = fminf(fmaxf(cx, 0.f), hix);  // every refined set is clamped before its L1 term (cpn.py:661-663)
                fy = fminf(fmaxf(cy, 0.f), hiy);
                if (!GRAD) {
                    e_ref = (double) fabsf(__fsub_rn(fx, tx)) + (double) fabsf(__fsub_rn(fy, ty));
                    if (a.detail_refined) {
                        a.detail_refined[(((size_t) it * d.P + p) * S + s) * 2] = fx;
                        a.detail_refined[(((size_t) it * d.P + p) * S + s) * 2 + 1] = fy;
                    }
                }
            }
            if (!GRAD) {
                e_ref = wave_sum(e_ref);
                if (lane == 0) sums[(FIXED_COLS + it) * PS] = (base ? sums[(FIXED_COLS + it) * PS] : 0.) + e_ref;
            }
        }
        if (on) {  // ascending s within a lane: a strict comparison keeps the first
            if (fx < mn[0]) { mn[0] = fx; amn[0] = s; }
            if (fy < mn[1]) { mn[1] = fy; amn[1] = s; }
            if (fx > mx[0]) { mx[0] = fx; amx[0] = s; }
            if (fy > mx[1]) { mx[1] = fy; amx[1] = s; }
        }
    }
    float box[4], tbox[4];
    int arg[4];
    for (int c = 0; c < 2; ++c) {
        wave_argmin(mn[c], amn[c]);
        float neg = -mx[c];
        wave_argmin(neg, amx[c]);
        box[c] = mn[c]; box[2 + c] = -neg;
        arg[c] = amn[c]; arg[2 + c] = amx[c];
        tbox[c] = wave_minf(tmn[c]);
        tbox[2 + c] = wave_maxf(tmx[c]);
    }
    const bool valid = __fsub_rn(box[2], box[0]) >= 1.f && __fsub_rn(box[3], box[1]) >= 1.f;  // remove_small_boxes, fp32
    double e_iou = 0., g_box[4] = {0., 0., 0., 0.};
    if (valid) giou_loss(box, tbox, e_iou, g_box);

    if (!GRAD) {
        // ---- L1 elements of the fourier and location terms (scale_fourier after the decode, cpn.py:647)
        const float *tf = a.t_fourier + ((size_t) b * a.K + row) * nc;
        double e_f = 0.;
        for (int i = lane; i < nc; i += 64) {
            const float fs = __fmul_rn(coef[i], (i & 3) < 2 ? sx : sy);
            const float e = fabsf(__fsub_rn(fs, tf[i]));
            e_f += (double) (a.order_weights ? __fmul_rn(e, a.order_weights[i >> 2]) : e);
        }
        e_f = wave_sum(e_f);
        if (lane == 0) {
            const float *tl = a.t_locations + ((size_t) b * a.K + row) * 2;
            sums[(COL_FOURIER) * PS] = e_f;
            sums[(COL_LOCATION) * PS] = (double) fabsf(__fsub_rn(__fmul_rn(lx, sx), tl[0])) + (double) fabsf(__fsub_rn(__fmul_rn(ly, sy), tl[1]));
            sums[(COL_IOU) * PS] = valid ? e_iou : 0.;
            sums[(COL_VALID) * PS] = valid ? 1. : 0.;
            if (a.detail_boxes)
                for (int j = 0; j < 4; ++j) a.detail_boxes[(size_t) p * 4 + j] = box[j];
        }
        return;
    }

    // ---- walk 2: gradients.  The iou term is a mean over the valid boxes, counted by the reduction before this launch.
    const double n_valid = d.reduced[COL_VALID];
    const double c_iou = (valid && n_valid > 0.) ? a.w_iou / n_valid : 0.;
    const bool to_maps = a.g_fourier != nullptr || a.g_locations != nullptr;
    for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        const bool on = s < S;
        double gx = 0., gy = 0.;  // gradient of the proposal point
        if (on) {
            const float tx = tc[s * 2], ty = tc[s * 2 + 1];
            float cx = __fmul_rn(synth(coef, a.order, S, s, 1, 0, cos_b, sin_b, lx), sx);
            float cy = __fmul_rn(synth(coef, a.order, S, s, 3, 2, cos_b, sin_b, ly), sy);
            const double ibx = (s == arg[0] ? g_box[0] : 0.) + (s == arg[2] ? g_box[2] : 0.);
            const double iby = (s == arg[1] ? g_box[1] : 0.) + (s == arg[3] ? g_box[3] : 0.);
            if (!refine) {  // clamp_ passes the gradient on the closed range
                const double mxk = (cx >= 0.f && cx <= hix) ? 1. : 0., myk = (cy >= 0.f && cy <= hiy) ? 1. : 0.;
                const float fx = fminf(fmaxf(cx, 0.f), hix), fy = fminf(fmaxf(cy, 0.f), hiy);
                gx = (d.c_contour * sign_of((double) fx - (double) tx) + c_iou * ibx) * mxk;
                gy = (d.c_contour * sign_of((double) fy - (double) ty) + c_iou * iby) * myk;
            } else {
                gx = d.c_contour * sign_of((double) cx - (double) tx);
                gy = d.c_contour * sign_of((double) cy - (double) ty);
                for (int it = 0; it < iters; ++it) {  // every iteration starts from a detached, rounded point
                    const size_t o = refine_step(cx, cy, ref_b, a.H, a.W, bk, s);
                    if (!d.keys) continue;
                    const double mxk = (cx >= 0.f && cx <= hix) ? 1. : 0., myk = (cy >= 0.f && cy <= hiy) ? 1. : 0.;
                    const float fx = fminf(fmaxf(cx, 0.f), hix), fy = fminf(fmaxf(cy, 0.f), hiy);
                    const bool last = it == iters - 1;
                    const double rx = (d.c_refine * sign_of((double) fx - (double) tx) + (last ? c_iou * ibx : 0.)) * mxk;
                    const double ry = (d.c_refine * sign_of((double) fy - (double) ty) + (last ? c_iou * iby : 0.)) * myk;
                    const size_t slot = (((size_t) p * iters + it) * S + s) * d.nk;
                    for (int k = 0; k < d.nk; ++k) {
                        const int bi = B > 1 ? bk.idx[k * S + s] : 0;
                        const double wk = B > 1 ? (double) bk.w[k * S + s] : 1.;
                        d.keys[slot + k] = (uint32_t) (((size_t) b * B + bi) * a.H * a.W + o);
                        d.perm[slot + k] = (uint32_t) (slot + k);
                        d.vals[slot + k] = make_double2(rx * wk, ry * wk);
                    }
                }
            }
        }
        if (!to_maps) continue;
        // decode backwards: lane i owns coefficient i and walks the 64 points of this chunk in sample order
        gp_s[wave][0][lane] = gx;
        gp_s[wave][1][lane] = gy;
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        const int cnt = S - base < 64 ? S - base : 64;
        for (int i = lane; i < nc + 2; i += 64) {
            double v = acc[i];
            if (i < nc) {
                const int c = (i & 3) >> 1;
                const double sc = (double) (c ? sy : sx);
                const float *table = ((i & 1) ? sin_b : cos_b) + (size_t) (i >> 2) * S + base;
                for (int j = 0; j < cnt; ++j) v += gp_s[wave][c][j] * sc * (double) table[j];
            } else {
                const int c = i - nc;
                const double sc = (double) (c ? sy : sx);
                for (int j = 0; j < cnt; ++j) v += gp_s[wave][c][j] * sc;
            }
            acc[i] = v;
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
    }
    // one proposal owns one head pixel: plain stores
    const float *tf = a.t_fourier + ((size_t) b * a.K + row) * nc;
    const float *tl = a.t_locations + ((size_t) b * a.K + row) * 2;
    for (int i = lane; i < nc + 2; i += 64) {
        if (i < nc) {
            if (!a.g_fourier) continue;
            const float sc = (i & 3) < 2 ? sx : sy;
            const double ow = a.order_weights ? (double) a.order_weights[i >> 2] : 1.;
            const double g = d.c_fourier * ow * sign_of((double) __fmul_rn(coef[i], sc) - (double) tf[i]) * (double) sc;
            a.g_fourier[((size_t) b * a.order_total * 4 + i) * hw + pos] = (float) (acc[i] + g);
        } else {
            if (!a.g_locations) continue;
            const int c = i - nc;
            const float sc = c ? sy : sx;
            const double g = d.c_location * sign_of((double) __fmul_rn(c ? ly : lx, sc) - (double) tl[c]) * (double) sc;
            a.g_locations[((size_t) b * 2 + c) * hw + pos] = (float) (acc[i] + g);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// reduction: one block, fixed order, float64.  Column sums of the proposals and the block sums of the score pass become the
// eight terms: mean, nan_to_num, weight (add_to_loss_dict), each rounded to float32 once; loss = float32 sum in key order.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double finite_or_zero(double v) {
    const float f = (float) v;
    return (f == f && fabsf(f) != __builtin_inff()) ? v : 0.;
}

__global__ __launch_bounds__(RBLK) void obj_reduce_kernel(const Dev d, const double *__restrict__ block_sums, long score_blocks,
                                                         const int32_t *__restrict__ meta_after_counts, int present,
                                                         float *__restrict__ out) {
    __shared__ double part[RBLK];
    const int cols = d.P > 0 ? d.cols : 0;
    for (int c = 0; c < cols + 2; ++c) {
        double s = 0.;
        if (c < cols)
            for (long p = threadIdx.x; p < d.P; p += RBLK) s += d.sums[(size_t) c * d.P + p];
        else
            for (long k = threadIdx.x; k < score_blocks; k += RBLK) s += block_sums[(size_t) k * 2 + (c - cols)];
        part[threadIdx.x] = s;
        __syncthreads();
        for (int w = RBLK / 2; w >= 1; w >>= 1) {
            if ((int) threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) d.reduced[(c < cols ? c : d.cols + (c - cols))] = part[0];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const CpnObjectiveArgs &a = d.a;
    const double P = (double) d.P, n_bg = (double) meta_after_counts[META_BG];
    double term[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    if (d.P > 0) {
        term[0] = finite_or_zero(d.reduced[COL_FOURIER] / (P * a.order * 4)) * a.w_fourier;
        term[1] = finite_or_zero(d.reduced[COL_LOCATION] / (P * 2)) * a.w_location;
        term[2] = finite_or_zero(d.reduced[COL_CONTOUR] / (P * a.samples * 2)) * a.w_contour;
        for (int it = 0; it < d.cols - FIXED_COLS; ++it)
            term[4] += finite_or_zero(d.reduced[FIXED_COLS + it] / (P * a.samples * 2)) * a.w_refinement;
        if (d.reduced[COL_VALID] > 0.) term[6] = finite_or_zero(d.reduced[COL_IOU] / d.reduced[COL_VALID]) * a.w_iou;
        term[3] += finite_or_zero(d.reduced[d.cols] / P) * a.w_score_fg;
    } else {
        d.reduced[COL_VALID] = 0.;
    }
    if (n_bg > 0.) term[3] += finite_or_zero(d.reduced[d.cols + 1] / n_bg) * a.w_score_bg;
    float loss = 0.f;
    for (int k = 0; k < 8; ++k) {
        const bool on = (present >> k) & 1;
        const float t = on ? (float) term[k] : __builtin_nanf("");
        out[k] = t;
        if (on) loss = __fadd_rn(loss, t);
    }
    out[8] = loss;
}

// ---------------------------------------------------------------------------------------------------------
// gradient of the refinement map: the contributions, sorted by element (stable), are summed per run of equal keys in an order
// that depends on the sorted list alone.  A run is cut at the multiples of SEG_CHUNK of the list position: pass 1 sums every
// piece that continues a run across such a cut, pass 2 lets the thread at the head of a run sum its own first piece and then
// the pieces of pass 1 in list order.  A run of L entries costs SEG_CHUNK + L / SEG_CHUNK steps of one thread instead of L.
// ---------------------------------------------------------------------------------------------------------
constexpr int SEG_CHUNK = 32;

__device__ __forceinline__ double2 sum_piece(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ perm,
                                             const double2 *__restrict__ vals, size_t i, size_t E, uint32_t key) {
    double sx = 0., sy = 0.;
    for (size_t j = i; j < E && keys[j] == key && (j == i || (j % SEG_CHUNK) != 0); ++j) {
        const double2 v = vals[perm[j]];
        sx += v.x;
        sy += v.y;
    }
    return make_double2(sx, sy);
}

__global__ __launch_bounds__(256) void obj_segment_pieces_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ perm,
                                                                const double2 *__restrict__ vals, size_t E,
                                                                double2 *__restrict__ pieces) {
    const size_t c = (size_t) blockIdx.x * 256 + threadIdx.x, i = c * SEG_CHUNK;
    if (i >= E || i == 0 || keys[i - 1] != keys[i]) return;  // a run that starts here belongs to pass 2
    pieces[c] = sum_piece(keys, perm, vals, i, E, keys[i]);
}

__global__ __launch_bounds__(256) void obj_segment_sum_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ perm,
                                                             const double2 *__restrict__ vals, const double2 *__restrict__ pieces,
                                                             size_t E, size_t plane, float *__restrict__ g_refinement) {
    const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= E) return;
    const uint32_t key = keys[i];
    if (i > 0 && keys[i - 1] == key) return;
    double2 s = sum_piece(keys, perm, vals, i, E, key);
    for (size_t c = i / SEG_CHUNK + 1; c * SEG_CHUNK < E && keys[c * SEG_CHUNK] == key; ++c) {
        s.x += pieces[c].x;
        s.y += pieces[c].y;
    }
    // pair plane (b * buckets + bucket) -> channels 2 * bucket and 2 * bucket + 1 of image b
    const size_t pair = key / plane, pix = key - pair * plane;
    g_refinement[(pair * 2) * plane + pix] = (float) s.x;
    g_refinement[(pair * 2 + 1) * plane + pix] = (float) s.y;
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct HeadLayout {
    size_t headlab, fgmap, compact, block_sums, total;
    long blocks;
};
HeadLayout head_layout(int64_t N, int64_t h, int64_t w) {
    HeadLayout L;
    const size_t px = (size_t) N * h * w;
    L.blocks = (long) ((px + HBLK - 1) / HBLK);
    size_t o = 0;
    L.headlab = o; o = align_up(o + px * 4, 256);
    L.fgmap = o; o = align_up(o + px * 4, 256);
    L.compact = o; o = align_up(o + (size_t) cpn_compact_workspace_bytes((int32_t) N, (int32_t) h, (int32_t) w), 256);
    L.block_sums = o; o = align_up(o + (size_t) L.blocks * 2 * 8, 256);
    L.total = o;
    return L;
}

struct WorkLayout {
    size_t sums, reduced, keys, keys_out, perm, perm_out, vals, pieces, sort_tmp, sort_tmp_bytes, total, E;
    int cols, nk, key_bits;
};
WorkLayout work_layout(const CpnObjectiveArgs &a, int64_t P) {
    WorkLayout L;
    const bool refine = a.refinement && a.iterations > 0;
    L.cols = FIXED_COLS + (refine ? a.iterations : 0);
    L.nk = a.buckets > 1 ? 3 : 1;
    L.E = (refine && a.g_refinement) ? (size_t) P * a.samples * a.iterations * L.nk : 0;
    const size_t planes = (size_t) a.N * (a.buckets < 1 ? 1 : a.buckets) * a.H * a.W;
    L.key_bits = 1;
    while (L.key_bits < 32 && (1ull << L.key_bits) < planes) ++L.key_bits;
    size_t o = 0;
    L.sums = o; o = align_up(o + (size_t) (P > 0 ? P : 1) * L.cols * 8, 256);
    L.reduced = o; o = align_up(o + (size_t) (L.cols + 2) * 8, 256);
    L.keys = o; o = align_up(o + L.E * 4, 256);
    L.keys_out = o; o = align_up(o + L.E * 4, 256);
    L.perm = o; o = align_up(o + L.E * 4, 256);
    L.perm_out = o; o = align_up(o + L.E * 4, 256);
    L.vals = o; o = align_up(o + L.E * 16, 256);
    L.pieces = o; o = align_up(o + (L.E / SEG_CHUNK + 1) * 16, 256);
    size_t tmp = 0;
    if (L.E)
        (void) rocprim::radix_sort_pairs(nullptr, tmp, (uint32_t *) nullptr, (uint32_t *) nullptr, (uint32_t *) nullptr,
                                         (uint32_t *) nullptr, L.E, 0, L.key_bits, (hipStream_t) 0);
    L.sort_tmp = o; L.sort_tmp_bytes = tmp; o = align_up(o + tmp, 256);
    L.total = o;
    return L;
}

// argument checks that answer before a device is touched
int check_args(const CpnObjectiveArgs *a, const char *who) {
    static thread_local char msg[256];
    auto bad = [&](int code, const char *what) {
        snprintf(msg, sizeof msg, "%s: %s", who, what);
        return cpn::fail(code, msg);
    };
    if (!a) return bad(CPN_E_INVALID, "args is NULL");
    if (a->N <= 0 || a->h <= 0 || a->w <= 0 || a->H <= 0 || a->W <= 0) return bad(CPN_E_INVALID, "N, h, w, H, W must be positive");
    if (a->h > a->H || a->w > a->W) return bad(CPN_E_INVALID, "the head grid (h, w) must not be larger than the labels (H, W)");
    if ((int64_t) a->N * a->h * a->w >= (1ll << 31))
        return bad(CPN_E_UNSUPPORTED, "N * h * w must stay below 2^31 (int32 proposal indices)");
    if (a->order < 1 || a->order > a->order_total || a->order * 4 > MAX_COEF)
        return bad(CPN_E_INVALID, "need 1 <= order <= min(order_total, 64)");
    if (a->samples < 1 || a->K < 0 || a->score_channels < 1) return bad(CPN_E_INVALID, "samples >= 1, K >= 0, score_channels >= 1");
    if (a->iterations < 0 || a->iterations > CPN_OBJECTIVE_MAX_ITERATIONS)
        return bad(CPN_E_INVALID, "refinement iterations must lie in 0 .. CPN_OBJECTIVE_MAX_ITERATIONS");
    if (a->buckets < 1) return bad(CPN_E_INVALID, "buckets >= 1");
    if (!a->scores || !a->locations || !a->fourier || !a->labels || !a->cos_table || !a->sin_table)
        return bad(CPN_E_INVALID, "scores, locations, fourier, labels and the sampling tables must be given");
    if (a->K > 0 && (!a->t_fourier || !a->t_locations || !a->t_contours))
        return bad(CPN_E_INVALID, "the fourier, locations and sampled_contours targets must be given");
    if (a->refinement && a->iterations > 0 && a->buckets > 1 && (!a->bucket_index || !a->bucket_weight))
        return bad(CPN_E_INVALID, "refinement buckets > 1 need the bucket tables");
    if (a->g_refinement && !a->refinement) return bad(CPN_E_INVALID, "a refinement gradient needs a refinement map");
    if (a->refinement && (int64_t) a->N * a->buckets * a->H * a->W >= (1ll << 32))
        return bad(CPN_E_UNSUPPORTED, "N * buckets * H * W must stay below 2^32 (uint32 sort keys)");
    return 0;
}

}  // namespace

extern "C" {

int64_t cpn_objective_head_workspace_bytes(int32_t N, int32_t h, int32_t w) {
    if (N <= 0 || h <= 0 || w <= 0 || (int64_t) N * h * w >= (1ll << 31)) return 0;
    return (int64_t) head_layout(N, h, w).total;
}

int cpn_objective_head(const CpnObjectiveArgs *a, int32_t *indices, int32_t *meta, void *workspace, int64_t workspace_bytes,
                       void *stream) {
    if (int rc = check_args(a, "cpn_objective_head")) return rc;
    if (!indices || !meta || !workspace) return cpn::fail(CPN_E_INVALID, "cpn_objective_head: indices, meta or workspace is NULL");
    const HeadLayout L = head_layout(a->N, a->h, a->w);
    if (workspace_bytes < (int64_t) L.total) return cpn::fail(CPN_E_WORKSPACE, "cpn_objective_head: workspace too small");
    hipStream_t st = (hipStream_t) stream;
    char *ws = (char *) workspace;
    int32_t *headlab = (int32_t *) (ws + L.headlab);
    float *fgmap = (float *) (ws + L.fgmap);
    int32_t *after = meta + a->N + 1;
    if (int rc = cpn::check_hip(hipMemsetAsync(after, 0, CPN_OBJECTIVE_META_WORDS * 4, st), "cpn_objective_head")) return rc;
    hipLaunchKernelGGL(obj_head_kernel, dim3((unsigned) L.blocks), dim3(HBLK), 0, st, a->labels, a->labels_i64, a->N, a->H, a->W,
                       a->h, a->w, a->K, headlab, fgmap, after);
    if (int rc = cpn_compact(fgmap, a->N, a->h, a->w, 0.f, indices, meta, ws + L.compact, stream)) return rc;
    hipLaunchKernelGGL(obj_score_kernel, dim3((unsigned) L.blocks), dim3(HBLK), 0, st, a->scores, headlab, a->t_classes, a->N,
                       a->score_channels, a->h * a->w, a->K, a->w_score_fg, a->w_score_bg, meta + a->N, after, a->g_scores,
                       (double *) (ws + L.block_sums));
    return cpn::check_hip(hipGetLastError(), "cpn_objective_head");
}

int64_t cpn_objective_workspace_bytes(const CpnObjectiveArgs *a, int64_t P) {
    if (check_args(a, "cpn_objective_workspace_bytes") || P < 0) return 0;
    const bool refine = a->refinement && a->iterations > 0;
    if (refine && a->g_refinement && (double) P * a->samples * a->iterations * (a->buckets > 1 ? 3 : 1) >= 4294967296.) return 0;
    return (int64_t) work_layout(*a, P).total;
}

int cpn_objective_proposals(const CpnObjectiveArgs *a, const int32_t *indices, int32_t P, const int32_t *meta, int32_t present,
                            void *head_workspace, void *workspace, int64_t workspace_bytes, float *out, void *stream) {
    if (int rc = check_args(a, "cpn_objective_proposals")) return rc;
    if (P < 0 || !meta || !head_workspace || !workspace || !out || (P > 0 && !indices))
        return cpn::fail(CPN_E_INVALID, "cpn_objective_proposals: bad arguments");
    if (P > 0 && a->K < 1) return cpn::fail(CPN_E_INVALID, "cpn_objective_proposals: proposals need target rows (K >= 1)");
    const bool refine = a->refinement && a->iterations > 0;
    if (refine && a->g_refinement && (double) P * a->samples * a->iterations * (a->buckets > 1 ? 3 : 1) >= 4294967296.)
        return cpn::fail(CPN_E_UNSUPPORTED, "cpn_objective_proposals: P * samples * iterations * (1 or 3) must stay below 2^32");
    const WorkLayout L = work_layout(*a, P);
    if (workspace_bytes < (int64_t) L.total) return cpn::fail(CPN_E_WORKSPACE, "cpn_objective_proposals: workspace too small");
    const HeadLayout HL = head_layout(a->N, a->h, a->w);
    hipStream_t st = (hipStream_t) stream;
    char *ws = (char *) workspace, *hws = (char *) head_workspace;
    Dev d;
    d.a = *a;
    d.indices = indices;
    d.headlab = (const int32_t *) (hws + HL.headlab);
    d.P = P;
    const double n = P > 0 ? (double) P : 1.;
    d.c_fourier = a->w_fourier / (n * a->order * 4);
    d.c_location = a->w_location / (n * 2);
    d.c_contour = a->w_contour / (n * a->samples * 2);
    d.c_refine = a->w_refinement / (n * a->samples * 2);
    d.sums = (double *) (ws + L.sums);
    d.reduced = (double *) (ws + L.reduced);
    d.keys = L.E ? (uint32_t *) (ws + L.keys) : nullptr;
    d.perm = L.E ? (uint32_t *) (ws + L.perm) : nullptr;
    d.vals = L.E ? (double2 *) (ws + L.vals) : nullptr;
    d.cols = L.cols;
    d.nk = L.nk;
    const size_t hw = (size_t) a->h * a->w;
    // a proposal writes its own head pixel only: every other element of the three maps is zero
    if (a->g_fourier)
        if (int rc = cpn::check_hip(hipMemsetAsync(a->g_fourier, 0, (size_t) a->N * a->order_total * 4 * hw * 4, st), "cpn_objective")) return rc;
    if (a->g_locations)
        if (int rc = cpn::check_hip(hipMemsetAsync(a->g_locations, 0, (size_t) a->N * 2 * hw * 4, st), "cpn_objective")) return rc;
    if (a->g_refinement)
        if (int rc = cpn::check_hip(hipMemsetAsync(a->g_refinement, 0, (size_t) a->N * 2 * a->buckets * a->H * a->W * 4, st), "cpn_objective"))
            return rc;
    const unsigned blocks = (unsigned) ((P + PWAVES - 1) / PWAVES);
    if (P > 0) hipLaunchKernelGGL(obj_proposal_kernel<false>, dim3(blocks), dim3(PWAVES * WAVE), 0, st, d);
    hipLaunchKernelGGL(obj_reduce_kernel, dim3(1), dim3(RBLK), 0, st, d, (const double *) (hws + HL.block_sums), HL.blocks,
                       meta + a->N + 1, present, out);
    if (P > 0 && (a->g_fourier || a->g_locations || a->g_refinement)) {
        hipLaunchKernelGGL(obj_proposal_kernel<true>, dim3(blocks), dim3(PWAVES * WAVE), 0, st, d);
        if (L.E) {
            size_t tmp = L.sort_tmp_bytes;
            if (int rc = cpn::check_hip(rocprim::radix_sort_pairs(ws + L.sort_tmp, tmp, d.keys, (uint32_t *) (ws + L.keys_out), d.perm,
                                                                  (uint32_t *) (ws + L.perm_out), L.E, 0, L.key_bits, st),
                                        "cpn_objective_proposals (sort)"))
                return rc;
            const size_t chunks = L.E / SEG_CHUNK + 1;
            hipLaunchKernelGGL(obj_segment_pieces_kernel, dim3((unsigned) ((chunks + 255) / 256)), dim3(256), 0, st,
                               (const uint32_t *) (ws + L.keys_out), (const uint32_t *) (ws + L.perm_out), d.vals, L.E,
                               (double2 *) (ws + L.pieces));
            hipLaunchKernelGGL(obj_segment_sum_kernel, dim3((unsigned) ((L.E + 255) / 256)), dim3(256), 0, st,
                               (const uint32_t *) (ws + L.keys_out), (const uint32_t *) (ws + L.perm_out), d.vals,
                               (const double2 *) (ws + L.pieces), L.E, (size_t) a->H * a->W, a->g_refinement);
        }
    }
    return cpn::check_hip(hipGetLastError(), "cpn_objective_proposals");
}

}  // extern "C"
