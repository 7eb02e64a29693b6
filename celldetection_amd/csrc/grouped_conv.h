// Index arithmetic of the trainable grouped 3x3 conv (csrc/grouped_conv_train.hip; the rule is the "Trainable grouped convolution"
// section of include/cpn_hip.h).  A grouped conv of C -> C channels in groups of cig channels runs as `bundles` block-diagonal dense
// convs of bw -> bw channels: bw = 32 holds 32 / cig groups (cig <= 32), bw = 64 is one group (cig = 64).
//   - the pack: element o of the records [bundle][item = (32-channel chunk, tap)][bw][32] -> the weight it holds, or an exact zero
//     (the padding item behind an odd item count of EVERY bundle; an input and an output channel in different groups);
//   - the weight gradient: only the diagonal 32 x 32 fragments of the (co, ci) matrix exist.  bw = 32: fragment f = bundle f;
//     bw = 64: the four fragments 4 g + 2 a + b of group g, (co chunk a, ci chunk b).  A workgroup ("span") holds four fragments,
//     one per wave: four bundles of a 128-channel span, or the four fragments of a group;
//   - the dilation of the stride-2 gradient: dZ[2 i][2 j] = dY[i][j], zero elsewhere.
// Integer arithmetic only; compiles for the device and for the host (tests/grouped_conv_host.cpp runs it against brute force under
// sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GCV_HD __host__ __device__ __forceinline__
#else
#define GCV_HD inline
#endif

constexpr int GCV_TAPS = 9;  // 3 x 3

struct GcGeo {
    int32_t C, cig;
    int32_t bw;            // bundle width: 32 | 64
    int32_t bundles;       // C / bw
    int32_t gpb;           // groups per bundle: bw / cig
    int32_t items;         // (bw / 32) * 9 real items per bundle
    int32_t items_packed;  // + one zero item when odd
    int32_t frags;         // diagonal 32 x 32 fragments: C / 32 | 4 * C / 64
    int32_t spans;         // workgroups along the channels: ceil(C / 128) | C / 64
};

// false for (C, cig) outside the family: cig in {4, 8, 16, 32, 64}, C a positive multiple of the bundle width
GCV_HD bool gc_geometry(int32_t C, int32_t cig, GcGeo *g) {
    if (cig != 4 && cig != 8 && cig != 16 && cig != 32 && cig != 64) return false;
    const int32_t bw = cig == 64 ? 64 : 32;
    if (C < bw || C % bw) return false;
    g->C = C;
    g->cig = cig;
    g->bw = bw;
    g->bundles = C / bw;
    g->gpb = bw / cig;
    g->items = bw / 32 * GCV_TAPS;
    g->items_packed = g->items + (g->items & 1);
    g->frags = bw == 64 ? C / 16 : C / 32;
    g->spans = bw == 64 ? C / 64 : (C + 127) / 128;
    return true;
}

GCV_HD int64_t gc_packed_elements(const GcGeo &g) { return (int64_t) g.bundles * g.items_packed * g.bw * 32; }

// element o of the packed records -> index into w [C][cig][3][3], or -1 for an exact zero.  dgrad: the taps flipped and the channel
// roles swapped inside the group (the record's output channel is an INPUT channel of the conv, its lane an output channel)
GCV_HD int64_t gc_pack_source(const GcGeo &g, int64_t o, int dgrad) {
    const int32_t c = (int32_t) (o & 31);
    const int64_t t = (o >> 5) / g.bw;
    const int32_t oc = (int32_t) ((o >> 5) % g.bw), item = (int32_t) (t % g.items_packed), bundle = (int32_t) (t / g.items_packed);
    if (item >= g.items) return -1;
    const int32_t rc = item / GCV_TAPS * 32 + c, tap = item % GCV_TAPS;
    if (oc / g.cig != rc / g.cig) return -1;
    int32_t ky = tap / 3, kx = tap % 3, co, cl;
    if (dgrad) {
        co = bundle * g.bw + rc;
        cl = oc % g.cig;
        ky = 2 - ky;
        kx = 2 - kx;
    } else {
        co = bundle * g.bw + oc;
        cl = rc % g.cig;
    }
    return (((int64_t) co * g.cig + cl) * 3 + ky) * 3 + kx;
}

// fragment f -> the 32-channel chunks of dY (output channels) and of X (input channels) it multiplies
GCV_HD void gc_frag_chunks(const GcGeo &g, int32_t f, int32_t *co_chunk, int32_t *ci_chunk) {
    if (g.bw == 64) {
        *co_chunk = 2 * (f >> 2) + ((f >> 1) & 1);
        *ci_chunk = 2 * (f >> 2) + (f & 1);
    } else {
        *co_chunk = *ci_chunk = f;
    }
}

// workgroup `span`: its first 32-channel chunk, the chunks it stages, and the fragment of wave `wave` (-1: behind the last)
GCV_HD int32_t gc_span_first_chunk(const GcGeo &g, int32_t span) { return (g.bw == 64 ? 2 : 4) * span; }
GCV_HD int32_t gc_span_chunks(const GcGeo &g) { return g.bw == 64 ? 2 : 4; }
GCV_HD int32_t gc_wave_frag(const GcGeo &g, int32_t span, int32_t wave) {
    const int32_t f = 4 * span + wave;
    return f < g.frags ? f : -1;
}

// dW element (co, cl): its fragment, and row i (output channel) and column j (input channel) inside it
GCV_HD void gc_locate(const GcGeo &g, int32_t co, int32_t cl, int32_t *f, int32_t *i, int32_t *j) {
    *i = co & 31;
    if (g.bw == 64) {
        *f = 4 * (co >> 6) + 2 * ((co >> 5) & 1) + (cl >> 5);
        *j = cl & 31;
    } else {
        *f = co >> 5;
        *j = (co & 31) / g.cig * g.cig + cl;
    }
}

// stride 2: spatial size of the output
GCV_HD int32_t gc_out_size(int32_t in, int32_t stride) { return (in - 1) / stride + 1; }

// 16-byte unit u (8 channels) of dZ [N][Hin][Win][C] -> the unit of dY [N][Hout][Wout][C] it copies, or -1 for zeros.  u < 2^32.
GCV_HD int64_t gc_dilate_source(uint32_t u, uint32_t Hin, uint32_t Win, uint32_t C8) {
    const uint32_t c = u % C8, p = u / C8, x = p % Win, r = p / Win, y = r % Hin, n = r / Hin;
    if ((x | y) & 1u) return -1;
    const uint32_t Hout = (Hin - 1) / 2 + 1, Wout = (Win - 1) / 2 + 1;
    return (((int64_t) n * Hout + (y >> 1)) * Wout + (x >> 1)) * C8 + c;
}

// The gather back: 16-byte unit u (8 channels) of xs [N][Hout][Wout][C] -> the unit of x [N][Hin][Win][C] it copies, the pixel
// (stride i, stride j) of the same image (stride >= 1; stride (Hout - 1) <= Hin - 1 for even and odd Hin).  u < 2^32.
GCV_HD int64_t gc_subsample_source(uint32_t u, uint32_t Hin, uint32_t Win, uint32_t C8, uint32_t stride) {
    const uint32_t Hout = (Hin - 1) / stride + 1, Wout = (Win - 1) / stride + 1;
    const uint32_t c = u % C8, p = u / C8, j = p % Wout, r = p / Wout, i = r % Hout, n = r / Hout;
    return (((int64_t) n * Hin + (int64_t) i * stride) * Win + (int64_t) j * stride) * C8 + c;
}
