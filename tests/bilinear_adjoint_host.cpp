// csrc/bilinear_adjoint.h and the weight gradient's partition on the host (tests/test_bilinear_resize.py builds this host program
// with AddressSanitizer and UBSan and runs it).  For every 1 <= in <= out <= 70 and a few large pairs, for both forms of the
// coordinate (split and fused; they must differ somewhere and nowhere by more than the product's rounding), against brute force over
// ba_tap:
//   - i0 is non-decreasing, stays in [0, in), i1 is i0 or i0 + 1 and stays in [0, in), 0 <= lambda < 1; in == out is the identity
//     (i0 = dst, lambda = 0);
//   - the footprint [ba_first(i - 1), ba_first(i + 1)) of every source index i is not empty and is exactly the set of dst with
//     i0 in {i - 1, i}; outside it ba_weight is an exact 0; inside it ba_weight is (i == i0) * (1 - lambda) + (i == i1) * lambda;
//   - every dst lies in the footprints of exactly its i0 and i0 + 1 -- two of them, one at the clamped last index -- and its
//     weights add up to 1 within one rounding;
//   - the staged X rows of the slab kernel (chunks of 128 pixels, K + 127 rows from the flat offset (ky - pad) * W - pad, per
//     wgs_partition over N * H rows): the four source pixels of every staged row inside the tensor lie inside [0, N * h * w), and
//     the centre tap stages every pixel exactly once.
// Output: "ok <checks>" or the first difference.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../celldetection_amd/csrc/bilinear_adjoint.h"
#include "../celldetection_amd/csrc/wgrad_slabs.h"

static long checks = 0;

static int check_axis(int in, int out, bool fused) {
    const float scale = ba_scale(in, out);
    std::vector<int> covered((size_t) out, 0);
    int prev = 0;
    for (int d = 0; d < out; ++d) {
        int i0, i1;
        float l;
        ba_tap(d, scale, in, fused, &i0, &i1, &l);
        if (i0 < prev || i0 < 0 || i0 >= in || i1 < i0 || i1 > i0 + 1 || i1 >= in || !(l >= 0.f && l < 1.f)) {
            std::printf("in %d out %d: tap(%d) = %d, %d, %g after %d\n", in, out, d, i0, i1, (double) l, prev);
            return 1;
        }
        if (in == out && (i0 != d || l != 0.f)) { std::printf("in == out == %d: tap(%d) = %d, %g\n", in, d, i0, (double) l); return 1; }
        if (d == 0 && i0 != 0) { std::printf("in %d out %d: dst 0 reads %d\n", in, out, i0); return 1; }
        if (d == out - 1 && i0 != in - 1) { std::printf("in %d out %d: the last dst reads %d\n", in, out, i0); return 1; }
        prev = i0;
        float sum = 0.f;
        for (int i = 0; i < in; ++i) sum += ba_weight(d, scale, in, fused, i);
        if (std::fabs(sum - 1.f) > 1.2e-7f) { std::printf("in %d out %d: weights of dst %d add up to %.9g\n", in, out, d, (double) sum); return 1; }
    }
    if (ba_first(0, scale, in, out, fused) != 0 || ba_first(-1, scale, in, out, fused) != 0 || ba_first(in, scale, in, out, fused) != out ||
        ba_first(in + 1, scale, in, out, fused) != out) {
        std::printf("in %d out %d: ends\n", in, out);
        return 1;
    }
    for (int i = 0; i < in; ++i) {
        const int lo = ba_first(i - 1, scale, in, out, fused), hi = ba_first(i + 1, scale, in, out, fused);
        if (lo < 0 || hi <= lo || hi > out) { std::printf("in %d out %d: footprint of %d is [%d, %d)\n", in, out, i, lo, hi); return 1; }
        for (int d = 0; d < out; ++d) {
            int i0, i1;
            float l;
            ba_tap(d, scale, in, fused, &i0, &i1, &l);
            const bool inside = d >= lo && d < hi;
            if (inside != (i0 == i - 1 || i0 == i)) { std::printf("in %d out %d: dst %d (i0 %d) and the footprint [%d, %d) of %d\n", in, out, d, i0, lo, hi, i); return 1; }
            float want = 0.f;
            if (i == i0) want = 1.f - l;
            if (i == i1) want += l;
            const float got = ba_weight(d, scale, in, fused, i);
            if (got != want || (!inside && got != 0.f)) { std::printf("in %d out %d: weight(%d, %d) = %.9g, want %.9g\n", in, out, d, i, (double) got, (double) want); return 1; }
            covered[(size_t) d] += inside;
            ++checks;
        }
    }
    for (int d = 0; d < out; ++d) {
        const int want = ba_i0(d, scale, in, fused) < in - 1 ? 2 : 1;
        if (covered[(size_t) d] != want) { std::printf("in %d out %d: dst %d lies in %d footprints\n", in, out, d, covered[(size_t) d]); return 1; }
    }
    return 0;
}

// the table of the slab kernel: the four source pixels of flat pixel f of the [N][H][W] map
static int check_staging(int N, int H, int W, int h, int w, int K, int slab_rows) {
    const WgSlabs part = wgs_partition((int64_t) N * H, W, slab_rows, 7);
    const int64_t P = (int64_t) N * H * W, p = (int64_t) N * h * w;
    const float sy = ba_scale(h, H), sx = ba_scale(w, W);
    std::vector<int> seen((size_t) P, 0);
    for (int32_t s = 0; s < part.slabs; ++s) {
        int64_t p0, p1;
        wgs_range(part, s, &p0, &p1);
        for (int64_t c0 = p0; c0 < p1; c0 += 128)
            for (int ky = 0; ky < K; ++ky)
                for (int u = 0; u < 128 + K - 1; ++u) {
                    const int64_t f = c0 + u + (int64_t) (ky - K / 2) * W - K / 2;
                    if (f < 0 || f >= P) continue;  // the table's negative index: a row of zeros
                    const int64_t row = f / W, x = f - row * W, n = row / H, y = row - n * H;
                    int y0, y1, x0, x1;
                    float ly, lx;
                    ba_tap((int) y, sy, h, true, &y0, &y1, &ly);
                    ba_tap((int) x, sx, w, true, &x0, &x1, &lx);
                    const int64_t g[4] = {(n * h + y0) * w + x0, (n * h + y0) * w + x1, (n * h + y1) * w + x0, (n * h + y1) * w + x1};
                    for (const int64_t v : g)
                        if (v < n * h * w || v >= (n + 1) * h * w || v >= p) { std::printf("staging %d x %d x %d <- %d x %d k %d: pixel %ld -> %ld\n", N, H, W, h, w, K, (long) f, (long) v); return 1; }
                    if (ky == K / 2 && u >= K / 2 && u < 128 + K / 2 && c0 + (u - K / 2) < p1) seen[(size_t) f] += 1;
                    ++checks;
                }
    }
    for (int64_t q = 0; q < P; ++q)
        if (seen[(size_t) q] != 1) { std::printf("staging %d x %d x %d k %d: pixel %ld staged %d times at the centre tap\n", N, H, W, K, (long) q, seen[(size_t) q]); return 1; }
    return 0;
}

int main() {
    long differ = 0;
    for (int out = 1; out <= 70; ++out)
        for (int in = 1; in <= out; ++in) {
            if (check_axis(in, out, false) || check_axis(in, out, true)) return 1;
            for (int d = 0; d < out; ++d) {  // the two forms of the coordinate: the same taps, or lambdas within 2^-24 * in of 0 and 1
                int a0, a1, b0, b1;
                float la, lb;
                ba_tap(d, ba_scale(in, out), in, false, &a0, &a1, &la);
                ba_tap(d, ba_scale(in, out), in, true, &b0, &b1, &lb);
                const float tol = 5.97e-8f * (float) in;
                const bool ok = a0 == b0 ? std::fabs(la - lb) <= tol : (a0 == b0 + 1 && la <= tol && lb >= 1.f - tol);
                if (!ok) { std::printf("in %d out %d dst %d: split (%d, %g), fused (%d, %g)\n", in, out, d, a0, (double) la, b0, (double) lb); return 1; }
                differ += a0 != b0 || la != lb;
            }
        }
    if (differ == 0) { std::printf("the two forms of the coordinate never differ\n"); return 1; }
    const int pairs[][2] = {{256, 512}, {255, 512}, {1, 4096}, {14, 46}, {341, 1024}, {511, 512}, {512, 512}};
    for (const auto &p : pairs)
        if (check_axis(p[0], p[1], false) || check_axis(p[0], p[1], true)) return 1;
    const int big[][4] = {{33, 70, 17, 35}, {46, 3, 14, 2}, {5, 69, 5, 21}, {6, 10, 1, 1}, {13, 14, 7, 7}};
    for (int K : {3, 5, 7})
        for (int slab_rows : {0, 1, 3})
            for (const auto &b : big)
                if (check_staging(2, b[0], b[1], b[2], b[3], K, slab_rows)) return 1;
    std::printf("ok %ld\n", checks);
    return 0;
}
