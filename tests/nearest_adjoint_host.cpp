// csrc/nearest_adjoint.h and the weight gradient's partition on the host (tests/test_cat_conv.py builds this host program with
// AddressSanitizer and UBSan and runs it).  For every 1 <= in <= out <= 70, against brute force over na_src:
//   - the footprints [na_first(i), na_first(i + 1)) of i = 0 ... in - 1 are contiguous, in ascending order, start at 0 and end at
//     out: every dst pixel lies in exactly one, and it is the footprint of the pixel it reads;
//   - na_src is non-decreasing, stays in [0, in) and is the identity for in == out; the exact x2 reads dst / 2;
//   - na_pixel_src agrees with the decomposition written out, for a batch of two images (every (H, W, h, w) with H, W <= 12 and
//     three larger odd shapes);
//   - the partition of the virtual concat's reduction (wgs_partition over N * H rows) covers every staged X row of every chunk of
//     every slab with an index inside [0, P) or marks it outside, as the kernel's table does.
// Output: "ok <checks>" or the first difference.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../celldetection_amd/csrc/nearest_adjoint.h"
#include "../celldetection_amd/csrc/wgrad_slabs.h"

static long checks = 0;

static int check_axis(int in, int out) {
    const float scale = na_scale(in, out);
    std::vector<int> owner((size_t) out, -1);
    int prev = 0;
    for (int d = 0; d < out; ++d) {
        const int s = na_src(d, scale, in);
        if (s < 0 || s >= in || s < prev) { std::printf("in %d out %d: src(%d) = %d after %d\n", in, out, d, s, prev); return 1; }
        if (in == out && s != d) { std::printf("in == out == %d: src(%d) = %d\n", in, d, s); return 1; }
        if (out == 2 * in && s != d / 2) { std::printf("in %d out %d: src(%d) = %d\n", in, out, d, s); return 1; }
        prev = s;
    }
    if (na_first(0, scale, in, out) != 0 || na_first(in, scale, in, out) != out) { std::printf("in %d out %d: ends\n", in, out); return 1; }
    for (int i = 0; i < in; ++i) {
        const int lo = na_first(i, scale, in, out), hi = na_first(i + 1, scale, in, out);
        if (lo < 0 || hi < lo || hi > out) { std::printf("in %d out %d: footprint of %d is [%d, %d)\n", in, out, i, lo, hi); return 1; }
        for (int d = lo; d < hi; ++d) {
            if (owner[(size_t) d] != -1) { std::printf("in %d out %d: dst %d lies in two footprints\n", in, out, d); return 1; }
            owner[(size_t) d] = i;
        }
        int count = 0;  // brute force: the dst pixels that read i
        for (int d = 0; d < out; ++d) count += na_src(d, scale, in) == i;
        if (count != hi - lo) { std::printf("in %d out %d: %d pixels read %d, footprint [%d, %d)\n", in, out, count, i, lo, hi); return 1; }
        ++checks;
    }
    for (int d = 0; d < out; ++d)
        if (owner[(size_t) d] != na_src(d, scale, in)) { std::printf("in %d out %d: dst %d owned by %d\n", in, out, d, owner[(size_t) d]); return 1; }
    return 0;
}

static int check_pixels(int N, int H, int W, int h, int w) {
    const float sy = na_scale(h, H), sx = na_scale(w, W);
    std::vector<int> table((size_t) N * H * W);
    for (int n = 0; n < N; ++n)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) table[((size_t) n * H + y) * W + x] = (n * h + na_src(y, sy, h)) * w + na_src(x, sx, w);
    for (int32_t f = 0; f < N * H * W; ++f) {
        const int32_t g = na_pixel_src(f, H, W, h, w, sy, sx);
        if (g != table[(size_t) f] || g < 0 || g >= N * h * w) { std::printf("pixel %d of %d x %d x %d <- %d x %d: %d\n", f, N, H, W, h, w, g); return 1; }
        ++checks;
    }
    return 0;
}

// the staged X rows of the slab kernel: chunk of 128 pixels, K + 127 rows from the flat offset (ky - pad) * W - pad
static int check_staging(int N, int H, int W, int K, int slab_rows) {
    const WgSlabs part = wgs_partition((int64_t) N * H, W, slab_rows, 7);
    const int64_t P = (int64_t) N * H * W;
    std::vector<int> seen((size_t) P, 0);
    for (int32_t s = 0; s < part.slabs; ++s) {
        int64_t p0, p1;
        wgs_range(part, s, &p0, &p1);
        for (int64_t c0 = p0; c0 < p1; c0 += 128)
            for (int ky = 0; ky < K; ++ky)
                for (int u = 0; u < 128 + K - 1; ++u) {
                    const int64_t f = c0 + u + (int64_t) (ky - K / 2) * W - K / 2;
                    if (f < 0 || f >= P) continue;  // the table's -1: a row of zeros
                    const int32_t g = na_pixel_src((int32_t) f, H, W, (H + 1) / 2, (W + 1) / 2, na_scale((H + 1) / 2, H), na_scale((W + 1) / 2, W));
                    if (g < 0 || g >= N * ((H + 1) / 2) * ((W + 1) / 2)) { std::printf("staging %d x %d x %d k %d: row %ld -> %d\n", N, H, W, K, (long) f, g); return 1; }
                    if (ky == K / 2 && u >= K / 2 && u < 128 + K / 2 && c0 + (u - K / 2) < p1) seen[(size_t) f] += 1;
                    ++checks;
                }
    }
    for (int64_t p = 0; p < P; ++p)
        if (seen[(size_t) p] != 1) { std::printf("staging %d x %d x %d k %d: pixel %ld staged %d times at the centre tap\n", N, H, W, K, (long) p, seen[(size_t) p]); return 1; }
    return 0;
}

int main() {
    for (int out = 1; out <= 70; ++out)
        for (int in = 1; in <= out; ++in)
            if (check_axis(in, out)) return 1;
    for (int H = 1; H <= 12; ++H)
        for (int W = 1; W <= 12; ++W)
            for (int h = 1; h <= H; ++h)
                for (int w = 1; w <= W; ++w)
                    if (check_pixels(2, H, W, h, w)) return 1;
    const int big[][4] = {{17, 33, 9, 17}, {46, 3, 14, 2}, {5, 69, 5, 21}};
    for (const auto &b : big)
        if (check_pixels(2, b[0], b[1], b[2], b[3])) return 1;
    for (int K : {1, 3, 7})
        for (int slab_rows : {0, 1, 3})
            for (const auto &b : big)
                if (check_staging(2, b[0], b[1], K, slab_rows)) return 1;
    std::printf("ok %ld\n", checks);
    return 0;
}
