// csrc/pool_adjoint.h (the index arithmetic of csrc/pool_train.hip) and the stem weight gradient's staging on the host (tests/test_stem.py builds this host program with
// AddressSanitizer and UBSan and runs it).  For every 1 <= H, W <= 12 that holds a window, in both geometries (3, 2, 1) and
// (2, 2, 0), against brute force over the windows:
//   - the windows [pa_first, pa_last] x [pa_first, pa_last] a pixel reports are exactly the windows that contain it, at most
//     2 x 2 of them, and the tap it reports for each is the position's own;
//   - a tap index round-trips: pa_index -> (ty, tx) -> pa_position gives the pixel back, and every in-image position of every
//     window is reported by its pixel (the forward and the gather see the same pairs);
//   - at (2, 2, 0) the odd last row and column lie in no window.
// And for the stem (H, W <= 12 and three larger shapes, slab_rows 0, 1, 3): the 64 bytes staged for every pixel of every 128-pixel
// chunk of every slab lie inside the padded input [N][H + 6][W + 8][4] bf16, and every output pixel is staged exactly once per
// filter row.
// Output: "ok <checks>" or the first difference.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../celldetection_amd/csrc/pool_adjoint.h"
#include "../celldetection_amd/csrc/wgrad_slabs.h"

static long checks = 0;

static int check_pool(int H, int W, int k, int s, int pad) {
    const int Ho = pa_out(H, k, s, pad), Wo = pa_out(W, k, s, pad);
    if (Ho < 1 || Wo < 1) return 0;  // no window: the launch refuses the call
    // brute force: contains[(iy, ix)][(oy, ox)] = tap index or -1
    std::vector<int> contains((size_t) H * W * Ho * Wo, -1);
    for (int oy = 0; oy < Ho; ++oy)
        for (int ox = 0; ox < Wo; ++ox)
            for (int ty = 0; ty < k; ++ty)
                for (int tx = 0; tx < k; ++tx) {
                    const int iy = oy * s - pad + ty, ix = ox * s - pad + tx;
                    if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
                    contains[(((size_t) iy * W + ix) * Ho + oy) * Wo + ox] = ty * k + tx;
                    const int index = pa_index(ty, tx, k);
                    if (index < 0 || index > 255 || pa_index_ty(index, k) != ty || pa_index_tx(index, k) != tx ||
                        pa_position(oy, pa_index_ty(index, k), s, pad) != iy || pa_position(ox, pa_index_tx(index, k), s, pad) != ix) {
                        std::printf("%d x %d (%d, %d, %d): tap (%d, %d) of window (%d, %d) does not round-trip\n", H, W, k, s, pad, ty, tx, oy, ox);
                        return 1;
                    }
                    ++checks;
                }
    for (int iy = 0; iy < H; ++iy)
        for (int ix = 0; ix < W; ++ix) {
            const int oy0 = pa_first(iy, k, s, pad), oy1 = pa_last(iy, s, pad, Ho);
            const int ox0 = pa_first(ix, k, s, pad), ox1 = pa_last(ix, s, pad, Wo);
            if (oy0 < 0 || ox0 < 0 || oy1 >= Ho || ox1 >= Wo || oy1 - oy0 > 1 || ox1 - ox0 > 1) {
                std::printf("%d x %d (%d, %d, %d): pixel (%d, %d) reports windows [%d, %d] x [%d, %d]\n", H, W, k, s, pad, iy, ix, oy0, oy1, ox0, ox1);
                return 1;
            }
            for (int oy = 0; oy < Ho; ++oy)
                for (int ox = 0; ox < Wo; ++ox) {
                    const bool reported = oy >= oy0 && oy <= oy1 && ox >= ox0 && ox <= ox1;
                    const int want = contains[(((size_t) iy * W + ix) * Ho + oy) * Wo + ox];
                    if (reported != (want >= 0)) {
                        std::printf("%d x %d (%d, %d, %d): pixel (%d, %d), window (%d, %d): reported %d, contained %d\n", H, W, k, s, pad, iy, ix, oy, ox, (int) reported, want);
                        return 1;
                    }
                    if (reported) {
                        const int ty = pa_tap(iy, oy, s, pad), tx = pa_tap(ix, ox, s, pad);
                        if (ty < 0 || ty >= k || tx < 0 || tx >= k || pa_index(ty, tx, k) != want) {
                            std::printf("%d x %d (%d, %d, %d): pixel (%d, %d) is tap (%d, %d) of window (%d, %d), not %d\n", H, W, k, s, pad, iy, ix, ty, tx, oy, ox, want);
                            return 1;
                        }
                    }
                    ++checks;
                }
            if (k == 2 && ((H % 2 && iy == H - 1) || (W % 2 && ix == W - 1)) && oy0 <= oy1 && ox0 <= ox1) {
                std::printf("%d x %d (2, 2, 0): the odd last pixel (%d, %d) lies in a window\n", H, W, iy, ix);
                return 1;
            }
        }
    return 0;
}

// the X staging of st_wgrad_slab_kernel (csrc/stem_train.hip; its dY staging is csrc/image_train.h): chunks of 128 flat output pixels, 64 bytes at Xp[n][2 oy + ky][2 ox]
static int check_stem_staging(int N, int H, int W, int slab_rows) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, Hp = H + 6, Wp = W + 8;
    const int64_t bytes = (int64_t) N * Hp * Wp * 8;
    const WgSlabs part = wgs_partition((int64_t) N * Ho, Wo, slab_rows, 256);
    std::vector<int> seen((size_t) N * Ho * Wo * 7, 0);
    for (int32_t sl = 0; sl < part.slabs; ++sl) {
        int64_t p0, p1;
        wgs_range(part, sl, &p0, &p1);
        if (p0 < 0 || p1 > (int64_t) N * Ho * Wo || p0 >= p1) { std::printf("stem %d x %d x %d: slab %d is [%ld, %ld)\n", N, H, W, sl, (long) p0, (long) p1); return 1; }
        for (int64_t c0 = p0; c0 < p1; c0 += 128)
            for (int ky = 0; ky < 7; ++ky)
                for (int t = 0; t < 128; ++t) {
                    const int64_t p = c0 + t;
                    if (p >= p1) continue;  // staged as zeros (the kernel re-reads pixel p1 - 1 there, which this loop has checked)
                    const unsigned row = (unsigned) p / (unsigned) Wo, ox = (unsigned) p - row * (unsigned) Wo;
                    const unsigned n = row / (unsigned) Ho, oy = row - n * (unsigned) Ho;
                    const int64_t at = (((int64_t) n * Hp + 2 * oy + ky) * Wp + 2 * ox) * 8;
                    if (at < 0 || at + 64 > bytes || at % 8) { std::printf("stem %d x %d x %d: pixel %ld row %d reads [%ld, %ld) of %ld\n", N, H, W, (long) p, ky, (long) at, (long) at + 64, (long) bytes); return 1; }
                    seen[(size_t) p * 7 + ky] += 1;
                    ++checks;
                }
    }
    for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] != 1) { std::printf("stem %d x %d x %d: pixel %zu row %zu staged %d times\n", N, H, W, i / 7, i % 7, seen[i]); return 1; }
    return 0;
}

int main() {
    for (int H = 1; H <= 12; ++H)
        for (int W = 1; W <= 12; ++W) {
            if (check_pool(H, W, 3, 2, 1) || check_pool(H, W, 2, 2, 0)) return 1;
            for (int slab_rows : {0, 1, 3})
                if (check_stem_staging(2, H, W, slab_rows)) return 1;
        }
    if (pa_out(1, 2, 2, 0) != 0 || pa_out(2, 2, 2, 0) != 1 || pa_out(1, 3, 2, 1) != 1 || pa_out(512, 3, 2, 1) != 256) { std::printf("pa_out\n"); return 1; }
    const int big[][2] = {{33, 70}, {4, 259}, {3, 66}};
    for (const auto &b : big)
        for (int slab_rows : {0, 1, 3})
            if (check_pool(b[0], b[1], 3, 2, 1) || check_pool(b[0], b[1], 2, 2, 0) || check_stem_staging(2, b[0], b[1], slab_rows)) return 1;
    std::printf("ok %ld\n", checks);
    return 0;
}
