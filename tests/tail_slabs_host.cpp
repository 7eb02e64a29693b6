// csrc/tail_slabs.h on the host (tests/test_readout_tail.py builds this host program with AddressSanitizer and UBSan and runs it):
// the partitions of the ReadOut-tail kernels against brute force, for every N <= 4, HW <= 2048 and slab_pixels in
// {0, 1, 3, 16, 130} (0 = auto, with 1 and 512 slabs wanted):
//   - every pixel (n, q) lies in exactly one slab, the slabs are in ascending (n, q) order and none is empty;
//   - no slab crosses an image: slab i belongs to image i / per_image and lies inside [0, HW);
//   - a slab holds slab_pixels pixels, the last one of an image what is left;
//   - the MFMA steps of a slab, counted one by one over its pixels (16 per step), are at most `steps`, those of the first slab
//     exactly `steps`; the chains count their own adds and steps + 2 + reduce chain <= ceil(N HW / 16) + 2 + slabs + 1;
//   - the forward tiles: every pixel in exactly one 32-pixel tile of exactly one workgroup, no tile crosses an image.
// Output: "ok <partitions>" or the first difference.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../celldetection_amd/csrc/tail_slabs.h"

static int check(int32_t N, int64_t HW, int64_t requested, int64_t wanted) {
    const TailSlabs s = tls_partition(N, HW, requested, wanted);
#define FAIL(...)                                                                                                         \
    do {                                                                                                                  \
        std::printf("N %d HW %ld slab_pixels %ld wanted %ld: ", N, (long) HW, (long) requested, (long) wanted);           \
        std::printf(__VA_ARGS__);                                                                                         \
        std::printf("\n");                                                                                                \
        return 1;                                                                                                         \
    } while (0)
    if (s.slab_pixels < 1 || s.slab_pixels > HW || s.per_image < 1 || s.slabs != s.per_image * N) FAIL("slab_pixels %ld slabs %ld", (long) s.slab_pixels, (long) s.slabs);
    if (requested > 0 && s.slab_pixels != (requested < HW ? requested : HW)) FAIL("slab_pixels %ld", (long) s.slab_pixels);
    if (requested == 0 && s.slab_pixels != HW && s.slab_pixels % TLS_MIN_SLAB) FAIL("auto slab of %ld pixels", (long) s.slab_pixels);
    if (requested == 0 && s.per_image > (wanted + N - 1) / N) FAIL("%ld slabs per image, wanted %ld in all", (long) s.per_image, (long) wanted);
    std::vector<int> seen((size_t) (N * HW), 0);
    int64_t next = 0;  // flat index n * HW + q the next slab must start at
    for (int64_t i = 0; i < s.slabs; ++i) {
        int32_t n;
        int64_t q0, q1;
        tls_range(s, i, &n, &q0, &q1);
        if (n != i / s.per_image || n < 0 || n >= N || q0 < 0 || q1 <= q0 || q1 > HW) FAIL("slab %ld: image %d [%ld, %ld)", (long) i, n, (long) q0, (long) q1);
        if (n * HW + q0 != next) FAIL("slab %ld starts at %ld, expected %ld", (long) i, (long) (n * HW + q0), (long) next);
        const bool last = (i + 1) % s.per_image == 0;
        if (q1 - q0 != (last ? HW - (s.per_image - 1) * s.slab_pixels : s.slab_pixels)) FAIL("slab %ld holds %ld pixels", (long) i, (long) (q1 - q0));
        int64_t steps = 0;
        for (int64_t q = q0; q < q1; ++q) {
            seen[(size_t) (n * HW + q)] += 1;
            if ((q - q0) % TLS_STEP == 0) ++steps;
        }
        if (steps != tls_steps(q1 - q0) || steps > s.steps || (i == 0 && steps != s.steps))
            FAIL("slab %ld takes %ld steps, header %ld, largest %ld", (long) i, (long) steps, (long) tls_steps(q1 - q0), (long) s.steps);
        next = n * HW + q1;
    }
    if (next != N * HW) FAIL("the slabs end at %ld of %ld pixels", (long) next, (long) (N * HW));
    for (int64_t p = 0; p < N * HW; ++p)
        if (seen[(size_t) p] != 1) FAIL("pixel %ld lies in %d slabs", (long) p, seen[(size_t) p]);
    if (tls_reduce_chain(s) != s.slabs + 1 || tls_chain(s) != s.steps + 2 + s.slabs + 1 ||
        tls_chain(s) > (N * HW + 15) / 16 + 2 + s.slabs + 1)
        FAIL("chain %ld", (long) tls_chain(s));
    int64_t longest = 0;  // the bias gradient's interleaved chains of the first slab, counted one by one
    for (int c = 0; c < TLS_BIAS_LANES; ++c) {
        int64_t adds = 0;
        for (int64_t q = c; q < s.slab_pixels; q += TLS_BIAS_LANES) ++adds;
        if (adds > longest) longest = adds;
    }
    if (tls_bias_chain(s) != longest + TLS_BIAS_LANES + s.slabs) FAIL("bias chain %ld, counted %ld", (long) tls_bias_chain(s), (long) longest);
    // ---- forward tiles
    const TailTiles t = tls_tiles(N, HW, wanted);
    if (t.per_image != (HW + 31) / 32 || t.group_tiles < 1 || t.group_tiles % 4 || t.groups < 1) FAIL("tiles %ld / %ld / %ld", (long) t.per_image, (long) t.group_tiles, (long) t.groups);
    std::vector<int> tiled((size_t) (N * HW), 0);
    for (int64_t grp = 0; grp < N * t.groups; ++grp) {
        int32_t n;
        int64_t t0, t1;
        tls_tile_range(t, grp, &n, &t0, &t1);
        if (n != grp / t.groups || n >= N || t0 < 0 || t1 <= t0 || t1 > t.per_image) FAIL("group %ld: image %d tiles [%ld, %ld)", (long) grp, n, (long) t0, (long) t1);
        for (int64_t tile = t0; tile < t1; ++tile)
            for (int64_t q = tile * TLS_TILE; q < tile * TLS_TILE + TLS_TILE && q < HW; ++q) tiled[(size_t) (n * HW + q)] += 1;
    }
    for (int64_t p = 0; p < N * HW; ++p)
        if (tiled[(size_t) p] != 1) FAIL("pixel %ld lies in %d tiles", (long) p, tiled[(size_t) p]);
    return 0;
#undef FAIL
}

int main() {
    static_assert(TLS_STEP == 16 && TLS_TILE == 32, "the bf16 MFMA reduces 16 pixels per step and holds 32 columns");
    const int64_t requested[] = {0, 1, 3, 16, 130}, wanted[] = {1, 512};
    long partitions = 0;
    for (int32_t N = 1; N <= 4; ++N)
        for (int64_t HW = 1; HW <= 2048; ++HW)
            for (int64_t r : requested)
                for (int64_t g : wanted) {
                    if (r != 0 && g != wanted[0]) continue;  // (a forced slab_pixels does not look at the slabs wanted)
                    if (check(N, HW, r, g)) return 1;
                    ++partitions;
                }
    // the largest arguments the launch accepts: no overflow on the way
    const int64_t big[][3] = {{1, 0x7fffffffll, 0}, {0x7fffffffll, 1, 0}, {3, 0x7fffffffll / 3, 1 << 20}, {1, 0x7fffffffll, 1}};
    for (const auto &b : big) {
        const TailSlabs s = tls_partition((int32_t) b[0], b[1], b[2], 512);
        int32_t n;
        int64_t q0, q1;
        tls_range(s, s.slabs - 1, &n, &q0, &q1);
        const TailTiles t = tls_tiles((int32_t) b[0], b[1], 1024);
        int64_t t0, t1;
        tls_tile_range(t, b[0] * t.groups - 1, &n, &t0, &t1);
        if (s.slabs < 1 || q1 != b[1] || q0 >= q1 || n != b[0] - 1 || s.steps != tls_steps(s.slab_pixels) || tls_chain(s) < 4 ||
            t1 != t.per_image || t0 >= t1) {
            std::printf("N %ld HW %ld: the last slab ends at %ld, the last tile at %ld\n", (long) b[0], (long) b[1], (long) q1, (long) t1);
            return 1;
        }
    }
    std::printf("ok %ld\n", partitions);
    return 0;
}
