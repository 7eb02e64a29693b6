// csrc/wgrad_slabs.h on the host (tests/test_conv_train.py builds this host program with AddressSanitizer and UBSan and runs it):
// the slab partition of the weight-gradient reduction against brute force, for every (rows = N * H, W) with rows * W <= 4096 and
// slab_rows in {0, 1, 2, 3, 8} (0 = auto, with 1, 7, 146 and 4096 slabs wanted):
//   - every pixel lies in exactly one slab, the slabs are in ascending order and none is empty;
//   - a slab holds slab_rows image rows, the last one what is left;
//   - the MFMA steps of a slab, counted one by one over its pixels (16 per step), are at most `steps`, and those of the first
//     slab are exactly `steps`;
//   - the chains: steps + 2 + slabs never exceeds ceil(rows * W / 16) + 2 + slabs; the bias chain counts its own adds.
// Output: "ok <partitions>" or the first difference.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../celldetection_amd/csrc/wgrad_slabs.h"

static int check(int64_t rows, int32_t W, int32_t requested, int32_t groups) {
    const WgSlabs s = wgs_partition(rows, W, requested, groups);
    const int64_t P = rows * W;
#define FAIL(...)                                                                      \
    do {                                                                               \
        std::printf("rows %ld W %d slab_rows %d slabs wanted %d: ", (long) rows, W, requested, groups); \
        std::printf(__VA_ARGS__);                                                      \
        std::printf("\n");                                                             \
        return 1;                                                                      \
    } while (0)
    if (s.slab_rows < 1 || s.slabs < 1) FAIL("slab_rows %d slabs %d", s.slab_rows, s.slabs);
    if (requested > 0 && s.slab_rows != (requested < rows ? requested : (int32_t) rows)) FAIL("slab_rows %d", s.slab_rows);
    if (requested == 0 && s.slabs > groups) FAIL("%d slabs, wanted at most %d", s.slabs, groups);
    std::vector<int> seen((size_t) P, 0);
    int64_t next = 0;
    for (int32_t i = 0; i < s.slabs; ++i) {
        int64_t p0, p1;
        wgs_range(s, i, &p0, &p1);
        if (p0 != next || p1 <= p0 || p1 > P) FAIL("slab %d covers [%ld, %ld), expected to start at %ld", i, (long) p0, (long) p1, (long) next);
        const int64_t want_rows = i + 1 < s.slabs ? s.slab_rows : rows - (int64_t) (s.slabs - 1) * s.slab_rows;
        if (p1 - p0 != want_rows * W) FAIL("slab %d holds %ld pixels, expected %ld rows", i, (long) (p1 - p0), (long) want_rows);
        int32_t steps = 0;
        for (int64_t p = p0; p < p1; ++p) {
            seen[(size_t) p] += 1;
            if ((p - p0) % WGS_STEP == 0) ++steps;
        }
        if (steps != wgs_steps(p1 - p0) || steps > s.steps || (i == 0 && steps != s.steps))
            FAIL("slab %d takes %d steps, header %d, largest %d", i, steps, wgs_steps(p1 - p0), s.steps);
        next = p1;
    }
    if (next != P) FAIL("the slabs end at %ld of %ld pixels", (long) next, (long) P);
    for (int64_t p = 0; p < P; ++p)
        if (seen[(size_t) p] != 1) FAIL("pixel %ld lies in %d slabs", (long) p, seen[(size_t) p]);
    if (wgs_chain(s) != s.steps + 2 + s.slabs || wgs_chain(s) > (P + 15) / 16 + 2 + s.slabs) FAIL("chain %ld", (long) wgs_chain(s));
    int64_t longest = 0;  // the bias gradient's interleaved chains of the first slab, counted one by one
    for (int c = 0; c < WGS_BIAS_LANES; ++c) {
        int64_t adds = 0;
        for (int64_t p = c; p < (int64_t) s.slab_rows * W; p += WGS_BIAS_LANES) ++adds;
        if (adds > longest) longest = adds;
    }
    if (wgs_bias_chain(s) != longest + WGS_BIAS_LANES + s.slabs) FAIL("bias chain %ld, counted %ld", (long) wgs_bias_chain(s), (long) longest);
    return 0;
#undef FAIL
}

int main() {
    static_assert(WGS_STEP == 16, "the bf16 MFMA reduces 16 pixels per step");
    const int32_t requested[] = {0, 1, 2, 3, 8}, groups[] = {1, 7, 146, 4096};
    long partitions = 0;
    for (int64_t rows = 1; rows <= 4096; ++rows)
        for (int32_t W = 1; rows * W <= 4096; ++W)
            for (int32_t r : requested)
                for (int32_t g : groups) {
                    if (r != 0 && g != groups[0]) continue;  // (a forced slab_rows does not look at the slabs wanted)
                    if (check(rows, W, r, g)) return 1;
                    ++partitions;
                }
    // the largest arguments the launch accepts: no overflow on the way
    const int64_t big[][3] = {{0x7fffffffll, 1, 0}, {1, 0x7fffffffll, 0}, {0x7fffffffll / 3, 3, 1 << 20}, {0x7fffffffll, 1, 1}};
    for (const auto &b : big) {
        const WgSlabs s = wgs_partition(b[0], (int32_t) b[1], (int32_t) b[2], 1);
        int64_t p0, p1;
        wgs_range(s, s.slabs - 1, &p0, &p1);
        if (s.slabs < 1 || p1 != b[0] * b[1] || p0 >= p1 || s.steps != wgs_steps((int64_t) s.slab_rows * s.W) || wgs_chain(s) < 3) {
            std::printf("rows %ld W %ld: the last slab ends at %ld\n", (long) b[0], (long) b[1], (long) p1);
            return 1;
        }
    }
    std::printf("ok %ld\n", partitions);
    return 0;
}
