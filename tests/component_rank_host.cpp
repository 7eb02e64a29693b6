// csrc/component_rank.h on the host (tests/test_components.py builds this host program with AddressSanitizer and UBSan and runs
// it): the rank of a root inside its block of 256 pixels, as the numbering kernels of csrc/components.hip compute it from the
// four wave ballots, against brute force (counting the roots before the pixel one by one).
//   - every one of the 65536 masks of 16 root flags, the flags spread over the block so that they sit on both sides of every wave
//     boundary and at both ends of the block; every pixel of the block is asked for its rank, root or not;
//   - 2000 seeded random blocks, among them the empty, the full and the checkerboard block;
//   - the encoding of a rank in a root's word at both ends of its range.
// Output: "ok <masks> <blocks>" or the first difference.
#include <cstdint>
#include <cstdio>

#include "../celldetection_amd/csrc/component_rank.h"

static const int POS[16] = {0, 1, 31, 32, 62, 63, 64, 65, 127, 128, 129, 190, 191, 192, 254, 255};

static int check(const bool *flags, const char *what, long id) {
    uint64_t ballots[CR_WAVES] = {0, 0, 0, 0};
    for (int i = 0; i < CR_BLOCK; ++i)
        if (flags[i]) ballots[i >> 6] |= (uint64_t) 1 << (i & 63);
    int before = 0;
    for (int i = 0; i < CR_BLOCK; ++i) {
        const int got = cr_block_rank(ballots, i);
        if (got != before) {
            std::printf("%s %ld: pixel %d has rank %d, brute force %d\n", what, id, i, got, before);
            return 1;
        }
        before += flags[i];
    }
    if (cr_block_count(ballots) != before) {
        std::printf("%s %ld: count %d, brute force %d\n", what, id, cr_block_count(ballots), before);
        return 1;
    }
    return 0;
}

int main() {
    static_assert(CR_BLOCK == 256 && CR_WAVES == 4, "a block is four waves of 64 lanes");
    bool flags[CR_BLOCK];
    long masks = 0, blocks = 0;
    for (long m = 0; m < 65536; ++m, ++masks) {
        for (int i = 0; i < CR_BLOCK; ++i) flags[i] = false;
        for (int k = 0; k < 16; ++k) flags[POS[k]] = (m >> k) & 1;
        if (check(flags, "mask", m)) return 1;
    }
    uint64_t s = 0x9e3779b97f4a7c15ull;
    for (long b = 0; b < 2000; ++b, ++blocks) {
        for (int i = 0; i < CR_BLOCK; ++i) {
            s ^= s << 13; s ^= s >> 7; s ^= s << 17;  // xorshift64
            flags[i] = b == 0 ? false : b == 1 ? true : b == 2 ? (i & 1) : b == 3 ? !(i & 1) : (s >> 33) % 100 < (uint64_t) (b % 101);
        }
        if (check(flags, "block", b)) return 1;
    }
    const int64_t top = 0x7fffffffll - 1;  // the largest rank of 2^31 - 1 components
    if (cr_encode(0) != -2 || cr_decode(-2) != 0 || cr_decode(cr_encode(top)) != top || cr_encode(top) != INT32_MIN ||
        cr_decode(cr_encode(12345)) != 12345) {
        std::printf("encoding differs\n");
        return 1;
    }
    std::printf("ok %ld %ld\n", masks, blocks);
    return 0;
}
