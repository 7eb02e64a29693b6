// The rank of a root inside its block of CR_BLOCK pixels (csrc/components.hip: the numbering of components).  A block is
// CR_WAVES waves of 64 lanes; lane l of wave w owns pixel 64 * w + l of the block, and bit l of ballots[w] is set when that pixel
// is a root.  Integer arithmetic only; compiles for the device and for the host (tests/component_rank_host.cpp runs it against
// brute force under sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CR_HD __host__ __device__ __forceinline__
#else
#define CR_HD inline
#endif

constexpr int CR_WAVES = 4, CR_BLOCK = 64 * CR_WAVES;

CR_HD int cr_popcount(uint64_t m) { return __builtin_popcountll(m); }

// roots of the block
CR_HD int cr_block_count(const uint64_t *ballots) {
    int n = 0;
    for (int w = 0; w < CR_WAVES; ++w) n += cr_popcount(ballots[w]);
    return n;
}

// roots of the block before pixel `tid` (0 <= tid < CR_BLOCK)
CR_HD int cr_block_rank(const uint64_t *ballots, int tid) {
    const int wave = tid >> 6, lane = tid & 63;
    int n = cr_popcount(ballots[wave] & (((uint64_t) 1 << lane) - 1));  // lane <= 63: the shift is defined
    for (int w = 0; w < wave; ++w) n += cr_popcount(ballots[w]);
    return n;
}

// The word a root carries once it is numbered: -2 - rank, for 0 <= rank <= 2^31 - 2 (-1 stays "takes no part").
CR_HD int32_t cr_encode(int64_t rank) { return (int32_t) (-2 - rank); }
CR_HD int64_t cr_decode(int32_t word) { return -2 - (int64_t) word; }
