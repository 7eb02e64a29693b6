// csrc/bn_slabs.h on the host (tests/test_batch_norm.py builds this host program with AddressSanitizer and UBSan and runs it): the
// slab partition and the lane mapping of the batch-norm kernels against brute force, for every M <= 4096, every V in 1 ... 256 and
// C in {2056, 4096} (V = 257: two channel blocks of 256 and 1 vectors; V = 512: two full ones) and slab_pixels in {0, 1, 3, 64}
// (0 = auto, with 1, 7 and 2048 slabs wanted).
//
// A workgroup owns (pixels of its slab) x (vectors of its block), and a lane of it (its pixel row) x (its vector).  "Every (pixel,
// vector) is owned exactly once" is therefore four statements, each counted one by one over everything it depends on:
//   1. lanes:   for every block size vb in 1 ... 256 the active lanes map one to one onto [0, R) x [0, vb), idle lanes own nothing;
//   2. rows:    for every slab length <= 4096 and every R that occurs, the rows' walks p = row, row + R, ... cover the slab's pixels
//               once; the terms per row, the longest walk and the rows that hold a pixel are the header's closed forms;
//   3. slabs:   for every (M, slab_pixels) the slabs are in ascending order, none is empty, together they are [0, M);
//   4. blocks:  for every V the blocks' vectors are [0, V) once.
// Then, for every (M, V, slab_pixels), the chain the header reports is the counted one: longest walk + rows holding a pixel + slabs
// + BNS_FINALISE_OPS, the longest over the blocks, never above M + slabs + 8.
// As a check of that decomposition itself, a subset of the cases (every M <= 24 with every V, larger M with a few V) is also walked
// whole, workgroup by workgroup and lane by lane as the kernels do, into one counter per (pixel, vector).
// Output: "ok <cases>" or the first difference.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../celldetection_amd/csrc/bn_slabs.h"

constexpr int MAX_M = 4096;
static int r_index[BNS_LANES + 1];                 // R -> index among the values of R that occur, or -1
static std::vector<int> r_values;
static std::vector<int32_t> walk_longest, walk_rows;  // [slab length][index of R]: counted

static int check_lanes() {
    for (int vb = 1; vb <= BNS_LANES; ++vb) {
        const int R = bns_rows(vb);
        if (R < 1 || R * vb > BNS_LANES || (R + 1) * vb <= BNS_LANES) return std::printf("vb %d: R %d\n", vb, R), 1;
        std::vector<int> owned((size_t) R * vb, 0);
        for (int lane = 0; lane < BNS_LANES; ++lane) {
            int32_t row, vec;
            const bool active = bns_lane(vb, lane, &row, &vec);
            if (active != (lane < R * vb)) return std::printf("vb %d lane %d: active %d\n", vb, lane, (int) active), 1;
            if (!active) continue;
            if (row < 0 || row >= R || vec < 0 || vec >= vb || row * vb + vec != lane) return std::printf("vb %d lane %d -> (%d, %d)\n", vb, lane, row, vec), 1;
            owned[(size_t) row * vb + vec] += 1;
        }
        for (int o : owned)
            if (o != 1) return std::printf("vb %d: a (row, vector) owned %d times\n", vb, o), 1;
        if (r_index[R] < 0) {
            r_index[R] = (int) r_values.size();
            r_values.push_back(R);
        }
    }
    return 0;
}

static int check_rows() {
    const size_t nr = r_values.size();
    walk_longest.assign((size_t) (MAX_M + 1) * nr, 0);
    walk_rows.assign((size_t) (MAX_M + 1) * nr, 0);
    std::vector<uint8_t> seen;
    for (int len = 1; len <= MAX_M; ++len)
        for (size_t k = 0; k < nr; ++k) {
            const int R = r_values[k], vb = BNS_LANES / R;  // (a block size with this R: 256 / (256 / R) == R for every R that occurs)
            if (bns_rows(vb) != R) return std::printf("R %d: no block size\n", R), 1;
            seen.assign((size_t) len, 0);
            int32_t longest = 0, rows = 0;
            for (int row = 0; row < R; ++row) {
                int32_t n = 0;
                for (int64_t p = row; p < len; p += R, ++n) seen[(size_t) p] += 1;
                if (n != bns_lane_terms(len, vb, row)) return std::printf("len %d R %d row %d: %d terms, header %ld\n", len, R, row, n, (long) bns_lane_terms(len, vb, row)), 1;
                if (n > longest) longest = n;
                if (n > 0) ++rows;
            }
            for (uint8_t s : seen)
                if (s != 1) return std::printf("len %d R %d: a pixel owned %d times\n", len, R, (int) s), 1;
            if (longest != bns_steps(len, vb) || rows != bns_partials(len, vb)) return std::printf("len %d R %d: %d steps, %d rows\n", len, R, longest, rows), 1;
            walk_longest[(size_t) len * nr + k] = longest;
            walk_rows[(size_t) len * nr + k] = rows;
        }
    return 0;
}

#define FAIL(...)                                                                                                  \
    do {                                                                                                           \
        std::printf("M %ld V %d slab_pixels %d slabs wanted %d: ", (long) M, V, requested, wanted);                \
        std::printf(__VA_ARGS__);                                                                                  \
        std::printf("\n");                                                                                         \
        return 1;                                                                                                  \
    } while (0)

static int check_slabs(int64_t M, int32_t requested, int32_t wanted) {
    const int32_t V = 1;
    const BnSlabs s = bns_partition(M, V, requested, wanted);
    if (s.slab_pixels < 1 || s.slabs < 1) FAIL("slab_pixels %d slabs %d", s.slab_pixels, s.slabs);
    if (requested > 0 && s.slab_pixels != (requested < M ? requested : (int32_t) M)) FAIL("slab_pixels %d", s.slab_pixels);
    if (requested == 0 && (s.slabs > wanted || (s.slab_pixels < BNS_MIN_SLAB && s.slab_pixels != M))) FAIL("%d slabs of %d pixels", s.slabs, s.slab_pixels);
    int64_t next = 0;
    for (int32_t i = 0; i < s.slabs; ++i) {
        int64_t p0, p1;
        bns_range(s, i, &p0, &p1);
        if (p0 != next || p1 <= p0 || p1 > M) FAIL("slab %d covers [%ld, %ld), expected to start at %ld", i, (long) p0, (long) p1, (long) next);
        if (p1 - p0 != (i + 1 < s.slabs ? s.slab_pixels : M - (int64_t) (s.slabs - 1) * s.slab_pixels)) FAIL("slab %d holds %ld pixels", i, (long) (p1 - p0));
        next = p1;
    }
    if (next != M) FAIL("the slabs end at %ld", (long) next);
    return 0;
}

static int check_case(int64_t M, int32_t V, int32_t requested, int32_t wanted, bool walk) {
    const BnSlabs s = bns_partition(M, V, requested, wanted), s1 = bns_partition(M, 1, requested, wanted);
    if (s.slab_pixels != s1.slab_pixels || s.slabs != s1.slabs || s.M != M || s.V != V) FAIL("the slabs depend on V");
    if (s.blocks != (V + BNS_LANES - 1) / BNS_LANES) FAIL("%d blocks", s.blocks);
    int32_t vectors = 0;
    int64_t longest = 0;
    const size_t nr = r_values.size();
    for (int32_t b = 0; b < s.blocks; ++b) {
        const int32_t vb = bns_block_vectors(s, b);
        if (vb < 1 || vb > BNS_LANES || (b + 1 < s.blocks && vb != BNS_LANES)) FAIL("block %d: %d vectors", b, vb);
        vectors += vb;
        const size_t e = (size_t) s.slab_pixels * nr + (size_t) r_index[bns_rows(vb)];
        const int64_t chain = (int64_t) walk_longest[e] + walk_rows[e] + s.slabs;
        if (chain != bns_sum_chain(s, b) || chain + BNS_FINALISE_OPS != bns_chain(s, b) || chain > M + 1 + s.slabs) FAIL("block %d: chain %ld, header %ld", b, (long) chain, (long) bns_sum_chain(s, b));
        if (chain > longest) longest = chain;
    }
    if (vectors != V) FAIL("the blocks hold %d vectors", vectors);
    if (bns_chain_max(s) != longest + BNS_FINALISE_OPS || bns_chain_max(s) > M + s.slabs + 8) FAIL("chain %ld, counted %ld", (long) bns_chain_max(s), (long) longest);
    if (!walk) return 0;
    std::vector<uint8_t> seen((size_t) (M * V), 0);
    for (int32_t i = 0; i < s.slabs; ++i) {
        int64_t p0, p1;
        bns_range(s, i, &p0, &p1);
        for (int32_t b = 0; b < s.blocks; ++b) {
            const int32_t vb = bns_block_vectors(s, b), R = bns_rows(vb);
            for (int32_t lane = 0; lane < BNS_LANES; ++lane) {
                int32_t row, vec;
                if (!bns_lane(vb, lane, &row, &vec)) continue;
                for (int64_t p = p0 + row; p < p1; p += R) {
                    const int64_t v = (int64_t) b * BNS_LANES + vec;  // the kernel's channel offset / 8
                    if (v >= V) FAIL("vector %ld", (long) v);
                    if (++seen[(size_t) (p * V + v)] != 1) FAIL("pixel %ld vector %ld owned twice", (long) p, (long) v);
                }
            }
        }
    }
    for (size_t e = 0; e < seen.size(); ++e)
        if (seen[e] != 1) FAIL("pixel %ld vector %ld owned %d times", (long) (e / V), (long) (e % V), (int) seen[e]);
    return 0;
}

int main() {
    static_assert(BNS_LANES == 256 && BNS_VEC == 8, "a workgroup of 256 lanes, 16 B of bf16 per lane");
    for (int &r : r_index) r = -1;
    if (check_lanes() || check_rows()) return 1;
    const int32_t requested[] = {0, 1, 3, 64}, wanted[] = {1, 7, 2048};
    const int64_t walk_m[] = {97, 127, 128, 129, 255, 256, 257, 511, 1000, 2048, 4095, 4096};
    const int32_t walk_v[] = {1, 3, 8, 85, 86, 128, 129, 256, 257, 512};
    long cases = 0;
    for (int64_t M = 1; M <= MAX_M; ++M) {
        bool listed = false;
        for (int64_t w : walk_m) listed = listed || w == M;
        for (int32_t r : requested)
            for (int32_t g : wanted) {
                if (r != 0 && g != wanted[0]) continue;  // (a forced slab_pixels does not look at the slabs wanted)
                if (check_slabs(M, r, g)) return 1;
                for (int32_t vi = 1; vi <= 258; ++vi) {
                    const int32_t V = vi <= 256 ? vi : (vi == 257 ? 2056 / 8 : 4096 / 8);
                    bool few = false;
                    for (int32_t w : walk_v) few = few || w == V;
                    if (check_case(M, V, r, g, M <= 24 || (few && (M <= 96 || (listed && g == wanted[0]))))) return 1;
                    ++cases;
                }
            }
    }
    // the largest arguments the launch accepts: no overflow on the way
    const int64_t big[][3] = {{0x7fffffffll, 1, 0}, {0x7fffffffll, 1, 1}, {0x7fffffffll, 65535 * 256, 0x7fffffffll}, {0x7fffffffll, 257, 3}};
    for (const auto &b : big) {
        const BnSlabs s = bns_partition(b[0], (int32_t) b[1], (int32_t) b[2], 2048);
        int64_t p0, p1;
        bns_range(s, s.slabs - 1, &p0, &p1);
        if (s.slabs < 1 || p1 != b[0] || p0 >= p1 || bns_chain_max(s) < 3 || bns_chain_max(s) > b[0] + s.slabs + 8) {
            std::printf("M %ld V %ld: the last slab ends at %ld\n", (long) b[0], (long) b[1], (long) p1);
            return 1;
        }
    }
    std::printf("ok %ld\n", cases);
    return 0;
}
