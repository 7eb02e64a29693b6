// Host build of csrc/optim_chunks.h against brute force: the chunks of a tensor and of a list, the lane mapping of a chunk in both
// vector widths, the final sum's runs, the launch grid and the alignment-flag rule.  A program of its own (tests/test_optim.py
// compiles it with AddressSanitizer and UBSan on the host code and runs it; nothing is preloaded).  Prints "ok <checks>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../celldetection_amd/csrc/optim_chunks.h"

static long long checks = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        ++checks;                                                           \
        if (!(cond)) {                                                      \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static void check_tensor(int64_t numel) {
    const int64_t chunks = opt_chunks(numel);
    CHECK(chunks == (numel + OPT_CHUNK - 1) / OPT_CHUNK && (numel > 0) == (chunks > 0));
    int64_t covered = 0;
    for (int64_t k = 0; k < chunks; ++k) {
        const int32_t c = opt_chunk_count(numel, k);
        CHECK(c >= 1 && c <= OPT_CHUNK && (c == OPT_CHUNK || k == chunks - 1));
        covered += c;
    }
    CHECK(covered == numel);
    CHECK(opt_chunk_count(numel, chunks) == 0 && opt_chunk_count(numel, chunks + 5) == 0);
    CHECK(opt_tail(numel) == (numel == 0 ? 0 : (int32_t) (numel - (chunks - 1) * OPT_CHUNK)));
}

// every element of a chunk of `count` elements belongs to exactly one (lane, item, position), in ascending order within a lane
static void check_lanes(int32_t count, int32_t vec) {
    std::vector<int> seen(count, 0);
    const int32_t items = opt_items(count, vec);
    CHECK((int64_t) items * OPT_LANES * vec >= count && (int64_t) (items - 1) * OPT_LANES * vec < count);
    for (int32_t lane = 0; lane < OPT_LANES; ++lane) {
        int32_t last = -1;
        for (int32_t item = 0; item < items; ++item) {
            const int32_t e0 = opt_item_first(item, lane, vec), ne = opt_item_elements(count, item, lane, vec);
            CHECK(ne >= 0 && ne <= vec && e0 % vec == 0 && (e0 / vec) % OPT_LANES == lane && e0 / vec / OPT_LANES == item);
            for (int32_t j = 0; j < ne; ++j) {
                CHECK(e0 + j < count && e0 + j > last);
                last = e0 + j;
                ++seen[e0 + j];
            }
            if (ne < vec) CHECK(e0 + ne >= count);  // a partial or empty item ends the chunk
        }
        CHECK(opt_item_elements(count, items, lane, vec) == 0);
    }
    for (int32_t e = 0; e < count; ++e) CHECK(seen[e] == 1);
}

static void check_list(const std::vector<int64_t> &numel) {
    const int32_t n = (int32_t) numel.size();
    const int64_t chunks = opt_total_chunks(numel.data(), n);
    int64_t want = 0;
    for (int64_t v : numel) want += (v + OPT_CHUNK - 1) / OPT_CHUNK;
    CHECK(chunks == want);
    std::vector<int32_t> map(2 * chunks + 2, -7);  // (one guard record behind the map)
    opt_fill_map(numel.data(), n, map.data());
    CHECK(map[2 * chunks] == -7 && map[2 * chunks + 1] == -7);
    // ordered (tensor, then chunk), disjoint, and covering every element of every tensor exactly once
    std::vector<int64_t> covered(n, 0);
    int32_t pt = -1, pk = -1;
    for (int64_t c = 0; c < chunks; ++c) {
        const int32_t t = map[2 * c], k = map[2 * c + 1];
        CHECK(t >= 0 && t < n && k >= 0 && k < opt_chunks(numel[t]));
        CHECK(t > pt ? k == 0 : (t == pt && k == pk + 1));
        CHECK(covered[t] == (int64_t) k * OPT_CHUNK);
        covered[t] += opt_chunk_count(numel[t], k);
        pt = t, pk = k;
    }
    for (int32_t t = 0; t < n; ++t) CHECK(covered[t] == numel[t]);
    // the launch grid and the final sum's runs
    const int32_t grid = opt_grid(chunks);
    CHECK(grid >= 1 && grid <= OPT_MAX_GRID && (chunks <= OPT_MAX_GRID ? grid == (chunks < 1 ? 1 : chunks) : grid == OPT_MAX_GRID));
    const int64_t per = opt_final_per(chunks);
    int64_t next = 0;
    for (int32_t l = 0; l < OPT_LANES; ++l) {
        int64_t b = l * per, e = (l + 1) * per;
        if (e > chunks) e = chunks;
        for (int64_t i = b; i < e; ++i) CHECK(i == next++);
    }
    CHECK(next == chunks && opt_sum_chain(chunks) >= OPT_CHUNK / OPT_LANES + per);
}

int main() {
    const int64_t C = OPT_CHUNK;
    CHECK(C % (OPT_LANES * 8) == 0 && opt_vec(OPT_F32) == 4 && opt_vec(OPT_BF16) == 8);
    for (int64_t numel = 0; numel <= 3 * C + 9; ++numel) check_tensor(numel);
    for (int64_t numel : {(int64_t) 1 << 31, ((int64_t) 1 << 31) + 1, ((int64_t) 1 << 40) - 1, (int64_t) OPT_MAX_CHUNKS * C}) check_tensor(numel);
    for (int32_t vec : {4, 8}) {
        for (int32_t count = 1; count <= 3 * OPT_LANES * vec + 9; ++count) check_lanes(count, vec);
        for (int32_t count : {(int32_t) C - 2 * vec - 1, (int32_t) C - vec, (int32_t) C - 1, (int32_t) C}) check_lanes(count, vec);
    }
    check_list({});
    check_list({0});
    check_list({0, 0, 1, 0});
    check_list({1, 3, 4, 5, 8, 33, C - 1, C, C + 1, 2 * C + 3});
    check_list(std::vector<int64_t>(300, 32));
    check_list(std::vector<int64_t>(3000, C + 1));  // more chunks than the grid
    uint64_t seed = 12345;
    for (int round = 0; round < 200; ++round) {
        std::vector<int64_t> sizes;
        for (int i = 0, n = 1 + (int) (seed % 40); i < n; ++i) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            const uint64_t r = seed >> 33;
            sizes.push_back(r % 5 == 0 ? 0 : (r % 7 == 0 ? (int64_t) (r % (6 * C)) : (int64_t) (r % 300)));
        }
        check_list(sizes);
    }
    {  // what the total refuses
        const int64_t negative[2] = {5, -1}, huge[2] = {(int64_t) OPT_MAX_CHUNKS * C, 1}, most[1] = {(int64_t) OPT_MAX_CHUNKS * C};
        const int64_t beyond[1] = {(int64_t) OPT_MAX_CHUNKS * C + 1};
        CHECK(opt_total_chunks(negative, 2) == -1 && opt_total_chunks(huge, 2) == -1 && opt_total_chunks(beyond, 1) == -1);
        CHECK(opt_total_chunks(most, 1) == OPT_MAX_CHUNKS);
    }
    // the alignment rule: flagged exactly when an address that is used (non-zero) is not a multiple of 16
    const uint64_t base = 0x7f0000001000ull;
    for (uint64_t a = 0; a < 32; a += 2)
        for (uint64_t b = 0; b < 32; b += 2)
            for (uint64_t c = 0; c < 32; c += 4)
                for (uint64_t d = 0; d < 32; d += 4) {
                    const bool odd = (a % 16) || (b % 16) || (c % 16) || (d % 16);
                    CHECK(opt_flags(base + a, base + b, base + c, base + d) == (odd ? OPT_FLAG_SCALAR : 0));
                    CHECK(opt_flags(0, base + b, 0, 0) == ((b % 16) ? OPT_FLAG_SCALAR : 0));
                }
    printf("ok %lld\n", checks);
    return 0;
}
