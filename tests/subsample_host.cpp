// gc_subsample_source of csrc/grouped_conv.h on the host (tests/test_bottleneck.py builds this host program with AddressSanitizer and
// UBSan and runs it): for N <= 3, sizes up to 10 x 10 (even and odd), 1 to 3 vectors per pixel, against brute force:
//   - unit (n, i, j, c) of xs [N][Hout][Wout][C8] reads unit (n, 2 i, 2 j, c) of x [N][Hin][Win][C8], inside x (it indexes a real
//     buffer here, so a source outside it is an AddressSanitizer report);
//   - every unit of xs is produced once, the sources are distinct, and they are exactly the units of the even grid: the dilation's
//     non-zero units, gc_dilate_source being its inverse there.
// Output: "ok <checks>" or the first difference.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../celldetection_amd/csrc/grouped_conv.h"

int main() {
    long checks = 0;
    for (uint32_t N = 1; N <= 3; ++N)
        for (uint32_t H = 1; H <= 10; ++H)
            for (uint32_t W = 1; W <= 10; ++W)
                for (uint32_t C8 = 1; C8 <= 3; ++C8) {
                    const uint32_t Ho = (uint32_t) gc_out_size((int32_t) H, 2), Wo = (uint32_t) gc_out_size((int32_t) W, 2);
                    std::vector<int64_t> x((size_t) N * H * W * C8);
                    for (size_t i = 0; i < x.size(); ++i) x[i] = (int64_t) i;
                    std::vector<char> used(x.size(), 0);
                    const uint32_t total = N * Ho * Wo * C8;
                    uint32_t u = 0;
                    for (uint32_t n = 0; n < N; ++n)
                        for (uint32_t i = 0; i < Ho; ++i)
                            for (uint32_t j = 0; j < Wo; ++j)
                                for (uint32_t c = 0; c < C8; ++c, ++u) {
                                    const int64_t s = gc_subsample_source(u, H, W, C8, 2);
                                    const int64_t want = (((int64_t) n * H + 2 * i) * W + 2 * j) * C8 + c;
                                    if (s != want || x[(size_t) s] != want || used[(size_t) s]) {
                                        std::printf("N %u H %u W %u C8 %u unit %u: source %ld, expected %ld\n", N, H, W, C8, u, (long) s, (long) want);
                                        return 1;
                                    }
                                    used[(size_t) s] = 1;
                                    if (gc_dilate_source((uint32_t) s, H, W, C8) != (int64_t) u) {
                                        std::printf("N %u H %u W %u C8 %u unit %u: the dilation does not read it back\n", N, H, W, C8, u);
                                        return 1;
                                    }
                                    ++checks;
                                }
                    if (u != total) return 1;
                    for (size_t v = 0; v < x.size(); ++v)
                        if ((gc_dilate_source((uint32_t) v, H, W, C8) >= 0) != (used[v] != 0)) {
                            std::printf("N %u H %u W %u C8 %u: unit %zu of x is on one grid only\n", N, H, W, C8, v);
                            return 1;
                        }
                }
    std::printf("ok %ld\n", checks);
    return 0;
}
