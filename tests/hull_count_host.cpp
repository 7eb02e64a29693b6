// csrc/hull_count.h on the host (tests/test_shape_props.py builds this host program with AddressSanitizer and UBSan and runs it):
//   hull_count_host all4x4:      every one of the 65536 masks of 4 x 4 against brute force.  Output: "ok <masks>" or the first
//                                mask that differs.
//   hull_count_host file <path>: "<masks>", then per mask "<h> <w>" and h * w values (0 / 1).  Output per mask: "<count> <brute>"
//                                (brute = -1 when the mask has more than 1500 hull candidates and brute force is skipped).
// Brute force: S = the diamond points of all pixels in doubled coordinates.  An ordered pair (a, b) of S supports the hull when
// no point of S lies on its right; a lattice point is in the closed hull when it lies on the right of no supporting pair (S is
// never collinear: one pixel already gives a diamond).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../celldetection_amd/csrc/hull_count.h"

struct Pt { int64_t y, x; };

static int64_t cross(const Pt &a, const Pt &b, const Pt &p) { return (b.y - a.y) * (p.x - a.x) - (b.x - a.x) * (p.y - a.y); }

static int64_t brute(const std::vector<int> &m, int h, int w) {
    std::vector<Pt> S;
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c)
            if (m[r * w + c]) {
                S.push_back({2 * r - 1, 2 * c}); S.push_back({2 * r + 1, 2 * c});
                S.push_back({2 * r, 2 * c - 1}); S.push_back({2 * r, 2 * c + 1});
            }
    if (S.empty()) return 0;
    if (S.size() > 1500) return -1;
    std::vector<std::pair<Pt, Pt>> support;
    for (const Pt &a : S)
        for (const Pt &b : S) {
            if (a.y == b.y && a.x == b.x) continue;
            bool ok = true;
            for (const Pt &q : S)
                if (cross(a, b, q) < 0) { ok = false; break; }
            if (ok) support.push_back({a, b});
        }
    int64_t n = 0;
    for (int r = -1; r <= h; ++r)
        for (int c = -1; c <= w; ++c) {
            const Pt p = {2 * r, 2 * c};
            bool in = true;
            for (const auto &e : support)
                if (cross(e.first, e.second, p) < 0) { in = false; break; }
            n += in;
        }
    return n;
}

// the extents as the shape pass leaves them, over the rows of the bounding box
static int64_t by_header(const std::vector<int> &m, int h, int w) {
    int r0 = h, r1 = -1;
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c)
            if (m[r * w + c]) { if (r < r0) r0 = r; if (r > r1) r1 = r; }
    if (r1 < 0) return 0;
    const int rows = r1 - r0 + 1;
    std::vector<uint32_t> lo(rows, 0), hi(rows, 0);
    for (int r = r0; r <= r1; ++r)
        for (int c = 0; c < w; ++c)
            if (m[r * w + c]) {
                if (lo[r - r0] == 0) lo[r - r0] = 65536u - (uint32_t) c;
                hi[r - r0] = (uint32_t) c + 1u;
            }
    std::vector<int32_t> stack(2 * (2 * rows + 1));
    return hull_count(lo.data(), hi.data(), rows, stack.data());
}

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "all4x4") {
        std::vector<int> m(16);
        for (int bits = 0; bits < 65536; ++bits) {
            for (int i = 0; i < 16; ++i) m[i] = (bits >> i) & 1;
            const int64_t a = by_header(m, 4, 4), b = brute(m, 4, 4);
            if (a != b) {
                std::printf("mask %d: hull_count %lld, brute force %lld\n", bits, (long long) a, (long long) b);
                return 1;
            }
        }
        std::printf("ok 65536\n");
        return 0;
    }
    if (argc == 3 && std::string(argv[1]) == "file") {
        FILE *f = std::fopen(argv[2], "r");
        int masks = 0;
        if (!f || std::fscanf(f, "%d", &masks) != 1) return 2;
        for (int k = 0; k < masks; ++k) {
            int h = 0, w = 0;
            if (std::fscanf(f, "%d %d", &h, &w) != 2 || h < 1 || w < 1 || h > 4096 || w > 4096) return 2;
            std::vector<int> m((size_t) h * w);
            for (int &v : m)
                if (std::fscanf(f, "%d", &v) != 1) return 2;
            std::printf("%lld %lld\n", (long long) by_header(m, h, w), (long long) brute(m, h, w));
        }
        std::fclose(f);
        return 0;
    }
    return 2;
}
