// TEST INFRASTRUCTURE ONLY: the two forms of the polygon fill rule of csrc/polygon_fill.h compared on the host.
// lb_filled answers for one pixel (labels.hip paints with it), lb_filled_row32 for 32 pixels of a row (overlay.hip); bit c of
// the row form must equal the pixel form at column x0 + c.  tests/test_overlay.py compiles and runs this file; it prints
// "checked <pixels> differ <count>" and returns 1 when any pixel differs.
#include <cstdio>
#include <vector>

#include <hip/hip_runtime.h>

#include "../celldetection_amd/csrc/polygon_fill.h"

namespace {

long checked = 0, differ = 0;

void compare(const std::vector<int2> &p, int x0, int y) {
    const int S = (int) p.size();
    std::vector<int> px(S), py(S);
    for (int s = 0; s < S; ++s) { px[s] = p[s].x; py[s] = p[s].y; }
    const unsigned int m = lb_filled_row32(x0, y, p.data(), S);
    for (int c = 0; c < 32; ++c) {
        const bool f = lb_filled(x0 + c, y, px.data(), py.data(), S);
        ++checked;
        if (f != ((m >> c & 1u) != 0u)) {
            if (differ < 5) std::printf("differs: S %d row %d window %d column %d pixel form %d\n", S, y, x0, c, (int) f);
            ++differ;
        }
    }
}

unsigned int state = 12345u;
int rnd(int n) {  // a small generator of its own: the same cases everywhere
    state = state * 1664525u + 1013904223u;
    return (int) ((state >> 8) % (unsigned int) n);
}

}  // namespace

int main() {
    // window edges: a crossing on column 30, 31 and 32 of the window, left of it and far right of it; S = 1 and 2
    const std::vector<int2> tri = {{40, 2}, {71, 30}, {35, 34}}, quad = {{3, 3}, {90, 5}, {88, 40}, {1, 37}};
    for (const auto &poly : {tri, quad})
        for (int y = 0; y < 44; ++y)
            for (int x0 = -40; x0 <= 100; ++x0) compare(poly, x0, y);
    for (int x = 0; x < 70; ++x) {  // vertical edges: the crossing sits on column x - x0 = 29 .. 33 and -2 .. 1
        const std::vector<int2> box = {{x, 1}, {x + 5, 1}, {x + 5, 9}, {x, 9}};
        for (int y = 0; y < 11; ++y)
            for (int x0 : {x - 33, x - 32, x - 31, x - 30, x - 29, x - 1, x, x + 1, x + 2}) compare(box, x0, y);
    }
    for (int x0 = -35; x0 < 10; ++x0)
        for (int y = 3; y < 8; ++y) {
            compare({{5, 5}}, x0, y);            // a point
            compare({{5, 5}, {5, 5}}, x0, y);    // a repeated point (the padding of a list)
            compare({{2, 4}, {9, 6}}, x0, y);    // a line
        }
    // random polygons, with repeated points, over windows inside, across and outside
    for (int it = 0; it < 3000; ++it) {
        const int S = 1 + rnd(12), R = it % 3 == 0 ? 200 : 40;
        std::vector<int2> p(S);
        for (int s = 0; s < S; ++s) {
            p[s].x = rnd(R); p[s].y = rnd(R);
            if (s && rnd(5) == 0) p[s] = p[s - 1];
        }
        for (int y = -2; y < R + 2; y += R > 100 ? 7 : 1)
            for (int x0 = -40; x0 < R + 10; x0 += 13) compare(p, x0, y);
    }
    std::printf("checked %ld differ %ld\n", checked, differ);
    return differ != 0;
}
