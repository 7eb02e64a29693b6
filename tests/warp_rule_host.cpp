// Host build of csrc/warp_rule.h (the index and weight arithmetic of the augmentation warp) against brute force, meant to run under
// AddressSanitizer and UBSan: a conversion of an out-of-range double to an integer is undefined behaviour, which UBSan reports, so
// this is the check that every index is tested or reduced in fp64 BEFORE it becomes an integer.  Prints "ok <checks>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../celldetection_amd/csrc/warp_rule.h"

static long checks = 0;
#define EXPECT(cond)                                                    \
    do {                                                                \
        ++checks;                                                       \
        if (!(cond)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

// reflect-101 by walking: one step at a time from 0, turning at 0 and n - 1
static int walk_reflect(long i, int n) {
    if (n == 1) return 0;
    int pos = 0, dir = 1;
    for (long s = 0, steps = i < 0 ? -i : i; s < steps; ++s) {
        if (pos + dir < 0 || pos + dir > n - 1) dir = -dir;
        pos += dir;
    }
    return pos;  // (symmetric about 0, so the sign of i does not matter)
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int sizes[] = {1, 2, 3, 5, 32, 131};
    for (int n : sizes) {
        for (long i = -5 * n - 7; i <= 5 * n + 7; ++i) {
            EXPECT(wr_reflect((double) i, n) == walk_reflect(i, n));
            EXPECT(wr_index((double) i, n, WR_REFLECT) == walk_reflect(i, n));
            EXPECT(wr_index((double) i, n, WR_CONSTANT) == (i >= 0 && i < n ? (int) i : -1));
        }
        const double wild[] = {nan, inf, -inf, 1e300, -1e300, 2147483648.0, -2147483648.0, 2147483649.0, 4294967296.0, 9.3e18, -9.3e18,
                               1073741824.0, -1073741825.0, -0.0};
        for (double f : wild) {
            const int r = wr_index(f, n, WR_REFLECT), c = wr_index(f, n, WR_CONSTANT);
            EXPECT(r >= 0 && r < n);
            EXPECT(c == (f == 0.0 ? 0 : -1) || (f >= 0.0 && f <= n - 1 && c == (int) f));
        }
        EXPECT(wr_index(nan, n, WR_REFLECT) == 0 && wr_index(inf, n, WR_REFLECT) == 0 && wr_index(3e9, n, WR_REFLECT) == 0);
    }
    // any bit pattern read as a double, floored: an index in range, or the fill
    for (int t = 0; t < 200000; ++t) {
        const uint64_t bits = rng();
        double s;
        std::memcpy(&s, &bits, 8);
        if (t & 1) s = (double) (int64_t) (bits >> 20) * 1e-3 - 4e9;  // also plain magnitudes around the source
        const int n = sizes[t % 6];
        float l;
        const double f = wr_floor(s, &l), nn = wr_nearest(s);
        for (double g : {f, f + 1.0, nn}) {
            const int r = wr_index(g, n, WR_REFLECT), c = wr_index(g, n, WR_CONSTANT);
            EXPECT(r >= 0 && r < n && c >= -1 && c < n);
        }
        if (std::isfinite(s)) EXPECT(l >= 0.f && l <= 1.f && f <= s && (s - f) <= 1.0 && nn >= s - 0.5 && nn <= s + 0.5);
    }
    // halves round up; the weight of an integer position is 0
    float l;
    EXPECT(wr_nearest(-0.5) == 0.0 && wr_nearest(0.5) == 1.0 && wr_nearest(-1.5) == -1.0 && wr_nearest(2.4999) == 2.0);
    EXPECT(wr_floor(-3.0, &l) == -3.0 && l == 0.f);
    EXPECT(wr_floor(-2.75, &l) == -3.0 && l == 0.25f);
    // the position: products and sums in the stated order
    const double m[6] = {0.1, 0.7, -3.3, 1e-3, 2.5, 1e6};
    double sx, sy;
    wr_position(m, 7, 11, &sx, &sy);
    {
        volatile double a = m[0] * 11.0, b = m[1] * 7.0, c = a + b, d = m[3] * 11.0, e = m[4] * 7.0, g = d + e;
        EXPECT(sx == c + m[2] && sy == g + m[5]);
    }
    // the blend: exact at weights 0 and 1, the stated order elsewhere
    EXPECT(wr_blend(3.f, 5.f, 7.f, 11.f, 0.f, 0.f) == 3.f && wr_blend(3.f, 5.f, 7.f, 11.f, 0.f, 1.f) == 5.f);
    EXPECT(wr_blend(3.f, 5.f, 7.f, 11.f, 1.f, 0.f) == 7.f && wr_blend(3.f, 5.f, 7.f, 11.f, 1.f, 1.f) == 11.f);
    {
        const float ly = 0.3f, lx = 0.7f, hy = 1.0f - ly, hx = 1.0f - lx;
        volatile float p0 = hx * 0.1f, p1 = lx * 0.2f, s0 = p0 + p1, p2 = hx * 0.3f, p3 = lx * 0.4f, s1 = p2 + p3, q0 = hy * s0, q1 = ly * s1;
        EXPECT(wr_blend(0.1f, 0.2f, 0.3f, 0.4f, ly, lx) == q0 + q1);
    }
    // bf16: to nearest, ties to even, overflow to infinity, NaN stays NaN
    EXPECT(wr_bf16(1.0f) == 0x3f80 && wr_bf16(-2.0f) == 0xc000 && wr_bf16(0.f) == 0 && wr_bf16(-0.f) == 0x8000);
    EXPECT(wr_bf16(1.00390625f) == 0x3f80 && wr_bf16(1.01171875f) == 0x3f82 && wr_bf16(1.0039064f) == 0x3f81);
    EXPECT(wr_bf16(3.4e38f) == 0x7f80 && wr_bf16((float) inf) == 0x7f80 && (wr_bf16((float) nan) & 0x7fff) > 0x7f80);
    for (int t = 0; t < 100000; ++t) {
        const uint32_t bits = (uint32_t) rng();
        float v;
        std::memcpy(&v, &bits, 4);
        if (std::isnan(v)) continue;
        const uint32_t lo = bits & 0xffff0000u, hi = lo + 0x10000u;  // the two neighbours (in magnitude)
        const uint32_t got = (uint32_t) wr_bf16(v) << 16;
        float a, b;
        std::memcpy(&a, &lo, 4), std::memcpy(&b, &hi, 4);
        const double da = std::fabs((double) v - (double) a), db = std::isinf(b) ? std::fabs((double) v - std::ldexp(v < 0 ? -1.0 : 1.0, 128)) : std::fabs((double) v - (double) b);
        EXPECT(got == (da < db ? lo : db < da ? hi : (lo & 0x10000u) ? hi : lo));
    }
    std::printf("ok %ld\n", checks);
    return 0;
}
