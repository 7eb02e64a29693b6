// Index and weight arithmetic of the augmentation warp (csrc/augment.hip): the "Augmentation warp" section of include/cpn_hip.h,
// function by function.  A destination pixel (row i, column j) maps to the source position (sx, sy) by six fp64 numbers; labels
// read the nearest source pixel, the image blends the four pixels around the position in fp32.  Every function clamps or tests
// in fp64 BEFORE a value becomes an integer, so no map -- NaN and infinities included -- can form an index outside [0, n).
// The arithmetic has one stated order of operations: every user compiles with -ffp-contract=off.  Compiles for the device and
// for the host (tests/warp_rule_host.cpp runs it against brute force under sanitizers).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WR_HD __host__ __device__ __forceinline__
#else
#define WR_HD inline
#endif

enum { WR_CONSTANT = 0, WR_REFLECT = 1 };  // CPN_AUGMENT_BORDER_*

// a coordinate further than this from the origin is outside the rule (the Python layer refuses a map that reaches 2^30): it
// counts as outside the source under WR_CONSTANT and reads index 0 under WR_REFLECT
#define WR_FAR 2147483648.0

// sx = (m0 * j + m1 * i) + m2,  sy = (m3 * j + m4 * i) + m5: two products, two sums each, all rounded to fp64
WR_HD void wr_position(const double *m, int i, int j, double *sx, double *sy) {
    const double x = (double) j, y = (double) i;
    *sx = (m[0] * x + m[1] * y) + m[2];
    *sy = (m[3] * x + m[4] * y) + m[5];
}

// the nearest pixel of a position, as an integer-valued double: halves round up
WR_HD double wr_nearest(double s) { return floor(s + 0.5); }

// the lower tap of a position (an integer-valued double) and the weight of the upper one: s - floor(s) is exact in fp64 and
// rounded once to fp32
WR_HD double wr_floor(double s, float *l) {
    const double f = floor(s);
    *l = (float) (s - f);
    return f;
}

// reflect-101 of an integer-valued double: p = 2 (n - 1), i mod p, p - i where that is >= n; n = 1: 0
WR_HD int wr_reflect(double f, int n) {
    if (n == 1 || !(f >= -WR_FAR && f <= WR_FAR)) return 0;  // (also NaN)
    const long long p = 2ll * (n - 1);
    long long i = (long long) f % p;
    if (i < 0) i += p;
    return (int) (i >= n ? p - i : i);
}

// the index along an axis of n pixels that the integer-valued double f reads, or -1: the fill of WR_CONSTANT
WR_HD int wr_index(double f, int n, int border) {
    if (f >= 0.0 && f <= (double) (n - 1)) return (int) f;
    return border == WR_REFLECT ? wr_reflect(f, n) : -1;
}

// (hy * (hx * t00 + lx * t01)) + (ly * (hx * t10 + lx * t11)): four products, two sums, two products, one sum, all fp32
WR_HD float wr_blend(float t00, float t01, float t10, float t11, float ly, float lx) {
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    return (hy * (hx * t00 + lx * t01)) + (ly * (hx * t10 + lx * t11));
}

// fp32 -> bf16 bits, to nearest even; a NaN stays a (quiet) NaN
WR_HD uint16_t wr_bf16(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t) ((u >> 16) | 0x40u);
    return (uint16_t) ((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
