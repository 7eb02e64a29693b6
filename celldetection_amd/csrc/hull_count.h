// Lattice points in the closed convex hull of one object's pixel diamonds (csrc/shape_props.hip: area_convex, solidity): one
// rule in one place, no HIP dependency (tests/hull_count_host.cpp runs this file on the host against brute force).
//
// The object is given by the column extent of each row of its bounding box.  Its hull K is the closed convex hull of the
// points (r +- 1/2, c) and (r, c +- 1/2) over its pixels (scikit-image's convex_hull_image with offset_coordinates=True,
// include_borders=True, restated).  Within a row only the first and the last pixel matter.  In doubled coordinates
// (y = 2 r, x = 2 c) every point is an integer; levels are y = 2 r - 1, 2 r, 2 r + 1 per row with a pixel.
//   chain:  Andrew's monotone chain over the levels in ascending y, once for the left boundary (the smallest x of a level,
//           a convex function of y) and once for the right boundary (the largest x, mirrored to u = -x so that both are the
//           same code); a point is dropped when the slopes around it do not strictly increase (64-bit cross products);
//   count:  on the integer row y = 2 r the hull covers the columns ceil(xl / 2) .. floor(xr / 2), where xl, xr are the
//           crossings of the two chains: exact integer ceil / floor of (u1 * dy + (u2 - u1) * (y - y1)) / (2 * dy).
// Rows without a pixel (fragmented labels) add no level.  Coordinates below 2^18 keep every product below 2^40.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define HC_HD __host__ __device__ inline
#else
#define HC_HD inline
#endif

// ceil(a / b) for b > 0
HC_HD int64_t hc_ceil_div(int64_t a, int64_t b) {
    const int64_t q = a / b;
    return (a % b != 0 && a > 0) ? q + 1 : q;
}

// pushes (y, u) on the chain stack[0 .. n) of (y, u) pairs, y not below the top's; -> the new length
HC_HD int hc_push(int32_t *stack, int n, int32_t y, int32_t u) {
    if (n > 0 && stack[2 * (n - 1)] == y) {  // a level seen before (the row above ends where this row begins): keep the smaller u
        if (stack[2 * (n - 1) + 1] <= u) return n;
        --n;
    }
    while (n >= 2) {
        const int64_t y1 = stack[2 * (n - 2)], u1 = stack[2 * (n - 2) + 1], y2 = stack[2 * (n - 1)], u2 = stack[2 * (n - 1) + 1];
        if ((u2 - u1) * ((int64_t) y - y2) < ((int64_t) u - u2) * (y2 - y1)) break;  // slopes strictly increase: a corner
        --n;
    }
    stack[2 * n] = y;
    stack[2 * n + 1] = u;
    return n + 1;
}

// lo[i] = 65536 - (first column of row i), 0: the row has no pixel; hi[i] = last column + 1.  stack: 2 * (2 * rows + 1) words.
// -> number of integer points in K
HC_HD int64_t hull_count(const uint32_t *lo, const uint32_t *hi, int64_t rows, int32_t *stack) {
    int64_t total = 0;
    for (int side = 0; side < 2; ++side) {
        int n = 0;
        for (int64_t i = 0; i < rows; ++i) {
            if (lo[i] == 0) continue;
            // u = x on the left, -x on the right, x in doubled coordinates
            const int32_t c = side == 0 ? 65536 - (int32_t) lo[i] : -((int32_t) hi[i] - 1);
            const int32_t y = (int32_t) (2 * i);
            n = hc_push(stack, n, y - 1, 2 * c);
            n = hc_push(stack, n, y, 2 * c - 1);
            n = hc_push(stack, n, y + 1, 2 * c);
        }
        if (n == 0) return 0;
        // the integer rows y = 2 r inside [first level, last level]
        int e = 0;
        const int32_t y_first = stack[0] + 1, y_last = stack[2 * (n - 1)] - 1;  // first and last levels are odd
        for (int32_t y = y_first; y <= y_last; y += 2) {
            while (stack[2 * (e + 1)] < y) ++e;
            const int64_t y1 = stack[2 * e], u1 = stack[2 * e + 1], y2 = stack[2 * (e + 1)], u2 = stack[2 * (e + 1) + 1];
            const int64_t dy = y2 - y1;
            total -= hc_ceil_div(u1 * dy + (u2 - u1) * (y - y1), 2 * dy);  // left: -ceil(xl / 2); right: floor(xr / 2) = -ceil(u / 2)
        }
        if (side == 1) total += (y_last - y_first) / 2 + 1;
    }
    return total;
}
