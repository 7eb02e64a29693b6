// The polygon fill rule of the label and overlay rasterisers (csrc/labels.hip, csrc/overlay.hip): one rule in one place.
//
// OpenCV's FillEdgeCollection + boundary lines for integer vertices, restated (cv2 is not available in the build image --
// see oracle/labels_oracle.py, "parity unpinned"):
//   boundary: every edge drawn with the 8-connected LineIterator (left-to-right, err0 = dmaj - 2*dmin, diagonal step
//             iff err < 0):  minor(t) = ceil((2*dmin*t - dmaj) / (2*dmaj));
//   interior: scanline y takes the edges with y0 <= y < y1 (horizontal edges skipped), crossing x in 16.16 fixed point
//             x = x_top * 65536 + (y - y_top) * trunc(dx * 65536 / dy), rounded (x + 32768) >> 16; sorted crossings are
//             paired and the pixels between a pair (inclusive) are filled.
// lb_filled answers for one pixel; lb_filled_row32 answers for 32 consecutive pixels of one row with ONE walk over the edges
// (the same predicate: boundary || odd number of crossings left of the pixel || a crossing on the pixel).  The functions also
// compile for the host: tests/polygon_fill_host.cpp compares the two forms there.
#pragma once

#include <hip/hip_runtime.h>

__host__ __device__ __forceinline__ bool on_line(int px, int py, int ax, int ay, int bx, int by) {
    // 8-connected LineIterator from the left end point (left_to_right)
    if (bx < ax) { int t = ax; ax = bx; bx = t; t = ay; ay = by; by = t; }
    const int dx = bx - ax, dyv = by - ay, dy = dyv < 0 ? -dyv : dyv, sy = dyv < 0 ? -1 : 1;
    if (dy <= dx) {  // x major
        const int t = px - ax;
        if (t < 0 || t > dx) return false;
        const int m = dx == 0 ? 0 : (2 * dy * t - dx + 2 * dx - 1) / (2 * dx);  // ceil((2 dy t - dx) / (2 dx)), numerator > -2dx
        return py == ay + sy * m;
    }
    const int t = (py - ay) * sy;  // y major (x is the minor axis and grows: left to right)
    if (t < 0 || t > dy) return false;
    const int m = (2 * dx * t - dy + 2 * dy - 1) / (2 * dy);
    return px == ax + m;
}

// pixel (xx, yy) belongs to the filled polygon (boundary lines + scanline interior, see the header)
__host__ __device__ __forceinline__ bool lb_filled(int xx, int yy, const int *px, const int *py, int S) {
    bool set = false;
    int n_lt = 0, n_le = 0;
    for (int s = 0; s < S && !set; ++s) {
        const int ax = px[s], ay = py[s], bx = px[s + 1 == S ? 0 : s + 1], by = py[s + 1 == S ? 0 : s + 1];
        set = on_line(xx, yy, ax, ay, bx, by);
        if (ay == by) continue;  // horizontal edges take no part in the scanline fill
        const int ty = ay < by ? ay : by, tx = ay < by ? ax : bx, byy = ay < by ? by : ay;
        if (yy < ty || yy >= byy) continue;
        const long long ddx = ((long long) (bx - ax) * 65536ll) / (long long) (by - ay);  // C division: truncation
        const long long xf = (long long) tx * 65536ll + (long long) (yy - ty) * ddx;
        const int xr = (int) ((xf + 32768ll) >> 16);
        n_lt += xr < xx;
        n_le += xr <= xx;
    }
    return set || (n_lt & 1) || n_le > n_lt;
}

// lb_filled for the 32 pixels (x0 .. x0 + 31, yy) at once: bit c of the result = lb_filled(x0 + c, yy, ...).  pts holds the
// S vertices as (x, y) pairs.  An edge that does not touch row yy costs two comparisons; one that does is tested with on_line
// on the pixels of the window it spans, and its crossing x_r toggles the parity of every pixel right of x_r (n_lt) and marks
// the pixel on x_r (n_le > n_lt).
__host__ __device__ __forceinline__ unsigned int lb_filled_row32(int x0, int yy, const int2 *__restrict__ pts, int S) {
    unsigned int line = 0u, parity = 0u, on = 0u;
    int2 a = pts[0];
    for (int s = 0; s < S; ++s) {
        const int2 b = pts[s + 1 == S ? 0 : s + 1];
        const int ax = a.x, ay = a.y, bx = b.x, by = b.y;
        a = b;
        if (yy < (ay < by ? ay : by) || yy > (ay < by ? by : ay)) continue;
        const int ex0 = ax < bx ? ax : bx, ex1 = ax < bx ? bx : ax;
        const int lo = x0 > ex0 ? x0 : ex0, hi = x0 + 31 < ex1 ? x0 + 31 : ex1;
        for (int xx = lo; xx <= hi; ++xx)
            if (on_line(xx, yy, ax, ay, bx, by)) line |= 1u << (xx - x0);
        if (ay == by) continue;  // horizontal edges take no part in the scanline fill
        const int ty = ay < by ? ay : by, tx = ay < by ? ax : bx, byy = ay < by ? by : ay;
        if (yy >= byy) continue;
        const long long ddx = ((long long) (bx - ax) * 65536ll) / (long long) (by - ay);  // C division: truncation
        const long long xf = (long long) tx * 65536ll + (long long) (yy - ty) * ddx;
        const int c = (int) ((xf + 32768ll) >> 16) - x0;  // the crossing, as a column of the window
        if (c < 0) {
            parity = ~parity;  // left of the window: every pixel has it on its left
        } else if (c < 31) {
            parity ^= ~0u << (c + 1);
            on |= 1u << c;
        } else if (c == 31) {
            on |= 1u << 31;
        }
    }
    return line | parity | on;
}
