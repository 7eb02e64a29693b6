// Border following of one 8-connected component (csrc/label_contours.hip): one rule in one place, no HIP dependency.
//
// Suzuki-Abe border following of the OUTER border, as cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE) does it, restated
// (cv2 is not available in the build image: third-party, unpinned; tests/label_contours_oracle.py states the same rule in
// numpy and tests/contour_trace_host.cpp runs this file on the host):
//   directions d = 0 .. 7 are E, NE, N, NW, W, SW, S, SE in image coordinates (y grows downwards): d + 1 turns
//              counter-clockwise on screen, d - 1 clockwise;
//   start:     the raster-first pixel of the component (smallest y, then smallest x): its W, NW, N and NE neighbours are outside;
//   first search: clockwise on screen from the west neighbour (NW, N, NE, E, SE, S, SW, W); nothing found: a single pixel, emitted
//              twice (the reference doubles a one-point contour, celldetection/data/cpn.py:133-134);
//   every further search: counter-clockwise, starting after the pixel just left (at most 8 probes: the pixel just left is a
//              neighbour, so a probe always succeeds);
//   every visit is a point: one-pixel-wide parts appear once per passage;
//   stop:      when the start pixel is re-entered from the neighbour that the first search found.
// Bound: a pixel is entered from at most 8 directions and (pixel, direction entered from) never repeats before the stop, so a
// trace of a component of n pixels emits at most 8 n points; `max_points` caps the loop, and reaching it returns -1 (it never spins).
#pragma once

#if defined(__HIPCC__)
#define CT_HD __host__ __device__ inline
#else
#define CT_HD inline
#endif

CT_HD int ct_dx(int d) { return d == 0 || d == 1 || d == 7 ? 1 : (d == 3 || d == 4 || d == 5 ? -1 : 0); }
CT_HD int ct_dy(int d) { return d == 1 || d == 2 || d == 3 ? -1 : (d == 5 || d == 6 || d == 7 ? 1 : 0); }

// first search from the start pixel: the direction of the first inside neighbour clockwise from west, or -1 (a single pixel)
template <class Inside>
CT_HD int ct_first(int sx, int sy, Inside inside) {
    int d = 4;
    for (int probe = 0; probe < 8; ++probe) {
        d = (d + 7) & 7;
        if (inside(sx + ct_dx(d), sy + ct_dy(d))) return d;
    }
    return -1;
}

// next search from (x, y): counter-clockwise, starting after direction `from` (the pixel just left, or for the start pixel the
// direction of the first search); -1 cannot happen on a component (kept as an answer so that no caller loops on it)
template <class Inside>
CT_HD int ct_next(int x, int y, int from, Inside inside) {
    int d = from;
    for (int probe = 0; probe < 8; ++probe) {
        d = (d + 1) & 7;
        if (inside(x + ct_dx(d), y + ct_dy(d))) return d;
    }
    return -1;
}

// Traces the component of the start pixel (sx, sy); emit(i, x, y) receives point i.  Returns the number of points (>= 2), or -1
// when more than max_points would be needed or a search fails (both: the component is not what the caller says it is).
template <class Inside, class Emit>
CT_HD long ct_trace(int sx, int sy, long max_points, Inside inside, Emit emit) {
    const int first = ct_first(sx, sy, inside);
    if (first < 0) {
        emit(0L, sx, sy);
        emit(1L, sx, sy);
        return 2;
    }
    const int ex = sx + ct_dx(first), ey = sy + ct_dy(first);  // the stop: (sx, sy) re-entered from here
    int x = sx, y = sy, from = first;
    for (long n = 0; n < max_points; ++n) {
        const int d = ct_next(x, y, from, inside);
        if (d < 0) return -1;
        emit(n, x, y);
        const int nx = x + ct_dx(d), ny = y + ct_dy(d);
        if (nx == sx && ny == sy && x == ex && y == ey) return n + 1;
        x = nx;
        y = ny;
        from = (d + 4) & 7;
    }
    return -1;
}
