// Elliptic Fourier descriptors of contours (csrc/contour_fourier.hip): the chunk decomposition and the per-segment arithmetic,
// one rule in one place, no HIP dependency (tests/efd_chunks_host.cpp runs this file on the host).
//
// The rule (the reference's cd.data.cpn.efd, celldetection/data/cpn.py:23-90).  A contour is n >= 1 points (x, y).
//   closing:   the contour is closed if |first - last| <= 1e-8 + 1e-5 |last| holds for both coordinates (numpy's allclose with
//              b = last).  When the first point is appended the contour has N = n segments, otherwise N = n - 1.
//   segments:  for i = 0 .. N - 1: dx_i, dy_i = the point differences, dt_i = sqrt(dx_i^2 + dy_i^2) + epsilon, t_0 = 0,
//              t_(i+1) = t_i + dt_i, T = t_N.
//   coefficients: for k = 1 .. order, phi_(k,i) = k * (2 pi t_i / T), C_k = T / (2 k^2 pi^2):
//              coeff[k-1] = C_k * (sum dx_i/dt_i dcos, sum dx_i/dt_i dsin, sum dy_i/dt_i dcos, sum dy_i/dt_i dsin) with
//              dcos = cos phi_(k,i+1) - cos phi_(k,i), dsin likewise.
//   location:  X_i = sum_(j<=i) dx_j; a0 = (1/T) sum [dx_i/(2 dt_i) (t_(i+1)^2 - t_i^2) + (X_i - dx_i/dt_i t_(i+1)) dt_i], c0 the
//              same with y; location = first point + (a0, c0).
//   N = 0 (one point) gives coefficients 0 and location NaN ((1/0) * 0); N = 1 with T = epsilon (the doubled point of
//   labels2contours) gives coefficients 0 and location exactly that point.
// All arithmetic is float64, without contraction.  X_i is taken as x_(i+1) - x_0 (one rounding, exact for integer points; the
// reference's running sum of differences rounds once per step).
//
// Decomposition and order of summation.  A CHUNK is up to CPN_EFD_CHUNK consecutive segments of one contour, counted from the
// contour's own first segment: chunk c holds segments c * CHUNK .. min(N, (c + 1) * CHUNK) - 1.  One wave of 64 lanes works on
// a chunk in ROUNDS of 64 segments: in round r lane l owns segment c * CHUNK + r * 64 + l (a lane without a segment carries
// dt = dx/dt = dy/dt = 0, which changes no sum, and adds no location term).
//   t:     within a round an inclusive Kogge-Stone scan of dt over the lanes (for d = 1, 2, 4, .., 32: v_l += v_(l-d), all lanes
//          at once), then + carry (0 in round 0, afterwards carry + lane 63's value): the chunk's local t; t = base + local t.
//          The chunk's sum of dt is its last local t; a contour's chunk bases (the first is 0) and T are those sums added in
//          chunk order, so the last t of the last chunk is T bit for bit.
//   sums:  every lane adds its own terms over the rounds in round order (4 sums per k, 2 for the location); then a butterfly
//          over the lanes (for d = 32, 16, .., 1: v_l += v_(l^d)); a contour's chunk partials are added in chunk order.
// None of this depends on where the contour lies in the packed array or on what else is in it.
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef CPN_EFD_CHUNK
#define CPN_EFD_CHUNK 256  // (include/cpn_hip.h states the same value)
#endif
#define EFD_WAVE 64
#define EFD_ROUNDS (CPN_EFD_CHUNK / EFD_WAVE)
#define EFD_PI 3.141592653589793  // numpy's np.pi

#if defined(__HIPCC__)
#define EFD_HD __host__ __device__ inline
#else
#define EFD_HD inline
#endif

// numpy's allclose(first, last) on one contour
EFD_HD bool efd_is_closed(double fx, double fy, double lx, double ly) {
    return fabs(fx - lx) <= 1e-8 + 1e-5 * fabs(lx) && fabs(fy - ly) <= 1e-8 + 1e-5 * fabs(ly);
}

// contour k = points[a .. b) of P points: inside the array and at least one point (the check every index rests on)
EFD_HD bool efd_range_ok(int64_t a, int64_t b, int64_t P) { return a >= 0 && b > a && b <= P; }
// offsets[0] and offsets[K]
EFD_HD bool efd_ends_ok(int64_t first, int64_t last, int64_t P) { return first == 0 && last == P; }

EFD_HD int64_t efd_num_segments(int64_t n_points, bool append_first) { return append_first ? n_points : n_points - 1; }
EFD_HD int64_t efd_num_chunks(int64_t N) { return (N + CPN_EFD_CHUNK - 1) / CPN_EFD_CHUNK; }
EFD_HD int64_t efd_chunk_begin(int64_t c) { return c * CPN_EFD_CHUNK; }
EFD_HD int efd_chunk_len(int64_t N, int64_t c) {
    const int64_t rest = N - c * CPN_EFD_CHUNK;
    return (int) (rest < CPN_EFD_CHUNK ? rest : CPN_EFD_CHUNK);
}

// what a lane keeps of its segment
struct EfdSeg {
    double dxdt, dydt;  // dx / dt, dy / dt
    double dt;
    double dx, dy;
    double X, Y;  // x_(i+1) - x_0, y_(i+1) - y_0
};

// segment from point p = (px, py) to q = (qx, qy) of a contour whose first point is (x0, y0)
EFD_HD EfdSeg efd_segment(double px, double py, double qx, double qy, double x0, double y0, double epsilon) {
    EfdSeg s;
    s.dx = qx - px;
    s.dy = qy - py;
    s.dt = sqrt(s.dx * s.dx + s.dy * s.dy) + epsilon;
    s.dxdt = s.dx / s.dt;
    s.dydt = s.dy / s.dt;
    s.X = qx - x0;
    s.Y = qy - y0;
    return s;
}

EFD_HD EfdSeg efd_no_segment() {
    EfdSeg s;
    s.dxdt = s.dydt = s.dt = s.dx = s.dy = s.X = s.Y = 0.;
    return s;
}

// the location terms of one segment with t0 = t_i, t1 = t_(i+1):  (d / (2 dt)) (t1^2 - t0^2) + (X - (d / dt) t1) dt
EFD_HD double efd_location_term(double d, double ddt, double dt, double X, double t0, double t1) {
    const double t_diff = t1 * t1 - t0 * t0;
    const double xi = X - ddt * t1;
    return (d / (2. * dt)) * t_diff + xi * dt;
}

// phi_(1,i) = (2 pi t_i) / T; phi_(k,i) = phi_(1,i) * k
EFD_HD double efd_phi1(double t, double T) { return (2. * EFD_PI * t) / T; }
// C_k = T / (2 k^2 pi^2)
EFD_HD double efd_constant(double T, int k) { return T / (2. * ((double) k * (double) k) * (EFD_PI * EFD_PI)); }
EFD_HD double efd_location(double first, double sum, double T) { return first + (1. / T) * sum; }

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the same decomposition run sequentially on the host: a wave is an array of 64 values ----
#include <vector>

inline void efd_host_scan(double *v) {  // inclusive Kogge-Stone over 64 lanes
    for (int d = 1; d < EFD_WAVE; d *= 2) {
        double w[EFD_WAVE];
        for (int l = 0; l < EFD_WAVE; ++l) w[l] = l >= d ? v[l] + v[l - d] : v[l];
        for (int l = 0; l < EFD_WAVE; ++l) v[l] = w[l];
    }
}

inline double efd_host_butterfly(double *v) {
    for (int d = EFD_WAVE / 2; d >= 1; d /= 2) {
        double w[EFD_WAVE];
        for (int l = 0; l < EFD_WAVE; ++l) w[l] = v[l] + v[l ^ d];
        for (int l = 0; l < EFD_WAVE; ++l) v[l] = w[l];
    }
    return v[0];
}

struct EfdHostChunk {
    EfdSeg seg[EFD_ROUNDS][EFD_WAVE];
    double t1[EFD_ROUNDS][EFD_WAVE];  // t at the end of the lane's segment
    int rounds, len;
};

// loads chunk c of a contour of n points (N segments; segment i ends at point i + 1, or at point 0 when i + 1 == n) and scans t
// from `base`; returns the chunk's sum of dt
template <class T>
inline double efd_host_load(const T *p, int64_t n, int64_t N, int64_t c, double epsilon, double base, EfdHostChunk &ch) {
    const int len = efd_chunk_len(N, c);
    ch.len = len;
    ch.rounds = (len + EFD_WAVE - 1) / EFD_WAVE;
    double carry = 0.;
    for (int r = 0; r < ch.rounds; ++r) {
        double v[EFD_WAVE];
        for (int l = 0; l < EFD_WAVE; ++l) {
            const int64_t i = efd_chunk_begin(c) + r * EFD_WAVE + l;
            if (r * EFD_WAVE + l < len) {
                const int64_t j = i + 1 == n ? 0 : i + 1;
                ch.seg[r][l] = efd_segment((double) p[2 * i], (double) p[2 * i + 1], (double) p[2 * j], (double) p[2 * j + 1],
                                           (double) p[0], (double) p[1], epsilon);
            } else {
                ch.seg[r][l] = efd_no_segment();
            }
            v[l] = ch.seg[r][l].dt;
        }
        efd_host_scan(v);
        for (int l = 0; l < EFD_WAVE; ++l) ch.t1[r][l] = base + (carry + v[l]);
        carry = carry + v[EFD_WAVE - 1];
    }
    return carry;  // the chunk's sum of dt: base + this is the chunk's last t
}

// partial sums of a loaded chunk whose first segment starts at t = base: out[4 * order + 2]
inline void efd_host_partials(const EfdHostChunk &ch, double base, double T, int order, double *out) {
    double ax[EFD_WAVE], ay[EFD_WAVE];
    for (int l = 0; l < EFD_WAVE; ++l) ax[l] = ay[l] = 0.;
    for (int r = 0; r < ch.rounds; ++r)
        for (int l = 0; l < EFD_WAVE; ++l) {
            if (r * EFD_WAVE + l >= ch.len) continue;  // no segment: no location term (its 0 / 0 must not enter the sum)
            const EfdSeg &s = ch.seg[r][l];
            const double t0 = l ? ch.t1[r][l - 1] : (r ? ch.t1[r - 1][EFD_WAVE - 1] : base);
            ax[l] = ax[l] + efd_location_term(s.dx, s.dxdt, s.dt, s.X, t0, ch.t1[r][l]);
            ay[l] = ay[l] + efd_location_term(s.dy, s.dydt, s.dt, s.Y, t0, ch.t1[r][l]);
        }
    out[4 * order] = efd_host_butterfly(ax);
    out[4 * order + 1] = efd_host_butterfly(ay);
    for (int k = 1; k <= order; ++k) {
        double acc[4][EFD_WAVE];
        for (int l = 0; l < EFD_WAVE; ++l) acc[0][l] = acc[1][l] = acc[2][l] = acc[3][l] = 0.;
        const double phi_base = efd_phi1(base, T) * (double) k;
        double c_prev = cos(phi_base), s_prev = sin(phi_base);
        for (int r = 0; r < ch.rounds; ++r)
            for (int l = 0; l < EFD_WAVE; ++l) {
                const double phi = efd_phi1(ch.t1[r][l], T) * (double) k;
                const double c1 = cos(phi), s1 = sin(phi);
                const double dc = c1 - c_prev, ds = s1 - s_prev;
                const EfdSeg &s = ch.seg[r][l];
                acc[0][l] = acc[0][l] + s.dxdt * dc;
                acc[1][l] = acc[1][l] + s.dxdt * ds;
                acc[2][l] = acc[2][l] + s.dydt * dc;
                acc[3][l] = acc[3][l] + s.dydt * ds;
                c_prev = c1;
                s_prev = s1;
            }
        for (int j = 0; j < 4; ++j) out[4 * (k - 1) + j] = efd_host_butterfly(acc[j]);
    }
}

// one contour of n points, N segments (N == n: the first point is appended): coeff[order][4], loc[2]
template <class T>
inline void efd_host_contour(const T *p, int64_t n, int64_t N, int order, double epsilon, double *coeff, double *loc) {
    const int nv = 4 * order + 2;
    const int64_t chunks = efd_num_chunks(N);
    std::vector<double> base((size_t) chunks + 1, 0.), sum((size_t) nv, 0.), part((size_t) nv);
    EfdHostChunk ch;
    for (int64_t c = 0; c < chunks; ++c) base[c + 1] = base[c] + efd_host_load(p, n, N, c, epsilon, 0., ch);
    const double T_ = base[chunks];
    for (int64_t c = 0; c < chunks; ++c) {
        efd_host_load(p, n, N, c, epsilon, base[c], ch);
        efd_host_partials(ch, base[c], T_, order, part.data());
        for (int j = 0; j < nv; ++j) sum[j] = c ? sum[j] + part[j] : part[j];
    }
    for (int k = 1; k <= order; ++k)
        for (int j = 0; j < 4; ++j) coeff[4 * (k - 1) + j] = efd_constant(T_, k) * sum[4 * (k - 1) + j];
    loc[0] = efd_location((double) p[0], sum[4 * order], T_);
    loc[1] = efd_location((double) p[1], sum[4 * order + 1], T_);
}
#endif
