// TEST INFRASTRUCTURE ONLY: the chunk decomposition and per-segment arithmetic of csrc/efd_chunks.h run sequentially on the host
// (the code the kernels of csrc/contour_fourier.hip run per lane, a wave being an array of 64 values here).
// tests/test_fourier.py compiles this file and judges its output against tests/fourier_oracle.py.
//   efd_chunks_host efd <file>:     "<contours> <order> <epsilon>", then per contour "<n> <N>" (n points, N segments: N == n appends
//                                   the first point) and n pairs "<x> <y>".  The contours are packed into ONE array first, as the
//                                   kernels see them.  Output: per contour one line of 4 * order + 2 hex floats: the
//                                   coefficients [order][4], then the location.
//   efd_chunks_host offsets <file>: "<K> <P>", then K + 1 offsets.  Output: "ok" or "bad" by the checks of efd_chunks.h.
//   efd_chunks_host chunk:          prints CPN_EFD_CHUNK.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../celldetection_amd/csrc/efd_chunks.h"

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "chunk")) {
        std::printf("%d\n", CPN_EFD_CHUNK);
        return 0;
    }
    if (argc != 3) return 2;
    std::FILE *f = std::fopen(argv[2], "r");
    if (!f) return 2;
    if (!std::strcmp(argv[1], "offsets")) {
        long long K = 0, P = 0;
        if (std::fscanf(f, "%lld %lld", &K, &P) != 2 || K < 1) return 2;
        std::vector<long long> off((size_t) K + 1);
        for (auto &o : off)
            if (std::fscanf(f, "%lld", &o) != 1) return 2;
        bool ok = efd_ends_ok(off[0], off[(size_t) K], P);
        for (long long k = 0; k < K; ++k) ok = ok && efd_range_ok(off[(size_t) k], off[(size_t) k + 1], P);
        std::printf(ok ? "ok\n" : "bad\n");
        return 0;
    }
    if (std::strcmp(argv[1], "efd")) return 2;
    long long count = 0;
    int order = 0;
    double epsilon = 0.;
    if (std::fscanf(f, "%lld %d %lf", &count, &order, &epsilon) != 3 || count < 0 || order < 1) return 2;
    std::vector<double> points;
    std::vector<long long> offsets{0}, segments;
    for (long long k = 0; k < count; ++k) {
        long long n = 0, N = 0;
        if (std::fscanf(f, "%lld %lld", &n, &N) != 2 || n < 1 || (N != n && N != n - 1)) return 2;
        for (long long i = 0; i < 2 * n; ++i) {
            double v = 0.;
            if (std::fscanf(f, "%lf", &v) != 1) return 2;
            points.push_back(v);
        }
        offsets.push_back(offsets.back() + n);
        segments.push_back(N);
    }
    std::fclose(f);
    std::vector<double> coeff((size_t) order * 4);
    double loc[2];
    for (long long k = 0; k < count; ++k) {
        const long long a = offsets[(size_t) k], n = offsets[(size_t) k + 1] - a;
        efd_host_contour(points.data() + 2 * a, (int64_t) n, (int64_t) segments[(size_t) k], order, epsilon, coeff.data(), loc);
        for (double v : coeff) std::printf("%a ", v);
        std::printf("%a %a\n", loc[0], loc[1]);
    }
    return 0;
}
