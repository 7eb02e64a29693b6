// csrc/grouped_conv.h on the host (tests/test_grouped_conv.py builds this host program with AddressSanitizer and UBSan and runs it):
// the index arithmetic of the trainable grouped conv against brute force, for every (C, cig) of the family up to C = 512:
//   - the pack, both modes: every element of the records holds exactly the weight the layout states (written out here loop by
//     loop from the weight's side), every weight occurs exactly once, everything else is a zero -- the padding item of every bundle
//     and the entries across two groups of a bundle;
//   - the weight gradient's tile mapping: every dW element (co, cl) lies in exactly one fragment element, that fragment multiplies
//     the 32-channel chunks that hold co and its group's input channel, and exactly one (span, wave) owns it and stages both chunks;
//   - the dilation, for N <= 2 and sizes up to 9 x 9, even and odd: dZ[2 i][2 j] = dY[i][j], zeros elsewhere, every unit of dY once.
// Output: "ok <checks>" or the first difference.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../celldetection_amd/csrc/grouped_conv.h"

static long checks = 0;

#define FAIL(...)                                    \
    do {                                             \
        std::printf("C %d cig %d: ", C, cig);        \
        std::printf(__VA_ARGS__);                    \
        std::printf("\n");                           \
        return 1;                                    \
    } while (0)

static int check_pack(int C, int cig, const GcGeo &g) {
    const int64_t total = gc_packed_elements(g), weights = (int64_t) C * cig * 9;
    if (total != (int64_t) g.bundles * g.items_packed * g.bw * 32) FAIL("packed elements %ld", (long) total);
    for (int dgrad = 0; dgrad < 2; ++dgrad) {
        std::vector<int64_t> want((size_t) total, -1);
        for (int co = 0; co < C; ++co)
            for (int cl = 0; cl < cig; ++cl)
                for (int ky = 0; ky < 3; ++ky)
                    for (int kx = 0; kx < 3; ++kx) {
                        const int ci = co / cig * cig + cl, bundle = co / g.bw;
                        if (ci / g.bw != bundle) FAIL("a group crosses two bundles");
                        // the record's output channel / reduced channel inside the bundle and its tap position
                        const int oc = (dgrad ? ci : co) % g.bw, rc = (dgrad ? co : ci) % g.bw;
                        const int tap = dgrad ? (2 - ky) * 3 + (2 - kx) : ky * 3 + kx;
                        const int item = rc / 32 * 9 + tap;
                        const int64_t o = (((int64_t) bundle * g.items_packed + item) * g.bw + oc) * 32 + rc % 32;
                        if (o < 0 || o >= total || want[(size_t) o] != -1) FAIL("brute force collides at %ld", (long) o);
                        want[(size_t) o] = (((int64_t) co * cig + cl) * 3 + ky) * 3 + kx;
                    }
        std::vector<char> seen((size_t) weights, 0);
        for (int64_t o = 0; o < total; ++o) {
            const int64_t got = gc_pack_source(g, o, dgrad);
            if (got != want[(size_t) o]) FAIL("mode %d element %ld: source %ld, expected %ld", dgrad, (long) o, (long) got, (long) want[(size_t) o]);
            if (got >= 0) {
                if (got >= weights || seen[(size_t) got]) FAIL("mode %d: weight %ld out of range or twice", dgrad, (long) got);
                seen[(size_t) got] = 1;
            }
            ++checks;
        }
        for (int64_t i = 0; i < weights; ++i)
            if (!seen[(size_t) i]) FAIL("mode %d: weight %ld is not packed", dgrad, (long) i);
    }
    return 0;
}

static int check_tiles(int C, int cig, const GcGeo &g) {
    const int nb = gc_span_chunks(g);
    std::vector<int> owner((size_t) g.frags, 0);
    for (int span = 0; span < g.spans; ++span)
        for (int wave = 0; wave < 4; ++wave) {
            const int f = gc_wave_frag(g, span, wave);
            if (f < 0) continue;
            if (f >= g.frags) FAIL("span %d wave %d owns fragment %d of %d", span, wave, f, g.frags);
            owner[(size_t) f] += 1;
            int a, b;
            gc_frag_chunks(g, f, &a, &b);
            const int first = gc_span_first_chunk(g, span);
            if (a < first || a >= first + nb || b < first || b >= first + nb || a >= C / 32 || b >= C / 32)
                FAIL("fragment %d reads chunks %d, %d outside the staged [%d, %d) or the tensor", f, a, b, first, first + nb);
        }
    for (int f = 0; f < g.frags; ++f)
        if (owner[(size_t) f] != 1) FAIL("fragment %d has %d owners", f, owner[(size_t) f]);
    if (g.spans != (g.frags + 3) / 4) FAIL("%d spans for %d fragments", g.spans, g.frags);
    std::vector<char> used((size_t) g.frags * 1024, 0);
    for (int co = 0; co < C; ++co)
        for (int cl = 0; cl < cig; ++cl) {
            int f, i, j, a, b;
            gc_locate(g, co, cl, &f, &i, &j);
            if (f < 0 || f >= g.frags || i < 0 || i >= 32 || j < 0 || j >= 32) FAIL("(%d, %d) -> fragment %d (%d, %d)", co, cl, f, i, j);
            gc_frag_chunks(g, f, &a, &b);
            const int ci = co / cig * cig + cl;
            if (a * 32 + i != co || b * 32 + j != ci) FAIL("(%d, %d): fragment %d (%d, %d) is (co %d, ci %d), expected ci %d", co, cl, f, i, j, a * 32 + i, b * 32 + j, ci);
            char &u = used[((size_t) f * 32 + (size_t) i) * 32 + (size_t) j];
            if (u) FAIL("(%d, %d) shares its fragment element", co, cl);
            u = 1;
            ++checks;
        }
    return 0;
}
#undef FAIL

static int check_dilate() {
    const uint32_t C8 = 4;
    for (uint32_t N = 1; N <= 2; ++N)
        for (uint32_t H = 1; H <= 9; ++H)
            for (uint32_t W = 1; W <= 9; ++W) {
                const uint32_t Ho = (uint32_t) gc_out_size((int32_t) H, 2), Wo = (uint32_t) gc_out_size((int32_t) W, 2);
                if (2 * (Ho - 1) > H - 1 || 2 * (Wo - 1) > W - 1 || 2 * Ho < H || 2 * Wo < W) {
                    std::printf("size %u x %u -> %u x %u\n", H, W, Ho, Wo);
                    return 1;
                }
                std::vector<int64_t> want((size_t) (N * H * W * C8), -1);
                for (uint32_t n = 0; n < N; ++n)
                    for (uint32_t i = 0; i < Ho; ++i)
                        for (uint32_t j = 0; j < Wo; ++j)
                            for (uint32_t c = 0; c < C8; ++c)
                                want[(size_t) (((n * H + 2 * i) * W + 2 * j) * C8 + c)] = (int64_t) (((n * Ho + i) * Wo + j) * C8 + c);
                for (uint32_t u = 0; u < N * H * W * C8; ++u) {
                    const int64_t got = gc_dilate_source(u, H, W, C8);
                    if (got != want[u]) {
                        std::printf("N %u, %u x %u: unit %u reads %ld, expected %ld\n", N, H, W, u, (long) got, (long) want[u]);
                        return 1;
                    }
                    ++checks;
                }
            }
    return 0;
}

int main() {
    const int widths[] = {4, 8, 16, 32, 64};
    int pairs = 0;
    for (int cig : widths)
        for (int C = 1; C <= 512; ++C) {
            GcGeo g;
            const int bw = cig == 64 ? 64 : 32;
            const bool family = C % bw == 0;
            if (gc_geometry(C, cig, &g) != family) {
                std::printf("C %d cig %d: gc_geometry disagrees with the family\n", C, cig);
                return 1;
            }
            if (!family) continue;
            if (g.bw != bw || g.bundles * bw != C || g.gpb * cig != bw || g.items != bw / 32 * 9 || g.items_packed % 2 ||
                g.items_packed - g.items != (bw == 32 ? 1 : 0)) {
                std::printf("C %d cig %d: geometry\n", C, cig);
                return 1;
            }
            if (check_pack(C, cig, g) || check_tiles(C, cig, g)) return 1;
            ++pairs;
        }
    GcGeo g;
    for (int cig : {0, 1, 2, 3, 5, 12, 24, 48, 128})
        if (gc_geometry(512, cig, &g)) {
            std::printf("cig %d accepted\n", cig);
            return 1;
        }
    if (gc_geometry(0, 32, &g) || gc_geometry(-32, 32, &g) || gc_geometry(32, 64, &g)) {
        std::printf("a non-positive or too small C accepted\n");
        return 1;
    }
    if (check_dilate()) return 1;
    if (pairs != 4 * 16 + 8) {
        std::printf("%d pairs\n", pairs);
        return 1;
    }
    std::printf("ok %ld\n", checks);
    return 0;
}
