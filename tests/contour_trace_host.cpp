// TEST INFRASTRUCTURE ONLY: the border following of csrc/contour_trace.h run on the host, the same code the trace kernel of
// csrc/label_contours.hip runs per lane.  tests/test_label_contours.py compiles this file and compares its output with
// tests/label_contours_oracle.py.
//   input  (file named by argv[1]): "<images>", then per image "<H> <W>" and H * W integers in raster order; every value > 0 of an
//          image is taken as ONE component (the test writes such images);
//   output: per image "image <index>", per value ascending "value <v> <points>" and one "<x> <y>" line per point; a trace that
//          reaches the cap of 8 x the pixel count prints "value <v> -1" and the program returns 1.
#include <cstdio>
#include <map>
#include <vector>

#include "../celldetection_amd/csrc/contour_trace.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int images = 0, bad = 0;
    if (std::fscanf(f, "%d", &images) != 1) return 2;
    for (int i = 0; i < images; ++i) {
        int H = 0, W = 0;
        if (std::fscanf(f, "%d %d", &H, &W) != 2 || H < 1 || W < 1) return 2;
        std::vector<int> img((size_t) H * W);
        for (int &v : img)
            if (std::fscanf(f, "%d", &v) != 1) return 2;
        std::map<int, std::pair<int, long>> objects;  // value -> (raster-first pixel, pixel count)
        for (int p = 0; p < H * W; ++p)
            if (img[p] > 0) {
                auto it = objects.find(img[p]);
                if (it == objects.end()) objects[img[p]] = {p, 1};
                else ++it->second.second;
            }
        std::printf("image %d\n", i);
        for (const auto &o : objects) {
            const int v = o.first, start = o.second.first;
            const int *data = img.data();
            auto inside = [=](int x, int y) { return x >= 0 && x < W && y >= 0 && y < H && data[y * W + x] == v; };
            std::vector<int> pts;
            const long n = ct_trace(start % W, start / W, 8 * o.second.second, inside, [&](long, int x, int y) {
                pts.push_back(x);
                pts.push_back(y);
            });
            std::printf("value %d %ld\n", v, n);
            if (n < 0 || n * 2 != (long) pts.size()) {
                bad = 1;
                continue;
            }
            for (long k = 0; k < n; ++k) std::printf("%d %d\n", pts[2 * k], pts[2 * k + 1]);
        }
    }
    std::fclose(f);
    return bad;
}
