// csrc/density_roi_math.h built with the host compiler (tests/test_density_host.py).  One rule per run, the answer as one byte
// per pixel on stdout:
//   e h w sx sy cx cy a2 b2   rule E for every pixel of an h x w slice, row by row
//   p h w n                   rule P for every pixel; the n points (x, y) as raw float64 on stdin
//   c w h n                   the predicate of k_polygon2mask: polygon_contains at (r, c) for r < w, c < h; points on stdin
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../invesalius3_amd/csrc/density_roi_math.h"

namespace dr = ivx_density_roi_math;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::vector<unsigned char> out;
    const char *rule = argv[1];
    if (!strcmp(rule, "e") && argc == 10) {
        const long h = atol(argv[2]), w = atol(argv[3]);
        double v[6];
        for (int k = 0; k < 6; k++) v[k] = strtod(argv[4 + k], nullptr);
        for (long j = 0; j < h; j++)
            for (long i = 0; i < w; i++) out.push_back(dr::ellipse_selects(i, j, v[0], v[1], v[2], v[3], v[4], v[5]) ? 1 : 0);
    } else if ((!strcmp(rule, "p") || !strcmp(rule, "c")) && argc == 5) {
        const long a = atol(argv[2]), b = atol(argv[3]), n = atol(argv[4]);
        std::vector<double> pts((size_t)(2 * n) + 1);
        if (fread(pts.data(), 16, (size_t)n, stdin) != (size_t)n) return 3;
        for (long j = 0; j < a; j++)
            for (long i = 0; i < b; i++)
                out.push_back((rule[0] == 'p' ? dr::polygon_selects(pts.data(), n, i, j) : dr::polygon_contains(pts.data(), n, (double)j, (double)i)) ? 1 : 0);
    } else
        return 2;
    return fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 4;
}
