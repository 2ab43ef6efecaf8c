// csrc/mesh_weld_math.h built with the host compiler (tests/test_surface_import_host.py).  One question per run:
//   k n     n points (3 float32 each, raw) on stdin -> per point 4 uint32 on stdout: the canonical key and its hash
//   s n     the table's slot count for n corners, as text (0: outside the limits)
//   o t k   the file offset of float k of STL record t, as text
//   b p     the histogram bucket of a walk of p extra slots, as text
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../invesalius3_amd/csrc/mesh_weld_math.h"

namespace mw = ivx_mesh_weld_math;

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const char *mode = argv[1];
    if (!strcmp(mode, "k")) {
        const long n = atol(argv[2]);
        std::vector<uint32_t> in((size_t)(3 * n) + 1), out((size_t)(4 * n) + 1);
        if (fread(in.data(), 12, (size_t)n, stdin) != (size_t)n) return 3;
        for (long i = 0; i < n; i++) {
            const uint32_t kx = mw::canon(in[3 * i]), ky = mw::canon(in[3 * i + 1]), kz = mw::canon(in[3 * i + 2]);
            out[4 * i] = kx, out[4 * i + 1] = ky, out[4 * i + 2] = kz, out[4 * i + 3] = mw::hash(kx, ky, kz);
        }
        return fwrite(out.data(), 16, (size_t)n, stdout) == (size_t)n ? 0 : 4;
    }
    if (!strcmp(mode, "s")) {
        printf("%llu\n", (unsigned long long)mw::slots(atoll(argv[2])));
        return 0;
    }
    if (!strcmp(mode, "o") && argc == 4) {
        printf("%lld\n", (long long)mw::stl_float_offset(atoll(argv[2]), atoi(argv[3])));
        return 0;
    }
    if (!strcmp(mode, "b")) {
        printf("%d\n", mw::probe_bucket(strtoull(argv[2], nullptr, 10)));
        return 0;
    }
    return 2;
}
