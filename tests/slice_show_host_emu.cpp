// csrc/slice_show_math.h built with the host compiler (tests/test_slice_display_host.py).  One rule per run, the answer as raw
// bytes on stdout:
//   r1 ww wl          every int16 value -32768 .. 32767: the grey byte (R1) and the plist index (R3), two bytes each
//   r1f ww wl n       n float64 values on stdin (raw): the grey byte of the float64 path
//   r2 tmin tmax      every grey byte 0 .. 255: the table index
//   r4 n v0 r0 g0 b0 ...   every int16 value: three bytes (the nodes sorted by value, colours as bytes)
//   r6 aux_max        every byte: the table index
//   r7 a0 .. a7       base 0 .. 255 x over 0 .. 255 x the eight alphas: the blended byte
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../invesalius3_amd/csrc/slice_show_math.h"

namespace ss = ivx_slice_show_math;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::vector<unsigned char> out;
    const char *rule = argv[1];
    if (!strcmp(rule, "r1") && argc == 4) {
        const ss::Window W = ss::make_window(strtod(argv[2], nullptr), strtod(argv[3], nullptr), 0, 0.0, 0.0, 0);
        for (int v = -32768; v <= 32767; v++) {
            out.push_back((unsigned char)ss::r1_grey(W, (double)v));
            out.push_back((unsigned char)ss::r3_index(W, (double)v));
        }
    } else if (!strcmp(rule, "r1f") && argc == 5) {
        const ss::Window W = ss::make_window(strtod(argv[2], nullptr), strtod(argv[3], nullptr), 1, 0.0, 0.0, 0);
        const long n = atol(argv[4]);
        std::vector<double> v((size_t)n);
        if (fread(v.data(), 8, (size_t)n, stdin) != (size_t)n) return 3;
        for (long i = 0; i < n; i++) out.push_back((unsigned char)ss::r1_grey(W, v[i]));
    } else if (!strcmp(rule, "r2") && argc == 4) {
        const ss::Window W = ss::make_window(1.0, 0.0, 0, strtod(argv[2], nullptr), strtod(argv[3], nullptr), 0);
        for (int g = 0; g < 256; g++) out.push_back((unsigned char)ss::r2_index(W, g));
    } else if (!strcmp(rule, "r4") && argc >= 3) {
        const int n = atoi(argv[2]);
        if (n < 1 || n > ss::MAX_NODES || argc != 3 + 4 * n) return 2;
        std::vector<double> values((size_t)n), colours((size_t)3 * n);
        for (int i = 0; i < n; i++) {
            values[i] = strtod(argv[3 + 4 * i], nullptr);
            for (int q = 0; q < 3; q++) colours[3 * i + q] = strtod(argv[4 + 4 * i + q], nullptr) / 255.0;
        }
        for (int v = -32768; v <= 32767; v++) {
            int c[3];
            ss::r4_colour(values.data(), colours.data(), n, (double)v, c);
            for (int q = 0; q < 3; q++) out.push_back((unsigned char)c[q]);
        }
    } else if (!strcmp(rule, "r6") && argc == 3) {
        const ss::Window W = ss::make_window(1.0, 0.0, 0, 0.0, 0.0, atoi(argv[2]));
        for (int v = 0; v < 256; v++) out.push_back((unsigned char)ss::r6_index(W, v));
    } else if (!strcmp(rule, "r7") && argc == 10) {
        for (int b = 0; b < 256; b++)
            for (int o = 0; o < 256; o++)
                for (int k = 0; k < 8; k++) out.push_back((unsigned char)ss::r7_blend(b, o, atoi(argv[2 + k])));
    } else
        return 2;
    return fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 4;
}
