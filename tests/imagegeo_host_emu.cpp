// csrc/imagegeo_math.h built with the host compiler (tests/test_imagegeo_host.py).  Records on stdin:
//   S H W K   then H * W samples, then K pairs "shift cval": K lines out, each the H * W samples of
//             scipy.ndimage.shift(slice, (shift, 0), cval=cval) as the header computes them
//   V D H W   then D shifts, then D * H * W samples: the whole tool, one slice after the other with the chain of fill
//             values; two lines out, the D * H * W samples and the D fill values
#include <stdio.h>

#include <vector>

#include "../invesalius3_amd/csrc/imagegeo_math.h"

namespace ig = ivx_imagegeo;

// the interior of one slice in place (what one launch of the kernel does for it); returns the minima
static void slice_interior(int16_t *img, int64_t H, int64_t W, double shift, int *old_min, int *new_min) {
    std::vector<double> c((size_t)(H * W));
    const double zn1 = ig::pole_power(H);
    *old_min = *new_min = ig::NO_MIN;
    for (int64_t x = 0; x < W; x++) {
        int a, b;
        ig::shift_column(img + x, W, c.data() + x, W, H, -shift, zn1, &a, &b);
        if (a < *old_min) *old_min = a;
        if (b < *new_min) *new_min = b;
    }
}

static void slice_fill(int16_t *img, int64_t H, int64_t W, double shift, int cval) {
    for (int64_t y = 0; y < H; y++) {
        double cc;
        if (ig::row_source(y, -shift, H, &cc)) continue;
        for (int64_t x = 0; x < W; x++) img[y * W + x] = (int16_t)cval;
    }
}

static bool read_samples(std::vector<int16_t> &v) {
    for (auto &s : v) {
        int t;
        if (scanf("%d", &t) != 1) return false;
        s = (int16_t)t;
    }
    return true;
}

static void print_samples(const std::vector<int16_t> &v) {
    for (size_t i = 0; i < v.size(); i++) printf(i ? " %d" : "%d", (int)v[i]);
    printf("\n");
}

int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'S') {
            long long H, W, K;
            if (scanf("%lld %lld %lld", &H, &W, &K) != 3) return 2;
            std::vector<int16_t> in((size_t)(H * W));
            if (!read_samples(in)) return 2;
            for (long long k = 0; k < K; k++) {
                double shift;
                int cval, a, b;
                if (scanf("%lf %d", &shift, &cval) != 2) return 2;
                std::vector<int16_t> out(in);
                slice_interior(out.data(), H, W, shift, &a, &b);
                slice_fill(out.data(), H, W, shift, cval);
                print_samples(out);
            }
        } else if (kind == 'V') {
            long long D, H, W;
            if (scanf("%lld %lld %lld", &D, &H, &W) != 3) return 2;
            std::vector<double> shifts((size_t)D);
            for (auto &s : shifts)
                if (scanf("%lf", &s) != 1) return 2;
            std::vector<int16_t> vol((size_t)(D * H * W));
            if (!read_samples(vol)) return 2;
            std::vector<int> old_min((size_t)D), new_min((size_t)D), cval((size_t)D);
            std::vector<uint8_t> fills((size_t)D);
            for (long long n = 0; n < D; n++) { // every interior first: it does not depend on the fill values
                slice_interior(vol.data() + n * H * W, H, W, shifts[(size_t)n], &old_min[(size_t)n], &new_min[(size_t)n]);
                fills[(size_t)n] = ig::has_fill_rows(H, -shifts[(size_t)n]);
            }
            ig::resolve_cvals(D, old_min.data(), new_min.data(), fills.data(), cval.data());
            for (long long n = 0; n < D; n++) slice_fill(vol.data() + n * H * W, H, W, shifts[(size_t)n], cval[(size_t)n]);
            print_samples(vol);
            for (long long n = 0; n < D; n++) printf(n ? " %d" : "%d", cval[(size_t)n]);
            printf("\n");
        } else
            return 2;
    }
    return 0;
}
