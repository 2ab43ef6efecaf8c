// Host build of the arithmetic k_scene3d.hip adds to the ray casters and the surface view (invesalius3_amd/csrc/scene3d_math.h),
// driven serially.  Test infrastructure (tests/test_scene3d_host.py): where there is no GPU it still shows that the C++ text of
// the rules equals their numpy restatement bit for bit.
// file in : int64 n_hit, n_tex, n_kf, n_ord;
//           n_hit x {double P0[3], dir[3], spacing[3]; int32 orientation, slice, h, w, off, pad}
//           n_tex x {int64 h, w, count; uint8 picture[h * w * 3]; float32 uv[2 * count]}
//           n_kf  x {double tin, dt; int64 kmax; float32 t; int32 pad}
//           n_ord x {uint64 sk[11]}
// file out: n_hit x {int32 hit; float32 t, u, v};  per texture block float32 rgb[3 * count];  n_kf x int64;  n_ord x int32[11]
#include <cstdio>
#include <vector>

#include "../invesalius3_amd/csrc/scene3d_math.h"

using namespace ivx_scene3d;

struct HitIn {
    double P0[3], dir[3], spacing[3];
    int32_t orientation, slice, h, w, off, pad;
};
struct KfIn {
    double tin, dt;
    int64_t kmax;
    float t;
    int32_t pad;
};

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 3;
    int64_t n[4];
    if (fread(n, 8, 4, f) != 4) return 4;
    for (int64_t i = 0; i < n[0]; i++) {
        HitIn q;
        if (fread(&q, sizeof(q), 1, f) != 1) return 4;
        float r[3] = {0.0f, 0.0f, 0.0f};
        const int32_t hit = plane_hit(q.P0, q.dir, q.spacing, q.orientation, q.slice, q.h, q.w, q.off, r[0], r[1], r[2]) ? 1 : 0;
        fwrite(&hit, 4, 1, o);
        fwrite(r, 4, 3, o);
    }
    for (int64_t i = 0; i < n[1]; i++) {
        int64_t m[3];
        if (fread(m, 8, 3, f) != 3) return 4;
        std::vector<uint8_t> pic((size_t)(m[0] * m[1] * 3));
        std::vector<float> uv((size_t)(2 * m[2]) + 1);
        if (fread(pic.data(), 1, pic.size(), f) != pic.size() || fread(uv.data(), 4, (size_t)(2 * m[2]), f) != (size_t)(2 * m[2])) return 4;
        for (int64_t k = 0; k < m[2]; k++) {
            float rgb[3];
            plane_texel(pic.data(), (int)m[0], (int)m[1], uv[2 * k], uv[2 * k + 1], rgb);
            fwrite(rgb, 4, 3, o);
        }
    }
    for (int64_t i = 0; i < n[2]; i++) {
        KfIn q;
        if (fread(&q, sizeof(q), 1, f) != 1) return 4;
        const int64_t k = frag_sample(q.t, q.tin, q.dt, q.kmax);
        fwrite(&k, 8, 1, o);
    }
    for (int64_t i = 0; i < n[3]; i++) {
        uint64_t sk[MAX_FRAGS], prev = 0, m;
        if (fread(sk, 8, MAX_FRAGS, f) != (size_t)MAX_FRAGS) return 4;
        int32_t order[MAX_FRAGS];
        bool first = true;
        for (int r = 0; r < MAX_FRAGS; r++) {
            order[r] = -1;
            if (next_fragment(sk, first, prev, m)) {
                order[r] = (int32_t)(m & LAYER_MASK);
                prev = m;
                first = false;
            } else {
                prev = KEY_EMPTY; // (nothing is above it)
                first = false;
            }
        }
        fwrite(order, 4, MAX_FRAGS, o);
    }
    fclose(f);
    fclose(o);
    return 0;
}
