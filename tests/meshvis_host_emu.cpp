// Host build of the arithmetic the kernels of k_meshvis.hip run (invesalius3_amd/csrc/meshvis_math.h), driven serially: mesh and
// views in, one depth buffer per view and the visibility flags out.  Test infrastructure (tests/test_meshvis_host.py): where
// there is no GPU it still shows that the C++ text of the rules equals their numpy restatement bit for bit.
// file in : int64 nverts, ntris, nviews; float32 verts[3 nverts]; int32 faces[3 ntris]; ivx_mesh_view views[nviews]
// file out: per view uint32 depth[height * width]; uint8 flags[nverts]
#include <cstdio>
#include <vector>

#include "../invesalius3_amd/csrc/meshvis_math.h"

using namespace ivx_meshvis;

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t n[3];
    if (fread(n, 8, 3, f) != 3) return 4;
    std::vector<float> verts(3 * n[0] + 1);
    std::vector<int32_t> faces(3 * n[1] + 1);
    std::vector<ivx_mesh_view> views(n[2] + 1);
    if (fread(verts.data(), 4, 3 * n[0], f) != (size_t)(3 * n[0]) || fread(faces.data(), 4, 3 * n[1], f) != (size_t)(3 * n[1]) ||
        fread(views.data(), sizeof(ivx_mesh_view), n[2], f) != (size_t)n[2])
        return 4;
    fclose(f);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 3;
    std::vector<uint8_t> flags(n[0] + 1, 0);
    for (int64_t q = 0; q < n[2]; q++) {
        const ivx_mesh_view &V = views[q];
        std::vector<uint32_t> depth((size_t)V.width * V.height, DEPTH_ONE);
        for (int64_t t = 0; t < n[1]; t++) {
            Tri T;
            if (!load_tri(V, verts.data(), n[0], faces.data(), t, T)) continue;
            for (int j = T.y0; j <= T.y1; j++)
                for (int i = T.x0; i <= T.x1; i++) {
                    uint32_t bits;
                    if (pixel_depth_bits(T, i, j, bits) && bits < depth[(size_t)j * V.width + i]) depth[(size_t)j * V.width + i] = bits;
                }
        }
        fwrite(depth.data(), 4, depth.size(), o);
        for (int64_t v = 0; v < n[0]; v++)
            if (!flags[v] && point_visible(V, verts.data() + 3 * v, (const float *)depth.data())) flags[v] = 1;
    }
    fwrite(flags.data(), 1, n[0], o);
    fclose(o);
    return 0;
}
