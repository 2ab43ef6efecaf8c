// Host build of the arithmetic the kernels of k_surfview.hip run (invesalius3_amd/csrc/surfview_math.h), driven serially: a scene
// in, the key buffers and the picture out.  Test infrastructure (tests/test_surface_view_host.py): where there is no GPU it still
// shows that the C++ text of the rules equals their numpy restatement bit for bit.
// file in : ivx_surface_camera; int64 nlayers, mode; float32 background[3];
//           per layer int64 nverts, ntris, has_normals; float32 rgb[3], opacity; verts[3 nverts]; int32 faces[3 ntris];
//           float32 normals[3 nverts] when has_normals
// file out: per layer uint64 keys[height * width]; float32 rgba[h * w * 4]; uint8 rgba8[h * w * 4]; int32 ids[h * w * 2];
//           float32 depth[h * w]
#include <cstdio>
#include <vector>

#include "../invesalius3_amd/csrc/surfview_math.h"

using namespace ivx_surfview;

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    ivx_surface_camera C;
    int64_t n[2];
    float bg[3];
    if (fread(&C, sizeof(C), 1, f) != 1 || fread(n, 8, 2, f) != 2 || fread(bg, 4, 3, f) != 3) return 4;
    if (n[0] < 0 || n[0] > IVX_SURFACE_MAX_LAYERS) return 5;
    const size_t npix = (size_t)C.width * C.height;
    std::vector<std::vector<float>> verts(n[0]), normals(n[0]);
    std::vector<std::vector<int32_t>> faces(n[0]);
    std::vector<std::vector<uint64_t>> keys(n[0]);
    ivx_surface_layer layers[IVX_SURFACE_MAX_LAYERS];
    for (int64_t k = 0; k < n[0]; k++) {
        int64_t m[3];
        float col[4];
        if (fread(m, 8, 3, f) != 3 || fread(col, 4, 4, f) != 4) return 4;
        verts[k].resize(3 * m[0] + 1);
        faces[k].resize(3 * m[1] + 1);
        normals[k].resize(3 * m[0] + 1);
        if (fread(verts[k].data(), 4, 3 * m[0], f) != (size_t)(3 * m[0]) || fread(faces[k].data(), 4, 3 * m[1], f) != (size_t)(3 * m[1]))
            return 4;
        if (m[2] && fread(normals[k].data(), 4, 3 * m[0], f) != (size_t)(3 * m[0])) return 4;
        keys[k].assign(npix, KEY_EMPTY);
        ivx_surface_layer &L = layers[k];
        L.verts = verts[k].data();
        L.nverts = m[0];
        L.faces = faces[k].data();
        L.ntris = m[1];
        L.normals = m[2] ? normals[k].data() : nullptr;
        L.keys = keys[k].data();
        L.rgb[0] = col[0], L.rgb[1] = col[1], L.rgb[2] = col[2], L.opacity = col[3];
    }
    fclose(f);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 3;
    for (int64_t k = 0; k < n[0]; k++) {
        const ivx_surface_layer &L = layers[k];
        for (int64_t t = 0; t < L.ntris; t++) {
            Tri T;
            if (!load_tri(C, L.verts, L.nverts, L.faces, t, T)) continue;
            for (int j = T.y0; j <= T.y1; j++)
                for (int i = T.x0; i <= T.x1; i++) {
                    uint64_t key;
                    if (pixel_key(T, i, j, (uint32_t)t, key) && key < keys[k][(size_t)j * C.width + i]) keys[k][(size_t)j * C.width + i] = key;
                }
        }
        fwrite(keys[k].data(), 8, npix, o);
    }
    std::vector<float> rgba(4 * npix), depth(npix);
    std::vector<uint8_t> rgba8(4 * npix);
    std::vector<int32_t> ids(2 * npix);
    for (int j = 0; j < C.height; j++)
        for (int i = 0; i < C.width; i++) {
            const size_t p = (size_t)j * C.width + i;
            resolve_pixel(C, layers, (int)n[0], (int)n[1], bg, i, j, &rgba[4 * p], &ids[2 * p], &depth[p]);
            for (int q = 0; q < 4; q++) rgba8[4 * p + q] = to_u8(rgba[4 * p + q]);
        }
    fwrite(rgba.data(), 4, rgba.size(), o);
    fwrite(rgba8.data(), 1, rgba8.size(), o);
    fwrite(ids.data(), 4, ids.size(), o);
    fwrite(depth.data(), 4, depth.size(), o);
    fclose(o);
    return 0;
}
