// mesh_compact.h -- the compaction that ends every "keep some triangles" stage of the indexed mesh (keep largest, k_mesh.hip;
// select by point flags, k_meshvis.hip): koff / voff are the exclusive scans of the triangles' keep marks (ntris + 1 entries) and
// of the vertices' used marks (nverts + 1 entries).  Kept triangles stay in order, the vertices they use are compacted in order.
// Included by the translation units that need it (kernels live in each unit's anonymous namespace).
#pragma once
#include "ivx_internal.h"

namespace {

__global__ __launch_bounds__(256) void k_mesh_compact_faces(const int32_t *__restrict__ faces, int64_t nt,
                                                            const uint32_t *__restrict__ koff,
                                                            const uint32_t *__restrict__ voff, int32_t *__restrict__ out,
                                                            int64_t max_out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const uint32_t o = koff[t];
    if (koff[t + 1] == o || (int64_t)o >= max_out) return;
#pragma unroll
    for (int q = 0; q < 3; q++) out[3 * (int64_t)o + q] = (int32_t)voff[(uint32_t)faces[3 * t + q]];
}

__global__ __launch_bounds__(256) void k_mesh_compact_verts(const float *__restrict__ verts, int64_t nv,
                                                            const uint32_t *__restrict__ voff, float *__restrict__ out,
                                                            int64_t max_out) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const uint32_t o = voff[v];
    if (voff[v + 1] == o || (int64_t)o >= max_out) return;
#pragma unroll
    for (int q = 0; q < 3; q++) out[3 * (int64_t)o + q] = verts[3 * v + q];
}

} // namespace
