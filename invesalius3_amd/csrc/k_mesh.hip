// k_mesh.hip -- what join_process_surface (invesalius/data/surface_process.py:204-472) does to the joined surface
// after the point merge, for the two stages that are plain scans over the mesh:
//   * "keep largest"      vtkPolyDataConnectivityFilter, SetExtractionModeToLargestRegion  (surface_process.py:376-391)
//   * area / volume       vtkMassProperties                                                (surface_process.py:452-458)
// Both VTK classes are third party and absent from the reference tree; the algorithms restated here are the
// published ones (connected regions over shared points, largest by CELL count, first region wins a tie;
// Alyassin et al. 1994 discrete-divergence volume with max-unit-normal-component weighting + Heron areas).
//
// MI355X design: both are HBM/L2-bound integer+double streams, no MFMA.
//   components   lock-free union-find over VERTEX ids (atomicMin links only -- plain stores into parent[] lose
//                links, see k_ccl.hip), one lane per triangle; roots flattened once; triangles per root counted with
//                workgroup-level pre-aggregation of the dominant root (otherwise ~every triangle of a real surface
//                would hit ONE address); compaction = two exclusive scans (faces kept, vertices used).
//   mass         one lane per triangle, double accumulators, fixed-shape tree reduction (wave shuffle -> LDS ->
//                per-workgroup partials -> one workgroup) so the result is reproducible run to run.
#include <algorithm>

#include "ivx_internal.h"
#include "mesh_compact.h"
#include "mesh_regions.h"
#include "scan_u32.h"

namespace {

// best = max over regions of (cells << 32) | ~first_cell  ->  most cells, then the earliest first cell
__global__ __launch_bounds__(256) void k_mesh_best(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ mintri,
                                                   int64_t nv, unsigned long long *__restrict__ best,
                                                   uint32_t *__restrict__ nreg) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long key = 0ull;
    uint32_t regions = 0;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
        const uint32_t c = cnt[v];
        if (c) {
            regions++;
            const unsigned long long k = ((unsigned long long)c << 32) | (unsigned long long)(~mintri[v]);
            key = k > key ? k : key;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long k = __shfl_xor(key, o, 64);
        key = k > key ? k : key;
        regions += __shfl_xor(regions, o, 64);
    }
    // one atomic pair per WORKGROUP (the grid is capped at 1024 of them): ~50 k same-address atomics took 1 ms
    __shared__ unsigned long long s_key[4];
    __shared__ uint32_t s_reg[4];
    if ((threadIdx.x & 63) == 0) {
        s_key[threadIdx.x >> 6] = key;
        s_reg[threadIdx.x >> 6] = regions;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; q++) {
            key = s_key[q] > key ? s_key[q] : key;
            regions += s_reg[q];
        }
        if (key) atomicMax(best, key);
        if (regions) atomicAdd(nreg, regions);
    }
}

// keep[t] = 1 for the triangles of the winning region (recognised by its first cell); used[v] = 1 for their vertices
__global__ __launch_bounds__(256) void k_mesh_mark(const int32_t *__restrict__ faces, int64_t nt,
                                                   const uint32_t *__restrict__ root, const uint32_t *__restrict__ mintri,
                                                   const unsigned long long *__restrict__ best, uint32_t *__restrict__ keep,
                                                   uint32_t *__restrict__ usedv) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > nt) return;
    if (t == nt) {
        keep[t] = 0u;
        return;
    }
    const uint32_t first = ~(uint32_t)(*best & 0xffffffffull);
    const uint32_t a = (uint32_t)faces[3 * t], b = (uint32_t)faces[3 * t + 1], c = (uint32_t)faces[3 * t + 2];
    const bool k = mintri[root[a]] == first;
    keep[t] = k ? 1u : 0u;
    if (k) {
        usedv[a] = 1u;
        usedv[b] = 1u;
        usedv[c] = 1u;
    }
}

// ---- mass properties (tri_mass, block_reduce_np, mass_finish: mesh_regions.h) ------------------------------------------
constexpr int MASS_TPL = 4;
__global__ __launch_bounds__(256) void k_mesh_mass(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                   int64_t nt, double *__restrict__ partial) {
    double acc[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) acc[q] = 0.0;
    const int64_t base = (int64_t)blockIdx.x * 256 * MASS_TPL;
#pragma unroll
    for (int q = 0; q < MASS_TPL; q++) {
        const int64_t t = base + (int64_t)q * 256 + threadIdx.x;
        if (t < nt) tri_mass(verts, faces, t, acc);
    }
    block_reduce_np(acc, partial + (int64_t)blockIdx.x * NP);
}
__global__ __launch_bounds__(256) void k_mesh_mass_final(const double *__restrict__ partial, int64_t nb, double ncells,
                                                         double *__restrict__ out) {
    __shared__ double s_tot[NP];
    double acc[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) acc[q] = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += 256)
#pragma unroll
        for (int q = 0; q < NP; q++) acc[q] += partial[b * NP + q];
    block_reduce_np(acc, s_tot);
    __syncthreads();
    if (threadIdx.x == 0) mass_finish(s_tot, ncells, out);
}

struct MeshLayout { // per-stream WS_MESH
    size_t off_parent, off_root, off_cnt, off_min, off_keep, off_used, off_bsum, off_misc, total;
};
static MeshLayout mesh_layout(int64_t nv, int64_t nt) {
    MeshLayout m;
    const size_t v4 = al256(((size_t)nv + 1) * 4), t4 = al256(((size_t)nt + 1) * 4);
    m.off_parent = 0;
    m.off_root = m.off_parent + v4;
    m.off_cnt = m.off_root + v4;
    m.off_min = m.off_cnt + v4;
    m.off_used = m.off_min + v4;
    m.off_keep = m.off_used + v4;
    m.off_bsum = m.off_keep + t4;
    const int64_t nmax = nv > nt ? nv : nt;
    m.off_misc = m.off_bsum + al256(((size_t)scan_u32_blocks(nmax + 1) + 16) * 4);
    m.total = m.off_misc + 256;
    return m;
}

} // namespace

extern "C" int ivx_dev_mesh_keep_largest(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                                         float *out_verts, int64_t max_verts, int32_t *out_faces, int64_t max_tris,
                                         int64_t *out_nverts, int64_t *out_ntris, int64_t *nregions, void *stream) {
    IVX_REQUIRE(nverts >= 0 && ntris >= 0, IVX_EINVAL, "mesh: negative size");
    IVX_REQUIRE(nverts < 0x7fffffffll && ntris < 0x7fffffffll, IVX_EINVAL, "mesh: more than 2^31 vertices / triangles");
    *out_nverts = 0;
    *out_ntris = 0;
    if (nregions) *nregions = 0;
    if (ntris == 0) return IVX_OK;
    hipStream_t st = ivx::S(stream);
    const MeshLayout m = mesh_layout(nverts, ntris);
    void *ws;
    int rc;
    if ((rc = ivx::ws_get_s(ivx::WS_MESH, st, m.total, &ws))) return rc;
    char *w = (char *)ws;
    uint32_t *parent = (uint32_t *)(w + m.off_parent), *root = (uint32_t *)(w + m.off_root);
    uint32_t *cnt = (uint32_t *)(w + m.off_cnt), *mintri = (uint32_t *)(w + m.off_min);
    uint32_t *usedv = (uint32_t *)(w + m.off_used), *keep = (uint32_t *)(w + m.off_keep);
    uint32_t *bsum = (uint32_t *)(w + m.off_bsum);
    unsigned long long *best = (unsigned long long *)(w + m.off_misc);
    uint32_t *nreg = (uint32_t *)(w + m.off_misc + 8), *tot_t = nreg + 1, *tot_v = nreg + 2;
    const unsigned gv = (unsigned)std::min<int64_t>(ivx::cdiv(nverts + 1, 256), 16384);
    const unsigned gt = (unsigned)ivx::cdiv(ntris + 1, 256);
    hipLaunchKernelGGL(k_mesh_init, dim3(gv), dim3(256), 0, st, parent, cnt, mintri, usedv, nverts, best, nreg);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_union, dim3(gt), dim3(256), 0, st, faces, ntris, parent);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_flatten, dim3(gv), dim3(256), 0, st, parent, root, nverts);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_tricount, dim3((unsigned)ivx::cdiv(ntris, 256 * TPL)), dim3(256), 0, st, faces, ntris, root, cnt,
                       mintri);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_best, dim3(std::min(gv, 1024u)), dim3(256), 0, st, cnt, mintri, nverts, best, nreg);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_mark, dim3(gt), dim3(256), 0, st, faces, ntris, root, mintri, best, keep, usedv);
    IVX_LAUNCH_CHECK();
    if ((rc = scan_u32_exclusive(keep, ntris + 1, bsum, tot_t, st))) return rc;
    if ((rc = scan_u32_exclusive(usedv, nverts + 1, bsum, tot_v, st))) return rc;
    uint32_t seq, got[3];
    if ((rc = ivx::mailbox_publish(nreg, 3, st, &seq))) return rc;
    if ((rc = ivx::mailbox_wait(seq, st, got, 3))) return rc;
    if (nregions) *nregions = got[0];
    *out_ntris = got[1];
    *out_nverts = got[2];
    if (!out_verts || !out_faces) return IVX_OK;
    IVX_REQUIRE(max_tris >= (int64_t)got[1] && max_verts >= (int64_t)got[2], IVX_ERANGE,
                "mesh: output buffers too small (%u verts, %u triangles needed)", got[2], got[1]);
    hipLaunchKernelGGL(k_mesh_compact_faces, dim3((unsigned)ivx::cdiv(ntris, 256)), dim3(256), 0, st, faces, ntris, keep, usedv,
                       out_faces, max_tris);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_compact_verts, dim3((unsigned)ivx::cdiv(nverts, 256)), dim3(256), 0, st, verts, nverts, usedv,
                       out_verts, max_verts);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_mesh_mass_properties(const float *verts, const int32_t *faces, int64_t ntris, double *out8,
                                            void *stream) {
    IVX_REQUIRE(ntris >= 0, IVX_EINVAL, "mesh: negative size");
    hipStream_t st = ivx::S(stream);
    if (ntris == 0) {
        IVX_HIP(hipMemsetAsync(out8, 0, 8 * sizeof(double), st));
        return IVX_OK;
    }
    const int64_t nb = ivx::cdiv(ntris, 256 * MASS_TPL);
    void *ws;
    int rc;
    if ((rc = ivx::ws_get_s(ivx::WS_MESH2, st, (size_t)nb * NP * 8, &ws))) return rc;
    hipLaunchKernelGGL(k_mesh_mass, dim3((unsigned)nb), dim3(256), 0, st, verts, faces, ntris, (double *)ws);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_mass_final, dim3(1), dim3(256), 0, st, (const double *)ws, nb, (double)ntris, out8);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

// ---- host forms -----------------------------------------------------------------------------------------------------
extern "C" int ivx_mesh_keep_largest(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                                     float *out_verts, int32_t *out_faces, int64_t *out_nverts, int64_t *out_ntris,
                                     int64_t *nregions) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(nverts >= 0 && ntris >= 0, IVX_EINVAL, "mesh: negative size");
    *out_nverts = *out_ntris = 0;
    if (nregions) *nregions = 0;
    if (ntris == 0) return IVX_OK;
    for (int64_t q = 0; q < 3 * ntris; q++)
        IVX_REQUIRE(faces[q] >= 0 && faces[q] < nverts, IVX_EDOM, "mesh: face index %d outside [0, %lld)", faces[q],
                    (long long)nverts);
    void *d_v, *d_f, *d_ov, *d_of;
    int rc;
    if ((rc = ws_get(WS_IN, (size_t)nverts * 12 + 16, &d_v))) return rc;
    if ((rc = ws_get(WS_AUX0, (size_t)ntris * 12 + 16, &d_f))) return rc;
    if ((rc = ws_get(WS_OUT, (size_t)nverts * 12 + 16, &d_ov))) return rc;
    if ((rc = ws_get(WS_AUX1, (size_t)ntris * 12 + 16, &d_of))) return rc;
    IVX_HIP(hipMemcpy(d_v, verts, (size_t)nverts * 12, hipMemcpyHostToDevice));
    IVX_HIP(hipMemcpy(d_f, faces, (size_t)ntris * 12, hipMemcpyHostToDevice));
    if ((rc = ivx_dev_mesh_keep_largest((const float *)d_v, nverts, (const int32_t *)d_f, ntris, (float *)d_ov, nverts,
                                        (int32_t *)d_of, ntris, out_nverts, out_ntris, nregions, nullptr)))
        return rc;
    IVX_HIP(hipDeviceSynchronize());
    if (out_verts && *out_nverts) IVX_HIP(hipMemcpy(out_verts, d_ov, (size_t)*out_nverts * 12, hipMemcpyDeviceToHost));
    if (out_faces && *out_ntris) IVX_HIP(hipMemcpy(out_faces, d_of, (size_t)*out_ntris * 12, hipMemcpyDeviceToHost));
    return IVX_OK;
}

extern "C" int ivx_mesh_mass_properties(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                                        double *out8) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(nverts >= 0 && ntris >= 0, IVX_EINVAL, "mesh: negative size");
    for (int q = 0; q < 8; q++) out8[q] = 0.0;
    if (ntris == 0) return IVX_OK;
    if (faces) {
        for (int64_t q = 0; q < 3 * ntris; q++)
            IVX_REQUIRE(faces[q] >= 0 && faces[q] < nverts, IVX_EDOM, "mesh: face index %d outside [0, %lld)", faces[q],
                        (long long)nverts);
    } else {
        IVX_REQUIRE(nverts == 3 * ntris, IVX_EINVAL, "mesh: a soup needs 3 vertices per triangle");
    }
    void *d_v, *d_f = nullptr, *d_o;
    int rc;
    if ((rc = ws_get(WS_IN, (size_t)nverts * 12 + 16, &d_v))) return rc;
    if (faces && (rc = ws_get(WS_AUX0, (size_t)ntris * 12 + 16, &d_f))) return rc;
    if ((rc = ws_get(WS_SMALL, 64, &d_o))) return rc;
    IVX_HIP(hipMemcpy(d_v, verts, (size_t)nverts * 12, hipMemcpyHostToDevice));
    if (faces) IVX_HIP(hipMemcpy(d_f, faces, (size_t)ntris * 12, hipMemcpyHostToDevice));
    if ((rc = ivx_dev_mesh_mass_properties((const float *)d_v, (const int32_t *)d_f, ntris, (double *)d_o, nullptr))) return rc;
    IVX_HIP(hipMemcpy(out8, d_o, 64, hipMemcpyDeviceToHost));
    return IVX_OK;
}
