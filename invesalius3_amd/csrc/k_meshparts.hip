// k_meshparts.hip -- the reference's "surface connectivity" tools beyond keep-largest (invesalius/data/surface.py:319-411,
// polydata_utils.py:206-278), DESIGN 7h:
//   * region labels   vtkPolyDataConnectivityFilter's region ids: region r = the r-th region in the order of its first triangle
//   * split           SplitDisconectedParts (AddSpecifiedRegion(r) for every r): ALL parts in one grouped mesh + a part table
//   * parts mass      vtkMassProperties of every part (surface.py:953-960) without a launch per part
//   * select seeded   JoinSeedsParts (SetExtractionModeToPointSeededRegions): the regions that hold a seed point
//   * nearest point   the point pick that turns a coordinate into a seed id
// VTK is third party and absent: the rules are the ones DESIGN 7h states, pinned against tests/_mesh_regions_ref.py.
//
// MI355X design: integer streams over HBM / L2, no MFMA.  Components are k_mesh.hip's union-find (mesh_regions.h); a region's
// number is the exclusive scan of "this triangle is its region's first"; grouping is a stable many-way partition by region id
// (partition_u32.h), once over the vertices (unused ones keyed past the last region and dropped) and once over the triangles;
// the mass of a small part is one wave's fixed-shape reduction, a large part's is k_mesh_mass's two kernels on its slice, the
// workgroups of all large parts in ONE launch (a workgroup finds its part by bisection of the scanned workgroup counts).
#include <algorithm>
#include <vector>

#include "ivx_internal.h"
#include "mesh_compact.h"
#include "mesh_regions.h"
#include "partition_u32.h"
#include "scan_u32.h"

namespace {

// flag[t] = 1 for the first triangle of every region; flag[nt] = 0 (the scan's total slot)
__global__ __launch_bounds__(256) void k_parts_flag(const int32_t *__restrict__ faces, int64_t nt, const uint32_t *__restrict__ root,
                                                    const uint32_t *__restrict__ mintri, uint32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > nt) return;
    flag[t] = (t < nt && mintri[root[(uint32_t)faces[3 * t]]] == (uint32_t)t) ? 1u : 0u;
}

// rank = the scanned flags: rank[first triangle of a region] is the region's number
__global__ __launch_bounds__(256) void k_parts_tlabel(const int32_t *__restrict__ faces, int64_t nt, const uint32_t *__restrict__ root,
                                                      const uint32_t *__restrict__ mintri, const uint32_t *__restrict__ rank,
                                                      uint32_t *__restrict__ label) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    label[t] = rank[mintri[root[(uint32_t)faces[3 * t]]]];
}

// per vertex: label (-1 when no triangle uses it) and / or partition key (*nreg for an unused vertex); *nused += used vertices
__global__ __launch_bounds__(256) void k_parts_vlabel(int64_t nv, const uint32_t *__restrict__ root, const uint32_t *__restrict__ cnt,
                                                      const uint32_t *__restrict__ mintri, const uint32_t *__restrict__ rank,
                                                      const uint32_t *__restrict__ nreg, int32_t *__restrict__ vlabel,
                                                      uint32_t *__restrict__ vkey, uint32_t *__restrict__ nused) {
    __shared__ uint32_t s_used;
    if (threadIdx.x == 0) s_used = 0u;
    __syncthreads();
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool used = false;
    if (v < nv) {
        const uint32_t r = root[v];
        used = cnt[r] != 0u;
        const uint32_t lab = used ? rank[mintri[r]] : 0u;
        if (vlabel) vlabel[v] = used ? (int32_t)lab : -1;
        if (vkey) vkey[v] = used ? lab : *nreg;
    }
    const unsigned long long b = __ballot(used);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&s_used, (uint32_t)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && s_used) atomicAdd(nused, s_used);
}

// sorted position p of the vertex partition: the point goes to slot p of the grouped array, its part-local id is p - offs[key]
__global__ __launch_bounds__(256) void k_parts_place_verts(const uint32_t *__restrict__ order, const uint32_t *__restrict__ sorted,
                                                           int64_t nv, const uint32_t *__restrict__ offs, uint32_t nreg,
                                                           const float *__restrict__ verts, uint32_t *__restrict__ newidx,
                                                           float *__restrict__ out, int64_t max_out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nv) return;
    const uint32_t v = order[p], k = sorted[p];
    if (k >= nreg || (int64_t)v >= nv) return; // unused points are dropped
    newidx[v] = (uint32_t)p - offs[k];
    if (p >= max_out) return;
#pragma unroll
    for (int q = 0; q < 3; q++) out[3 * p + q] = verts[3 * (int64_t)v + q];
}

__global__ __launch_bounds__(256) void k_parts_place_faces(const uint32_t *__restrict__ order, int64_t nt, const int32_t *__restrict__ faces,
                                                           const uint32_t *__restrict__ newidx, int32_t *__restrict__ out,
                                                           int64_t max_out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nt || p >= max_out) return;
    const uint32_t t = order[p];
    if ((int64_t)t >= nt) return;
#pragma unroll
    for (int q = 0; q < 3; q++) out[3 * p + q] = (int32_t)newidx[(uint32_t)faces[3 * (int64_t)t + q]];
}

__global__ __launch_bounds__(256) void k_parts_table(const uint32_t *__restrict__ offs_t, const uint32_t *__restrict__ offs_v,
                                                     int64_t nreg, int64_t *__restrict__ table) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nreg) return;
    table[4 * r] = offs_t[r];
    table[4 * r + 1] = (int64_t)offs_t[r + 1] - (int64_t)offs_t[r];
    table[4 * r + 2] = offs_v[r];
    table[4 * r + 3] = (int64_t)offs_v[r + 1] - (int64_t)offs_v[r];
}

// ---- per-part mass --------------------------------------------------------------------------------------------------
// parts of up to small_max triangles: one wave each, lanes stride the part's triangles, shuffle tree
__global__ __launch_bounds__(256) void k_parts_mass_small(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                          const int64_t *__restrict__ table, int64_t nparts, int64_t small_max,
                                                          double *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= nparts) return;
    const int64_t toff = table[4 * r], nt = table[4 * r + 1], voff = table[4 * r + 2];
    if (nt > small_max) return;
    double acc[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) acc[q] = 0.0;
    for (int64_t t = threadIdx.x & 63; t < nt; t += 64) tri_mass(verts + 3 * voff, faces + 3 * toff, t, acc);
#pragma unroll
    for (int q = 0; q < NP; q++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_xor(acc[q], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (nt > 0) mass_finish(acc, (double)nt, out + 8 * r);
        else
            for (int q = 0; q < 8; q++) out[8 * r + q] = 0.0;
    }
}

// larger parts: k_mesh_mass's workgroups (1024 triangles each, the same lane order) on the part's slice
constexpr int PARTS_MASS_TPL = 4;
constexpr int PARTS_MASS_BLOCK = 256 * PARTS_MASS_TPL;
constexpr int64_t PARTS_SMALL_MAX = 1024; // default of small_max

__global__ __launch_bounds__(256) void k_parts_mass_nblocks(const int64_t *__restrict__ table, int64_t nparts, int64_t small_max,
                                                            uint32_t *__restrict__ boff) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nparts) return;
    const int64_t nt = r < nparts ? table[4 * r + 1] : 0;
    boff[r] = nt > small_max ? (uint32_t)((nt + PARTS_MASS_BLOCK - 1) / PARTS_MASS_BLOCK) : 0u;
}
__global__ __launch_bounds__(256) void k_parts_mass_large(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                          const int64_t *__restrict__ table, int64_t nparts,
                                                          const uint32_t *__restrict__ boff, double *__restrict__ partial) {
    const uint32_t b = blockIdx.x;
    if (b >= boff[nparts]) return;
    int64_t lo = 0, hi = nparts; // the part r with boff[r] <= b < boff[r + 1]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (boff[mid] <= b) lo = mid;
        else hi = mid;
    }
    const int64_t r = lo, toff = table[4 * r], nt = table[4 * r + 1], voff = table[4 * r + 2];
    double acc[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) acc[q] = 0.0;
    const int64_t base = (int64_t)(b - boff[r]) * PARTS_MASS_BLOCK;
#pragma unroll
    for (int q = 0; q < PARTS_MASS_TPL; q++) {
        const int64_t t = base + (int64_t)q * 256 + threadIdx.x;
        if (t < nt) tri_mass(verts + 3 * voff, faces + 3 * toff, t, acc);
    }
    block_reduce_np(acc, partial + (int64_t)b * NP);
}
__global__ __launch_bounds__(256) void k_parts_mass_final(const double *__restrict__ partial, const int64_t *__restrict__ table,
                                                          const uint32_t *__restrict__ boff, double *__restrict__ out) {
    const int64_t r = blockIdx.x;
    const int64_t b0 = boff[r], nb = (int64_t)boff[r + 1] - b0;
    if (nb <= 0) return; // a small part: k_parts_mass_small wrote it
    __shared__ double s_tot[NP];
    double acc[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) acc[q] = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += 256)
#pragma unroll
        for (int q = 0; q < NP; q++) acc[q] += partial[(b0 + b) * NP + q];
    block_reduce_np(acc, s_tot);
    __syncthreads();
    if (threadIdx.x == 0) mass_finish(s_tot, (double)table[4 * r + 1], out + 8 * r);
}

// ---- seeded select ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_parts_seed_mark(const int32_t *__restrict__ seeds, int64_t nseeds, int64_t nv,
                                                         const uint32_t *__restrict__ root, uint32_t *__restrict__ mark) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseeds) return;
    const int64_t v = seeds[s];
    if (v >= 0 && v < nv) mark[root[v]] = 1u;
}
__global__ __launch_bounds__(256) void k_parts_seed_keep(const int32_t *__restrict__ faces, int64_t nt, const uint32_t *__restrict__ root,
                                                         const uint32_t *__restrict__ mark, uint32_t *__restrict__ keep,
                                                         uint32_t *__restrict__ usedv) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > nt) return;
    if (t == nt) {
        keep[t] = 0u;
        return;
    }
    const uint32_t a = (uint32_t)faces[3 * t], b = (uint32_t)faces[3 * t + 1], c = (uint32_t)faces[3 * t + 2];
    const bool k = mark[root[a]] != 0u;
    keep[t] = k ? 1u : 0u;
    if (k) {
        usedv[a] = 1u;
        usedv[b] = 1u;
        usedv[c] = 1u;
    }
}

// ---- nearest point ---------------------------------------------------------------------------------------------------
// (distance^2 in double, id), smaller distance first, then the smaller id: exact and order-free
constexpr int NEAR_BLOCKS = 1024;
__device__ __forceinline__ void near_take(double &d, uint32_t &id, double d2, uint32_t id2) {
    if (d2 < d || (d2 == d && id2 < id)) {
        d = d2;
        id = id2;
    }
}
__device__ __forceinline__ void near_block(double &d, uint32_t &id) {
    __shared__ double s_d[4];
    __shared__ uint32_t s_id[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double d2 = __shfl_xor(d, o, 64);
        const uint32_t i2 = __shfl_xor(id, o, 64);
        near_take(d, id, d2, i2);
    }
    if ((threadIdx.x & 63) == 0) {
        s_d[threadIdx.x >> 6] = d;
        s_id[threadIdx.x >> 6] = id;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < 4; q++) near_take(d, id, s_d[q], s_id[q]);
}
__global__ __launch_bounds__(256) void k_parts_nearest(const float *__restrict__ verts, int64_t nv, double qx, double qy, double qz,
                                                       double *__restrict__ pd, uint32_t *__restrict__ pid) {
    double d = __builtin_huge_val();
    uint32_t id = 0xffffffffu;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
        const double dx = (double)verts[3 * v] - qx, dy = (double)verts[3 * v + 1] - qy, dz = (double)verts[3 * v + 2] - qz;
        near_take(d, id, (dx * dx + dy * dy) + dz * dz, (uint32_t)v);
    }
    near_block(d, id);
    if (threadIdx.x == 0) {
        pd[blockIdx.x] = d;
        pid[blockIdx.x] = id;
    }
}
__global__ __launch_bounds__(256) void k_parts_nearest_final(const double *__restrict__ pd, const uint32_t *__restrict__ pid, int nb,
                                                             int32_t *__restrict__ out) {
    double d = __builtin_huge_val();
    uint32_t id = 0xffffffffu;
    for (int b = threadIdx.x; b < nb; b += 256) near_take(d, id, pd[b], pid[b]);
    near_block(d, id);
    if (threadIdx.x == 0) *out = id == 0xffffffffu ? -1 : (int32_t)id;
}

// ---- workspace -------------------------------------------------------------------------------------------------------
struct PartsLayout { // per-stream WS_MESH; the words from off_key on only when `with_partition`
    size_t off_parent, off_root, off_cnt, off_min, off_used, off_rank, off_bsum, off_misc, off_key[2], off_val[2], off_hist, off_ot,
        off_ov, total;
};
// words of misc: 0-1 k_mesh_init's best, 2 its region counter, 3 the number of regions (the scan's total), 4 used vertices,
// 5-6 the totals of the compaction scans
static PartsLayout parts_layout(int64_t nv, int64_t nt, bool with_partition) {
    PartsLayout m;
    const size_t v4 = al256(((size_t)nv + 1) * 4), t4 = al256(((size_t)nt + 1) * 4);
    const int64_t nmax = std::max<int64_t>(std::max(nv, nt), 1);
    m.off_parent = 0;
    m.off_root = m.off_parent + v4;
    m.off_cnt = m.off_root + v4;
    m.off_min = m.off_cnt + v4;
    m.off_used = m.off_min + v4;
    m.off_rank = m.off_used + v4;
    m.off_bsum = m.off_rank + t4;
    m.off_misc = m.off_bsum + al256(((size_t)scan_u32_blocks(nmax + 1) + 16) * 4);
    size_t end = m.off_misc + 256;
    m.off_key[0] = m.off_key[1] = m.off_val[0] = m.off_val[1] = m.off_hist = m.off_ot = m.off_ov = end;
    if (with_partition) {
        const size_t n4 = al256((size_t)nmax * 4);
        m.off_key[0] = end;
        m.off_key[1] = m.off_key[0] + n4;
        m.off_val[0] = m.off_key[1] + n4;
        m.off_val[1] = m.off_val[0] + n4;
        m.off_hist = m.off_val[1] + n4;
        m.off_ot = m.off_hist + al256(partition_u32_hist_words(nmax) * 4);
        m.off_ov = m.off_ot + al256(((size_t)nt + 2) * 4);
        end = m.off_ov + al256(((size_t)nv + 3) * 4);
    }
    m.total = end;
    return m;
}
struct PartsWs {
    uint32_t *parent, *root, *cnt, *mintri, *usedv, *rank, *bsum, *misc, *key[2], *val[2], *hist, *offs_t, *offs_v;
};
static int parts_ws(int64_t nv, int64_t nt, bool with_partition, hipStream_t st, PartsWs *W) {
    const PartsLayout m = parts_layout(nv, nt, with_partition);
    void *ws;
    int rc;
    if ((rc = ivx::ws_get_s(ivx::WS_MESH, st, m.total, &ws))) return rc;
    char *w = (char *)ws;
    W->parent = (uint32_t *)(w + m.off_parent);
    W->root = (uint32_t *)(w + m.off_root);
    W->cnt = (uint32_t *)(w + m.off_cnt);
    W->mintri = (uint32_t *)(w + m.off_min);
    W->usedv = (uint32_t *)(w + m.off_used);
    W->rank = (uint32_t *)(w + m.off_rank);
    W->bsum = (uint32_t *)(w + m.off_bsum);
    W->misc = (uint32_t *)(w + m.off_misc);
    for (int q = 0; q < 2; q++) {
        W->key[q] = (uint32_t *)(w + m.off_key[q]);
        W->val[q] = (uint32_t *)(w + m.off_val[q]);
    }
    W->hist = (uint32_t *)(w + m.off_hist);
    W->offs_t = (uint32_t *)(w + m.off_ot);
    W->offs_v = (uint32_t *)(w + m.off_ov);
    return IVX_OK;
}

static int check_sizes(int64_t nverts, int64_t ntris) {
    IVX_REQUIRE(nverts >= 0 && ntris >= 0, IVX_EINVAL, "mesh: negative size");
    IVX_REQUIRE(nverts < 0x7fffffffll && ntris < 0x7fffffffll, IVX_EINVAL, "mesh: more than 2^31 vertices / triangles");
    return IVX_OK;
}
static int check_faces(const int32_t *faces, int64_t ntris, int64_t nverts) {
    for (int64_t q = 0; q < 3 * ntris; q++)
        IVX_REQUIRE(faces[q] >= 0 && faces[q] < nverts, IVX_EDOM, "mesh: face index %d outside [0, %lld)", faces[q], (long long)nverts);
    return IVX_OK;
}

// the union-find up to the flattened roots (ntris > 0)
static int roots_stage(const int32_t *faces, int64_t nv, int64_t nt, const PartsWs &W, hipStream_t st) {
    const unsigned gv = (unsigned)std::min<int64_t>(ivx::cdiv(nv + 1, 256), 16384);
    IVX_HIP(hipMemsetAsync(W.misc, 0, 256, st));
    hipLaunchKernelGGL(k_mesh_init, dim3(gv), dim3(256), 0, st, W.parent, W.cnt, W.mintri, W.usedv, nv, (unsigned long long *)W.misc,
                       W.misc + 2);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_union, dim3((unsigned)ivx::cdiv(nt, 256)), dim3(256), 0, st, faces, nt, W.parent);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_flatten, dim3(gv), dim3(256), 0, st, W.parent, W.root, nv);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}
// ... and on to the numbered regions: W.rank[first triangle of a region] = its number, W.misc[3] = how many there are
static int regions_stage(const int32_t *faces, int64_t nv, int64_t nt, const PartsWs &W, hipStream_t st) {
    int rc;
    if ((rc = roots_stage(faces, nv, nt, W, st))) return rc;
    hipLaunchKernelGGL(k_mesh_tricount, dim3((unsigned)ivx::cdiv(nt, 256 * TPL)), dim3(256), 0, st, faces, nt, W.root, W.cnt, W.mintri);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_parts_flag, dim3((unsigned)ivx::cdiv(nt + 1, 256)), dim3(256), 0, st, faces, nt, W.root, W.mintri, W.rank);
    IVX_LAUNCH_CHECK();
    return scan_u32_exclusive(W.rank, nt + 1, W.bsum, W.misc + 3, st);
}
static int read_words(const uint32_t *dsrc, int n, uint32_t *got, hipStream_t st) {
    uint32_t seq;
    int rc;
    if ((rc = ivx::mailbox_publish(dsrc, n, st, &seq))) return rc;
    return ivx::mailbox_wait(seq, st, got, n);
}

} // namespace

extern "C" int ivx_dev_mesh_region_labels(int64_t nverts, const int32_t *faces, int64_t ntris, int32_t *tri_labels,
                                          int32_t *vert_labels, int64_t *nregions, int64_t *nused_verts, void *stream) {
    int rc;
    if ((rc = check_sizes(nverts, ntris))) return rc;
    if (nregions) *nregions = 0;
    if (nused_verts) *nused_verts = 0;
    hipStream_t st = ivx::S(stream);
    if (ntris == 0) {
        if (vert_labels && nverts) IVX_HIP(hipMemsetAsync(vert_labels, 0xff, (size_t)nverts * 4, st));
        return IVX_OK;
    }
    PartsWs W;
    if ((rc = parts_ws(nverts, ntris, false, st, &W))) return rc;
    if ((rc = regions_stage(faces, nverts, ntris, W, st))) return rc;
    if (tri_labels) {
        hipLaunchKernelGGL(k_parts_tlabel, dim3((unsigned)ivx::cdiv(ntris, 256)), dim3(256), 0, st, faces, ntris, W.root, W.mintri, W.rank,
                           (uint32_t *)tri_labels);
        IVX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_parts_vlabel, dim3((unsigned)ivx::cdiv(std::max<int64_t>(nverts, 1), 256)), dim3(256), 0, st, nverts, W.root, W.cnt,
                       W.mintri, W.rank, W.misc + 3, vert_labels, (uint32_t *)nullptr, W.misc + 4);
    IVX_LAUNCH_CHECK();
    uint32_t got[2];
    if ((rc = read_words(W.misc + 3, 2, got, st))) return rc;
    if (nregions) *nregions = got[0];
    if (nused_verts) *nused_verts = got[1];
    return IVX_OK;
}

extern "C" int ivx_dev_partition_u32(const uint32_t *keys, int64_t n, uint32_t nkeys, uint32_t *order, uint32_t *offsets, void *stream) {
    IVX_REQUIRE(n >= 0 && n < 0x7fffffffll && nkeys >= 1, IVX_EINVAL, "partition: bad sizes");
    hipStream_t st = ivx::S(stream);
    if (n == 0) {
        IVX_HIP(hipMemsetAsync(offsets, 0, ((size_t)nkeys + 1) * 4, st));
        return IVX_OK;
    }
    PartsWs W;
    int rc;
    if ((rc = parts_ws(n, n, true, st, &W))) return rc;
    IVX_HIP(hipMemcpyAsync(W.key[0], keys, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    const uint32_t *ord, *sorted;
    if ((rc = partition_u32(W.key, W.val, n, nkeys, W.hist, offsets, &ord, &sorted, st))) return rc;
    IVX_HIP(hipMemcpyAsync(order, ord, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return IVX_OK;
}

extern "C" int ivx_dev_mesh_split(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, float *out_verts,
                                  int64_t max_verts, int32_t *out_faces, int64_t max_tris, int64_t *table, int64_t max_parts,
                                  int64_t *out_nverts, int64_t *nparts, void *stream) {
    int rc;
    if ((rc = check_sizes(nverts, ntris))) return rc;
    *out_nverts = 0;
    *nparts = 0;
    if (ntris == 0) return IVX_OK;
    hipStream_t st = ivx::S(stream);
    const bool fill = out_verts && out_faces && table;
    PartsWs W;
    if ((rc = parts_ws(nverts, ntris, fill, st, &W))) return rc;
    if ((rc = regions_stage(faces, nverts, ntris, W, st))) return rc;
    const unsigned gv = (unsigned)ivx::cdiv(std::max<int64_t>(nverts, 1), 256), gt = (unsigned)ivx::cdiv(ntris, 256);
    hipLaunchKernelGGL(k_parts_vlabel, dim3(gv), dim3(256), 0, st, nverts, W.root, W.cnt, W.mintri, W.rank, W.misc + 3,
                       (int32_t *)nullptr, fill ? W.key[0] : (uint32_t *)nullptr, W.misc + 4);
    IVX_LAUNCH_CHECK();
    uint32_t got[2];
    if ((rc = read_words(W.misc + 3, 2, got, st))) return rc;
    const int64_t R = got[0], nused = got[1];
    *nparts = R;
    *out_nverts = nused;
    if (!fill) return IVX_OK;
    IVX_REQUIRE(max_tris >= ntris && max_verts >= nused && max_parts >= R, IVX_ERANGE,
                "mesh split: output buffers too small (%lld verts, %lld triangles, %lld parts needed)", (long long)nused,
                (long long)ntris, (long long)R);
    const uint32_t *ord, *sorted;
    // points: unused ones carry the key R and end up behind every part
    if ((rc = partition_u32(W.key, W.val, nverts, (uint32_t)R + 1, W.hist, W.offs_v, &ord, &sorted, st))) return rc;
    hipLaunchKernelGGL(k_parts_place_verts, dim3(gv), dim3(256), 0, st, ord, sorted, nverts, (const uint32_t *)W.offs_v, (uint32_t)R, verts,
                       W.usedv, out_verts, max_verts);
    IVX_LAUNCH_CHECK();
    // triangles
    hipLaunchKernelGGL(k_parts_tlabel, dim3(gt), dim3(256), 0, st, faces, ntris, W.root, W.mintri, W.rank, W.key[0]);
    IVX_LAUNCH_CHECK();
    if ((rc = partition_u32(W.key, W.val, ntris, (uint32_t)R, W.hist, W.offs_t, &ord, &sorted, st))) return rc;
    hipLaunchKernelGGL(k_parts_place_faces, dim3(gt), dim3(256), 0, st, ord, ntris, faces, (const uint32_t *)W.usedv, out_faces, max_tris);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_parts_table, dim3((unsigned)ivx::cdiv(R, 256)), dim3(256), 0, st, (const uint32_t *)W.offs_t,
                       (const uint32_t *)W.offs_v, R, table);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_mesh_parts_mass(const float *verts, const int32_t *faces, const int64_t *table, int64_t nparts,
                                       int64_t ntris, int64_t small_max, double *out, void *stream) {
    int rc;
    if ((rc = check_sizes(0, ntris))) return rc;
    IVX_REQUIRE(nparts >= 0 && nparts <= ntris, IVX_EINVAL, "mesh parts: %lld parts of %lld triangles", (long long)nparts, (long long)ntris);
    if (nparts == 0) return IVX_OK;
    if (small_max <= 0) small_max = PARTS_SMALL_MAX;
    hipStream_t st = ivx::S(stream);
    hipLaunchKernelGGL(k_parts_mass_small, dim3((unsigned)ivx::cdiv(nparts, 4)), dim3(256), 0, st, verts, faces, table, nparts, small_max, out);
    IVX_LAUNCH_CHECK();
    // workgroups of the large parts: at most one per 1024 triangles plus one per large part
    const int64_t nlarge_max = std::min(nparts, ntris / (small_max + 1));
    if (nlarge_max == 0) return IVX_OK;
    const int64_t gmax = ntris / PARTS_MASS_BLOCK + nlarge_max;
    const size_t off_bsum = al256(((size_t)nparts + 1) * 4);
    const size_t off_part = off_bsum + al256(((size_t)scan_u32_blocks(nparts + 1) + 16) * 4);
    void *ws;
    if ((rc = ivx::ws_get_s(ivx::WS_MESH2, st, off_part + (size_t)gmax * NP * 8, &ws))) return rc;
    uint32_t *boff = (uint32_t *)ws, *bsum = (uint32_t *)((char *)ws + off_bsum);
    double *partial = (double *)((char *)ws + off_part);
    hipLaunchKernelGGL(k_parts_mass_nblocks, dim3((unsigned)ivx::cdiv(nparts + 1, 256)), dim3(256), 0, st, table, nparts, small_max, boff);
    IVX_LAUNCH_CHECK();
    if ((rc = scan_u32_exclusive(boff, nparts + 1, bsum, bsum + scan_u32_blocks(nparts + 1) + 8, st))) return rc;
    hipLaunchKernelGGL(k_parts_mass_large, dim3((unsigned)gmax), dim3(256), 0, st, verts, faces, table, nparts, (const uint32_t *)boff, partial);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_parts_mass_final, dim3((unsigned)nparts), dim3(256), 0, st, (const double *)partial, table, (const uint32_t *)boff, out);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_mesh_select_seeded(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, const int32_t *seeds,
                                          int64_t nseeds, float *out_verts, int64_t max_verts, int32_t *out_faces, int64_t max_tris,
                                          int64_t *out_nverts, int64_t *out_ntris, void *stream) {
    int rc;
    if ((rc = check_sizes(nverts, ntris))) return rc;
    IVX_REQUIRE(nseeds >= 0 && nseeds < 0x7fffffffll, IVX_EINVAL, "mesh seeds: bad count");
    *out_nverts = 0;
    *out_ntris = 0;
    if (ntris == 0 || nseeds == 0) return IVX_OK;
    hipStream_t st = ivx::S(stream);
    PartsWs W;
    if ((rc = parts_ws(nverts, ntris, false, st, &W))) return rc;
    if ((rc = roots_stage(faces, nverts, ntris, W, st))) return rc;
    uint32_t *mark = W.cnt, *keep = W.rank; // (k_mesh_init left cnt and usedv zero)
    hipLaunchKernelGGL(k_parts_seed_mark, dim3((unsigned)ivx::cdiv(nseeds, 256)), dim3(256), 0, st, seeds, nseeds, nverts, W.root, mark);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_parts_seed_keep, dim3((unsigned)ivx::cdiv(ntris + 1, 256)), dim3(256), 0, st, faces, ntris, W.root, mark, keep, W.usedv);
    IVX_LAUNCH_CHECK();
    if ((rc = scan_u32_exclusive(keep, ntris + 1, W.bsum, W.misc + 5, st))) return rc;
    if ((rc = scan_u32_exclusive(W.usedv, nverts + 1, W.bsum, W.misc + 6, st))) return rc;
    uint32_t got[2];
    if ((rc = read_words(W.misc + 5, 2, got, st))) return rc;
    *out_ntris = got[0];
    *out_nverts = got[1];
    if (!out_verts || !out_faces || got[0] == 0) return IVX_OK;
    IVX_REQUIRE(max_tris >= (int64_t)got[0] && max_verts >= (int64_t)got[1], IVX_ERANGE,
                "mesh: output buffers too small (%u verts, %u triangles needed)", got[1], got[0]);
    hipLaunchKernelGGL(k_mesh_compact_faces, dim3((unsigned)ivx::cdiv(ntris, 256)), dim3(256), 0, st, faces, ntris, keep, W.usedv, out_faces,
                       max_tris);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_compact_verts, dim3((unsigned)ivx::cdiv(nverts, 256)), dim3(256), 0, st, verts, nverts, W.usedv, out_verts,
                       max_verts);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_mesh_nearest_point(const float *verts, int64_t nverts, const double *xyz, int32_t *out_id, void *stream) {
    int rc;
    if ((rc = check_sizes(nverts, 0))) return rc;
    IVX_REQUIRE(xyz && out_id, IVX_EINVAL, "mesh nearest point: null argument");
    hipStream_t st = ivx::S(stream);
    if (nverts == 0) {
        IVX_HIP(hipMemsetAsync(out_id, 0xff, 4, st));
        return IVX_OK;
    }
    const int nb = (int)std::min<int64_t>(ivx::cdiv(nverts, 256), NEAR_BLOCKS);
    void *ws;
    if ((rc = ivx::ws_get_s(ivx::WS_MESH2, st, (size_t)NEAR_BLOCKS * 12, &ws))) return rc;
    double *pd = (double *)ws;
    uint32_t *pid = (uint32_t *)(pd + NEAR_BLOCKS);
    hipLaunchKernelGGL(k_parts_nearest, dim3((unsigned)nb), dim3(256), 0, st, verts, nverts, xyz[0], xyz[1], xyz[2], pd, pid);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_parts_nearest_final, dim3(1), dim3(256), 0, st, (const double *)pd, (const uint32_t *)pid, nb, out_id);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

// ---- host forms -----------------------------------------------------------------------------------------------------
namespace {
// the mesh into WS_IN (points, may be absent) / WS_AUX0 (triangles)
int upload_mesh(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, void **d_v, void **d_f) {
    using namespace ivx;
    int rc;
    if ((rc = check_sizes(nverts, ntris)) || (rc = check_faces(faces, ntris, nverts))) return rc;
    if (verts) {
        if ((rc = ws_get(WS_IN, (size_t)nverts * 12 + 16, d_v))) return rc;
        if (nverts) IVX_HIP(hipMemcpy(*d_v, verts, (size_t)nverts * 12, hipMemcpyHostToDevice));
    }
    if ((rc = ws_get(WS_AUX0, (size_t)ntris * 12 + 16, d_f))) return rc;
    if (ntris) IVX_HIP(hipMemcpy(*d_f, faces, (size_t)ntris * 12, hipMemcpyHostToDevice));
    return IVX_OK;
}
} // namespace

extern "C" int ivx_mesh_region_labels(int64_t nverts, const int32_t *faces, int64_t ntris, int32_t *tri_labels, int32_t *vert_labels,
                                      int64_t *nregions) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    int rc;
    IVX_REQUIRE(nregions, IVX_EINVAL, "mesh region labels: null argument");
    *nregions = 0;
    void *d_v = nullptr, *d_f, *d_tl, *d_vl;
    if ((rc = upload_mesh(nullptr, nverts, faces, ntris, &d_v, &d_f))) return rc;
    if ((rc = ws_get(WS_OUT, (size_t)ntris * 4 + 16, &d_tl))) return rc;
    if ((rc = ws_get(WS_AUX1, (size_t)nverts * 4 + 16, &d_vl))) return rc;
    if ((rc = ivx_dev_mesh_region_labels(nverts, (const int32_t *)d_f, ntris, (int32_t *)d_tl, vert_labels ? (int32_t *)d_vl : nullptr,
                                         nregions, nullptr, nullptr)))
        return rc;
    IVX_HIP(hipDeviceSynchronize());
    if (tri_labels && ntris) IVX_HIP(hipMemcpy(tri_labels, d_tl, (size_t)ntris * 4, hipMemcpyDeviceToHost));
    if (vert_labels && nverts) IVX_HIP(hipMemcpy(vert_labels, d_vl, (size_t)nverts * 4, hipMemcpyDeviceToHost));
    return IVX_OK;
}

extern "C" int ivx_mesh_split(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, float *out_verts,
                              int32_t *out_faces, int64_t *table, int64_t *out_nverts, int64_t *nparts) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    int rc;
    IVX_REQUIRE(out_nverts && nparts, IVX_EINVAL, "mesh split: null argument");
    const bool fill = out_verts && out_faces && table;
    const int64_t cap_v = *out_nverts, cap_p = *nparts; // (second call: the capacities come in here)
    *out_nverts = *nparts = 0;
    void *d_v, *d_f, *d_ov = nullptr, *d_of = nullptr, *d_tb = nullptr;
    if ((rc = upload_mesh(verts, nverts, faces, ntris, &d_v, &d_f))) return rc;
    if (ntris == 0) return IVX_OK;
    if (fill) {
        IVX_REQUIRE(cap_v >= 0 && cap_p >= 0, IVX_EINVAL, "mesh split: negative capacity");
        if ((rc = ws_get(WS_OUT, (size_t)std::min(cap_v, nverts) * 12 + 16, &d_ov))) return rc;
        if ((rc = ws_get(WS_AUX1, (size_t)ntris * 12 + 16, &d_of))) return rc;
        if ((rc = ws_get(WS_AUX2, (size_t)std::min(cap_p, ntris) * 32 + 16, &d_tb))) return rc;
    }
    if ((rc = ivx_dev_mesh_split((const float *)d_v, nverts, (const int32_t *)d_f, ntris, (float *)d_ov, std::min(cap_v, nverts),
                                 (int32_t *)d_of, ntris, (int64_t *)d_tb, std::min(cap_p, ntris), out_nverts, nparts, nullptr)))
        return rc;
    if (!fill) return IVX_OK;
    IVX_HIP(hipDeviceSynchronize());
    if (*out_nverts) IVX_HIP(hipMemcpy(out_verts, d_ov, (size_t)*out_nverts * 12, hipMemcpyDeviceToHost));
    IVX_HIP(hipMemcpy(out_faces, d_of, (size_t)ntris * 12, hipMemcpyDeviceToHost));
    if (*nparts) IVX_HIP(hipMemcpy(table, d_tb, (size_t)*nparts * 32, hipMemcpyDeviceToHost));
    return IVX_OK;
}

extern "C" int ivx_mesh_parts_mass(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, const int64_t *table,
                                   int64_t nparts, double *out) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    int rc;
    if ((rc = check_sizes(nverts, ntris))) return rc;
    IVX_REQUIRE(nparts >= 0 && nparts <= ntris, IVX_EINVAL, "mesh parts: %lld parts of %lld triangles", (long long)nparts, (long long)ntris);
    if (nparts == 0) return IVX_OK;
    // a part's rows lie inside the arrays and its triangles index its own points
    for (int64_t r = 0; r < nparts; r++) {
        const int64_t to = table[4 * r], tn = table[4 * r + 1], vo = table[4 * r + 2], vn = table[4 * r + 3];
        IVX_REQUIRE(to >= 0 && tn >= 0 && vo >= 0 && vn >= 0 && to <= ntris - tn && vo <= nverts - vn, IVX_EDOM,
                    "mesh parts: part %lld lies outside the arrays", (long long)r);
        for (int64_t q = 3 * to; q < 3 * (to + tn); q++)
            IVX_REQUIRE(faces[q] >= 0 && faces[q] < vn, IVX_EDOM, "mesh parts: face index %d outside part %lld's [0, %lld)", faces[q],
                        (long long)r, (long long)vn);
    }
    void *d_v, *d_f, *d_tb, *d_o;
    if ((rc = ws_get(WS_IN, (size_t)nverts * 12 + 16, &d_v))) return rc;
    if ((rc = ws_get(WS_AUX0, (size_t)ntris * 12 + 16, &d_f))) return rc;
    if ((rc = ws_get(WS_AUX2, (size_t)nparts * 32 + 16, &d_tb))) return rc;
    if ((rc = ws_get(WS_AUX3, (size_t)nparts * 64 + 16, &d_o))) return rc;
    if (nverts) IVX_HIP(hipMemcpy(d_v, verts, (size_t)nverts * 12, hipMemcpyHostToDevice));
    IVX_HIP(hipMemcpy(d_f, faces, (size_t)ntris * 12, hipMemcpyHostToDevice));
    IVX_HIP(hipMemcpy(d_tb, table, (size_t)nparts * 32, hipMemcpyHostToDevice));
    if ((rc = ivx_dev_mesh_parts_mass((const float *)d_v, (const int32_t *)d_f, (const int64_t *)d_tb, nparts, ntris, 0, (double *)d_o, nullptr)))
        return rc;
    IVX_HIP(hipMemcpy(out, d_o, (size_t)nparts * 64, hipMemcpyDeviceToHost));
    return IVX_OK;
}

extern "C" int ivx_mesh_select_seeded(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, const int64_t *seeds,
                                      int64_t nseeds, float *out_verts, int32_t *out_faces, int64_t *out_nverts, int64_t *out_ntris) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    int rc;
    IVX_REQUIRE(out_nverts && out_ntris && nseeds >= 0 && nseeds < 0x7fffffffll, IVX_EINVAL, "mesh seeds: bad arguments");
    *out_nverts = *out_ntris = 0;
    if ((rc = check_sizes(nverts, ntris))) return rc;
    for (int64_t q = 0; q < nseeds; q++)
        IVX_REQUIRE(seeds[q] >= 0 && seeds[q] < nverts, IVX_EDOM, "mesh seeds: point id %lld outside [0, %lld)", (long long)seeds[q],
                    (long long)nverts);
    void *d_v, *d_f, *d_s, *d_ov = nullptr, *d_of = nullptr;
    if ((rc = upload_mesh(verts, nverts, faces, ntris, &d_v, &d_f))) return rc;
    if (ntris == 0 || nseeds == 0) return IVX_OK;
    std::vector<int32_t> s32((size_t)nseeds);
    for (int64_t q = 0; q < nseeds; q++) s32[(size_t)q] = (int32_t)seeds[q];
    if ((rc = ws_get(WS_AUX2, (size_t)nseeds * 4 + 16, &d_s))) return rc;
    IVX_HIP(hipMemcpy(d_s, s32.data(), (size_t)nseeds * 4, hipMemcpyHostToDevice));
    const bool fill = out_verts && out_faces;
    if (fill) {
        if ((rc = ws_get(WS_OUT, (size_t)nverts * 12 + 16, &d_ov))) return rc;
        if ((rc = ws_get(WS_AUX1, (size_t)ntris * 12 + 16, &d_of))) return rc;
    }
    if ((rc = ivx_dev_mesh_select_seeded((const float *)d_v, nverts, (const int32_t *)d_f, ntris, (const int32_t *)d_s, nseeds, (float *)d_ov,
                                         nverts, (int32_t *)d_of, ntris, out_nverts, out_ntris, nullptr)))
        return rc;
    IVX_HIP(hipDeviceSynchronize());
    if (fill && *out_nverts) IVX_HIP(hipMemcpy(out_verts, d_ov, (size_t)*out_nverts * 12, hipMemcpyDeviceToHost));
    if (fill && *out_ntris) IVX_HIP(hipMemcpy(out_faces, d_of, (size_t)*out_ntris * 12, hipMemcpyDeviceToHost));
    return IVX_OK;
}

extern "C" int ivx_mesh_nearest_point(const float *verts, int64_t nverts, const double *xyz, int64_t *id) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    int rc;
    IVX_REQUIRE(xyz && id, IVX_EINVAL, "mesh nearest point: null argument");
    *id = -1;
    if ((rc = check_sizes(nverts, 0))) return rc;
    if (nverts == 0) return IVX_OK;
    void *d_v, *d_o;
    if ((rc = ws_get(WS_IN, (size_t)nverts * 12 + 16, &d_v))) return rc;
    if ((rc = ws_get(WS_SMALL, 64, &d_o))) return rc;
    IVX_HIP(hipMemcpy(d_v, verts, (size_t)nverts * 12, hipMemcpyHostToDevice));
    if ((rc = ivx_dev_mesh_nearest_point((const float *)d_v, nverts, xyz, (int32_t *)d_o, nullptr))) return rc;
    int32_t got = -1;
    IVX_HIP(hipMemcpy(&got, d_o, 4, hipMemcpyDeviceToHost));
    *id = got;
    return IVX_OK;
}
