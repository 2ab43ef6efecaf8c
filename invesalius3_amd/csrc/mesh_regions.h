// mesh_regions.h -- what k_mesh.hip (keep largest, mass properties) and k_meshparts.hip (region labels, split, seeded parts,
// per-part mass) share: the lock-free union-find over vertex ids with its init / union / flatten / triangle-count kernels, and
// the per-triangle terms and fixed-shape workgroup reduction of the mass properties.  Moved here unchanged from k_mesh.hip.
// Included by the translation units that need it (kernels live in each unit's anonymous namespace).
#pragma once
#include "ivx_internal.h"

namespace {

__device__ __forceinline__ uint32_t uf_find(const uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = parent[x];
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void uf_union(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; } // the larger root goes under the smaller
        const uint32_t old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(256) void k_mesh_init(uint32_t *__restrict__ parent, uint32_t *__restrict__ cnt,
                                                   uint32_t *__restrict__ mintri, uint32_t *__restrict__ usedv, int64_t nv,
                                                   unsigned long long *__restrict__ best, uint32_t *__restrict__ nreg) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v <= nv; v += stride) {
        if (v < nv) {
            parent[v] = (uint32_t)v;
            cnt[v] = 0u;
            mintri[v] = 0xffffffffu;
        }
        usedv[v] = 0u; // nv + 1 entries: the scan leaves the total in the last one
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *best = 0ull;
        *nreg = 0u;
    }
}

__global__ __launch_bounds__(256) void k_mesh_union(const int32_t *__restrict__ faces, int64_t nt,
                                                    uint32_t *__restrict__ parent) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const uint32_t a = (uint32_t)faces[3 * t], b = (uint32_t)faces[3 * t + 1], c = (uint32_t)faces[3 * t + 2];
    uf_union(parent, a, b);
    uf_union(parent, a, c);
}

__global__ __launch_bounds__(256) void k_mesh_flatten(const uint32_t *__restrict__ parent, uint32_t *__restrict__ root,
                                                      int64_t nv) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride)
        root[v] = uf_find(parent, (uint32_t)v);
}

// triangles per region + the smallest triangle id of each region (the tie-break: VTK numbers regions by their first
// cell and keeps the FIRST region among equally large ones)
constexpr int TPL = 8; // triangles per lane
__global__ __launch_bounds__(256) void k_mesh_tricount(const int32_t *__restrict__ faces, int64_t nt,
                                                       const uint32_t *__restrict__ root, uint32_t *__restrict__ cnt,
                                                       uint32_t *__restrict__ mintri) {
    __shared__ uint32_t s_hot, s_hot_cnt, s_hot_min;
    const int64_t base = (int64_t)blockIdx.x * 256 * TPL;
    if (threadIdx.x == 0) {
        s_hot = base < nt ? root[(uint32_t)faces[3 * base]] : 0xffffffffu;
        s_hot_cnt = 0u;
        s_hot_min = 0xffffffffu;
    }
    __syncthreads();
    const uint32_t hot = s_hot;
    uint32_t my_hot = 0, my_min = 0xffffffffu;
#pragma unroll
    for (int q = 0; q < TPL; q++) {
        const int64_t t = base + (int64_t)q * 256 + threadIdx.x;
        const bool ok = t < nt;
        const uint32_t r = ok ? root[(uint32_t)faces[3 * t]] : 0xffffffffu;
        if (ok && r == hot) {
            my_hot++;
            my_min = my_min < (uint32_t)t ? my_min : (uint32_t)t;
        }
        // everything else: one atomic per distinct root per wave
        bool todo = ok && r != hot;
        while (__ballot(todo)) {
            const unsigned long long pending = __ballot(todo);
            const int leader = __builtin_ctzll(pending);
            const uint32_t lr = __shfl(r, leader, 64);
            const bool mine = todo && r == lr;
            const unsigned long long grp = __ballot(mine);
            if ((int)(threadIdx.x & 63) == leader) {
                atomicAdd(&cnt[lr], (uint32_t)__popcll(grp));
                atomicMin(&mintri[lr], (uint32_t)(base + (int64_t)q * 256 + (threadIdx.x & ~63) + __builtin_ctzll(grp)));
            }
            todo = todo && !mine;
        }
    }
    // workgroup total for the hot root
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        my_hot += __shfl_xor(my_hot, o, 64);
        const uint32_t m = __shfl_xor(my_min, o, 64);
        my_min = my_min < m ? my_min : m;
    }
    if ((threadIdx.x & 63) == 0 && my_hot) {
        atomicAdd(&s_hot_cnt, my_hot);
        atomicMin(&s_hot_min, my_min);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_hot_cnt) {
        atomicAdd(&cnt[hot], s_hot_cnt);
        atomicMin(&mintri[hot], s_hot_min);
    }
}

// ---- mass properties ------------------------------------------------------------------------------------------------
// partial record: area, vol x/y/z, then the seven counters munc x/y/z, wxyz, wxy, wxz, wyz (as doubles: exact < 2^53)
constexpr int NP = 11;
__device__ __forceinline__ void tri_mass(const float *__restrict__ verts, const int32_t *__restrict__ faces, int64_t t,
                                         double acc[NP]) {
    double x[3], y[3], z[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int64_t v = faces ? (int64_t)faces[3 * t + q] : 3 * t + q;
        x[q] = (double)verts[3 * v];
        y[q] = (double)verts[3 * v + 1];
        z[q] = (double)verts[3 * v + 2];
    }
    const double i0 = x[1] - x[0], j0 = y[1] - y[0], k0 = z[1] - z[0];
    const double i1 = x[2] - x[0], j1 = y[2] - y[0], k1 = z[2] - z[0];
    const double i2 = x[2] - x[1], j2 = y[2] - y[1], k2 = z[2] - z[1];
    double u0 = j0 * k1 - k0 * j1, u1 = k0 * i1 - i0 * k1, u2 = i0 * j1 - j0 * i1;
    const double len = sqrt(u0 * u0 + u1 * u1 + u2 * u2);
    if (len != 0.0) {
        u0 /= len;
        u1 /= len;
        u2 /= len;
    } else {
        u0 = u1 = u2 = 0.0;
    }
    const double a0 = fabs(u0), a1 = fabs(u1), a2 = fabs(u2);
    int slot = -1;
    if (a0 > a1 && a0 > a2) slot = 4;
    else if (a1 > a0 && a1 > a2) slot = 5;
    else if (a2 > a0 && a2 > a1) slot = 6;
    else if (a0 == a1 && a0 == a2) slot = 7;
    else if (a0 == a1 && a0 > a2) slot = 8;
    else if (a0 == a2 && a0 > a1) slot = 9;
    else if (a1 == a2 && a0 < a2) slot = 10;
    const double a = sqrt(i1 * i1 + j1 * j1 + k1 * k1);
    const double b = sqrt(i0 * i0 + j0 * j0 + k0 * k0);
    const double c = sqrt(i2 * i2 + j2 * j2 + k2 * k2);
    const double s = 0.5 * (a + b + c);
    const double area = sqrt(fabs(s * (s - a) * (s - b) * (s - c)));
    acc[0] += area;
    acc[1] += area * u0 * ((x[0] + x[1] + x[2]) / 3.0);
    acc[2] += area * u1 * ((y[0] + y[1] + y[2]) / 3.0);
    acc[3] += area * u2 * ((z[0] + z[1] + z[2]) / 3.0);
#pragma unroll
    for (int q = 4; q < NP; q++) acc[q] += (slot == q) ? 1.0 : 0.0;
}

__device__ __forceinline__ void block_reduce_np(double acc[NP], double *__restrict__ out) {
    __shared__ double s_part[4][NP];
#pragma unroll
    for (int q = 0; q < NP; q++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_xor(acc[q], o, 64);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int q = 0; q < NP; q++) s_part[wv][q] = acc[q];
    __syncthreads();
    if (threadIdx.x < NP) out[threadIdx.x] = (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
}

// the eight numbers of out8 from a reduced record m[NP] and the cell count the weights are taken over
__device__ __forceinline__ void mass_finish(const double *m, double ncells, double *__restrict__ out) {
    const double kx = (m[4] + m[7] / 3.0 + (m[8] + m[9]) / 2.0) / ncells;
    const double ky = (m[5] + m[7] / 3.0 + (m[8] + m[10]) / 2.0) / ncells;
    const double kz = (m[6] + m[7] / 3.0 + (m[9] + m[10]) / 2.0) / ncells;
    out[0] = fabs(kx * m[1] + ky * m[2] + kz * m[3]);
    out[1] = m[0];
    out[2] = m[1];
    out[3] = m[2];
    out[4] = m[3];
    out[5] = kx;
    out[6] = ky;
    out[7] = kz;
}

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

} // namespace
