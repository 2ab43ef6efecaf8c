// k_mci.hip -- the indexed mesh of a marching-cubes piece (coincident points merged) and the stitch of such meshes across
// Z-slabs.  Both follow a count of k_mc.hip on the same parameters, scratch and stream: they read its inside planes, per-word
// counts and triangle list (mc_common.h: the shared geometry, scratch layout and launchers; mc_piece.h: what the host remembers
// about the piece counted into a scratch).
#include <cmath>

#include "mc_common.h"
#include "scan_u32.h"

#define MC_TABLE_QUAL static __device__ __attribute__((aligned(16))) const
#include "../../include/ivx_mc_tables.h"

using namespace ivx;

namespace {

// ---- padded + flipped view of the source bit planes -----------------------------------------------------
// Words w and w+1 of padded point row (k, jf): padded x = 64w .. 64w+127.  Pad rows / pad columns carry pbits.
// Written without branches around the loads: the three source words are always fetched (clamped, always-valid
// addresses) and masked afterwards, so the 12 loads of a cell word are all in flight together.
__device__ __forceinline__ void padded_pair(const uint64_t *__restrict__ S, const Geom &g, int64_t k, int64_t jf,
                                            int64_t w, uint64_t pbits, uint64_t &lo, uint64_t &hi) {
    const int64_t ja = (g.NY - 1 - jf) - g.pxy, ka = k - g.pb;
    const bool row_in = ja >= 0 && ja < g.ny && ka >= 0 && ka < g.nz;
    // clamp into [0, n-1], and to 0 when the piece is EMPTY along that axis (n == 0: every row is padding, the loads
    // then hit word 0 of the scratch block, which always exists, and are masked away)
    const auto clampi = [](int64_t v, int64_t n) { return v >= n ? (n > 0 ? n - 1 : 0) : (v < 0 ? 0 : v); };
    const int64_t rj = clampi(ja, g.ny), rk = clampi(ka, g.nz);
    const uint64_t *row = S + (rk * g.ny + rj) * g.ws;
    // source words w-1, w, w+1 (clamped index, masked when outside [0, ws) or when the row is padding)
    const int64_t wm = clampi(w - 1, g.ws), wc = clampi(w, g.ws), wp = clampi(w + 1, g.ws);
    uint64_t sm = row[wm], sc = row[wc], sp = row[wp];
    sm = (row_in && w - 1 >= 0 && w - 1 < g.ws) ? sm : 0ull;
    sc = (row_in && w < g.ws) ? sc : 0ull;
    sp = (row_in && w + 1 < g.ws) ? sp : 0ull;
    // bits of source x in [64w - pxy, 64w + 64 - pxy) and the following 64
    uint64_t v0 = g.pxy ? ((sc << 1) | (sm >> 63)) : sc;
    uint64_t v1 = g.pxy ? ((sp << 1) | (sc >> 63)) : sp;
    // positions of each word that exist in the padded row, and those backed by source voxels
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int64_t ww = w + q;
        const int64_t rem = g.NX - ww * 64; // padded points in this word
        const uint64_t exist = rem >= 64 ? ~0ull : (rem <= 0 ? 0ull : ((1ull << rem) - 1ull));
        uint64_t src = row_in ? exist : 0ull;
        if (g.pxy && ww == 0) src &= ~1ull;
        const int64_t top = g.pxy + g.nx - ww * 64; // first padded-x (relative) beyond the source
        src &= top >= 64 ? ~0ull : (top <= 0 ? 0ull : ((1ull << top) - 1ull));
        uint64_t &v = q == 0 ? v0 : v1;
        v = (v & src) | (pbits & exist & ~src);
    }
    lo = v0;
    hi = v1;
}

// =====================================================================================================================
// Indexed mesh ("point merge" of join_process_surface, invesalius/data/surface_process.py:229-268: the reference appends
// the pieces and runs vtkCleanPolyData to merge coincident points).  Here the merge needs no hashing or sorting: a
// vertex IS a grid edge whose end points differ in the inside-bit plane, so
//   crossing planes   cx = P ^ (P >> 1 | carry), cy = P(j) ^ P(j+1), cz = P(k) ^ P(k+1)   (P = padded point words)
//   vertex id         = (scan of popcounts over point words in raster order) + rank of the edge inside its word
//                       (x edges first, then y, then z)
//   k_mci_vertices    one interpolation per UNIQUE vertex (3.2 M instead of 19 M for the bench surface)
//   k_mci_faces       one lane per triangle of the flat list: three edge -> id look-ups (bit planes + popcounts)
// verts[faces] reproduces the soup of ivx_dev_mc_emit bit for bit.
// =====================================================================================================================
struct Cross {
    uint64_t cx, cy, cz; // regular crossings: bit b = the edge leaving point (64w+b, jf, k) in +x / +y / +z
    uint64_t cp;         // point vertices (only with POINTS): the point's value IS the iso-value and a neighbour is outside
    uint64_t e0, ex, ey, ez; // "value == iso" at the point itself and at its +x / +y / +z neighbour
};
// S = inside plane (value >= iso), Q = strictly-inside plane (value > iso); E = S & ~Q marks points sitting exactly
// on the iso-value.  A crossing edge with such an end point puts its vertex ON that grid point (t is exactly 0 or 1),
// and every such edge around the point yields the same position: those become ONE "point vertex", owned by the point.
template <bool POINTS>
__device__ __forceinline__ Cross crossings(const uint64_t *__restrict__ S, const uint64_t *__restrict__ Q, const Geom &g,
                                           int64_t k, int64_t jf, int64_t w, uint64_t pbits, uint64_t qbits) {
    uint64_t p0, p0n, py, pyn, pz, pzn, q0, q0n, qy, qyn, qz, qzn;
    padded_pair(S, g, k, jf, w, pbits, p0, p0n);
    padded_pair(S, g, k, jf + 1, w, pbits, py, pyn);
    padded_pair(S, g, k + 1, jf, w, pbits, pz, pzn);
    padded_pair(Q, g, k, jf, w, qbits, q0, q0n);
    padded_pair(Q, g, k, jf + 1, w, qbits, qy, qyn);
    padded_pair(Q, g, k + 1, jf, w, qbits, qz, qzn);
    const int64_t rem = g.NX - w * 64;                 // points of this word
    const uint64_t pts = rem >= 64 ? ~0ull : (rem <= 0 ? 0ull : ((1ull << rem) - 1ull));
    const int64_t remx = g.NX - 1 - w * 64;            // x edges of this word (last point has none)
    const uint64_t xed = remx >= 64 ? ~0ull : (remx <= 0 ? 0ull : ((1ull << remx) - 1ull));
    const bool hasy = jf + 1 < g.NY, hasz = k + 1 < g.NZ;
    Cross c;
    c.e0 = p0 & ~q0 & pts;
    c.ex = (((p0 & ~q0) >> 1) | ((p0n & ~q0n) << 63)) & xed;
    c.ey = hasy ? (py & ~qy & pts) : 0ull;
    c.ez = hasz ? (pz & ~qz & pts) : 0ull;
    const uint64_t rx = (p0 ^ ((p0 >> 1) | (p0n << 63))) & xed;
    const uint64_t ry = hasy ? ((p0 ^ py) & pts) : 0ull;
    const uint64_t rz = hasz ? ((p0 ^ pz) & pts) : 0ull;
    c.cx = rx & ~(c.e0 | c.ex);
    c.cy = ry & ~(c.e0 | c.ey);
    c.cz = rz & ~(c.e0 | c.ez);
    c.cp = 0ull;
    if (POINTS && c.e0) {
        uint64_t prev = 0ull, t0, t1, rxm, rym = 0ull, rzm = 0ull;
        if (w > 0) {
            padded_pair(S, g, k, jf, w - 1, pbits, t0, t1);
            prev = t0 >> 63;
        }
        rxm = (p0 ^ ((p0 << 1) | prev)) & (w > 0 ? ~0ull : ~1ull);
        if (jf > 0) {
            padded_pair(S, g, k, jf - 1, w, pbits, t0, t1);
            rym = p0 ^ t0;
        }
        if (k > 0) {
            padded_pair(S, g, k - 1, jf, w, pbits, t0, t1);
            rzm = p0 ^ t0;
        }
        c.cp = c.e0 & (rx | ry | rz | rxm | rym | rzm);
    }
    return c;
}

// The crossing words of every point word are derived ONCE (k_mci_count) and kept as 32-byte records: the vertex pass reads
// its word's record, and a face corner is two gathers (record + vertex base) instead of six padded row pairs of the two
// planes (a dozen loads and the masking around them) per corner -- three corners per triangle, 394 M triangles at 2048^3.
struct __attribute__((aligned(32))) CrossRec {
    uint64_t cx, cy, cz, cp;
};
__global__ __launch_bounds__(256) void k_mci_count(const uint64_t *__restrict__ bits, const uint64_t *__restrict__ qb,
                                                   Geom g, int64_t npw, uint64_t pbits, uint64_t qbits,
                                                   uint32_t *__restrict__ vcnt, CrossRec *__restrict__ rec) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npw; i += stride) {
        const int64_t w = i % g.WX, r = i / g.WX, jf = r % g.NY, k = r / g.NY;
        const Cross c = crossings<true>(bits, qb, g, k, jf, w, pbits, qbits);
        vcnt[i] = (uint32_t)(__popcll(c.cx) + __popcll(c.cy) + __popcll(c.cz) + __popcll(c.cp));
        rec[i] = CrossRec{c.cx, c.cy, c.cz, c.cp};
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_mci_vertices(const T *__restrict__ a, const CrossRec *__restrict__ rec, Geom g,
                                                      int64_t npw, double iso, const uint32_t *__restrict__ vbase,
                                                      uint32_t id0, float *__restrict__ verts, uint64_t max_verts) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t pw = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pw < npw; pw += stride) {
        const CrossRec c = rec[pw];
        if (!(c.cx | c.cy | c.cz | c.cp)) continue;
        const int64_t w = pw % g.WX, r = pw / g.WX, jf = r % g.NY, k = r / g.NY;
        uint64_t id = (uint64_t)id0 + vbase[pw];
#pragma unroll
        for (int ax = 0; ax < 4; ax++) {
            uint64_t m = ax == 0 ? c.cx : (ax == 1 ? c.cy : (ax == 2 ? c.cz : c.cp));
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                const int64_t i = w * 64 + b;
                double p0 = (double)(i - g.pxy), p1 = (double)(jf - g.yoff), p2 = (double)(k + g.zoff);
                if (ax < 3) {
                    const double s0 = mc_at(a, g, k, jf, i);
                    const double s1 = mc_at(a, g, k + (ax == 2), jf + (ax == 1), i + (ax == 0));
                    const double tt = (iso - s0) / (s1 - s0);
                    if (ax == 0) p0 += tt;
                    else if (ax == 1) p1 += tt;
                    else p2 += tt;
                }
                if (id < max_verts) {
                    float *o = verts + id * 3;
                    o[0] = (float)(g.sx * p0);
                    o[1] = (float)(g.sy * p1);
                    o[2] = (float)(g.sz * p2);
                }
                id++;
            }
        }
    }
}

// k_mci_vertices for a uint8 mask whose bytes are KNOWN (McLevels: v_out outside the inside plane -- the padding too --,
// v_sel where `sel` has a bit, v_in elsewhere inside): no voxel is read.  Which end of a crossing edge is inside is the
// point's bit of the padded inside row, the interpolation factor one of four constants, and no point sits on the iso-value
// (no point vertices: cp is empty).  Same vertices, same order, same bits as k_mci_vertices on that mask.
__global__ __launch_bounds__(256) void k_mci_vertices_levels(const uint64_t *__restrict__ bits, const CrossRec *__restrict__ rec,
                                                             Geom g, int64_t npw, uint64_t pbits, McLevels lv,
                                                             const uint32_t *__restrict__ vbase, uint32_t id0,
                                                             float *__restrict__ verts, uint64_t max_verts) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t pw = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pw < npw; pw += stride) {
        const CrossRec c = rec[pw];
        if (!(c.cx | c.cy | c.cz)) continue;
        const int64_t w = pw % g.WX, r = pw / g.WX, jf = r % g.NY, k = r / g.NY;
        uint64_t p0, p0n;
        padded_pair(bits, g, k, jf, w, pbits, p0, p0n);
        uint64_t id = (uint64_t)id0 + vbase[pw];
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            uint64_t m = ax == 0 ? c.cx : (ax == 1 ? c.cy : c.cz);
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                const int64_t i = w * 64 + b;
                const bool in0 = (p0 >> b) & 1ull;
                int sel = 0;
                if (lv.sel) { // the inside end is a source voxel: its bit of the selection plane
                    const int64_t ii = i + (!in0 && ax == 0), jj = jf + (!in0 && ax == 1), kk = k + (!in0 && ax == 2);
                    const int64_t sk = kk - g.pb, sj = (g.NY - 1 - jj) - g.pxy, si = ii - g.pxy;
                    sel = (int)((lv.sel[(sk * g.ny + sj) * g.ws + (si >> 6)] >> (si & 63)) & 1ull);
                }
                const double tt = lv.tt[(in0 ? 2 : 0) + sel];
                double q0 = (double)(i - g.pxy), q1 = (double)(jf - g.yoff), q2 = (double)(k + g.zoff);
                if (ax == 0) q0 += tt;
                else if (ax == 1) q1 += tt;
                else q2 += tt;
                if (id < max_verts) {
                    float *o = verts + id * 3;
                    o[0] = (float)(g.sx * q0);
                    o[1] = (float)(g.sy * q1);
                    o[2] = (float)(g.sz * q2);
                }
                id++;
            }
        }
    }
}

// id of the vertex on the edge leaving point (i, jf, k) along axis ax -- a crossing edge of a triangle, so exactly one of
// three holds: the edge's bit is set in its point word's c{x,y,z} (a regular crossing: rank among the word's crossings);
// or the point's bit is set in cp (the point's value IS the iso-value: the vertex is that point's, cp = e0 & "some crossing
// leaves or reaches the point", and this very edge is such a crossing); or the far end point is the one on the iso-value.
__device__ __forceinline__ uint32_t vertex_id(const CrossRec *__restrict__ rec, const Geom &g, const uint32_t *__restrict__ vbase,
                                              int64_t k, int64_t jf, int64_t i, int ax) {
    int64_t w = i >> 6;
    int b = (int)(i & 63);
    int64_t pw = (k * g.NY + jf) * g.WX + w;
    CrossRec c = rec[pw];
    const uint64_t below = (1ull << b) - 1ull;
    if (((ax == 0 ? c.cx : (ax == 1 ? c.cy : c.cz)) >> b) & 1ull) {
        uint32_t rank;
        if (ax == 0) rank = (uint32_t)__popcll(c.cx & below);
        else if (ax == 1) rank = (uint32_t)(__popcll(c.cx) + __popcll(c.cy & below));
        else rank = (uint32_t)(__popcll(c.cx) + __popcll(c.cy) + __popcll(c.cz & below));
        return vbase[pw] + rank;
    }
    // the vertex sits on a grid point: it is that point's vertex
    if (!((c.cp >> b) & 1ull)) {
        if (ax == 0) i++;
        else if (ax == 1) jf++;
        else k++;
        w = i >> 6;
        b = (int)(i & 63);
        pw = (k * g.NY + jf) * g.WX + w;
        c = rec[pw];
    }
    const uint32_t rank = (uint32_t)(__popcll(c.cx) + __popcll(c.cy) + __popcll(c.cz) + __popcll(c.cp & ((1ull << b) - 1ull)));
    return vbase[pw] + rank;
}

__global__ __launch_bounds__(256) void k_mci_faces(const CrossRec *__restrict__ rec, Geom g,
                                                   const uint32_t *__restrict__ vbase, uint32_t id0,
                                                   const uint64_t *__restrict__ list, uint64_t ntris,
                                                   int32_t *__restrict__ faces) {
    __shared__ uint8_t s_tri[256 * 16];
#pragma unroll
    for (int q = 0; q < 15; q++) s_tri[threadIdx.x * 16 + q] = MC_TRI[threadIdx.x][q];
    __syncthreads();
    const uint64_t T_ = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (T_ >= ntris) return;
    const uint64_t d = list[T_];
    const int b = (int)(d >> 11) & 63, idx = (int)(d >> 3) & 255, rel = (int)d & 7;
    const uint32_t w = (uint32_t)(d >> 17) & 0x7fffu;
    const int64_t k = (int64_t)(d >> 48), j = (int64_t)((d >> 32) & 0xffffull);
    const int64_t i = (int64_t)w * 64 + b;
#pragma unroll
    for (int v = 0; v < 3; v++) {
        const int e = s_tri[idx * 16 + 3 * rel + v];
        int ax, bx, by, bz;
        edge_decode(e, ax, bx, by, bz);
        faces[T_ * 3 + v] = (int32_t)(id0 + vertex_id(rec, g, vbase, k + bz, j + by, i + bx, ax));
    }
}

// =====================================================================================================================
// Cross-slab stitch on the device (the vtkAppendPolyData + vtkCleanPolyData of join_process_surface,
// invesalius/data/surface_process.py:229-268, across the Z-slabs of SURVEY.md 8e).  Rank r's TOP point plane and rank r+1's
// BOTTOM point plane are the same slice of voxels, so both carry the vertices of that plane's x / y edges (and its point
// vertices).  A vertex IS a grid edge: the two copies are matched by edge identity -- same point word, same kind, same bit
// -- never by comparing floats:
//   k_mci_sig      per point word of a plane: (first local vertex id, cx, cy, cp)                 32 bytes per word
//   k_mci_match    bottom plane of this piece AND the signature received from below -> the copies to drop, per word + total
//   k_mci_gid0     global id of every vertex of the bottom plane's words: a dropped copy takes the id its twin has in the
//                  rank below, a kept one moves down by the copies dropped before it
//   k_mci_stitch_faces / _verts   faces -> global ids, vertices compacted; everything above the bottom plane just shifts
// Global numbering: rank r's kept vertices follow rank r-1's, base_r = sum over q < r of (V_q - D_q); the (V, D) pairs
// travel through ONE all-gather of 8 bytes per rank.  The result equals the host stitch (tests/_stitch_ref.py) array for
// array.
// =====================================================================================================================
struct PlaneSig {
    uint32_t vbase, pad;
    uint64_t cx, cy, cp;
};
static_assert(sizeof(PlaneSig) == 32, "plane signatures travel as raw bytes");

__global__ __launch_bounds__(256) void k_mci_sig(const uint64_t *__restrict__ bits, const uint64_t *__restrict__ qb, Geom g,
                                                 uint64_t pbits, uint64_t qbits, const uint32_t *__restrict__ vbase, int64_t k,
                                                 PlaneSig *__restrict__ sig) {
    const int64_t nwp = g.NY * g.WX;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwp) return;
    const int64_t w = i % g.WX, jf = i / g.WX;
    const Cross c = crossings<true>(bits, qb, g, k, jf, w, pbits, qbits);
    PlaneSig sgn;
    sgn.vbase = vbase[k * nwp + i];
    sgn.pad = 0;
    sgn.cx = c.cx;
    sgn.cy = c.cy;
    sgn.cp = c.cp;
    sig[i] = sgn;
}

// vd[0] = this piece's vertex count, vd[1] (zeroed before) += copies dropped; rmcnt[word] = copies dropped in that word
__global__ __launch_bounds__(256) void k_mci_match(const uint64_t *__restrict__ bits, const uint64_t *__restrict__ qb, Geom g,
                                                   uint64_t pbits, uint64_t qbits, const PlaneSig *__restrict__ nbr,
                                                   uint32_t *__restrict__ rmcnt, uint32_t *vd, uint32_t nverts) {
    const int64_t nwp = g.NY * g.WX;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) vd[0] = nverts;
    uint32_t n = 0;
    if (i < nwp && nbr) {
        const int64_t w = i % g.WX, jf = i / g.WX;
        const Cross c = crossings<true>(bits, qb, g, 0, jf, w, pbits, qbits);
        const PlaneSig o = nbr[i];
        n = (uint32_t)(__popcll(c.cx & o.cx) + __popcll(c.cy & o.cy) + __popcll(c.cp & o.cp));
    }
    if (i < nwp) rmcnt[i] = n;
    uint32_t sum = n;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&vd[1], sum);
}

__device__ __forceinline__ void stitch_bases(const uint32_t *__restrict__ vd_all, int rank, uint32_t &base, uint32_t &base_below,
                                             uint32_t &d_below) {
    uint32_t b = 0;
    base_below = 0;
    d_below = 0;
    for (int q = 0; q < rank; q++) {
        if (q == rank - 1) {
            base_below = b;
            d_below = vd_all[2 * q + 1];
        }
        b += vd_all[2 * q] - vd_all[2 * q + 1];
    }
    base = b;
}

// rmoff = exclusive scan of rmcnt over the bottom plane's words
__global__ __launch_bounds__(256) void k_mci_gid0(const uint64_t *__restrict__ bits, const uint64_t *__restrict__ qb, Geom g,
                                                  uint64_t pbits, uint64_t qbits, const uint32_t *__restrict__ vbase,
                                                  const PlaneSig *__restrict__ nbr, const uint32_t *__restrict__ rmoff,
                                                  const uint32_t *__restrict__ vd_all, int rank, uint32_t *__restrict__ gid0) {
    const int64_t nwp = g.NY * g.WX;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwp) return;
    const int64_t w = i % g.WX, jf = i / g.WX;
    const Cross c = crossings<true>(bits, qb, g, 0, jf, w, pbits, qbits);
    if (!(c.cx | c.cy | c.cz | c.cp)) return;
    uint32_t base, base_below, d_below;
    stitch_bases(vd_all, rank, base, base_below, d_below);
    PlaneSig o;
    o.vbase = 0; o.pad = 0; o.cx = 0; o.cy = 0; o.cp = 0;
    if (nbr) o = nbr[i];
    uint32_t local = vbase[i];
    uint32_t kept = local - rmoff[i]; // position among this piece's kept vertices
    // the rank below numbers the word's vertices cx, cy, (no cz on its top plane), cp
    const uint32_t ocx = (uint32_t)__popcll(o.cx), ocy = (uint32_t)__popcll(o.cy);
#pragma unroll
    for (int ax = 0; ax < 4; ax++) {
        uint64_t m = ax == 0 ? c.cx : (ax == 1 ? c.cy : (ax == 2 ? c.cz : c.cp));
        const uint64_t om = ax == 0 ? o.cx : (ax == 1 ? o.cy : (ax == 2 ? 0ull : o.cp));
        const uint32_t obefore = ax == 0 ? 0u : (ax == 1 ? ocx : ocx + ocy);
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            if (om >> b & 1ull) // a copy: the twin's id in the rank below, after ITS dropped copies (all of which precede its top plane)
                gid0[local] = base_below + (o.vbase + obefore + (uint32_t)__popcll(om & ((1ull << b) - 1ull))) - d_below;
            else
                gid0[local] = base + kept++;
            local++;
        }
    }
}

__global__ __launch_bounds__(256) void k_mci_stitch_faces(int32_t *__restrict__ faces, int64_t n3, uint32_t p0,
                                                          const uint32_t *__restrict__ gid0, const uint32_t *__restrict__ vd_all,
                                                          int rank) {
    uint32_t base, bb, db;
    stitch_bases(vd_all, rank, base, bb, db);
    const uint32_t d = vd_all[2 * rank + 1];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += stride) {
        const uint32_t v = (uint32_t)faces[i];
        faces[i] = (int32_t)(v < p0 ? gid0[v] : base + v - d);
    }
}

__global__ __launch_bounds__(256) void k_mci_stitch_verts(const float *__restrict__ verts, int64_t nverts, uint32_t p0,
                                                          const uint32_t *__restrict__ gid0, const uint32_t *__restrict__ vd_all,
                                                          int rank, float *__restrict__ out) {
    uint32_t base, bb, db;
    stitch_bases(vd_all, rank, base, bb, db);
    const uint32_t d = vd_all[2 * rank + 1];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nverts; v += stride) {
        const uint32_t gid = v < (int64_t)p0 ? gid0[v] : base + (uint32_t)v - d;
        if (gid < base) continue; // a dropped copy: its twin lives in the rank below
        const uint32_t o = gid - base;
        out[3 * (size_t)o] = verts[3 * v];
        out[3 * (size_t)o + 1] = verts[3 * v + 1];
        out[3 * (size_t)o + 2] = verts[3 * v + 2];
    }
}

// per-stream workspace WS_MCV: strict[niso][bits_words] u64 | per iso: vbase[npw] u32, bsum[nsb], total[16] | per iso:
// crossing records[npw] (32 B each)
struct MciLayout {
    int64_t npw, nsb;
    size_t off_v, per_iso, off_rec, per_iso_rec, total;
};
static MciLayout mci_layout(const Geom &g, const Scratch &s, int niso) {
    MciLayout m;
    m.npw = g.NZ * g.NY * g.WX;
    m.nsb = ivx::cdiv(m.npw, 256 * 16);
    m.off_v = al256((size_t)niso * s.bits_words * 8 + 16);
    m.per_iso = al256(((size_t)m.npw + (size_t)m.nsb + 16) * 4);
    m.off_rec = m.off_v + (size_t)niso * m.per_iso;
    m.per_iso_rec = al256((size_t)m.npw * sizeof(CrossRec));
    m.total = m.off_rec + (size_t)niso * m.per_iso_rec;
    return m;
}
static inline uint64_t pad_qbits(const ivx_mc_params *p, int q) { return p->pad_value > p->iso[q] ? ~0ull : 0ull; }

} // namespace

// ---- indexed mesh API: must follow ivx_dev_mc_count on the same params / scratch / stream --------------------------
static int mc_indexed_count_impl(const ivx_mc_params *p, const void *a, const void *scratch_, int64_t *nverts, void *stream,
                                 bool levels);
extern "C" int ivx_dev_mc_indexed_count(const ivx_mc_params *p, const void *a, const void *scratch_, int64_t *nverts,
                                        void *stream) {
    return mc_indexed_count_impl(p, a, scratch_, nverts, stream, false);
}
// ivx_dev_mc_indexed_count for a mask whose bytes are known to lie strictly on either side of the iso-value (the levels of
// ivx_dev_mc_emit_levels; follows ivx_dev_mc_count_bits): "value > iso" IS the inside plane, so the pass over the mask that
// derives the strictly-inside plane is a copy of 1/8 byte per voxel instead of a read of the volume.
extern "C" int ivx_dev_mc_indexed_count_levels(const ivx_mc_params *p, const void *scratch_, int64_t *nverts, void *stream) {
    IVX_REQUIRE(p && p->dtype == IVX_U8 && p->niso == 1, IVX_EINVAL, "mc_indexed_count_levels: uint8 mask, one iso-value");
    return mc_indexed_count_impl(p, nullptr, scratch_, nverts, stream, true);
}
static int mc_indexed_count_impl(const ivx_mc_params *p, const void *a, const void *scratch_, int64_t *nverts, void *stream,
                                 bool levels) {
    Geom g;
    Scratch s;
    bool empty;
    int rc = mc_piece_layout(p, &g, &s, &empty);
    if (rc) return rc;
    *nverts = 0;
    if (empty) return IVX_OK;
    hipStream_t st = S(stream);
    const MciLayout m = mci_layout(g, s, p->niso);
    void *d_v;
    if ((rc = ivx::ws_get_s(ivx::WS_MCV, st, m.total, &d_v))) return rc;
    // strictly-inside planes: value > iso  <=>  value >= nextafter(iso, +inf)
    const double n0 = std::nextafter(p->iso[0], HUGE_VAL), n1 = std::nextafter(p->iso[1], HUGE_VAL);
    if (levels) {
        IVX_REQUIRE(p->pad_value < p->iso[0], IVX_EINVAL, "mc_indexed_count_levels: the padding must lie below the iso-value");
        IVX_HIP(hipMemcpyAsync(d_v, mc_bits_ptr(scratch_, s, 0), s.bits_words * 8, hipMemcpyDeviceToDevice, st));
    } else if ((rc = mc_inside_planes(p, g, s, a, d_v, n0, n1, st)))
        return rc;
    uint32_t tot[2] = {0, 0};
    for (int q = 0; q < p->niso; q++) {
        uint32_t *vbase = (uint32_t *)((char *)d_v + m.off_v + (size_t)q * m.per_iso);
        uint32_t *bsum = vbase + m.npw, *d_total = bsum + m.nsb;
        const uint64_t *bits = mc_bits_ptr(scratch_, s, q);
        const uint64_t *qb = (const uint64_t *)d_v + (size_t)q * s.bits_words;
        const int64_t blocks = ivx::cdiv(m.npw, 256);
        hipLaunchKernelGGL(k_mci_count, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, bits, qb, g,
                           m.npw, pad_bits(p, q), pad_qbits(p, q), vbase, (CrossRec *)((char *)d_v + m.off_rec + (size_t)q * m.per_iso_rec));
        IVX_LAUNCH_CHECK();
        if ((rc = scan_u32_exclusive(vbase, m.npw, bsum, d_total, st))) return rc;
        uint32_t seq;
        if ((rc = ivx::mailbox_publish(d_total, 1, st, &seq))) return rc;
        if ((rc = ivx::mailbox_wait(seq, st, &tot[q], 1))) return rc;
    }
    mc_pieces().set_vsplit(scratch_, tot[0]);
    *nverts = (int64_t)tot[0] + (int64_t)tot[1];
    return IVX_OK;
}

template <typename T>
static int run_indexed(const ivx_mc_params *p, const Geom &g, const Scratch &s, const void *a, const char *scratch,
                       float *verts, int64_t max_verts, int32_t *faces, int64_t max_tris, hipStream_t st, const McLevels *lv) {
    const MciLayout m = mci_layout(g, s, p->niso);
    void *d_v, *d_list;
    int rc;
    if ((rc = ivx::ws_get_s(ivx::WS_MCV, st, m.total, &d_v))) return rc;
    if ((rc = ivx::ws_get_s(ivx::WS_MCLIST, st, (size_t)max_tris * 8 + 64, &d_list))) return rc;
    const bool have_list = mc_pieces().list_ready(scratch, d_list, max_tris); // else: marks the buffer as about to be overwritten
    uint64_t tb[3] = {0, (uint64_t)max_tris, (uint64_t)max_tris};
    uint32_t vsplit = 0;
    IVX_REQUIRE(mc_pieces().get_vsplit(scratch, &vsplit), IVX_EINVAL, "mc: ivx_dev_mc_indexed_emit must follow ivx_dev_mc_indexed_count");
    if (p->niso == 2) // (where iso 0's triangles end: known once the count's total has been read)
        IVX_REQUIRE(mc_pieces().get_split(scratch, &tb[1]), IVX_EINVAL, "mc: ivx_dev_mc_indexed_emit must follow ivx_dev_mc_count");
    if (!have_list && (rc = mc_queue_list(p, g, s, scratch, d_list, max_tris, st))) return rc;
    for (int q = 0; q < p->niso; q++) {
        const uint64_t *bits = mc_bits_ptr(scratch, s, q);
        const uint32_t *vbase = (const uint32_t *)((const char *)d_v + m.off_v + (size_t)q * m.per_iso);
        const uint32_t id0 = q == 0 ? 0u : vsplit;
        const int64_t blocks = ivx::cdiv(m.npw, 256);
        const CrossRec *rec = (const CrossRec *)((const char *)d_v + m.off_rec + (size_t)q * m.per_iso_rec);
        if (lv)
            hipLaunchKernelGGL(k_mci_vertices_levels, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, bits, rec,
                               g, m.npw, pad_bits(p, q), *lv, vbase, id0, verts, (uint64_t)max_verts);
        else
            hipLaunchKernelGGL((k_mci_vertices<T>), dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st,
                               (const T *)a, rec, g, m.npw, p->iso[q], vbase, id0, verts, (uint64_t)max_verts);
        IVX_LAUNCH_CHECK();
        const uint64_t first = tb[q], last = tb[q + 1] < (uint64_t)max_tris ? tb[q + 1] : (uint64_t)max_tris;
        if (last > first) {
            hipLaunchKernelGGL(k_mci_faces, dim3((unsigned)ivx::cdiv((int64_t)(last - first), 256)), dim3(256), 0, st, rec, g, vbase,
                               id0, (const uint64_t *)d_list + first, last - first, faces + first * 3);
            IVX_LAUNCH_CHECK();
        }
    }
    return IVX_OK;
}

extern "C" int ivx_dev_mc_indexed_emit(const ivx_mc_params *p, const void *a, const void *scratch, float *verts,
                                       int64_t max_verts, int32_t *faces, int64_t max_tris, void *stream) {
    Geom g;
    Scratch s;
    bool empty;
    int rc = mc_piece_layout(p, &g, &s, &empty);
    if (rc) return rc;
    if (empty || max_tris <= 0) return IVX_OK;
    IVX_REQUIRE(max_verts < 0x7fffffffll, IVX_EINVAL, "mc: more than 2^31 vertices do not fit int32 face indices");
    return MC_BY_DTYPE(p->dtype, run_indexed, p, g, s, a, (const char *)scratch, verts, max_verts, faces, max_tris, S(stream), nullptr);
}

// ivx_dev_mc_indexed_emit after ivx_dev_mc_indexed_count_levels: the vertices from the mask's known byte levels (see
// ivx_dev_mc_emit_levels), no voxel is read; same vertices and faces, bit for bit, as the voxel path gives on that mask.
extern "C" int ivx_dev_mc_indexed_emit_levels(const ivx_mc_params *p, const void *scratch, const uint64_t *sel_bits, double v_out,
                                              double v_in, double v_sel, float *verts, int64_t max_verts, int32_t *faces,
                                              int64_t max_tris, void *stream) {
    Geom g;
    Scratch s;
    bool empty;
    int rc = mc_piece_layout(p, &g, &s, &empty);
    if (rc) return rc;
    IVX_REQUIRE(p->dtype == IVX_U8 && p->niso == 1, IVX_EINVAL, "mc_indexed_emit_levels: uint8 mask, one iso-value");
    IVX_REQUIRE(v_out < p->iso[0] && v_in > p->iso[0] && v_sel > p->iso[0] && p->pad_value == v_out, IVX_EINVAL,
                "mc_indexed_emit_levels: v_out (= the padding) must lie below the iso-value, v_in and v_sel above it");
    if (empty || max_tris <= 0) return IVX_OK;
    IVX_REQUIRE(max_verts < 0x7fffffffll, IVX_EINVAL, "mc: more than 2^31 vertices do not fit int32 face indices");
    const McLevels lv = make_levels(sel_bits, p->iso[0], v_out, v_in, v_sel);
    return run_indexed<uint8_t>(p, g, s, nullptr, (const char *)scratch, verts, max_verts, faces, max_tris, S(stream), &lv);
}

// ---- cross-slab stitch API: follows ivx_dev_mc_indexed_emit on the same params / scratch / stream (one iso-value) ------
struct StitchWs {
    PlaneSig *top;     // this piece's top-plane signature (what the rank above receives)
    uint32_t *rmcnt;   // copies dropped per bottom-plane word, then their exclusive scan
    uint32_t *bsum, *total, *gid0;
    size_t bytes;
};
static StitchWs stitch_layout(const Geom &g, uint32_t p0, char *base) {
    StitchWs w;
    const size_t nwp = (size_t)(g.NY * g.WX);
    size_t o = 0;
    auto take = [&](size_t n) { char *q = base ? base + o : nullptr; o += al256(n); return q; };
    w.top = (PlaneSig *)take(nwp * sizeof(PlaneSig));
    w.rmcnt = (uint32_t *)take((nwp + 1) * 4);
    w.bsum = (uint32_t *)take(((size_t)scan_u32_blocks((int64_t)nwp) + 2) * 4);
    w.total = (uint32_t *)take(64);
    w.gid0 = (uint32_t *)take(((size_t)p0 + 1) * 4);
    w.bytes = o;
    return w;
}
static int stitch_ctx(const ivx_mc_params *p, const void *scratch, hipStream_t st, Geom *g, Scratch *s, MciLayout *m, void **d_v) {
    int rc = make_geom(p, g);
    if (rc) return rc;
    IVX_REQUIRE(p->niso == 1, IVX_EINVAL, "mc stitch: one iso-value only");
    *s = make_scratch(*g, p->niso);
    IVX_REQUIRE(s->nwords > 0 && g->NZ >= 2, IVX_EINVAL, "mc stitch: the piece needs at least one cell layer");
    *m = mci_layout(*g, *s, p->niso);
    return ivx::ws_get_s(ivx::WS_MCV, st, m->total, d_v); // (the block ivx_dev_mc_indexed_count filled)
}

extern "C" int ivx_dev_mc_stitch_sig_bytes(const ivx_mc_params *p, size_t *nbytes) {
    Geom g;
    int rc = make_geom(p, &g);
    if (rc) return rc;
    *nbytes = (size_t)(g.NY * g.WX) * sizeof(PlaneSig);
    return IVX_OK;
}

// the signature of this piece's TOP point plane -> `sig` (device, ivx_dev_mc_stitch_sig_bytes): send it to the rank above
extern "C" int ivx_dev_mc_stitch_top_sig(const ivx_mc_params *p, const void *scratch, void *sig, void *stream) {
    Geom g;
    Scratch s;
    MciLayout m;
    void *d_v;
    hipStream_t st = ivx::S(stream);
    int rc = stitch_ctx(p, scratch, st, &g, &s, &m, &d_v);
    if (rc) return rc;
    const uint32_t *vbase = (const uint32_t *)((char *)d_v + m.off_v);
    const int64_t nwp = g.NY * g.WX;
    hipLaunchKernelGGL(k_mci_sig, dim3((unsigned)ivx::cdiv(nwp, 256)), dim3(256), 0, st, mc_bits_ptr(scratch, s, 0),
                       (const uint64_t *)d_v, g, pad_bits(p, 0), pad_qbits(p, 0), vbase, g.NZ - 1, (PlaneSig *)sig);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

// this piece's BOTTOM plane against the signature received from the rank below (NULL on the lowest rank):
// vd[0] = nverts, vd[1] = copies this piece drops (two device words: all-gather them over the ranks)
extern "C" int ivx_dev_mc_stitch_match(const ivx_mc_params *p, const void *scratch, const void *nbr_sig, int64_t nverts,
                                       uint32_t *vd, void *stream) {
    Geom g;
    Scratch s;
    MciLayout m;
    void *d_v, *d_w;
    hipStream_t st = ivx::S(stream);
    int rc = stitch_ctx(p, scratch, st, &g, &s, &m, &d_v);
    if (rc) return rc;
    IVX_REQUIRE(nverts >= 0 && nverts < 0x7fffffffll && vd, IVX_EINVAL, "mc stitch: bad vertex count");
    const int64_t nwp = g.NY * g.WX;
    StitchWs w = stitch_layout(g, 0, nullptr);
    if ((rc = ivx::ws_get_s(ivx::WS_MCST, st, w.bytes + ((size_t)nverts + 1) * 4 + 256, &d_w))) return rc;
    w = stitch_layout(g, (uint32_t)nverts, (char *)d_w); // (gid0 sized for the worst case: every vertex in the bottom plane)
    IVX_HIP(hipMemsetAsync(vd, 0, 8, st));
    hipLaunchKernelGGL(k_mci_match, dim3((unsigned)ivx::cdiv(nwp, 256)), dim3(256), 0, st, mc_bits_ptr(scratch, s, 0),
                       (const uint64_t *)d_v, g, pad_bits(p, 0), pad_qbits(p, 0), (const PlaneSig *)nbr_sig, w.rmcnt, vd,
                       (uint32_t)nverts);
    IVX_LAUNCH_CHECK();
    return scan_u32_exclusive(w.rmcnt, nwp, w.bsum, w.total, st);
}

// vd_all = the (nverts, dropped) pairs of every rank in rank order (device, 2 * world words).  `faces` (ntris x 3 local
// ids) become global ids in place; the vertices this piece keeps are written to `verts_out` in their old order
// (nverts - dropped of them; global id of the first one = sum over the ranks below of nverts - dropped).
extern "C" int ivx_dev_mc_stitch_apply(const ivx_mc_params *p, const void *scratch, const void *nbr_sig, const uint32_t *vd_all,
                                       int rank, const float *verts, int64_t nverts, int32_t *faces, int64_t ntris,
                                       float *verts_out, void *stream) {
    Geom g;
    Scratch s;
    MciLayout m;
    void *d_v, *d_w;
    hipStream_t st = ivx::S(stream);
    int rc = stitch_ctx(p, scratch, st, &g, &s, &m, &d_v);
    if (rc) return rc;
    IVX_REQUIRE(rank >= 0 && vd_all && nverts >= 0 && nverts < 0x7fffffffll, IVX_EINVAL, "mc stitch: bad arguments");
    const int64_t nwp = g.NY * g.WX;
    StitchWs w = stitch_layout(g, 0, nullptr);
    if ((rc = ivx::ws_get_s(ivx::WS_MCST, st, w.bytes + ((size_t)nverts + 1) * 4 + 256, &d_w))) return rc;
    w = stitch_layout(g, (uint32_t)nverts, (char *)d_w);
    const uint32_t *vbase = (const uint32_t *)((char *)d_v + m.off_v);
    // first local id above the bottom plane's words: read through the mailbox (sizes nothing, but the kernels need it)
    uint32_t p0 = (uint32_t)nverts;
    if (g.NZ > 1) {
        uint32_t seq;
        if ((rc = ivx::mailbox_publish(vbase + nwp, 1, st, &seq))) return rc;
        if ((rc = ivx::mailbox_wait(seq, st, &p0, 1))) return rc;
    }
    hipLaunchKernelGGL(k_mci_gid0, dim3((unsigned)ivx::cdiv(nwp, 256)), dim3(256), 0, st, mc_bits_ptr(scratch, s, 0),
                       (const uint64_t *)d_v, g, pad_bits(p, 0), pad_qbits(p, 0), vbase, (const PlaneSig *)nbr_sig, w.rmcnt,
                       vd_all, rank, w.gid0);
    IVX_LAUNCH_CHECK();
    if (ntris > 0) {
        const int64_t n3 = ntris * 3, blocks = ivx::cdiv(n3, 256);
        hipLaunchKernelGGL(k_mci_stitch_faces, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, faces, n3, p0,
                           w.gid0, vd_all, rank);
        IVX_LAUNCH_CHECK();
    }
    if (nverts > 0) {
        const int64_t blocks = ivx::cdiv(nverts, 256);
        hipLaunchKernelGGL(k_mci_stitch_verts, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, verts, nverts,
                           p0, w.gid0, vd_all, rank, verts_out);
        IVX_LAUNCH_CHECK();
    }
    return IVX_OK;
}

// Host form: strided piece in, indexed mesh out.  verts == NULL -> counts only (*nverts, *ntris).
extern "C" int ivx_marching_cubes_indexed(const ivx_mc_params *p, const void *a, const int64_t strides[3], float *verts,
                                          int64_t max_verts, int32_t *faces, int64_t max_tris, int64_t *nverts,
                                          int64_t *ntris) {
    ivx::HostCallGuard host_guard__;
    void *d_a, *d_scr;
    int rc = mc_upload_piece(p, a, strides, &d_a, &d_scr);
    if (rc) return rc;
    int64_t nt = 0, nv = 0;
    if ((rc = ivx_dev_mc_count(p, d_a, d_scr, &nt, nullptr))) return rc;
    if ((rc = ivx_dev_mc_indexed_count(p, d_a, d_scr, &nv, nullptr))) return rc;
    *ntris = nt;
    *nverts = nv;
    if (!verts || !faces || nt == 0) return IVX_OK;
    IVX_REQUIRE(max_tris >= nt && max_verts >= nv, IVX_ERANGE, "mc: output buffers too small (%lld verts, %lld triangles needed)",
                (long long)nv, (long long)nt);
    void *d_verts, *d_faces;
    if ((rc = ws_get(WS_OUT, (size_t)nv * 12 + 64, &d_verts))) return rc;
    if ((rc = ws_get(WS_AUX1, (size_t)nt * 12 + 64, &d_faces))) return rc;
    if ((rc = ivx_dev_mc_indexed_emit(p, d_a, d_scr, (float *)d_verts, nv, (int32_t *)d_faces, nt, nullptr))) return rc;
    IVX_HIP(hipMemcpy(verts, d_verts, (size_t)nv * 12, hipMemcpyDeviceToHost));
    IVX_HIP(hipMemcpy(faces, d_faces, (size_t)nt * 12, hipMemcpyDeviceToHost));
    return IVX_OK;
}
