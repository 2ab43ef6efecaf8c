// k_meshgeo.hip -- the geodesic measure: shortest paths along the triangle edges of the indexed surface.
//
// Reference: GeodesicMeasure._draw_line, invesalius/data/measures.py:1202-1256 -- vtkDijkstraGraphGeodesicPath between
// consecutive picks (a serial heap Dijkstra that settles the whole mesh), the summed edge length shown in mm.
//
// What is computed.  The graph is the set of triangle sides (a side with two equal ids is no edge), the weight of an edge
// w = sqrt((dx dx + dy dy) + dz dz) in float64 from the float32 positions, and the distance field the least fixed point of
// d[v] = min_u fl(d[u] + w(u, v)).  fl(a + w) is monotone in a and never below a, so no relaxation order can change a bit
// of it: the field is pinned to scipy.sparse.csgraph.dijkstra bit for bit, whatever delta / rounds_per_look are.
//
// MI355X design.  Gather / scatter over a mesh that sits in L2 + Infinity Cache; no MFMA.
//   * graph: count -> scan -> fill -> per-point sort + de-duplication -> scan -> compact, into a caller-owned buffer that is
//     built once per mesh.  No bound on the valence: long lists are heap-sorted in place.
//   * distances: rounds over a frontier kept as one byte per point and read 16 bytes per lane (a wave whose 1024 flags are
//     all zero ends there).  A round is two relaxation phases (atomicMin on the bits of the candidate, then the smallest id
//     among the winners becomes the predecessor -- the `seed` mechanism of k_pw_relax), a commit and a one-thread step that
//     moves the threshold.  Between rounds nd == dist, np == NONE and nf == 0 everywhere, so a round touches the frontier
//     and its neighbours only.
//   * the host queues rounds_per_look rounds and then reads the control block through the mailbox; rounds queued behind the
//     last one return at their first load.  Every wait is bounded: rounds by 4 nverts + 64, the back-trace by nverts steps.
#include <algorithm>
#include <math.h>

#include "ivx_internal.h"
#include "scan_u32.h"

namespace {

constexpr unsigned long long INF_BITS = 0x7ff0000000000000ull;
constexpr uint32_t NONE = 0xffffffffu;
constexpr int64_t GRAPH_MAGIC = 0x31304f4547585649ll; // "IVXGEO01"
// the defaults: the pair with the lowest median for the half-way pair in the sweep of DESIGN 7j
constexpr int DEFAULT_ROUNDS_PER_LOOK = 16;
constexpr double DEFAULT_DELTA_EDGES = 4.0; // x the mesh's mean edge length
constexpr int SUM_BLOCKS = 1024;

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline unsigned grid_for(int64_t n) { return (unsigned)std::max<int64_t>(1, ivx::cdiv(n, 256)); }

// ---- the graph buffer: header (32 int64), offsets (nv + 1 uint32), neighbours --------------------------------------------
struct GraphLayout {
    size_t off, adj, total;
};
static GraphLayout graph_layout(int64_t nv, int64_t nt) {
    GraphLayout g;
    g.off = 256;
    g.adj = g.off + al256(((size_t)nv + 2) * 4);
    g.total = g.adj + al256((size_t)nt * 6 * 4 + 16);
    return g;
}

__global__ __launch_bounds__(256) void k_geo_zero(uint32_t *__restrict__ a, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) a[i] = 0u;
}
// one thread per triangle side (a, b), a != b: an entry in a's list and one in b's; what atomicAdd returns is the entry's slot
__global__ __launch_bounds__(256) void k_geo_count(const int32_t *__restrict__ faces, int64_t nt, uint32_t *__restrict__ cnt,
                                                   uint32_t *__restrict__ slot) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= 3 * nt) return;
    const int64_t t = s / 3;
    const int k = (int)(s - 3 * t);
    const uint32_t a = (uint32_t)faces[s], b = (uint32_t)faces[3 * t + (k == 2 ? 0 : k + 1)];
    if (a == b) return;
    slot[2 * s] = atomicAdd(&cnt[a], 1u);
    slot[2 * s + 1] = atomicAdd(&cnt[b], 1u);
}
__global__ __launch_bounds__(256) void k_geo_fill(const int32_t *__restrict__ faces, int64_t nt, const uint32_t *__restrict__ poff,
                                                  const uint32_t *__restrict__ slot, uint32_t *__restrict__ padj) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= 3 * nt) return;
    const int64_t t = s / 3;
    const int k = (int)(s - 3 * t);
    const uint32_t a = (uint32_t)faces[s], b = (uint32_t)faces[3 * t + (k == 2 ? 0 : k + 1)];
    if (a == b) return;
    padj[poff[a] + slot[2 * s]] = b;
    padj[poff[b] + slot[2 * s + 1]] = a;
}
__device__ __forceinline__ void sift_down(uint32_t *__restrict__ a, uint32_t i, uint32_t n) {
    const uint32_t x = a[i];
    for (;;) {
        uint32_t c = 2 * i + 1;
        if (c >= n) break;
        if (c + 1 < n && a[c + 1] > a[c]) c++;
        if (a[c] <= x) break;
        a[i] = a[c];
        i = c;
    }
    a[i] = x;
}
// one lane per point: sort its list in place (insertion sort when short, heap sort past that: no bound on the valence),
// then squeeze the duplicates out; deg[v] = unique neighbours
__global__ __launch_bounds__(256) void k_geo_sort_unique(int64_t nv, const uint32_t *__restrict__ poff, uint32_t *__restrict__ padj,
                                                         uint32_t *__restrict__ deg) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v > nv) return;
    if (v == nv) {
        deg[v] = 0u;
        return;
    }
    const uint32_t b = poff[v], n = poff[v + 1] - b;
    uint32_t *a = padj + b;
    if (n <= 32u) {
        for (uint32_t i = 1; i < n; i++) {
            const uint32_t x = a[i];
            uint32_t j = i;
            while (j > 0 && a[j - 1] > x) {
                a[j] = a[j - 1];
                j--;
            }
            a[j] = x;
        }
    } else {
        for (uint32_t i = n / 2; i-- > 0;) sift_down(a, i, n);
        for (uint32_t m = n - 1; m > 0; m--) {
            const uint32_t top = a[0];
            a[0] = a[m];
            a[m] = top;
            sift_down(a, 0, m);
        }
    }
    uint32_t u = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t x = a[i];
        if (u == 0 || a[u - 1] != x) a[u++] = x;
    }
    deg[v] = u;
}
__global__ __launch_bounds__(256) void k_geo_compact(int64_t nv, const uint32_t *__restrict__ poff, const uint32_t *__restrict__ padj,
                                                     const uint32_t *__restrict__ off, uint32_t *__restrict__ adj) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const uint32_t a = off[v], n = off[v + 1] - a;
    const uint32_t *src = padj + poff[v];
    for (uint32_t k = 0; k < n; k++) adj[a + k] = src[k];
}
__global__ void k_geo_header(int64_t *__restrict__ h, int64_t nv, int64_t nt, const uint32_t *__restrict__ off, int64_t at_off,
                             int64_t at_adj) {
    if (threadIdx.x || blockIdx.x) return;
    h[0] = GRAPH_MAGIC;
    h[1] = nv;
    h[2] = nt;
    h[3] = (int64_t)off[nv];
    h[4] = at_off;
    h[5] = at_adj;
}

// ---- distances -----------------------------------------------------------------------------------------------------------
// the control block: written by the one-thread step and by the commit's counters, read by every kernel of a round; its
// first 6 dwords are what the host looks at
struct GeoCtl {
    uint32_t done, rounds, advances, pad;
    unsigned long long relaxations;
    uint32_t near_n, far_n;
    unsigned long long far_min, thr, dstop;
};
struct GeoState {
    unsigned long long *dist, *nd;
    uint32_t *pred, *np;
    uint8_t *front, *nf;
    GeoCtl *ctl;
    double *delta; // one double on the device: the caller's, or the default made from the mean edge length
};
struct GeoWs {
    size_t nd, np, front, nf, ctl, dist, pred, trace, delta, partial, total;
};
static inline int64_t pad16(int64_t nv) { return (nv + 15) & ~(int64_t)15; }
static GeoWs geo_ws(int64_t nv) {
    GeoWs m;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += al256(bytes + 16);
        return at;
    };
    m.nd = take((size_t)nv * 8);
    m.np = take((size_t)nv * 4);
    m.front = take((size_t)pad16(nv));
    m.nf = take((size_t)pad16(nv));
    m.ctl = take(256);
    m.dist = take((size_t)nv * 8);
    m.pred = take((size_t)nv * 4);
    m.trace = take(256);
    m.delta = take(256);
    m.partial = take((size_t)SUM_BLOCKS * 8);
    m.total = o;
    return m;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)x, o, 64), hi = __shfl_xor((uint32_t)(x >> 32), o, 64);
        const unsigned long long y = ((unsigned long long)hi << 32) | lo;
        x = y < x ? y : x;
    }
    return x;
}

// the default delta: DEFAULT_DELTA_EDGES x the mean edge length.  It decides the schedule and with it the predecessors, which
// must not change from run to run: a fixed grid, every thread its points in order, trees in LDS -- no atomics on doubles
__global__ __launch_bounds__(256) void k_geo_edge_sum(const float *__restrict__ pos, int64_t nv, const uint32_t *__restrict__ off,
                                                      const uint32_t *__restrict__ adj, double *__restrict__ partial) {
    __shared__ double s_sum[256];
    double acc = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += (int64_t)SUM_BLOCKS * 256) {
        const double px = (double)pos[3 * v], py = (double)pos[3 * v + 1], pz = (double)pos[3 * v + 2];
        const uint32_t e1 = off[v + 1];
        for (uint32_t e = off[v]; e < e1; e++) {
            const int64_t u = adj[e];
            const double dx = (double)pos[3 * u] - px, dy = (double)pos[3 * u + 1] - py, dz = (double)pos[3 * u + 2] - pz;
            acc += __dsqrt_rn((dx * dx + dy * dy) + dz * dz);
        }
    }
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = s_sum[0];
}
__global__ __launch_bounds__(SUM_BLOCKS) void k_geo_default_delta(const double *__restrict__ partial, const uint32_t *__restrict__ off,
                                                                  int64_t nv, double edges, double *__restrict__ delta) {
    __shared__ double s_sum[SUM_BLOCKS];
    s_sum[threadIdx.x] = partial[threadIdx.x];
    __syncthreads();
    for (int o = SUM_BLOCKS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t stored = off[nv];
        const double d = stored ? edges * (s_sum[0] / (double)stored) : 0.0;
        *delta = d > 0.0 ? d : __longlong_as_double((long long)INF_BITS); // no edges, or only zero-length ones: plain relaxation
    }
}
__global__ void k_geo_set_delta(double *__restrict__ delta, double value) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *delta = value;
}

__global__ __launch_bounds__(256) void k_geo_init(int64_t nv, int64_t nvpad, int64_t source, int64_t stop, GeoState s) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nvpad) return;
    const bool src = v == source;
    s.front[v] = src ? 1 : 0; // (the flags' padding up to a multiple of 16 stays zero for good)
    s.nf[v] = 0;
    if (v >= nv) return;
    s.dist[v] = src ? 0ull : INF_BITS;
    s.nd[v] = src ? 0ull : INF_BITS;
    s.pred[v] = NONE;
    s.np[v] = NONE;
    if (src) {
        GeoCtl c;
        c.done = 0, c.rounds = 0, c.advances = 0, c.pad = 0, c.relaxations = 0ull, c.near_n = 0, c.far_n = 0;
        c.far_min = INF_BITS;
        c.thr = (unsigned long long)__double_as_longlong(*s.delta); // smallest distance (0) + delta
        c.dstop = stop == source ? 0ull : INF_BITS;
        *s.ctl = c;
    }
}

__device__ __forceinline__ double as_d(unsigned long long b) { return __longlong_as_double((long long)b); }

// The flags are read 16 bytes per lane -- a wave whose 1024 flags are all zero ends there -- and then turned round through
// LDS so that in each of 16 passes the 64 lanes hold 64 CONSECUTIVE points: the dependent loads of a point (distance, list
// bounds, neighbour ids, their positions and distances) then overlap across the lanes instead of queueing up in one.
// Only lanes of one wave talk through their 1 KB of the block's LDS; LDS operations of a wave complete in order.
__device__ __forceinline__ void wave_lds_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

// a frontier point below the threshold and below d[stop_at] offers fl(d + w) to every neighbour.  PHASE 0: the smallest offer
// per neighbour (atomicMin on the bits); PHASE 1: among the neighbours whose offer won, the smallest id becomes the predecessor
template <int PHASE>
__global__ __launch_bounds__(256) void k_geo_relax(const float *__restrict__ pos, int64_t nvpad, const uint32_t *__restrict__ off,
                                                   const uint32_t *__restrict__ adj, GeoState s) {
    __shared__ uint4 s_front[256];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint4 w4 = make_uint4(0u, 0u, 0u, 0u);
    if (16 * t < nvpad) w4 = reinterpret_cast<const uint4 *>(s.front)[t];
    if (!__ballot((w4.x | w4.y | w4.z | w4.w) != 0u)) return; // the whole wave
    if (s.ctl->done) return;                                  // (the same word for every lane)
    const double thr = as_d(s.ctl->thr), dstop = as_d(s.ctl->dstop);
    const unsigned long long *__restrict__ dist = s.dist;
    unsigned long long *__restrict__ nd = s.nd;
    uint32_t *__restrict__ np = s.np;
    uint8_t *__restrict__ nf = s.nf;
    const int lane = threadIdx.x & 63, wbase = threadIdx.x & ~63;
    s_front[threadIdx.x] = w4;
    wave_lds_fence();
    const uint8_t *flags = reinterpret_cast<const uint8_t *>(s_front + wbase);
    const int64_t v0 = 16 * (t - lane);
    uint32_t relaxed = 0;
    for (int c = 0; c < 16; c++) {
        const bool mine = flags[64 * c + lane] != 0;
        if (!__ballot(mine)) continue;
        if (!mine) continue;
        const int64_t v = v0 + 64 * c + lane; // (a set flag: v < nverts)
        const double dv = as_d(dist[v]);
        if (!(dv < thr) || !(dv < dstop)) continue;
        relaxed++;
        const double px = (double)pos[3 * v], py = (double)pos[3 * v + 1], pz = (double)pos[3 * v + 2];
        const uint32_t e1 = off[v + 1];
        for (uint32_t e = off[v]; e < e1; e++) {
            const int64_t u = adj[e];
            const double dx = (double)pos[3 * u] - px, dy = (double)pos[3 * u + 1] - py, dz = (double)pos[3 * u + 2] - pz;
            const double cand = dv + __dsqrt_rn((dx * dx + dy * dy) + dz * dz);
            if (!(cand < as_d(dist[u]))) continue;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(cand);
            if (PHASE == 0) {
                atomicMin(&nd[u], bits);
            } else if (nd[u] == bits) {
                atomicMin(&np[u], (uint32_t)v);
                nf[u] = 1;
            }
        }
    }
    if (PHASE == 0) { // one same-address atomic per wave, not per lane
        const uint32_t total = wave_sum(relaxed);
        if (total && lane == 0) atomicAdd(&s.ctl->relaxations, (unsigned long long)total);
    }
}

// improved points take their new distance and predecessor and join the frontier; points that relaxed, or that d[stop_at]
// shuts out for good, leave it; the rest (the far set) wait.  Counts the new frontier on either side of the threshold.
__global__ __launch_bounds__(256) void k_geo_commit(int64_t nvpad, GeoState s) {
    __shared__ uint4 s_front[256], s_nf[256], s_out[256];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool inside = 16 * t < nvpad;
    uint4 f4 = make_uint4(0u, 0u, 0u, 0u), n4 = f4;
    if (inside) {
        f4 = reinterpret_cast<const uint4 *>(s.front)[t];
        n4 = reinterpret_cast<const uint4 *>(s.nf)[t];
    }
    if (!__ballot((f4.x | f4.y | f4.z | f4.w | n4.x | n4.y | n4.z | n4.w) != 0u)) return; // the whole wave
    if (s.ctl->done) return;                                                              // (the same word for every lane)
    const double thr = as_d(s.ctl->thr), dstop = as_d(s.ctl->dstop);
    const int lane = threadIdx.x & 63, wbase = threadIdx.x & ~63;
    s_front[threadIdx.x] = f4;
    s_nf[threadIdx.x] = n4;
    s_out[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    wave_lds_fence();
    const uint8_t *ff = reinterpret_cast<const uint8_t *>(s_front + wbase), *nn = reinterpret_cast<const uint8_t *>(s_nf + wbase);
    uint8_t *oo = reinterpret_cast<uint8_t *>(s_out + wbase);
    const int64_t v0 = 16 * (t - lane);
    uint32_t near_n = 0, far_n = 0;
    unsigned long long far_min = INF_BITS;
    for (int c = 0; c < 16; c++) {
        const uint32_t f = ff[64 * c + lane], n = nn[64 * c + lane];
        if (!__ballot((f | n) != 0u)) continue;
        if (!(f | n)) continue;
        const int64_t v = v0 + 64 * c + lane;
        unsigned long long d = s.dist[v];
        bool keep = f && !(as_d(d) < thr) && as_d(d) < dstop;
        if (n) {
            d = s.nd[v];
            s.dist[v] = d;
            s.pred[v] = s.np[v];
            s.np[v] = NONE;
            keep = true;
        }
        if (!keep) continue;
        oo[64 * c + lane] = 1;
        if (as_d(d) < thr) {
            near_n++;
        } else {
            far_n++;
            far_min = d < far_min ? d : far_min;
        }
    }
    wave_lds_fence();
    if (inside) {
        reinterpret_cast<uint4 *>(s.front)[t] = s_out[threadIdx.x];
        if (n4.x | n4.y | n4.z | n4.w) reinterpret_cast<uint4 *>(s.nf)[t] = make_uint4(0u, 0u, 0u, 0u);
    }
    near_n = wave_sum(near_n); // one same-address atomic per wave and counter, not per lane
    far_n = wave_sum(far_n);
    far_min = wave_min(far_min);
    if (lane == 0) {
        if (near_n) atomicAdd(&s.ctl->near_n, near_n);
        if (far_n) {
            atomicAdd(&s.ctl->far_n, far_n);
            atomicMin(&s.ctl->far_min, far_min);
        }
    }
}

// one thread, after the commit: an empty near set moves the threshold to (smallest far distance) + delta, or ends the run
// when nothing is left that d[stop_at] lets through
__global__ void k_geo_step(int64_t stop, GeoState s) {
    if (threadIdx.x || blockIdx.x) return;
    GeoCtl *c = s.ctl;
    if (c->done) return;
    const double delta = *s.delta;
    c->rounds++;
    const unsigned long long dstop = stop >= 0 ? s.dist[stop] : INF_BITS;
    c->dstop = dstop;
    if (c->near_n == 0) {
        if (c->far_n == 0 || !(as_d(c->far_min) < as_d(dstop))) {
            c->done = 1;
        } else {
            unsigned long long thr = (unsigned long long)__double_as_longlong(as_d(c->far_min) + delta);
            if (thr <= c->far_min) thr = c->far_min + 1; // a delta below the spacing of doubles there: the next double up
            c->thr = thr;
            c->advances++;
        }
    }
    c->near_n = 0;
    c->far_n = 0;
    c->far_min = INF_BITS;
}

// ---- back-trace: one wave.  Lane 0 walks pred from the end, the wave turns the ids round -------------------------------
// res[0] = ids written, res[1] = status (0 fine, 1 no room, 2 the walk did not end at the start), res[2..3] = bits of d[end]
__global__ __launch_bounds__(64) void k_geo_trace(const unsigned long long *__restrict__ dist, const uint32_t *__restrict__ pred,
                                                  int64_t nv, int64_t start, int64_t end, int32_t *__restrict__ path, int64_t room,
                                                  uint32_t *__restrict__ res) {
    __shared__ uint32_t s_n, s_status;
    if (threadIdx.x == 0) {
        const unsigned long long de = dist[end];
        uint32_t n = 0, status = 0;
        if (de != INF_BITS) {
            int64_t v = end;
            for (int64_t step = 0; step < nv; step++) { // a path visits a point once: nv steps at the most
                if ((int64_t)n < room) path[n] = (int32_t)v;
                else status = 1;
                n++;
                if (v == start) break;
                const uint32_t p = pred[v];
                if (p == NONE) {
                    status = 2;
                    break;
                }
                v = p;
            }
            if (status == 0 && v != start) status = 2;
        }
        s_n = n;
        s_status = status;
        res[0] = n;
        res[1] = status;
        res[2] = (uint32_t)de;
        res[3] = (uint32_t)(de >> 32);
    }
    __syncthreads();
    if (s_status) return;
    const uint32_t n = s_n;
    for (uint32_t i = threadIdx.x; i < n / 2; i += 64) {
        const int32_t a = path[i], b = path[n - 1 - i];
        path[i] = b;
        path[n - 1 - i] = a;
    }
}
__global__ void k_geo_one(int32_t *__restrict__ path, int32_t id) {
    if (threadIdx.x == 0 && blockIdx.x == 0) path[0] = id;
}

static int check_sizes(int64_t nverts, int64_t ntris, const char *who) {
    IVX_REQUIRE(nverts >= 0 && ntris >= 0, IVX_EINVAL, "%s: negative size", who);
    IVX_REQUIRE(nverts < 0x7fffffffll && ntris < 0x2aaaaaaall, IVX_EINVAL, "%s: mesh too large for 32-bit ids", who);
    return IVX_OK;
}
static int check_faces(const int32_t *faces, int64_t ntris, int64_t nverts) {
    for (int64_t q = 0; q < 3 * ntris; q++)
        IVX_REQUIRE(faces[q] >= 0 && faces[q] < nverts, IVX_EDOM, "mesh: face index %d outside [0, %lld)", faces[q],
                    (long long)nverts);
    return IVX_OK;
}

static int geo_state(int64_t nv, hipStream_t st, double *dist, int32_t *pred, GeoState *s, char **ws_out) {
    const GeoWs m = geo_ws(nv);
    void *ws;
    int rc = ivx::ws_get_s(ivx::WS_MESH2, st, m.total, &ws);
    if (rc) return rc;
    char *w = (char *)ws;
    s->nd = (unsigned long long *)(w + m.nd);
    s->np = (uint32_t *)(w + m.np);
    s->front = (uint8_t *)(w + m.front);
    s->nf = (uint8_t *)(w + m.nf);
    s->ctl = (GeoCtl *)(w + m.ctl);
    s->delta = (double *)(w + m.delta);
    s->dist = dist ? (unsigned long long *)dist : (unsigned long long *)(w + m.dist);
    s->pred = pred ? (uint32_t *)pred : (uint32_t *)(w + m.pred);
    *ws_out = w;
    return IVX_OK;
}

// the rounds: `s` is set up by geo_state; adds to stats[0..3]
static int run_distances(const float *verts, int64_t nv, const void *graph, int64_t source, int64_t stop, double delta,
                         int rounds_per_look, const GeoState &s, int64_t *stats, hipStream_t st) {
    const GraphLayout g = graph_layout(nv, 0);
    const uint32_t *off = (const uint32_t *)((const char *)graph + g.off);
    const uint32_t *adj = (const uint32_t *)((const char *)graph + g.adj);
    if (rounds_per_look <= 0) rounds_per_look = DEFAULT_ROUNDS_PER_LOOK;
    const int64_t nvpad = pad16(nv);
    if (delta > 0.0) {
        hipLaunchKernelGGL(k_geo_set_delta, dim3(1), dim3(64), 0, st, s.delta, delta);
        IVX_LAUNCH_CHECK();
    } else { // (a NaN takes the default as well)
        double *partial = (double *)((char *)s.delta + (geo_ws(nv).partial - geo_ws(nv).delta));
        hipLaunchKernelGGL(k_geo_edge_sum, dim3(SUM_BLOCKS), dim3(256), 0, st, verts, nv, off, adj, partial);
        IVX_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_geo_default_delta, dim3(1), dim3(SUM_BLOCKS), 0, st, (const double *)partial, off, nv, DEFAULT_DELTA_EDGES,
                           s.delta);
        IVX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_geo_init, dim3(grid_for(nvpad)), dim3(256), 0, st, nv, nvpad, source, stop, s);
    IVX_LAUNCH_CHECK();
    const unsigned gw = grid_for(nvpad / 16);
    const int64_t max_rounds = 4 * nv + 64; // a round lowers a distance, empties the near set or moves the threshold
    int64_t queued = 0, looks = 0;
    uint32_t got[6] = {0, 0, 0, 0, 0, 0};
    while (queued < max_rounds) {
        const int64_t batch = std::min<int64_t>(rounds_per_look, max_rounds - queued);
        for (int64_t r = 0; r < batch; r++) {
            hipLaunchKernelGGL((k_geo_relax<0>), dim3(gw), dim3(256), 0, st, verts, nvpad, off, adj, s);
            IVX_LAUNCH_CHECK();
            hipLaunchKernelGGL((k_geo_relax<1>), dim3(gw), dim3(256), 0, st, verts, nvpad, off, adj, s);
            IVX_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_geo_commit, dim3(gw), dim3(256), 0, st, nvpad, s);
            IVX_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_geo_step, dim3(1), dim3(64), 0, st, stop, s);
            IVX_LAUNCH_CHECK();
        }
        queued += batch;
        uint32_t seq;
        int rc;
        if ((rc = ivx::mailbox_publish(s.ctl, 6, st, &seq))) return rc;
        if ((rc = ivx::mailbox_wait(seq, st, got, 6))) return rc;
        looks++;
        if (got[0]) break;
    }
    if (stats) {
        stats[0] += (int64_t)got[1];
        stats[1] += (int64_t)(((unsigned long long)got[5] << 32) | got[4]);
        stats[2] += (int64_t)got[2];
        stats[3] += looks;
    }
    IVX_REQUIRE(got[0], IVX_EHIP, "mesh_geodesic: the frontier did not empty within %lld rounds", (long long)max_rounds);
    return IVX_OK;
}

static int check_graph_args(const void *verts, int64_t nverts, const void *graph, const char *who) {
    int rc;
    if ((rc = check_sizes(nverts, 0, who))) return rc;
    IVX_REQUIRE(nverts == 0 || (verts && graph), IVX_EINVAL, "%s: null argument", who);
    return IVX_OK;
}

} // namespace

extern "C" int ivx_mesh_graph_bytes(int64_t nverts, int64_t ntris, size_t *bytes) {
    int rc;
    IVX_REQUIRE(bytes, IVX_EINVAL, "mesh_graph_bytes: null argument");
    if ((rc = check_sizes(nverts, ntris, "mesh_graph_bytes"))) return rc;
    *bytes = graph_layout(nverts, ntris).total;
    return IVX_OK;
}

extern "C" int ivx_dev_mesh_graph_build(const int32_t *faces, int64_t nverts, int64_t ntris, void *graph, size_t graph_bytes,
                                        void *stream) {
    int rc;
    if ((rc = check_sizes(nverts, ntris, "mesh_graph_build"))) return rc;
    const GraphLayout g = graph_layout(nverts, ntris);
    IVX_REQUIRE(graph && (faces || ntris == 0), IVX_EINVAL, "mesh_graph_build: null argument");
    IVX_REQUIRE(graph_bytes >= g.total, IVX_ERANGE, "mesh_graph_build: room for %zu bytes, %zu needed", graph_bytes, g.total);
    hipStream_t st = ivx::S(stream);
    const int64_t nv = nverts, nt = ntris;
    // scratch: padded offsets, padded lists, the scan's block sums; the entries' slots wait in the graph's own neighbour block
    const size_t at_poff = 0, at_padj = at_poff + al256(((size_t)nv + 2) * 4), at_bsum = at_padj + al256((size_t)nt * 6 * 4 + 16),
                 at_misc = at_bsum + al256(((size_t)scan_u32_blocks(nv + 2) + 16) * 4), total = at_misc + 256;
    void *ws;
    if ((rc = ivx::ws_get_s(ivx::WS_MESH, st, total, &ws))) return rc;
    char *w = (char *)ws;
    uint32_t *poff = (uint32_t *)(w + at_poff), *padj = (uint32_t *)(w + at_padj), *bsum = (uint32_t *)(w + at_bsum),
             *misc = (uint32_t *)(w + at_misc);
    uint32_t *off = (uint32_t *)((char *)graph + g.off), *adj = (uint32_t *)((char *)graph + g.adj);
    uint32_t *slot = adj;
    hipLaunchKernelGGL(k_geo_zero, dim3(std::min(grid_for(nv + 2), 16384u)), dim3(256), 0, st, poff, nv + 2);
    IVX_LAUNCH_CHECK();
    if (nt) {
        hipLaunchKernelGGL(k_geo_count, dim3(grid_for(3 * nt)), dim3(256), 0, st, faces, nt, poff, slot);
        IVX_LAUNCH_CHECK();
    }
    if ((rc = scan_u32_exclusive(poff, nv + 1, bsum, misc, st))) return rc;
    if (nt) {
        hipLaunchKernelGGL(k_geo_fill, dim3(grid_for(3 * nt)), dim3(256), 0, st, faces, nt, poff, slot, padj);
        IVX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_geo_sort_unique, dim3(grid_for(nv + 1)), dim3(256), 0, st, nv, poff, padj, off);
    IVX_LAUNCH_CHECK();
    if ((rc = scan_u32_exclusive(off, nv + 1, bsum, misc + 1, st))) return rc;
    if (nv) {
        hipLaunchKernelGGL(k_geo_compact, dim3(grid_for(nv)), dim3(256), 0, st, nv, poff, padj, off, adj);
        IVX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_geo_header, dim3(1), dim3(64), 0, st, (int64_t *)graph, nv, nt, off, (int64_t)g.off, (int64_t)g.adj);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_mesh_geodesic_distances(const float *verts, int64_t nverts, const void *graph, int64_t source, int64_t stop_at,
                                               double delta, int rounds_per_look, double *dist, int32_t *pred, int64_t *stats,
                                               void *stream) {
    int rc;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if ((rc = check_graph_args(verts, nverts, graph, "mesh_geodesic_distances"))) return rc;
    IVX_REQUIRE(source >= 0 && source < nverts, IVX_EDOM, "mesh_geodesic_distances: source %lld outside [0, %lld)", (long long)source,
                (long long)nverts);
    IVX_REQUIRE(stop_at < nverts, IVX_EDOM, "mesh_geodesic_distances: stop_at %lld outside [0, %lld)", (long long)stop_at,
                (long long)nverts);
    IVX_REQUIRE(dist, IVX_EINVAL, "mesh_geodesic_distances: null argument");
    hipStream_t st = ivx::S(stream);
    GeoState s;
    char *w;
    if ((rc = geo_state(nverts, st, dist, pred, &s, &w))) return rc;
    return run_distances(verts, nverts, graph, source, stop_at < 0 ? -1 : stop_at, delta, rounds_per_look, s, stats, st);
}

extern "C" int ivx_dev_mesh_geodesic_path(const float *verts, int64_t nverts, const void *graph, const int32_t *ids, int64_t nids,
                                          int32_t *path, int64_t max_path, int64_t *seg_points, double *seg_length, int64_t *stats,
                                          void *stream) {
    int rc;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if ((rc = check_graph_args(verts, nverts, graph, "mesh_geodesic_path"))) return rc;
    IVX_REQUIRE(nids >= 2, IVX_EINVAL, "mesh_geodesic_path: %lld points, at least two needed", (long long)nids);
    IVX_REQUIRE(ids && seg_points && seg_length && max_path >= 0 && (path || max_path == 0), IVX_EINVAL,
                "mesh_geodesic_path: null argument");
    for (int64_t q = 0; q < nids; q++)
        IVX_REQUIRE(ids[q] >= 0 && ids[q] < nverts, IVX_EDOM, "mesh_geodesic_path: point id %d outside [0, %lld)", ids[q],
                    (long long)nverts);
    hipStream_t st = ivx::S(stream);
    GeoState s;
    char *w;
    if ((rc = geo_state(nverts, st, nullptr, nullptr, &s, &w))) return rc;
    uint32_t *res = (uint32_t *)(w + geo_ws(nverts).trace);
    int64_t used = 0;
    for (int64_t q = 0; q + 1 < nids; q++) {
        const int64_t a = ids[q], b = ids[q + 1];
        if (a == b) { // one id, length 0: nothing to search
            IVX_REQUIRE(used < max_path, IVX_ERANGE, "mesh_geodesic_path: room for %lld ids, more needed", (long long)max_path);
            hipLaunchKernelGGL(k_geo_one, dim3(1), dim3(64), 0, st, path + used, (int32_t)a);
            IVX_LAUNCH_CHECK();
            seg_points[q] = 1;
            seg_length[q] = 0.0;
            used += 1;
            continue;
        }
        if ((rc = run_distances(verts, nverts, graph, a, b, 0.0, 0, s, stats, st))) return rc;
        hipLaunchKernelGGL(k_geo_trace, dim3(1), dim3(64), 0, st, s.dist, s.pred, nverts, a, b, path + used, max_path - used, res);
        IVX_LAUNCH_CHECK();
        uint32_t seq, got[4];
        if ((rc = ivx::mailbox_publish(res, 4, st, &seq))) return rc;
        if ((rc = ivx::mailbox_wait(seq, st, got, 4))) return rc;
        IVX_REQUIRE(got[1] != 1, IVX_ERANGE, "mesh_geodesic_path: room for %lld ids, %lld needed so far", (long long)max_path,
                    (long long)(used + got[0]));
        IVX_REQUIRE(got[1] == 0, IVX_EHIP, "mesh_geodesic_path: the predecessors of point %lld do not lead back to point %lld",
                    (long long)b, (long long)a);
        const unsigned long long bits = ((unsigned long long)got[3] << 32) | got[2];
        double len;
        memcpy(&len, &bits, 8);
        seg_points[q] = (int64_t)got[0];
        seg_length[q] = len;
        used += (int64_t)got[0];
    }
    return IVX_OK;
}

// ---- host forms -----------------------------------------------------------------------------------------------------------
namespace {
static int upload_mesh_and_graph(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, void **d_v, void **d_g) {
    using namespace ivx;
    int rc;
    if ((rc = check_faces(faces, ntris, nverts))) return rc;
    void *d_f;
    size_t gbytes = graph_layout(nverts, ntris).total;
    if ((rc = ws_get(WS_IN, (size_t)nverts * 12 + 16, d_v))) return rc;
    if ((rc = ws_get(WS_AUX0, (size_t)ntris * 12 + 16, &d_f))) return rc;
    if ((rc = ws_get(WS_AUX1, gbytes, d_g))) return rc;
    IVX_HIP(hipMemcpy(*d_v, verts, (size_t)nverts * 12, hipMemcpyHostToDevice));
    if (ntris) IVX_HIP(hipMemcpy(d_f, faces, (size_t)ntris * 12, hipMemcpyHostToDevice));
    return ivx_dev_mesh_graph_build((const int32_t *)d_f, nverts, ntris, *d_g, gbytes, nullptr);
}
} // namespace

extern "C" int ivx_mesh_geodesic_distances(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, int64_t source,
                                           int64_t stop_at, double delta, int rounds_per_look, double *dist, int32_t *pred,
                                           int64_t *stats) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    int rc;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if ((rc = check_sizes(nverts, ntris, "mesh_geodesic_distances"))) return rc;
    IVX_REQUIRE(source >= 0 && source < nverts, IVX_EDOM, "mesh_geodesic_distances: source %lld outside [0, %lld)", (long long)source,
                (long long)nverts);
    IVX_REQUIRE(stop_at < nverts, IVX_EDOM, "mesh_geodesic_distances: stop_at %lld outside [0, %lld)", (long long)stop_at,
                (long long)nverts);
    IVX_REQUIRE(verts && dist && (faces || ntris == 0), IVX_EINVAL, "mesh_geodesic_distances: null argument");
    void *d_v, *d_g, *d_d, *d_p;
    if ((rc = upload_mesh_and_graph(verts, nverts, faces, ntris, &d_v, &d_g))) return rc;
    if ((rc = ws_get(WS_AUX2, (size_t)nverts * 8 + 16, &d_d))) return rc;
    if ((rc = ws_get(WS_AUX3, (size_t)nverts * 4 + 16, &d_p))) return rc;
    if ((rc = ivx_dev_mesh_geodesic_distances((const float *)d_v, nverts, d_g, source, stop_at, delta, rounds_per_look, (double *)d_d,
                                              (int32_t *)d_p, stats, nullptr)))
        return rc;
    IVX_HIP(hipDeviceSynchronize());
    IVX_HIP(hipMemcpy(dist, d_d, (size_t)nverts * 8, hipMemcpyDeviceToHost));
    if (pred) IVX_HIP(hipMemcpy(pred, d_p, (size_t)nverts * 4, hipMemcpyDeviceToHost));
    return IVX_OK;
}

extern "C" int ivx_mesh_geodesic_path(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, const int32_t *ids,
                                      int64_t nids, int32_t *path, int64_t max_path, int64_t *seg_points, double *seg_length,
                                      int64_t *stats) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    int rc;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if ((rc = check_sizes(nverts, ntris, "mesh_geodesic_path"))) return rc;
    IVX_REQUIRE(nids >= 2, IVX_EINVAL, "mesh_geodesic_path: %lld points, at least two needed", (long long)nids);
    IVX_REQUIRE(verts && ids && seg_points && seg_length && max_path >= 0 && (path || max_path == 0) && (faces || ntris == 0),
                IVX_EINVAL, "mesh_geodesic_path: null argument");
    for (int64_t q = 0; q < nids; q++)
        IVX_REQUIRE(ids[q] >= 0 && ids[q] < nverts, IVX_EDOM, "mesh_geodesic_path: point id %d outside [0, %lld)", ids[q],
                    (long long)nverts);
    void *d_v, *d_g, *d_p;
    if ((rc = upload_mesh_and_graph(verts, nverts, faces, ntris, &d_v, &d_g))) return rc;
    if ((rc = ws_get(WS_AUX3, (size_t)max_path * 4 + 16, &d_p))) return rc;
    if ((rc = ivx_dev_mesh_geodesic_path((const float *)d_v, nverts, d_g, ids, nids, (int32_t *)d_p, max_path, seg_points, seg_length,
                                         stats, nullptr)))
        return rc;
    IVX_HIP(hipDeviceSynchronize());
    int64_t used = 0;
    for (int64_t q = 0; q + 1 < nids; q++) used += seg_points[q];
    if (used) IVX_HIP(hipMemcpy(path, d_p, (size_t)used * 4, hipMemcpyDeviceToHost));
    return IVX_OK;
}
