// k_costlevels.hip -- the two watersheds' cost maps, level by level, as floods on bit planes.
//   ivx_dev_ws_cost_levels   the IFT watershed (k_wsift.hip): arc planes, scipy's linear-index neighbourhood
//   ivx_dev_sk_cost_levels   the scikit-image branch (k_wssk.hip): candidate planes {I <= c}, lattice neighbours
// Both prepare a level's planes and dirty tiles here and hand the flood itself to the region-growing engine
// (ivx::flood_run, k_flood.hip), whose tile grid and scratch layout they read through flood_tiles.h.
#include "flood_tiles.h"

// ---- the IFT watershed's cost map, level by level, on bit planes (ivx_dev_ws_cost_levels) ------------------------------
// C(p) = min over paths from a marker of the largest arc |I(a) - I(b)| on the path.  {C <= c} is the set the markers reach
// through arcs of weight <= c: a flood on bit planes with arc planes instead of a candidate plane, and {C == c} is what
// level c adds to level c - 1.  The chaotic relaxation of the cost map (k_ws_relax) spends its time on the levels where the
// bulk of a noise volume connects (percolation: long winding paths, every tile revisited ~15 times with 16-bit costs in
// LDS); here those levels cost bit-parallel tile visits (64 voxels per lane and operation).  The caller stops after the
// bulk is in and hands the rest -- isolated pockets whose cost is decided by their own few arcs -- to the relaxation,
// which starts from exact costs and has nothing left to correct.
namespace {
template <typename MT>
__global__ __launch_bounds__(256) void k_wsa_seed(const MT *__restrict__ mk, int64_t n, unsigned long long *__restrict__ R) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long b = __ballot(p < n && mk[p] != 0);
    if ((threadIdx.x & 63) == 0 && p < n) R[p >> 6] = b;
}

// Arc weights once, as bytes: wx / wy / wz[p] = min(|I(p) - I(p + 1 / W / HW)|, 127), 127 also when the neighbour's linear
// index is >= n (levels stop far below 127: the caller caps them at 120).  Lane = 8 voxels; the ALU-heavy part of the arc
// planes (field extraction, absolute differences) then happens once instead of once per level.
__global__ __launch_bounds__(256) void k_wsa_weights(const uint16_t *__restrict__ I, int64_t n, int64_t W, int64_t HW,
                                                     unsigned long long *__restrict__ wts) {
    const int64_t nch = n >> 3;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nch; i += stride) {
        const int64_t p0 = i << 3;
        const bool hy = p0 + W < n, hz = p0 + HW < n;
        const uint4 v = *reinterpret_cast<const uint4 *>(I + p0);
        const uint4 vy = *reinterpret_cast<const uint4 *>(I + (hy ? p0 + W : p0));
        const uint4 vz = *reinterpret_cast<const uint4 *>(I + (hz ? p0 + HW : p0));
        const int next = p0 + 8 < n ? (int)I[p0 + 8] : -1000000;
        const unsigned int vw[4] = {v.x, v.y, v.z, v.w}, yw[4] = {vy.x, vy.y, vy.z, vy.w}, zw[4] = {vz.x, vz.y, vz.z, vz.w};
        unsigned long long bx = 0, by = 0, bz = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int iv = (int)((vw[e >> 1] >> (16 * (e & 1))) & 0xffffu);
            const int nx = e < 7 ? (int)((vw[(e + 1) >> 1] >> (16 * ((e + 1) & 1))) & 0xffffu) : next;
            const int ny = (int)((yw[e >> 1] >> (16 * (e & 1))) & 0xffffu), nz = (int)((zw[e >> 1] >> (16 * (e & 1))) & 0xffffu);
            const int dx = min(abs(iv - nx), 127), dy = hy ? min(abs(iv - ny), 127) : 127, dz = hz ? min(abs(iv - nz), 127) : 127;
            bx |= (unsigned long long)dx << (8 * e);
            by |= (unsigned long long)dy << (8 * e);
            bz |= (unsigned long long)dz << (8 * e);
        }
        wts[i] = bx;
        wts[nch + i] = by;
        wts[2 * nch + i] = bz;
    }
}

// the arc planes of level c from the weight bytes: lane = word = 8 x 8 bytes per direction; "byte <= c" for eight bytes at
// once: (x | 0x80) - (c + 1) keeps bit 7 exactly when x >= c + 1 (x, c < 128: no borrow between bytes), and the eight
// sign bits are gathered with one multiply
__device__ __forceinline__ unsigned long long le8(unsigned long long x, unsigned long long c1) {
    const unsigned long long t = (x | 0x8080808080808080ull) - c1;
    return ((~t & 0x8080808080808080ull) * 0x0002040810204081ull) >> 56;
}
// The arc planes of L consecutive levels c .. c + L - 1 in one pass over the weight bytes (level l's three planes at
// E + l * 3 * nwords): the weights are 3 bytes per voxel, a level's planes 3 bits -- one pass per level read 400 MB to write 48
// (84 us x 15 levels at 512^3, 0.67 ms x 12 at 1024^3).
template <int L>
__global__ __launch_bounds__(256) void k_wsa_planes(const unsigned long long *__restrict__ wts, int64_t nwords, int c,
                                                    unsigned long long *__restrict__ E) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    const int64_t nch = nwords * 8;
    unsigned long long c1[L];
#pragma unroll
    for (int l = 0; l < L; l++) c1[l] = (unsigned long long)(c + l + 1) * 0x0101010101010101ull;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(wts + d * nch + w * 8);
        unsigned long long m[L];
#pragma unroll
        for (int l = 0; l < L; l++) m[l] = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const ulonglong2 x = src[q];
#pragma unroll
            for (int l = 0; l < L; l++) {
                m[l] |= le8(x.x, c1[l]) << (16 * q);
                m[l] |= le8(x.y, c1[l]) << (16 * q + 8);
            }
        }
#pragma unroll
        for (int l = 0; l < L; l++) E[((int64_t)l * 3 + d) * nwords + w] = m[l];
    }
}

// lane = word: would ONE relaxation step add a bit to this word?  Then its tile starts the level's flood.
__global__ __launch_bounds__(256) void k_wsa_frontier(Tiles t, const unsigned long long *__restrict__ R,
                                                      const unsigned long long *__restrict__ E, uint8_t *__restrict__ dirty) {
    const int64_t nwords = t.dz * t.dy * t.wx, hwx = t.dy * t.wx;
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    const unsigned long long *Ex = E, *Ey = E + nwords, *Ez = E + 2 * nwords;
    const unsigned long long r = R[w];
    if (r == ~0ull) return;
    const unsigned long long exp = Ex[w];
    unsigned long long nr = r;
    if (w > 0) nr |= (R[w - 1] & Ex[w - 1]) >> 63;
    if (w + 1 < nwords) nr |= ((R[w + 1] & 1ull) & (exp >> 63)) << 63;
    if (w - t.wx >= 0) nr |= R[w - t.wx] & Ey[w - t.wx];
    if (w + t.wx < nwords) nr |= R[w + t.wx] & Ey[w];
    if (w - hwx >= 0) nr |= R[w - hwx] & Ez[w - hwx];
    if (w + hwx < nwords) nr |= R[w + hwx] & Ez[w];
    nr |= ((nr & exp) << 1) | ((nr & (exp << 1)) >> 1); // one step along x inside the word is enough to see a gain
    if (nr != r) {
        const int64_t row = w / t.wx, txi = w - row * t.wx, z = row / t.dy, y = row - z * t.dy;
        dirty[((z / TZ) * t.nty + (y >> TY_LOG)) * t.wx + txi] = 1;
    }
}

// reached voxels so far (grid-stride, one atomic per workgroup)
__global__ __launch_bounds__(256) void k_wsa_count(const unsigned long long *__restrict__ R, int64_t nwords,
                                                   unsigned long long *__restrict__ count) {
    __shared__ unsigned long long s_part[4];
    unsigned long long mine = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += stride) mine += (unsigned long long)__popcll(R[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        if (t) atomicAdd(count, t);
    }
}

// After the last level: snap[l] = the reached plane as level l left it (planes nested: a bit set at level l is set at every
// later one).  C[p] = the first level that has p; voxels no level reached keep their cost.  Lane = 16 voxels.
__global__ __launch_bounds__(256) void k_wsa_costs(const uint16_t *__restrict__ snap, int64_t nchunks, int64_t plane_chunks, int levels,
                                                   uint16_t *__restrict__ C) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nchunks; i += stride) {
        const unsigned int last = snap[(int64_t)(levels - 1) * plane_chunks + i];
        if (!last) continue;
        uint16_t *dst = C + i * 16;
        unsigned int lev[16];
#pragma unroll
        for (int e = 0; e < 16; e++) lev[e] = 0xffffu;
        unsigned int have = 0;
        for (int l = 0; l < levels && have != last; l++) {
            const unsigned int m = snap[(int64_t)l * plane_chunks + i];
            unsigned int nw = m & ~have;
            have |= m;
#pragma unroll
            for (int e = 0; e < 16; e++)
                if (nw >> e & 1u) lev[e] = (unsigned int)l;
        }
        if (last == 0xffffu) {
            reinterpret_cast<uint4 *>(dst)[0] = make_uint4(lev[0] | lev[1] << 16, lev[2] | lev[3] << 16, lev[4] | lev[5] << 16, lev[6] | lev[7] << 16);
            reinterpret_cast<uint4 *>(dst)[1] = make_uint4(lev[8] | lev[9] << 16, lev[10] | lev[11] << 16, lev[12] | lev[13] << 16, lev[14] | lev[15] << 16);
        } else {
#pragma unroll
            for (int e = 0; e < 16; e++)
                if (last >> e & 1u) dst[e] = (uint16_t)lev[e];
        }
    }
}

// ---- the scikit-image branch's cost map, level by level (ivx_dev_sk_cost_levels) ---------------------------------------
// There a path costs the largest image VALUE on it (markers cost their own value), so {C <= c} is what the markers of value
// <= c reach inside the candidate plane {I <= c}: the ordinary region-growing engine, coarse pass included.  The gradient
// of a windowed image is zero over everything the window saturates: level 0 alone is ~95 % of such a volume, one flood.
// Eight lanes' bytes of bits -> one word in the first of them (lane & 7 == 0): three exchanges.
__device__ __forceinline__ unsigned long long gather_word8(uint32_t bits8, int lane) {
    unsigned long long w = (unsigned long long)bits8 << (8 * (lane & 7));
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)w, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(w >> 32), o, 64);
        w |= ((unsigned long long)hi << 32) | lo;
    }
    return w;
}
// The markers as a bit plane, once per call (lane = 8 voxels: one 16-byte load of int16 markers): a level's seeds are then
// marker & candidate & ~reached per WORD.  (Rounds 1 - 5 read the marker volume voxel by voxel at every level: 170 us x 3 at
// 512^3, 1.35 ms x 3 at 1024^3.)
template <typename MT>
__global__ __launch_bounds__(256) void k_ska_marker_bits(const MT *__restrict__ mk, int64_t n8, unsigned long long *__restrict__ mb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; // (n8 is a multiple of 8: whole words, whole groups of eight lanes)
    uint32_t bits = 0;
    if (i < n8) {
        MT v[8];
        if (sizeof(MT) == 2) *reinterpret_cast<uint4 *>(v) = reinterpret_cast<const uint4 *>(mk)[i];
        else *reinterpret_cast<uint2 *>(v) = reinterpret_cast<const uint2 *>(mk)[i];
#pragma unroll
        for (int e = 0; e < 8; e++) bits |= (v[e] != 0 ? 1u : 0u) << e;
    }
    const unsigned long long w = gather_word8(bits, threadIdx.x & 63);
    if ((threadIdx.x & 7) == 0 && i < n8) mb[i >> 3] = w;
}
// ... and the candidate planes {I <= l} of the first L levels in one pass over the image (L <= 4)
template <int L>
__global__ __launch_bounds__(256) void k_ska_cands(const uint16_t *__restrict__ I, int64_t n8, int64_t nwords, unsigned long long *__restrict__ cand) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t bits[L];
#pragma unroll
    for (int l = 0; l < L; l++) bits[l] = 0;
    if (i < n8) {
        uint16_t v[8];
        *reinterpret_cast<uint4 *>(v) = reinterpret_cast<const uint4 *>(I)[i];
#pragma unroll
        for (int e = 0; e < 8; e++)
#pragma unroll
            for (int l = 0; l < L; l++) bits[l] |= (v[e] <= (uint16_t)l ? 1u : 0u) << e;
    }
#pragma unroll
    for (int l = 0; l < L; l++) {
        const unsigned long long w = gather_word8(bits[l], threadIdx.x & 63);
        if ((threadIdx.x & 7) == 0 && i < n8) cand[(int64_t)l * nwords + (i >> 3)] = w;
    }
}
// seeds of level c, lane = word
__global__ __launch_bounds__(256) void k_ska_seed_bits(Tiles t, const unsigned long long *__restrict__ mb, const unsigned long long *__restrict__ cand,
                                                       unsigned long long *__restrict__ R, uint8_t *__restrict__ dirty) {
    const int64_t nwords = t.dz * t.dy * t.wx;
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    const unsigned long long add = mb[w] & cand[w] & ~R[w];
    if (!add) return;
    R[w] |= add;
    const int64_t row = w / t.wx, txi = w - row * t.wx, z = row / t.dy, y = row - z * t.dy;
    mark_tile_nbhd(t, dirty, z / TZ, y / TY, txi);
}

// lane = word: a candidate bit that is not reached and has a reached neighbour under the structure -> its tile (and the
// tiles around it) start the level's flood
__global__ __launch_bounds__(256) void k_ska_frontier(Tiles t, const unsigned long long *__restrict__ cand,
                                                      const unsigned long long *__restrict__ R, uint8_t *__restrict__ dirty) {
    const int64_t nwords = t.dz * t.dy * t.wx;
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    const unsigned long long open = cand[w] & ~R[w];
    if (!open) return;
    const int64_t row = w / t.wx, txi = w - row * t.wx, z = row / t.dy, y = row - z * t.dy;
    unsigned long long nb = 0;
    for (int kk = 0; kk < 3; kk++)
        for (int jj = 0; jj < 3; jj++) {
            const uint32_t m3 = (t.strct >> (kk * 9 + jj * 3)) & 7u;
            if (!m3) continue;
            // voxel q reached => q + (kk-1, jj-1, ii-1) reached: the source row of this word is (z - (kk-1), y - (jj-1))
            const int64_t zs = z - (kk - 1), ys = y - (jj - 1);
            if (zs < 0 || zs >= t.dz || ys < 0 || ys >= t.dy) continue;
            const unsigned long long *rr = R + (zs * t.dy + ys) * t.wx;
            const unsigned long long c0 = rr[txi];
            const unsigned long long cl = txi > 0 ? rr[txi - 1] >> 63 : 0ull, cr = txi + 1 < t.wx ? rr[txi + 1] & 1ull : 0ull;
            if (m3 & 2u) nb |= c0;
            if (m3 & 4u) nb |= (c0 << 1) | cl;        // ii = 2: source bit x - 1
            if (m3 & 1u) nb |= (c0 >> 1) | (cr << 63); // ii = 0: source bit x + 1
        }
    if (nb & open) mark_tile_nbhd(t, dirty, z / TZ, y / TY, txi);
}

// ---- what both cost maps do with a level's flood -----------------------------------------------------------------------
// the end of a level: keep the reached plane as this level left it, count its voxels and read the count back
static int end_level(const unsigned long long *R, int64_t nwords, char *snap, unsigned long long *d_count, hipStream_t st,
                     int64_t *reached) {
    const unsigned gw = (unsigned)ivx::cdiv(nwords, 256);
    IVX_HIP(hipMemcpyAsync(snap, R, (size_t)nwords * 8, hipMemcpyDeviceToDevice, st));
    IVX_HIP(hipMemsetAsync(d_count, 0, 8, st));
    hipLaunchKernelGGL(k_wsa_count, dim3(gw < 1024 ? gw : 1024), dim3(256), 0, st, R, nwords, d_count);
    IVX_LAUNCH_CHECK();
    uint32_t seq, got[2] = {0, 0};
    int rc;
    if ((rc = ivx::mailbox_publish(d_count, 2, st, &seq))) return rc;
    if ((rc = ivx::mailbox_wait(seq, st, got, 2))) return rc;
    *reached = (int64_t)(((uint64_t)got[1] << 32) | got[0]);
    return IVX_OK;
}
// the end of the call: the snapshots of the `levels` completed levels -> C, and the three results
static int end_call(const char *snaps, int64_t n, int levels, uint16_t *C, int64_t reached, int64_t rounds, int *levels_done,
                    int64_t *reached_out, int64_t *rounds_out, hipStream_t st) {
    const int64_t nchunks = n / 16, blocks = ivx::cdiv(nchunks, 256);
    hipLaunchKernelGGL(k_wsa_costs, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, (const uint16_t *)snaps,
                       nchunks, nchunks, levels, C); // (a plane is n / 64 words = n / 16 chunks)
    IVX_LAUNCH_CHECK();
    if (levels_done) *levels_done = levels;
    if (reached_out) *reached_out = reached;
    if (rounds_out) *rounds_out = rounds;
    return IVX_OK;
}
} // namespace

// Levels 0, 1, 2, ... of the IFT cost map until `stop_frac` of the voxels are in (or `max_levels` are done): C[p] = level for
// every voxel reached (the others keep what the caller put there: 0xFFFF), *levels_done = number of levels completed,
// *reached_out = voxels with a final cost.  6-neighbour structure, scipy's linear-index neighbourhood; needs dx % 64 == 0
// and dy % 16 == 0 (IVX_EINVAL otherwise: the caller then runs its relaxation from the markers alone).
extern "C" int ivx_dev_ws_cost_levels(const uint16_t *I, int mdtype, const void *markers, int64_t dz, int64_t dy, int64_t dx,
                                      uint16_t *C, int max_levels, double stop_frac, int *levels_done, int64_t *reached_out,
                                      int64_t *rounds_out, void *stream) {
    IVX_REQUIRE(I && markers && C && dz > 0 && dy > 0 && dx > 0, IVX_EINVAL, "ws_cost_levels: bad arguments");
    IVX_REQUIRE(dx % 64 == 0 && dy % TY == 0, IVX_EINVAL, "ws_cost_levels: needs dx %% 64 == 0 and dy %% 16 == 0");
    IVX_REQUIRE(mdtype == IVX_I16 || mdtype == IVX_I8, IVX_EINVAL, "ws_cost_levels: markers must be int16 or int8");
    ivx_flood_plan plan;
    plan.dz = dz; plan.dy = dy; plan.dx = dx; plan.wx = dx / 64;
    plan.strct_bits = (1u << 4) | (1u << 10) | (1u << 12) | (1u << 13) | (1u << 14) | (1u << 16) | (1u << 22);
    Tiles t;
    int rc = make_tiles(&plan, &t);
    if (rc) return rc;
    hipStream_t st = ivx::S(stream);
    const int64_t n = dz * dy * dx, nwords = n >> 6;
    const FScratch fs = make_fscratch(t);
    IVX_REQUIRE(max_levels >= 1, IVX_EINVAL, "ws_cost_levels: max_levels");
    if (max_levels > 120) max_levels = 120; // (the weight bytes saturate at 127)
    // workspace: R | arc planes Ex Ey Ez | weight bytes x y z | flood scratch | one snapshot of R per level
    constexpr int PL = 4; // levels whose arc planes are made by one pass over the weights
    const size_t pw = (size_t)nwords * 8, o_E = al256(pw), o_W = al256(o_E + (size_t)PL * 3 * pw), o_S = al256(o_W + 3 * (size_t)n);
    const size_t o_P = al256(o_S + fs.total);
    void *mem;
    if ((rc = ivx::ws_get_s(ivx::WS_WSA, st, o_P + (size_t)max_levels * pw + 256, &mem))) return rc;
    unsigned long long *R = (unsigned long long *)mem;
    unsigned long long *E_all = (unsigned long long *)((char *)mem + o_E); // PL levels x (Ex | Ey | Ez), nwords each
    unsigned long long *wts = (unsigned long long *)((char *)mem + o_W); // n bytes per direction
    char *scr = (char *)mem + o_S;
    char *snaps = (char *)mem + o_P;
    unsigned long long *d_count = (unsigned long long *)(scr + fs.off_status) + 2;
    IVX_HIP(hipMemsetAsync(scr, 0, fs.off_seeds, st)); // dirty flags, counters
    const unsigned gv = (unsigned)ivx::cdiv(n, 256), gw = (unsigned)ivx::cdiv(nwords, 256);
    if (mdtype == IVX_I16) hipLaunchKernelGGL(k_wsa_seed<int16_t>, dim3(gv), dim3(256), 0, st, (const int16_t *)markers, n, R);
    else hipLaunchKernelGGL(k_wsa_seed<int8_t>, dim3(gv), dim3(256), 0, st, (const int8_t *)markers, n, R);
    IVX_LAUNCH_CHECK();
    {
        const int64_t blocks = ivx::cdiv(n >> 3, 256);
        hipLaunchKernelGGL(k_wsa_weights, dim3((unsigned)(blocks < 32768 ? blocks : 32768)), dim3(256), 0, st, I, n, dx, dy * dx, wts);
        IVX_LAUNCH_CHECK();
    }
    int64_t rounds_total = 0, reached = 0;
    int c = 0;
    for (; c < max_levels; c++) {
        if (c % PL == 0) { // (weights above 127 saturate: levels beyond max_levels <= 120 are never asked for, their planes cost nothing extra)
            hipLaunchKernelGGL(k_wsa_planes<PL>, dim3(gw), dim3(256), 0, st, wts, nwords, c, E_all);
            IVX_LAUNCH_CHECK();
        }
        unsigned long long *E = E_all + (size_t)(c % PL) * 3 * nwords;
        hipLaunchKernelGGL(k_wsa_frontier, dim3(gw), dim3(256), 0, st, t, R, E, (uint8_t *)(scr + fs.off_dirty0));
        IVX_LAUNCH_CHECK();
        int rounds = 0;
        if ((rc = ivx::flood_run(&plan, (const uint64_t *)E, ivx::FLOOD_LINEAR, (uint64_t *)R, scr, &rounds, stream))) return rc;
        rounds_total += rounds;
        if ((rc = end_level(R, nwords, snaps + (size_t)c * pw, d_count, st, &reached))) return rc;
        if ((double)reached >= stop_frac * (double)n) {
            c++;
            break;
        }
    }
    return end_call(snaps, n, c, C, reached, rounds_total, levels_done, reached_out, rounds_out, st);
}

// Levels 0, 1, 2, ... of scikit-image's cost map (value-on-path minimax, lattice neighbours, any symmetric 3x3x3 structure)
// until `stop_frac` of the voxels are in or `max_levels` are done; C[p] = level for every voxel reached.  Needs dx % 64 == 0,
// 16-byte aligned image and markers.
extern "C" int ivx_dev_sk_cost_levels(const uint16_t *I, int mdtype, const void *markers, int64_t dz, int64_t dy, int64_t dx,
                                      const uint8_t strct[27], uint16_t *C, int max_levels, double stop_frac, int *levels_done,
                                      int64_t *reached_out, int64_t *rounds_out, void *stream) {
    IVX_REQUIRE(I && markers && C && strct && dz > 0 && dy > 0 && dx > 0, IVX_EINVAL, "sk_cost_levels: bad arguments");
    IVX_REQUIRE(dx % 64 == 0, IVX_EINVAL, "sk_cost_levels: needs dx %% 64 == 0");
    IVX_REQUIRE(mdtype == IVX_I16 || mdtype == IVX_I8, IVX_EINVAL, "sk_cost_levels: markers must be int16 or int8");
    IVX_REQUIRE(max_levels >= 1, IVX_EINVAL, "sk_cost_levels: max_levels");
    IVX_REQUIRE((((uintptr_t)I | (uintptr_t)markers) & 15) == 0, IVX_EINVAL, "sk_cost_levels: image and markers must be 16-byte aligned");
    ivx_flood_plan plan;
    plan.dz = dz; plan.dy = dy; plan.dx = dx; plan.wx = dx / 64;
    const int64_t s3[3] = {3, 3, 3};
    int rc = ivx_flood_strct_bits(strct, s3, &plan.strct_bits);
    if (rc) return rc;
    Tiles t;
    if ((rc = make_tiles(&plan, &t))) return rc;
    hipStream_t st = ivx::S(stream);
    const int64_t n = dz * dy * dx, nwords = n >> 6;
    const FScratch fs = make_fscratch(t);
    // workspace: R | candidate planes (the first `ahead` levels' made in one pass, then one at a time) | marker plane | flood scratch | snapshots
    const int ahead = max_levels < 4 ? max_levels : 4;
    const size_t pw = (size_t)nwords * 8, o_C = al256(pw), o_M = al256(o_C + (size_t)ahead * pw), o_S = al256(o_M + pw), o_P = al256(o_S + fs.total);
    void *mem;
    if ((rc = ivx::ws_get_s(ivx::WS_WSA, st, o_P + (size_t)max_levels * pw + 256, &mem))) return rc;
    unsigned long long *R = (unsigned long long *)mem, *cand0 = (unsigned long long *)((char *)mem + o_C);
    unsigned long long *mb = (unsigned long long *)((char *)mem + o_M);
    char *scr = (char *)mem + o_S, *snaps = (char *)mem + o_P;
    unsigned long long *d_count = (unsigned long long *)(scr + fs.off_status) + 2;
    if ((rc = ivx_dev_flood_clear(&plan, (uint64_t *)R, scr, stream))) return rc;
    const unsigned gw = (unsigned)ivx::cdiv(nwords, 256);
    uint8_t *dirty = (uint8_t *)(scr + fs.off_dirty0);
    int64_t rounds_total = 0, reached = 0;
    {
        const int64_t n8 = n >> 3;
        const unsigned g8 = (unsigned)ivx::cdiv(n8, 256);
        if (mdtype == IVX_I16) hipLaunchKernelGGL(k_ska_marker_bits<int16_t>, dim3(g8), dim3(256), 0, st, (const int16_t *)markers, n8, mb);
        else hipLaunchKernelGGL(k_ska_marker_bits<int8_t>, dim3(g8), dim3(256), 0, st, (const int8_t *)markers, n8, mb);
        IVX_LAUNCH_CHECK();
        switch (ahead) {
        case 1: hipLaunchKernelGGL(k_ska_cands<1>, dim3(g8), dim3(256), 0, st, I, n8, nwords, cand0); break;
        case 2: hipLaunchKernelGGL(k_ska_cands<2>, dim3(g8), dim3(256), 0, st, I, n8, nwords, cand0); break;
        case 3: hipLaunchKernelGGL(k_ska_cands<3>, dim3(g8), dim3(256), 0, st, I, n8, nwords, cand0); break;
        default: hipLaunchKernelGGL(k_ska_cands<4>, dim3(g8), dim3(256), 0, st, I, n8, nwords, cand0); break;
        }
        IVX_LAUNCH_CHECK();
    }
    int c = 0;
    for (; c < max_levels; c++) {
        unsigned long long *cand = c < ahead ? cand0 + (size_t)c * nwords : cand0;
        if (c >= ahead && (rc = ivx_dev_flood_candidates(&plan, IVX_U16, I, 0.0, (double)c, nullptr, 0, 0.0, (uint64_t *)cand, stream))) return rc;
        if (c > 0) {
            // "closed" tiles were closed for the previous level's candidate plane: this one has more candidates
            IVX_HIP(hipMemsetAsync(scr + fs.off_dirty0, 0, fs.off_cnt - fs.off_dirty0, st));
            hipLaunchKernelGGL(k_ska_frontier, dim3(gw), dim3(256), 0, st, t, cand, R, dirty);
            IVX_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_ska_seed_bits, dim3(gw), dim3(256), 0, st, t, mb, cand, R, dirty);
        IVX_LAUNCH_CHECK();
        ivx::ccl_invalidate(scr);
        int rounds = 0;
        if ((rc = ivx::flood_run(&plan, (const uint64_t *)cand, ivx::FLOOD_SYMMETRIC, (uint64_t *)R, scr, &rounds, stream))) return rc;
        rounds_total += rounds;
        if ((rc = end_level(R, nwords, snaps + (size_t)c * pw, d_count, st, &reached))) return rc;
        // enough is in -- or level 0 shows that this image has no plateau to speak of (a raw gradient: the bulk connects
        // dozens of levels up, and walking there level by level costs more than the relaxation it would save)
        if ((double)reached >= stop_frac * (double)n || (c == 0 && (double)reached < 0.05 * (double)n)) {
            c++;
            break;
        }
    }
    return end_call(snaps, n, c, C, reached, rounds_total, levels_done, reached_out, rounds_out, st);
}
