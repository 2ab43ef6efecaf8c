// k_flood.hip -- seeded region growing (connected threshold flood) on bit planes.
//
// Reference semantics (bit-exact):
//   generic_floodfill_threshold          invesalius_rs/src/floodfill.rs:96-166
//   generic_floodfill_threshold_inplace  invesalius_rs/src/floodfill.rs:168-237
//   floodfill_internal                   invesalius_rs/src/floodfill.rs:5-49       (data == v, forced seed: ivx_floodfill)
//   floodfill_auto_threshold             invesalius_rs/src/floodfill_py.rs:12-85   (directed: edge planes, tile_update_dir)
// The reference walks a LIFO stack; the set it fills does not depend on the visiting order:
//   filled = connected component (under `strct`) of the in-range seeds inside
//            C = { v : t0 <= data[v] <= t1  and  barrier[v] != fill }   (+ the in-range seeds themselves),
// so a parallel fix-point gives the same bytes.
//
// MI355X design (memory-bound, no MFMA):
//   k_flood_candidates16  ONE streaming pass over data (+ barrier): 2 B + 1 B read per voxel, 1 bit written (lane = 16
//                       voxels).  C is 1 bit/voxel (64 voxels of an x-row per uint64): 16 MiB at 512^3, i.e. it lives
//                       in L2 / Infinity Cache for the whole flood.
//   k_flood_round_list  one workgroup per DIRTY tile of 64(x) x 16(y) x 16(z) voxels = 256 words, one lane per word,
//                       tiles taken from a compact per-round list.  The reached bits of the tile plus a one-row halo
//                       are staged in LDS together with their x-dilated twins (tile_update) and iterated to the
//                       tile-local fix-point:
//                         - 26/18/6-neighbour gather = OR of <= 9 LDS words, a compile-time pattern for the three
//                           standard structures so the reads issue back to back,
//                         - propagation ALONG x inside a word is closed in O(1) with the carry trick
//                           ((C + R) ^ C) & C  (and its bit-reversed twin), i.e. a 64-voxel run fills in one step,
//                         - one s_barrier per iteration (wave ballot + LDS flag vote).
//                       A visit enlists the neighbour tiles that hold an unreached candidate next to one of its new
//                       bits (tile_update; byte flags de-duplicate); every round reports its list length to a pinned
//                       progress line as it starts and the host keeps a few rounds queued ahead of the newest one it has seen.  Global
//                       rounds are bounded by the number of TILES on the longest path, not voxels; past 48 rounds the
//                       union-find engine (k_ccl.hip) takes over.
//   k_flood_coarse      before the rounds: tiles that are ALL candidate are flooded as units on the tile graph (one
//                       workgroup, rows of tile bits), so the solid interior of a region costs no rounds at all.
//   k_flood_apply(2)    reached bits -> out[v] = fill (only words with reached bits touch memory).
#include <math.h>
#include <map>
#include <mutex>
#include <stdlib.h>

#include "flood_tiles.h"
#include "levels_write.h"
#include "words_from_records.h" // short8_t, words_from_records

using ivx::ApplyWhen;

namespace {

constexpr int NT = TY * TZ;           // lanes per tile workgroup (one per word)
constexpr int HY = TY + 2, HZ = TZ + 2;
constexpr int BATCH = 8;              // most rounds the host may keep queued ahead (the counter ring has 2 * BATCH entries)
constexpr int SUB = 1;                // gather/update steps per termination vote (measured: 4 doubles the tile time)
// dirty-byte bits: bit 0 = "on (or to be put on) a round's list"; CLOSED = every candidate of the tile is reached, so no
// news can ever change it again (sticky for the rest of the flood; the byte is then never 0 and the enlisting atomicOr of a
// neighbour finds it "already marked": closed tiles cost no visits -- in the model of tools/sim_flood.py 147 of the 1 313
// tiles that the first round's visits wake on the bench volume, a ninth; the "about a third" this comment used to give does
// not hold for the rule before this one either: 147 of 1 952); ENLISTED (coarse pass) further down
constexpr unsigned int CLOSED = 0x40u;
// (Tried in round 3: the round's list as 8 sublists with a counter each on its own 128-byte line.  ~10^3 appends that arrive
// together serialise on one counter at 5 - 10 ns each -- tools/micro/atomic_tail.hip: 1 024 workgroups x 1 append cost 5.5 us
// more than none, x 4 appends 40 us more, spread over 8 counters 0.3 / 1.3 us -- but the rounds' appends do not arrive
// together: region growing 0.192 -> 0.195 ms, the IFT cost levels 13.8 -> 14.3 ms.  Dropped.)

template <typename T> __device__ __forceinline__ double as_double(T v) { return (double)v; }

// ---- candidates: one lane per output byte (8 voxels) ------------------------------------------------
// BAR: 0 none, 1 uint8 barrier array (out != fill), 2 in-place (data value != fill)
// fast path: int16/uint16 data, dx % 16 == 0, 16-B aligned pointers: one lane = 16 voxels (2 x 16-B data loads,
// one 16-B barrier load, one 2-B store), the same access shape as the threshold kernel
template <typename T, int BAR>
__global__ __launch_bounds__(256) void k_flood_candidates16(const short8_t *__restrict__ data,
                                                            const uint4 *__restrict__ bar, int64_t nchunks, double t0,
                                                            double t1, double fill, uint16_t *__restrict__ cand) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int lo = (int)ceil(t0 < -70000.0 ? -70000.0 : t0), hi = (int)floor(t1 > 70000.0 ? 70000.0 : t1); // integer data
    const unsigned fb = (unsigned)(uint8_t)fill;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nchunks; c += stride) {
        const short8_t a = __builtin_nontemporal_load(&data[2 * c]);
        const short8_t b = __builtin_nontemporal_load(&data[2 * c + 1]);
        uint4 q = make_uint4(0, 0, 0, 0);
        if (BAR == 1) q = bar[c];
        const unsigned bw[4] = {q.x, q.y, q.z, q.w};
        unsigned m = 0;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int v = (int)(T)(e < 8 ? a[e & 7] : b[e & 7]);
            bool ok = v >= lo && v <= hi;
            if (BAR == 1) ok = ok && ((bw[e >> 2] >> (8 * (e & 3))) & 0xffu) != fb;
            if (BAR == 2) ok = ok && (double)v != fill;
            m |= ok ? (1u << e) : 0u;
        }
        cand[c] = (uint16_t)m;
    }
}

// int16 data with valid per-word (min, max) records (k_threshold.hip).  Without a barrier the candidates are the threshold's
// plane: one word per lane, words_from_records.h.
__global__ __launch_bounds__(256) void k_flood_candidates_words(const short8_t *__restrict__ data, const unsigned *__restrict__ ranges,
                                                                int64_t nwords, double t0, double t1,
                                                                unsigned long long *__restrict__ cand) {
    const int lo = (int)ceil(t0 < -70000.0 ? -70000.0 : t0), hi = (int)floor(t1 > 70000.0 ? 70000.0 : t1); // integer data
    words_from_records(data, ranges, nwords, lo, hi, cand);
}

// With a uint8 barrier (out != fill): lane = 16 voxels as in k_flood_candidates16, every lane reads its word's record first.
// Wholly outside [lo, hi]: 0, nothing loaded.  Wholly inside: the image is skipped, the barrier alone decides.  Mixed: the
// arithmetic above.  The next trip's record is loaded ahead in the source only: the compiler waits for it at the loop's head.
__global__ __launch_bounds__(256) void k_flood_candidates16_ranges(const short8_t *__restrict__ data,
                                                                   const uint4 *__restrict__ bar,
                                                                   const unsigned *__restrict__ ranges, int64_t nchunks,
                                                                   double t0, double t1, double fill,
                                                                   uint16_t *__restrict__ cand) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int lo = (int)ceil(t0 < -70000.0 ? -70000.0 : t0), hi = (int)floor(t1 > 70000.0 ? 70000.0 : t1); // integer data
    const unsigned fb = (unsigned)(uint8_t)fill;
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    unsigned rec = ranges[c >> 2];
    for (;;) {
        const int64_t cn = c + stride;
        unsigned rec_next = 0;
        if (cn < nchunks) rec_next = ranges[cn >> 2];
        const int mn = (int)(short)(rec & 0xffffu), mx = (int)(short)(rec >> 16);
        unsigned m = 0;
        if (!(mx < lo || mn > hi)) {
            const bool inside = mn >= lo && mx <= hi;
            if (inside) {
                m = 0xffffu;
            } else {
                const short8_t a = __builtin_nontemporal_load(&data[2 * c]);
                const short8_t b = __builtin_nontemporal_load(&data[2 * c + 1]);
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const int v = (int)(e < 8 ? a[e & 7] : b[e & 7]);
                    m |= (v >= lo && v <= hi) ? (1u << e) : 0u;
                }
            }
            if (m) {
                const uint4 q = bar[c];
                const unsigned bw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int e = 0; e < 16; e++)
                    if (((bw[e >> 2] >> (8 * (e & 3))) & 0xffu) == fb) m &= ~(1u << e);
            }
        }
        cand[c] = (uint16_t)m;
        if (cn >= nchunks) break;
        c = cn;
        rec = rec_next;
    }
}

template <typename T, int BAR>
__global__ __launch_bounds__(256) void k_flood_candidates(const T *__restrict__ data, const uint8_t *__restrict__ bar,
                                                          Tiles t, double t0, double t1, double fill,
                                                          uint8_t *__restrict__ cand) {
    const int64_t bpr = t.wx * 8; // bytes per bit-row
    const int64_t total = t.dz * t.dy * bpr;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const bool vec = (sizeof(T) == 2) && (t.dx % 8 == 0) && (((uintptr_t)data & 15) == 0) &&
                     (BAR != 1 || ((uintptr_t)bar & 7) == 0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t row = i / bpr, q = i - row * bpr;
        const int64_t x0 = q * 8;
        unsigned m = 0;
        if (x0 < t.dx) {
            const int64_t base = row * t.dx + x0;
            if (vec) { // x0+8 <= dx because dx % 8 == 0
                const short8_t v = *reinterpret_cast<const short8_t *>(data + base);
                unsigned long long b8 = 0;
                if (BAR == 1) b8 = *reinterpret_cast<const unsigned long long *>(bar + base);
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const double d = (double)(T)v[e];
                    bool ok = d >= t0 && d <= t1;
                    if (BAR == 1) ok = ok && (((b8 >> (8 * e)) & 0xff) != (unsigned long long)(uint8_t)fill);
                    if (BAR == 2) ok = ok && d != fill;
                    m |= ok ? (1u << e) : 0u;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    if (x0 + e < t.dx) {
                        const double d = as_double(data[base + e]);
                        bool ok = d >= t0 && d <= t1;
                        if (BAR == 1) ok = ok && bar[base + e] != (uint8_t)fill;
                        if (BAR == 2) ok = ok && d != fill;
                        m |= ok ? (1u << e) : 0u;
                    }
                }
            }
        }
        cand[i] = (uint8_t)m;
    }
}

// ---- seeds (they wake tiles with mark_tile_nbhd, flood_tiles.h) ---------------------------------------------------
template <typename T>
__global__ void k_flood_seed(const T *__restrict__ data, Tiles t, double t0, double t1, const int64_t *__restrict__ seeds,
                             int64_t nseeds, unsigned long long *__restrict__ cand,
                             unsigned long long *__restrict__ reached, uint8_t *__restrict__ dirty) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= nseeds) return;
    const int64_t x = seeds[3 * n], y = seeds[3 * n + 1], z = seeds[3 * n + 2];
    const double v = as_double(data[(z * t.dy + y) * t.dx + x]);
    if (!(v >= t0 && v <= t1)) return; // floodfill.rs:123: only in-range seeds start a flood
    const int64_t w = (z * t.dy + y) * t.wx + (x >> 6);
    const unsigned long long bit = 1ull << (x & 63);
    atomicOr(&cand[w], bit); // a seed expands even when its barrier byte already equals `fill`
    atomicOr(&reached[w], bit);
    mark_tile_nbhd(t, dirty, z / TZ, y / TY, x >> 6);
}

struct SeedPack {
    int64_t xyz[16][3];
    int n;
};
template <typename T>
__global__ void k_flood_seed_args(const T *__restrict__ data, Tiles t, double t0, double t1, SeedPack sp,
                                  unsigned long long *__restrict__ cand, unsigned long long *__restrict__ reached,
                                  uint8_t *__restrict__ dirty) {
    const int n = threadIdx.x;
    if (n >= sp.n) return;
    const int64_t x = sp.xyz[n][0], y = sp.xyz[n][1], z = sp.xyz[n][2];
    const double v = as_double(data[(z * t.dy + y) * t.dx + x]);
    if (!(v >= t0 && v <= t1)) return;
    const int64_t w = (z * t.dy + y) * t.wx + (x >> 6);
    const unsigned long long bit = 1ull << (x & 63);
    atomicOr(&cand[w], bit);
    atomicOr(&reached[w], bit);
    mark_tile_nbhd(t, dirty, z / TZ, y / TY, x >> 6);
}

// ---- one round over the dirty tiles ---------------------------------------------------------------
__device__ __forceinline__ unsigned long long fill_up(unsigned long long seed, unsigned long long m) {
    return (((m + seed) ^ m) & m) | seed;
}
__device__ __forceinline__ unsigned long long fill_runs(unsigned long long seed, unsigned long long m) {
    unsigned long long f = fill_up(seed, m);
    return __brevll(fill_up(__brevll(f), __brevll(m)));
}

// Tile update of the per-round kernel.
// LDS holds, for the 18x18 rows of the tile + halo: sN = the row's word, sD = the row's word dilated by one voxel
// along x including the carry bits of the x-neighbour words (so a full 3-wide strct row costs ONE LDS read), and the
// two carry bits themselves (generic structuring elements).  The local fix-point is a chaotic relaxation: reached
// bits only ever get OR'ed in, so a lane may read a neighbour's word while it is being rewritten -- any mix of old
// and new bits is a valid intermediate state -- and ONE barrier per iteration (the termination vote) is enough.
// Staging loads and the publish store are plain: a round's visits never share a tile, a neighbour's publish can only add
// bits to a halo row, and the kernel boundary between two rounds orders one round's stores before the next one's loads.
// workgroup barrier that only waits for this wave's LDS traffic (lgkmcnt), NOT for its global stores/atomics in flight:
// __syncthreads() also drains vmcnt, which would park the whole tile behind the publish stores (~2.5 us).
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0), vmcnt/expcnt untouched
    __builtin_amdgcn_s_barrier();
}
// tile_update's wake-up test: per staged row, the candidates of the centre word that were unreached (halo rows outside the
// tile only).  Apart from TileLds: the directed and the linear tile update have no use for it.
struct TileOpen {
    unsigned long long sO[HZ * HY];
};
struct TileLds {
    unsigned long long sN[HZ * HY];
    unsigned long long sD[HZ * HY];
    unsigned char sCL[HZ * HY], sCR[HZ * HY];
    unsigned int dirs;
    unsigned int open; // some candidate of the tile is still unreached after this visit
    unsigned int vote[2]; // workgroup "anything changed" vote, double-buffered: ONE s_barrier per iteration
};
// a visit's direction bits -> L.dirs: OR across the wave in registers, then ONE LDS atomic per wave (256 same-address LDS
// atomics serialise)
__device__ __forceinline__ void post_dirs(TileLds &L, unsigned dirs) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dirs |= __shfl_xor(dirs, o, 64);
    if ((threadIdx.x & 63) == 0 && dirs) atomicOr(&L.dirs, dirs);
}

template <int CONN>
__device__ __forceinline__ void tile_update(const Tiles &t, const unsigned long long *__restrict__ cand,
                                            unsigned long long *reached, int64_t tile, TileLds &L, TileOpen &O) {
    const int64_t txi = tile % t.wx, r1 = tile / t.wx;
    const int64_t tyi = r1 % t.nty, tzi = r1 / t.nty;
    const int64_t z0 = tzi * TZ, y0 = tyi * TY;
    // stage: lane idx <-> halo row idx (324 rows = 2 rows per lane for the first 68 lanes); 3 words per row; all six
    // loads of a lane are issued before any of them is consumed
    // (the candidate words the wake-up test at the end of the visit needs ride along, issued with the other loads before
    // anything is consumed: the centre word of the 68 halo rows outside the tile; the planes sit in L2 / MALL)
    unsigned long long w3[2][3] = {{0ull, 0ull, 0ull}, {0ull, 0ull, 0ull}};
    unsigned long long hc[2] = {0ull, 0ull};
    unsigned int hx[2] = {0u, 0u}; // the row exists (rows past the volume's end wake nobody)
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const int idx = threadIdx.x + pass * NT;
        if (idx < HZ * HY) {
            const int yy = idx % HY, zz = idx / HY;
            const int64_t z = z0 + zz - 1, y = y0 + yy - 1;
            if (z >= 0 && z < t.dz && y >= 0 && y < t.dy) {
                unsigned long long *row = reached + (z * t.dy + y) * t.wx;
#pragma unroll
                for (int xx = 0; xx < 3; xx++) {
                    const int64_t w = txi + xx - 1;
                    if (w >= 0 && w < t.wx) w3[pass][xx] = row[w];
                }
                if (zz == 0 || zz == HZ - 1 || yy == 0 || yy == HY - 1) hc[pass] = cand[(z * t.dy + y) * t.wx + txi];
                hx[pass] = 1u;
            }
        }
    }
    // sCL: bit 0 = the carry bit; bits 1 and 2 (wake-up test) = the voxel left / right of the word was unreached.  sO: the
    // candidates that were unreached in the centre word of a halo row outside the tile (0 for the tile's own rows).
    // Neither is rewritten during the visit.
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const int idx = threadIdx.x + pass * NT;
        if (idx < HZ * HY) {
            const unsigned long long cl = w3[pass][0] >> 63, cr = w3[pass][2] & 1ull, n = w3[pass][1];
            L.sN[idx] = n;
            L.sD[idx] = n | (n << 1) | (n >> 1) | cl | (cr << 63);
            const unsigned int ul = hx[pass] & ~(unsigned int)cl, ur = hx[pass] & ~(unsigned int)cr;
            L.sCL[idx] = (unsigned char)(cl | (ul << 1) | (ur << 2));
            L.sCR[idx] = (unsigned char)cr;
            O.sO[idx] = hc[pass] & ~n;
        }
    }
    const int ty = threadIdx.x & (TY - 1), tz = threadIdx.x >> TY_LOG;
    const int64_t z = z0 + tz, y = y0 + ty;
    const bool inside = z < t.dz && y < t.dy;
    const unsigned long long c = inside ? cand[(z * t.dy + y) * t.wx + txi] : 0ull;
    if (threadIdx.x == 0) L.vote[0] = 0u;
    __syncthreads();
    const int me = (tz + 1) * HY + (ty + 1);
    const unsigned long long r_in = L.sN[me];
    const unsigned long long mycl = L.sCL[me] & 1u, mycr = L.sCR[me];
    unsigned long long r = r_in;
    const uint32_t st = t.strct;
    const bool xrun = (st >> 12 & 1) && (st >> 14 & 1); // both x neighbours of the centre row present
    bool exhausted = true;
    for (int it = 0; it < t.itcap; it++) {
      bool changed = false;
      // SUB gather/update steps per vote: LDS is coherent inside the workgroup and bits are only OR'ed in, so steps need
      // no barrier between them -- a wave always sees its own rows' previous step (program order), other waves' rows
      // whenever they land.  Only the termination vote needs the barrier.
#pragma unroll
      for (int sub = 0; sub < SUB; sub++) {
        unsigned long long nb = 0;
        if (CONN != 0) {
            // standard 6 / 18 / 26 structures: the row pattern is known at compile time, so the nine LDS reads are
            // issued back to back (no scalar branches between them) and OR'ed once they land
            unsigned long long v[9];
#pragma unroll
            for (int kk = 0; kk < 3; kk++)
#pragma unroll
                for (int jj = 0; jj < 3; jj++) {
                    const int nz = (kk != 1) + (jj != 1); // non-zero offsets among (dz, dy)
                    const int src = (tz + 1 - (kk - 1)) * HY + (ty + 1 - (jj - 1));
                    const bool full = CONN == 26 || (CONN == 18 && nz <= 1) || (CONN == 6 && nz == 0); // x pattern 111
                    const bool mid = (CONN == 18 && nz == 2) || (CONN == 6 && nz == 1);                // x pattern 010
                    v[kk * 3 + jj] = full ? L.sD[src] : (mid ? L.sN[src] : 0ull);
                }
#pragma unroll
            for (int q = 0; q < 9; q++) nb |= v[q];
        } else {
#pragma unroll
        for (int kk = 0; kk < 3; kk++)
#pragma unroll
            for (int jj = 0; jj < 3; jj++) {
                const uint32_t m3 = (st >> (kk * 9 + jj * 3)) & 7u;
                if (!m3) continue; // uniform
                // voxel p reached => p + (kk-1, jj-1, ii-1) reached; gather: source row = (z-(kk-1), y-(jj-1))
                const int src = (tz + 1 - (kk - 1)) * HY + (ty + 1 - (jj - 1));
                if (m3 == 7u) nb |= L.sD[src];
                else {
                    const unsigned long long n = L.sN[src];
                    if (m3 & 2u) nb |= n;
                    if (m3 & 4u) nb |= (n << 1) | (unsigned long long)(L.sCL[src] & 1u);        // ii = 2: source bit x-1
                    if (m3 & 1u) nb |= (n >> 1) | ((unsigned long long)L.sCR[src] << 63); // ii = 0: source bit x+1
                }
            }
        }
        unsigned long long nr = r | (nb & c);
        if (xrun) nr = fill_runs(nr, c);
        const bool ch = nr != r;
        if (ch) {
            r = nr;
            L.sN[me] = r;
            L.sD[me] = r | (r << 1) | (r >> 1) | mycl | (mycr << 63);
        }
        changed |= ch;
      }
        // vote: __syncthreads_or() costs ~1500 cycles on gfx950 (library workgroup reduction); a wave ballot + one
        // LDS flag + one barrier does the same in ~200.  Flag it&1 is read now, flag (it+1)&1 is cleared for the next
        // iteration (nobody touches it between this barrier and the next one's writers).
        // (Tried: one flag per wave, a wave whose own and whose neighbour waves' slices stood still in the last iteration
        // skips its gather -- 0.192 -> 0.213 ms on the bench volume: the fronts move along y as much as along z, so all
        // four waves stay busy, and the flag read at the loop head is one more dependent LDS round trip.)
        if (__any(changed) && (threadIdx.x & 63) == 0) L.vote[it & 1] = 1u;
        if (threadIdx.x == 0) L.vote[(it + 1) & 1] = 0u;
        __syncthreads();
        if (!L.vote[it & 1]) {
            exhausted = false;
            break;
        }
    }
    const unsigned long long chg = r ^ r_in;
    unsigned dirs = 0;
    if (chg) {
        reached[(z * t.dy + y) * t.wx + txi] = r;
        if (exhausted) dirs |= 1u << 13; // iteration cap hit before the local fix-point: revisit this tile
    }
    // Wake a neighbour tile only for an OPEN candidate: a voxel of it that is a candidate, was unreached when this visit
    // staged its halo, and lies in the 3 x 3 x 3 neighbourhood of one of the visit's new bits.  Every structuring element
    // is a subset of that neighbourhood, so the test can wake one tile too many and never one too few.  For the voxels
    // beside the word (the directions with dx in them) "unreached" alone stands in for "an unreached candidate": their
    // candidate bits would be 650 more loads per visit, and that measured slower (profiles/flood_wake_ab.md).
    // Why no candidate stays behind: let v (tile B) be a candidate that is unreached when the flood ends and touches a
    // reached voxel u of tile A != B.  Either u came from the coarse pass, a seed or a neighbour slab's plane -- those
    // bits enlist the tiles around them by their own path (k_flood_block_apply, mark_tile_nbhd) -- or u was a new bit of
    // some visit of A.  Reached bits are only ever added, so that visit's staged halo shows v unreached too (a stale
    // halo can only show fewer reached bits than there are): v was in its front and B was enlisted -- unless B was closed,
    // which a tile with the unreached candidate v is not -- and B's visit, which stages after A's publish (the next
    // round), reaches v.  Contradiction.  Most changes have nowhere to go: on the bench volume a flood takes 3 520 visits
    // instead of 4 590 -- what goes are visits that found nothing -- and one round fewer.
    // A lane tests the new bits of its own row against the open candidates, as staged, of the 3 x 3 rows around it: sO is 0
    // for the tile's own rows, so only the lanes on the tile's boundary can wake a direction with dz or dy in it; bits 1
    // and 2 of sCL are the unreached voxels beside a row's word, for the directions with dx in it.  No barrier: a lane
    // needs nobody else's new bits.
    if (chg) {
        const unsigned long long nd = chg | (chg << 1) | (chg >> 1);
        const unsigned int nl = (unsigned int)(chg & 1ull), nh = (unsigned int)(chg >> 63);
        // direction d = (dz+1)*9 + (dy+1)*3 + (dx+1); the row at offset (a, b) lies outside the tile only from a boundary
        // lane
        const unsigned int ys[3] = {ty == 0 ? 0u : 3u, 3u, ty == TY - 1 ? 6u : 3u};
#pragma unroll 1
        for (int a = -1; a <= 1; a++) { // (one slice of rows at a time: six LDS reads in flight, not eighteen -- registers)
            const unsigned int zs = a < 0 ? (tz == 0 ? 0u : 9u) : (a > 0 ? (tz == TZ - 1 ? 18u : 9u) : 9u);
            unsigned long long oc[3];
            unsigned int ox[3];
#pragma unroll
            for (int b = 0; b < 3; b++) {
                oc[b] = O.sO[me + a * HY + b - 1];
                ox[b] = L.sCL[me + a * HY + b - 1];
            }
#pragma unroll
            for (int b = 0; b < 3; b++) {
                const unsigned int d0 = zs + ys[b];
                dirs |= (unsigned int)((nd & oc[b]) != 0ull) << (d0 + 1);
                dirs |= (nl & (ox[b] >> 1)) << d0;
                dirs |= (nh & (ox[b] >> 2)) << (d0 + 2);
            }
        }
    }
    post_dirs(L, dirs);
    if (__any((c & ~r) != 0ull) && (threadIdx.x & 63) == 0) L.open = 1u;
}

// the structuring element's gather is a compile-time pattern for the three standard structures (see tile_update)
__device__ __forceinline__ void tile_update_conn(const Tiles &t, const unsigned long long *__restrict__ cand,
                                                 unsigned long long *reached, int64_t tile, TileLds &L, TileOpen &O) {
    if (t.conn == 26) tile_update<26>(t, cand, reached, tile, L, O);
    else if (t.conn == 18) tile_update<18>(t, cand, reached, tile, L, O);
    else if (t.conn == 6) tile_update<6>(t, cand, reached, tile, L, O);
    else tile_update<0>(t, cand, reached, tile, L, O);
}

// ---- tile hand-off: what a visit leaves for the next round ------------------------------------------------------------
// Mark tile nt in the next round's byte flags (four tiles per word: the atomicOr goes to the byte's word); whoever marks
// a byte first appends the tile to the next round's list.  MARK / SEEN: the bit set and the bits that mean "somebody was
// here before" (the coarse pass enlists with a bit of its own, see ENLISTED).  The list entry is a plain store: the next
// round reads it behind a kernel boundary.
template <unsigned int MARK = 1u, unsigned int SEEN = 0xffu>
__device__ __forceinline__ void enlist_tile(uint8_t *dirty_next, unsigned int *list_next, unsigned int *n_next, int64_t nt) {
    unsigned int *wp = (unsigned int *)(dirty_next + (nt & ~(int64_t)3));
    const unsigned int sh = 8 * (unsigned int)(nt & 3);
    const unsigned int old = atomicOr(wp, MARK << sh);
    if (!((old >> sh) & SEEN)) {
        unsigned int *slot = &list_next[atomicAdd(n_next, 1u)];
        *slot = (unsigned int)nt;
    }
}
// After the tile update (L.dirs and L.open complete): a tile with no candidate left is closed for good, so nobody needs to
// enlist it again (see CLOSED), and lane d < 27 wakes the neighbour tile in direction d when the visit's new bits touch an
// open candidate of that tile (bit 13 = the tile itself: the iteration cap ended the visit).
__device__ __forceinline__ void publish_tile(const Tiles &t, int64_t tile, const TileLds &L, uint8_t *dirty_cur,
                                             uint8_t *dirty_next, unsigned int *list_next, unsigned int *n_next) {
    const int64_t txi = tile % t.wx, r1 = tile / t.wx;
    const int64_t tyi = r1 % t.nty, tzi = r1 / t.nty;
    if (threadIdx.x == 32 && !L.open) {
        const unsigned int bit = CLOSED << (8 * (unsigned int)(tile & 3));
        atomicOr((unsigned int *)(dirty_cur + (tile & ~(int64_t)3)), bit);
        atomicOr((unsigned int *)(dirty_next + (tile & ~(int64_t)3)), bit);
    }
    if (threadIdx.x < 27 && (L.dirs >> threadIdx.x & 1u)) {
        const int d = threadIdx.x;
        const int64_t nz = tzi + d / 9 - 1, ny = tyi + (d / 3) % 3 - 1, nx = txi + d % 3 - 1;
        if (nz >= 0 && nz < t.ntz && ny >= 0 && ny < t.nty && nx >= 0 && nx < t.wx)
            enlist_tile(dirty_next, list_next, n_next, (nz * t.nty + ny) * t.wx + nx);
    }
}

// ---- arc-plane relaxation, shared by the directed and the linear-index tile update ------------------------------------
// Lane = word `me` of the staged rows.  e_ym / e_yp / e_zm / e_zp: the arcs arriving from the four row neighbours; exp /
// bexm: the arcs along +x inside the word and, bit-reversed, along -x; carry: what the x-neighbour words hand in (constant
// during a visit).  Same votes as tile_update.  Returns true when the iteration cap ended the loop before the local fix-point.
__device__ __forceinline__ bool relax_arcs(int itcap, TileLds &L, int me, bool inside, unsigned long long exp,
                                           unsigned long long bexm, unsigned long long e_ym, unsigned long long e_yp,
                                           unsigned long long e_zm, unsigned long long e_zp, unsigned long long carry,
                                           unsigned long long &r) {
    for (int it = 0; it < itcap; it++) {
        unsigned long long nr = r | carry | (L.sN[me - 1] & e_ym) | (L.sN[me + 1] & e_yp) | (L.sN[me - HY] & e_zm) |
                                (L.sN[me + HY] & e_zp);
        nr |= (exp + (nr & exp)) ^ exp;
        unsigned long long rn = __brevll(nr);
        rn |= (bexm + (rn & bexm)) ^ bexm;
        nr = __brevll(rn);
        if (!inside) nr = 0ull;
        const bool ch = nr != r;
        if (ch) {
            r = nr;
            L.sN[me] = r;
        }
        if (__any(ch) && (threadIdx.x & 63) == 0) L.vote[it & 1] = 1u;
        if (threadIdx.x == 0) L.vote[(it + 1) & 1] = 0u;
        __syncthreads();
        if (!L.vote[it & 1]) return false;
    }
    return true;
}

// ---- directed tile update (floodfill_auto_threshold) -------------------------------------------------------------
// The admissible range of a step depends on the voxel it LEAVES (floodfill_py.rs:32-35), so reachability is directed:
// six edge planes say, per source voxel, whether the step to its +x / -x / +y / -y / +z / -z neighbour is allowed
// (k_flood_edges_auto folds "the target is not a barrier" into them).  Same tile, same relaxation, same votes as
// tile_update; a lane gathers  reached(neighbour row) & edge(neighbour row -> me)  for its four row neighbours (the edge
// words are loaded once per visit), and closes x-chains inside its word with the carry trick along the edge bits:
// (E + (R & E)) ^ E  sets every bit a run of consecutive edges carries a reached bit to (bit-reversed twin for -x).
__device__ __forceinline__ void tile_update_dir(const Tiles &t, const unsigned long long *__restrict__ edges,
                                                unsigned long long *reached, int64_t tile, TileLds &L) {
    const int64_t txi = tile % t.wx, r1 = tile / t.wx;
    const int64_t tyi = r1 % t.nty, tzi = r1 / t.nty;
    const int64_t z0 = tzi * TZ, y0 = tyi * TY;
    const int64_t plane = t.dz * t.dy * t.wx; // words per edge plane
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const int idx = threadIdx.x + pass * NT;
        if (idx < HZ * HY) {
            const int yy = idx % HY, zz = idx / HY;
            const int64_t z = z0 + zz - 1, y = y0 + yy - 1;
            L.sN[idx] = (z >= 0 && z < t.dz && y >= 0 && y < t.dy) ? reached[(z * t.dy + y) * t.wx + txi] : 0ull;
        }
    }
    const int ty = threadIdx.x & (TY - 1), tz = threadIdx.x >> TY_LOG;
    const int64_t z = z0 + tz, y = y0 + ty;
    const bool inside = z < t.dz && y < t.dy;
    const int64_t me_w = (z * t.dy + y) * t.wx + txi;
    unsigned long long exp = 0, bexm = 0, e_ym = 0, e_yp = 0, e_zm = 0, e_zp = 0, carry = 0;
    if (inside) {
        exp = edges[me_w];
        bexm = __brevll(edges[plane + me_w]);
        if (y > 0) e_ym = edges[2 * plane + me_w - t.wx];                  // row y-1 stepping +y
        if (y + 1 < t.dy) e_yp = edges[3 * plane + me_w + t.wx];           // row y+1 stepping -y
        if (z > 0) e_zm = edges[4 * plane + me_w - t.dy * t.wx];           // slice z-1 stepping +z
        if (z + 1 < t.dz) e_zp = edges[5 * plane + me_w + t.dy * t.wx];    // slice z+1 stepping -z
        // steps across the word boundary come from the x-neighbour tiles: constant during this visit
        if (txi > 0) carry |= (reached[me_w - 1] & edges[me_w - 1]) >> 63;
        if (txi + 1 < t.wx) carry |= (reached[me_w + 1] & edges[plane + me_w + 1] & 1ull) << 63;
    }
    if (threadIdx.x == 0) L.vote[0] = 0u;
    __syncthreads();
    const int me = (tz + 1) * HY + (ty + 1);
    const unsigned long long r_in = L.sN[me];
    unsigned long long r = r_in;
    const bool exhausted = relax_arcs(t.itcap, L, me, inside, exp, bexm, e_ym, e_yp, e_zm, e_zp, carry, r);
    const unsigned long long chg = r ^ r_in;
    unsigned dirs = 0;
    if (chg) {
        reached[me_w] = r;
        const bool zlo = tz == 0, zhi = tz == TZ - 1, ylo = ty == 0, yhi = ty == TY - 1;
        const bool xlo = chg & 1ull, xhi = chg >> 63;
        // face neighbours only: every step moves along one axis
        if (zlo) dirs |= 1u << 4;
        if (zhi) dirs |= 1u << 22;
        if (ylo) dirs |= 1u << 10;
        if (yhi) dirs |= 1u << 16;
        if (xlo) dirs |= 1u << 12;
        if (xhi) dirs |= 1u << 14;
        if (exhausted) dirs |= 1u << 13;
    }
    post_dirs(L, dirs);
    if (threadIdx.x == 0) L.open = 1u; // (edge planes: no candidate plane to be exhausted)
}

// ---- linear-index tile update (the IFT watershed's cost levels, ivx_dev_ws_cost_levels) --------------------------------
// scipy's watershed_ift takes neighbours by LINEAR index (ni_measure.c: only indices outside [0, size) are refused), so the
// last voxel of a row neighbours the first voxel of the next row, and the last row of a slice the first row of the next
// slice.  With rows of whole 64-voxel words the volume is ONE flat bit array: the x-neighbour of a word is word +- 1, the
// y-neighbour word +- wx, the z-neighbour word +- dy * wx, and "in bounds" means 0 <= word < nwords -- nothing else.  Arcs are
// symmetric, so three planes suffice: bit b of Ex / Ey / Ez[word] = the arc from voxel (word, b) to its +1 / +W / +HW
// neighbour is enabled; the arc arriving from the other side is the neighbour word's bit.  The staged halo rows are the
// LINEAR neighbours (row index z * dy + y, taken as it comes), which is the wrap-around for free; only the wake-up of the
// tiles that read a changed word has to look the reader up when it is not the lattice neighbour (border tiles).
// (returns true when the reader is this very tile -- a volume one tile wide: the caller then revisits itself)
__device__ __forceinline__ bool lin_enlist(const Tiles &t, int64_t word, int64_t self, uint8_t *dirty_next, unsigned int *list_next,
                                           unsigned int *n_next) {
    const int64_t row = word / t.wx, txi = word - row * t.wx, z = row / t.dy, y = row - z * t.dy;
    const int64_t nt = ((z / TZ) * t.nty + (y >> TY_LOG)) * t.wx + txi;
    if (nt == self) return true;
    enlist_tile(dirty_next, list_next, n_next, nt);
    return false;
}

__device__ __forceinline__ void tile_update_lin(const Tiles &t, const unsigned long long *__restrict__ E,
                                                unsigned long long *reached, int64_t tile, TileLds &L, uint8_t *dirty_next,
                                                unsigned int *list_next, unsigned int *n_next) {
    const int64_t txi = tile % t.wx, r1 = tile / t.wx;
    const int64_t tyi = r1 % t.nty, tzi = r1 / t.nty;
    const int64_t z0 = tzi * TZ, y0 = tyi * TY;
    const int64_t nrows = t.dz * t.dy, nwords = nrows * t.wx, hwx = t.dy * t.wx;
    const unsigned long long *Ex = E, *Ey = E + nwords, *Ez = E + 2 * nwords;
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const int idx = threadIdx.x + pass * NT;
        if (idx < HZ * HY) {
            const int yy = idx % HY, zz = idx / HY;
            const int64_t row = (z0 + zz - 1) * t.dy + (y0 + yy - 1); // linear: row -1 of a slice IS the last row of the slice below
            L.sN[idx] = (row >= 0 && row < nrows) ? reached[row * t.wx + txi] : 0ull;
        }
    }
    const int ty = threadIdx.x & (TY - 1), tz = threadIdx.x >> TY_LOG;
    const int64_t row = (z0 + tz) * t.dy + (y0 + ty);
    const bool inside = row < nrows; // (dy is a multiple of TY: only whole slices can be missing)
    const int64_t me_w = row * t.wx + txi;
    unsigned long long exp = 0, bexm = 0, e_ym = 0, e_yp = 0, e_zm = 0, e_zp = 0, carry = 0, xgain = 0;
    if (inside) {
        exp = Ex[me_w];
        bexm = __brevll(exp << 1); // stepping down from bit b needs the arc (b - 1, b) = bit b - 1 of Ex
        if (me_w - t.wx >= 0) e_ym = Ey[me_w - t.wx];
        if (me_w + t.wx < nwords) e_yp = Ey[me_w];
        if (me_w - hwx >= 0) e_zm = Ez[me_w - hwx];
        if (me_w + hwx < nwords) e_zp = Ez[me_w];
        // steps across the word boundary come from the neighbour WORDS (other tiles): constant during this visit
        if (me_w > 0) {
            const unsigned long long lr = reached[me_w - 1] >> 63, le = Ex[me_w - 1] >> 63;
            carry |= lr & le;
            xgain |= le & ~lr;              // my bit 0 could still hand something to the left word
        }
        if (me_w + 1 < nwords) {
            const unsigned long long rr = reached[me_w + 1] & 1ull, re = exp >> 63;
            carry |= (rr & re) << 63;
            xgain |= (re & ~rr) << 63;      // my bit 63 to the right word
        }
    }
    if (threadIdx.x == 0) L.vote[0] = 0u;
    __syncthreads();
    const int me = (tz + 1) * HY + (ty + 1);
    const unsigned long long r_in = L.sN[me];
    unsigned long long r = r_in;
    const bool exhausted = relax_arcs(t.itcap, L, me, inside, exp, bexm, e_ym, e_yp, e_zm, e_zp, carry, r);
    const unsigned long long chg = r ^ r_in;
    unsigned dirs = 0;
    if (chg) {
        reached[me_w] = r;
        // A neighbour tile is woken only when one of the NEW bits has an enabled arc to a voxel of it that was not
        // reached when this visit staged its halo (a stale halo can only wake one tile too many): in a flood near the
        // percolation threshold most changes have nowhere to go, and most wake-ups were visits that found nothing.
        const bool zlo = tz == 0 && (chg & e_zm & ~L.sN[me - HY]), zhi = tz == TZ - 1 && (chg & e_zp & ~L.sN[me + HY]);
        const bool ylo = ty == 0 && (chg & e_ym & ~L.sN[me - 1]), yhi = ty == TY - 1 && (chg & e_yp & ~L.sN[me + 1]);
        const bool xlo = chg & xgain & 1ull, xhi = (chg & xgain) >> 63;
        // readers that ARE the lattice neighbour tile: one direction bit per workgroup (enlisted by the caller);
        // readers across a row / slice end (border tiles only): looked up word by word
        if (zlo) dirs |= 1u << 4;
        if (zhi) dirs |= 1u << 22;
        if (ylo) {
            if (y0 > 0) dirs |= 1u << 10;
            else if (me_w - t.wx >= 0 && lin_enlist(t, me_w - t.wx, tile, dirty_next, list_next, n_next)) dirs |= 1u << 13;
        }
        if (yhi) {
            if (y0 + TY < t.dy) dirs |= 1u << 16;
            else if (me_w + t.wx < nwords && lin_enlist(t, me_w + t.wx, tile, dirty_next, list_next, n_next)) dirs |= 1u << 13;
        }
        if (xlo) {
            if (txi > 0) dirs |= 1u << 12;
            else if (me_w > 0 && lin_enlist(t, me_w - 1, tile, dirty_next, list_next, n_next)) dirs |= 1u << 13;
        }
        if (xhi) {
            if (txi + 1 < t.wx) dirs |= 1u << 14;
            else if (me_w + 1 < nwords && lin_enlist(t, me_w + 1, tile, dirty_next, list_next, n_next)) dirs |= 1u << 13;
        }
        if (exhausted) dirs |= 1u << 13;
    }
    post_dirs(L, dirs);
    if (threadIdx.x == 0) L.open = 1u; // (arc planes change from level to level: a tile is never closed for good)
}

// ---- list-driven round: only as many workgroups as there are dirty tiles do any work ------------------------------------
// The dirty set of a round is a compact list (plus the byte flags, which de-duplicate marks).  A workgroup takes list
// entries blockIdx.x, blockIdx.x + gridDim.x, ...; an idle round costs one small launch instead of ntiles empty workgroups,
// and the dirty tiles of a busy round start at once instead of waiting for the dispatcher to walk past the clean ones.
__global__ void k_flood_build_list(Tiles t, const uint8_t *__restrict__ dirty, unsigned int *__restrict__ list,
                                   unsigned int *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < t.ntiles && (dirty[i] & 1u)) list[atomicAdd(count, 1u)] = (unsigned int)i;
}

// Statistics in the counter block, cleared with it (ivx_dev_flood_visits): round k = 1 .. HIST stores the length of its
// list in a word of its own -- one plain store beside the others thread 0 of workgroup 0 issues as the round starts, no load, so
// no visit waits for it -- and the rounds past HIST (the union-find escape takes a plain flood over long before; the
// directed and the linear floods can get there) add theirs to one more word; the stream orders the rounds.
// (Dwords 32 .. 35, right below STATS_AT, are a reserved gap: cleared with the block, used by nothing.)
constexpr int STATS_AT = 36, HIST_AT = 64, HIST = 64, CNT_CLEARED = HIST_AT + HIST;
static_assert(CNT_CLEARED == FLOOD_CNT_DWORDS, "the counter block of flood_tiles.h");
__device__ __forceinline__ void count_visits(unsigned int *cnt, unsigned int round, unsigned int n) {
    if (!n) return;
    if (round <= (unsigned int)HIST) cnt[HIST_AT + round - 1u] = n;
    else cnt[STATS_AT] += n;
}
// `line` (pinned host memory, ivx::progress_line): word 0 = tag | round + 1 | tiles on this round's list, stored as the
// round STARTS (everything before it in the stream is complete, so the count is final); word 1 = tag | round + 1 of the
// last round that had any work.  The host polls word 0, keeps up to a few rounds queued ahead of the newest one it has
// seen start, and stops when a round starts with an empty list -- or when word 2 = tag | rounds in front | 1 arrives: the
// report of a write that was queued among the rounds and found the next list empty (ApplyWhen).
// MODE 0: candidate plane; 1 (directed): `cand` holds the six edge planes of k_flood_edges_auto instead; 2 (linear): the
// three arc planes of k_wsa_planes (k_costlevels.hip) and scipy's linear-index neighbourhood (tile_update_lin)
template <int MODE>
__global__ __launch_bounds__(NT, 6) void k_flood_round_list(Tiles t, const unsigned long long *__restrict__ cand,
                                                             unsigned long long *reached, const unsigned int *__restrict__ list_cur,
                                                             const unsigned int *__restrict__ n_cur, uint8_t *dirty_cur,
                                                             uint8_t *dirty_next, unsigned int *list_next,
                                                             unsigned int *n_next, unsigned int *n_clear,
                                                             unsigned int *cnt_all, unsigned long long *line,
                                                             unsigned int tag_round, unsigned int *gate,
                                                             unsigned int gate_val, unsigned int gate_below) {
    __shared__ TileLds L;
    const unsigned int n = *n_cur;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // a short list: the busy rounds are over, let background work gated on this word start (ivx_dev_flood_arm_gate)
        if (gate && n < gate_below) __hip_atomic_store(gate, gate_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *n_clear = 0u; // the counter the round AFTER the next one appends to
        count_visits(cnt_all, tag_round & 0xffffffu, n);
        const unsigned long long hi = (unsigned long long)tag_round << 32;
        __hip_atomic_store(&line[0], hi | n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (n) __hip_atomic_store(&line[1], hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    for (unsigned int li = blockIdx.x; li < n; li += gridDim.x) {
        const int64_t tile = list_cur[li];
        if (threadIdx.x == 0) {
            dirty_cur[tile] = 0;
            L.dirs = 0;
            L.open = 0;
        }
        __syncthreads();
        if constexpr (MODE == 2) tile_update_lin(t, cand, reached, tile, L, dirty_next, list_next, n_next);
        else if constexpr (MODE == 1) tile_update_dir(t, cand, reached, tile, L);
        else {
            __shared__ TileOpen O; // (the candidate-plane flood only)
            tile_update_conn(t, cand, reached, tile, L, O);
        }
        lds_barrier(); // L.dirs complete; the publish stores keep flying (the kernel boundary orders them for the next round)
        publish_tile(t, tile, L, dirty_cur, dirty_next, list_next, n_next);
        __syncthreads(); // L is reused by the next list entry of this workgroup
    }
}

__global__ void k_flood_mark(Tiles t, int64_t tz0, int64_t tz1, uint8_t *dirty) {
    const int64_t per = t.nty * t.wx;
    const int64_t n = (tz1 - tz0) * per;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dirty[tz0 * per + i] = 1;
}

// ---- coarse pass: whole tiles at once ---------------------------------------------------------------
// A tile whose in-bounds voxels are ALL candidates is connected in itself under every structuring element that
// contains the six face offsets, so one reached voxel in it means the whole tile is reached, and two such tiles that
// touch (by a face; by an edge for 18/26; by a corner for 26) reach each other.  The interior of a solid region is made
// of such tiles, and crossing it voxel-tile by voxel-tile costs one ~11 us round per tile hop.  The coarse pass floods
// the TILE graph instead: flags (k_flood_tile_flags) -> fix-point over rows of tile bits in ONE workgroup
// (k_flood_coarse: a row of tiles along x is one 64-bit word, the same dilate / carry-fill update as the voxel tiles)
// -> reached = cand for the tiles it reached and a dirty mark on their other neighbours (k_flood_coarse_apply).
// The ordinary rounds then only have the boundary shell left.  Result bits are identical with or without it.
constexpr int CT = 1024, CRP = 8, CROWS_MAX = 7680; // coarse workgroup size, rows per lane, LDS rows incl. halo (60 KB)
constexpr unsigned int ENLISTED = 0x80u;             // dirty-byte bit: "already on the round-0 list" (coarse pass only)

// Granularity of the coarse graph: blocks of BXS x 16 x 16 voxels, BXS = 16, 32 or 64 (a quarter, half or whole tile along
// x; the y / z extent is the tile's, so a row of blocks along x is still one row of the tile grid).  A row of blocks is one
// 64-bit word (bit = block index along x), so BXS is the smallest of the three with 64 / BXS * wx <= 64: 16 up to 1024
// voxels along x, 32 up to 2048, 64 (= the tile itself) up to 4096.  Finer blocks reach closer to the region's surface:
// on the bench volume the rounds that follow drop from 13 to 8 (tools/sim_flood.c reproduces the round structure on the CPU).
//   rowF[g]  the block is all-candidate,   rowW[g]  the block is wholly reached (seeded here / by k_flood_coarse, closed by it).
struct Blocks {
    int q;   // blocks per tile along x (4, 2, 1)
    int bxs; // voxels per block along x (16, 32, 64)
};
__device__ __forceinline__ unsigned long long block_mask(const Blocks &b, unsigned long long qbits) {
    // qbits: one bit per block of a word -> the voxel bits of those blocks
    const unsigned long long one = b.bxs == 64 ? ~0ull : ((1ull << b.bxs) - 1ull);
    unsigned long long m = 0;
    for (int q = 0; q < b.q; q++)
        if (qbits >> q & 1ull) m |= one << (b.bxs * q);
    return m;
}
// the blocks of tile column txi that exist (hold at least one in-bounds voxel), as a q-bit mask
__device__ __forceinline__ unsigned int block_exist(const Tiles &t, const Blocks &b, int64_t txi) {
    unsigned int m = 0;
    for (int q = 0; q < b.q; q++)
        if (txi * 64 + (int64_t)b.bxs * q < t.dx) m |= 1u << q;
    return m;
}

__device__ __forceinline__ double load_as_double(const void *data, int dtype, int64_t i) {
    switch (dtype) {
    case IVX_I16: return (double)((const int16_t *)data)[i];
    case IVX_U8: return (double)((const uint8_t *)data)[i];
    case IVX_U16: return (double)((const uint16_t *)data)[i];
    default: return ((const double *)data)[i];
    }
}

// One workgroup per tile row: the 16 rows of a slice are contiguous, so the loads coalesce across the row's tiles.
// FRESH: the flood starts from the seeds in `sp` and nothing else -- `reached` and the dirty flags are not read (their old
// contents are dead: k_flood_block_apply<true> rewrites every word of the plane), this kernel zeroes the dirty flags and
// the round counters, and workgroup 0 tests the seeds (floodfill.rs:123: only in-range seeds start a flood; an accepted
// seed is a candidate even when its barrier byte already equals `fill`) and leaves the accepted ones as a bit mask.
template <bool FRESH>
__global__ __launch_bounds__(256) void k_flood_block_flags(Tiles t, Blocks bk, unsigned long long *cand,
                                                           const unsigned long long *__restrict__ reached,
                                                           uint8_t *dirty, uint8_t *dirty1,
                                                           unsigned long long *__restrict__ rowF,
                                                           unsigned long long *__restrict__ rowW,
                                                           unsigned int *__restrict__ cnt, int ncnt, SeedPack sp, int dtype,
                                                           const void *__restrict__ data, double t0, double t1,
                                                           unsigned int *__restrict__ seed_ok) {
    __shared__ unsigned int s_bad[64], s_has[64];
    const int64_t tyi = blockIdx.x % t.nty, tzi = blockIdx.x / t.nty;
    if (threadIdx.x < 64) {
        s_bad[threadIdx.x] = 0u;
        s_has[threadIdx.x] = 0u;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < ncnt) cnt[threadIdx.x] = 0u; // the round counters (k_flood_block_apply appends)
    const int wx = (int)t.wx, per_z = TY * wx, nw = TZ * per_z;
    const int64_t tile0 = (int64_t)blockIdx.x * t.wx;
    if (FRESH) {
        if ((int)threadIdx.x < wx) {
            dirty[tile0 + threadIdx.x] = 0;
            dirty1[tile0 + threadIdx.x] = 0;
        }
        if (blockIdx.x == 0) {
            __shared__ unsigned int s_ok;
            if (threadIdx.x == 0) s_ok = 0u;
            __syncthreads();
            if ((int)threadIdx.x < sp.n) {
                const int64_t x = sp.xyz[threadIdx.x][0], y = sp.xyz[threadIdx.x][1], z = sp.xyz[threadIdx.x][2];
                const double v = load_as_double(data, dtype, (z * t.dy + y) * t.dx + x);
                if (v >= t0 && v <= t1) {
                    atomicOr(&cand[(z * t.dy + y) * t.wx + (x >> 6)], 1ull << (x & 63));
                    atomicOr(&s_ok, 1u << threadIdx.x);
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) *seed_ok = s_ok;
        }
    }
    __syncthreads();
    const unsigned long long last = (t.dx & 63) ? (1ull << (t.dx & 63)) - 1ull : ~0ull;
    const unsigned long long one = bk.bxs == 64 ? ~0ull : ((1ull << bk.bxs) - 1ull);
    for (int i0 = threadIdx.x; i0 < nw; i0 += 4 * 256) { // four loads in flight per lane: the kernel is latency-bound
        unsigned long long cv[4], rv[4];
        int64_t wi[4];
        int tx[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * 256;
            const int tz = i / per_z, rem = i - tz * per_z, ty = rem / wx;
            tx[u] = rem - ty * wx;
            const int64_t z = tzi * TZ + tz, y = tyi * TY + ty;
            wi[u] = (i < nw && z < t.dz && y < t.dy) ? (z * t.dy + y) * t.wx + tx[u] : -1;
            cv[u] = wi[u] >= 0 ? cand[wi[u]] : 0ull;
            rv[u] = 0ull;
            if (!FRESH && wi[u] >= 0 && (dirty[tile0 + tx[u]] & 1u)) rv[u] = reached[wi[u]]; // only freshly seeded / marked tiles start a coarse flood
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (wi[u] < 0) continue;
            const unsigned long long miss = ~cv[u] & (tx[u] == wx - 1 ? last : ~0ull); // in-bounds voxels that are no candidates
            for (int q = 0; q < bk.q; q++) {
                if ((miss >> (bk.bxs * q)) & one) s_bad[tx[u] * bk.q + q] = 1u;
                else if (!FRESH && ((rv[u] >> (bk.bxs * q)) & one)) s_has[tx[u] * bk.q + q] = 1u;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int b = threadIdx.x, btx = b / bk.q;
        const bool in = btx < wx && (int64_t)btx * 64 + (int64_t)bk.bxs * (b % bk.q) < t.dx; // the block exists
        const unsigned long long f = __ballot(in && !s_bad[b]);
        const unsigned long long h = __ballot(in && s_has[b]);
        if (threadIdx.x == 0) {
            rowF[blockIdx.x] = f;
            rowW[blockIdx.x] = FRESH ? 0ull : (f & h);
        }
    }
}

// SEEDED: the accepted seeds of `sp` (mask *seed_ok) that sit in an all-candidate block start the coarse flood
template <int CONN, bool SEEDED>
__global__ __launch_bounds__(CT) void k_flood_coarse(Tiles t, Blocks bk, const unsigned long long *__restrict__ rowF,
                                                     unsigned long long *__restrict__ rowW, SeedPack sp,
                                                     const unsigned int *__restrict__ seed_ok) {
    __shared__ unsigned long long sR[CROWS_MAX];
    __shared__ unsigned int vote[2];
    const int nty = (int)t.nty, ntz = (int)t.ntz, hy = nty + 2;
    const int nrows = nty * ntz, nh = hy * (ntz + 2);
    unsigned long long F[CRP], R[CRP];
    int me[CRP];
#pragma unroll
    for (int k = 0; k < CRP; k++) { // issue the loads before the LDS clear
        const int j = threadIdx.x + k * (int)blockDim.x;
        F[k] = j < nrows ? rowF[j] : 0ull;
        R[k] = (j < nrows && !SEEDED) ? rowW[j] : 0ull;
        me[k] = j < nrows ? (j / nty + 1) * hy + (j % nty) + 1 : 0;
    }
    for (int i = threadIdx.x; i < nh; i += blockDim.x) sR[i] = 0ull;
    if (threadIdx.x == 0) vote[0] = 0u;
    __syncthreads();
    if (SEEDED) {
        if ((int)threadIdx.x < sp.n && (*seed_ok >> threadIdx.x & 1u)) {
            const int64_t x = sp.xyz[threadIdx.x][0], y = sp.xyz[threadIdx.x][1], z = sp.xyz[threadIdx.x][2];
            const int j = (int)((z / TZ) * nty + y / TY);
            const unsigned long long bit = 1ull << (x / bk.bxs);
            if (rowF[j] & bit) atomicOr(&sR[(j / nty + 1) * hy + (j % nty) + 1], bit);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CRP; k++) R[k] = sR[me[k]]; // (unused slots read the all-zero corner row)
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < CRP; k++)
        if (R[k]) {
            R[k] = fill_runs(R[k], F[k]);
            sR[me[k]] = R[k];
        }
    __syncthreads();
    for (int it = 0; it < 65536; it++) {
        bool changed = false;
#pragma unroll
        for (int k = 0; k < CRP; k++) {
            if (!(F[k] & ~R[k])) continue; // nothing left to gain in this row (also skips the unused slots)
            unsigned long long nb = 0;
#pragma unroll
            for (int kk = -1; kk <= 1; kk++)
#pragma unroll
                for (int jj = -1; jj <= 1; jj++) {
                    const int nz = (kk != 0) + (jj != 0);
                    const bool wide = CONN == 26 || (CONN == 18 && nz <= 1) || (CONN == 6 && nz == 0);
                    const bool mid = (CONN == 18 && nz == 2) || (CONN == 6 && nz == 1);
                    if (!wide && !mid) continue;
                    const unsigned long long n = sR[me[k] + kk * hy + jj];
                    nb |= wide ? (n | (n << 1) | (n >> 1)) : n;
                }
            const unsigned long long nr = fill_runs(R[k] | (nb & F[k]), F[k]);
            if (nr != R[k]) {
                R[k] = nr;
                sR[me[k]] = nr;
                changed = true;
            }
        }
        if (__any(changed) && (threadIdx.x & 63) == 0) vote[it & 1] = 1u;
        if (threadIdx.x == 0) vote[(it + 1) & 1] = 0u;
        __syncthreads();
        if (!vote[it & 1]) break;
    }
#pragma unroll
    for (int k = 0; k < CRP; k++) {
        const int j = threadIdx.x + k * (int)blockDim.x;
        if (j < nrows) rowW[j] = R[k];
    }
}

// reached = cand for the wholly reached blocks; the tiles around them that are not wholly reached themselves (and the
// seeded tiles that are not whole) go straight onto the round-0 list: a dirty byte is enlisted by whoever sets its
// ENLISTED bit first (enlist_tile with that bit; a CLOSED byte counts as taken).
// FRESH: every word of the plane is written (whole blocks: their candidates; the accepted seeds' bits; zero elsewhere), so
// the plane needs no clearing pass before the flood
template <bool FRESH>
__global__ __launch_bounds__(256) void k_flood_block_apply(Tiles t, Blocks bk, const unsigned long long *__restrict__ cand,
                                                           unsigned long long *__restrict__ reached,
                                                           const unsigned long long *__restrict__ rowW, uint8_t *dirty,
                                                           unsigned int *__restrict__ list, unsigned int *count, SeedPack sp,
                                                           const unsigned int *__restrict__ seed_ok) {
    __shared__ unsigned int s_chg[64];
    __shared__ unsigned int s_all[64]; // the tile's news is not (only) whole blocks: a seed, bits that arrived from outside
    __shared__ unsigned int s_seeds; // FRESH: the accepted seeds that sit in this tile row
    const int64_t tyi = blockIdx.x % t.nty, tzi = blockIdx.x / t.nty;
    const int wx = (int)t.wx, per_z = TY * wx, nw = TZ * per_z;
    const int64_t tile0 = (int64_t)blockIdx.x * t.wx;
    const unsigned long long whole = rowW[blockIdx.x];
    const unsigned int qm = (1u << bk.q) - 1u;
    if (threadIdx.x < 64) s_chg[threadIdx.x] = s_all[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s_seeds = 0u;
    __syncthreads();
    if (FRESH) {
        if ((int)threadIdx.x < sp.n && (*seed_ok >> threadIdx.x & 1u) && sp.xyz[threadIdx.x][2] / TZ == tzi &&
            sp.xyz[threadIdx.x][1] / TY == tyi) {
            const int64_t sx = sp.xyz[threadIdx.x][0] >> 6;
            s_chg[sx] = s_all[sx] = 1u; // a seed starts its tile (and wakes the tiles around it)
            atomicOr(&s_seeds, 1u << threadIdx.x);
        }
    } else if ((int)threadIdx.x < wx && (dirty[tile0 + threadIdx.x] & 1u)) {
        const unsigned int ex = block_exist(t, bk, threadIdx.x);
        if (((unsigned int)(whole >> (bk.q * threadIdx.x)) & ex) == ex) {
            dirty[tile0 + threadIdx.x] = 0; // final: a wholly reached tile has nothing to gain
            // ... but it was marked because bits arrived in it from OUTSIDE the flood (a seed, a neighbour slab's plane
            // OR-ed into a halo slice): even when those bits already fill the tile, nobody has told its neighbours yet
            s_chg[threadIdx.x] = s_all[threadIdx.x] = 1u;
        } else {
            enlist_tile<ENLISTED, ENLISTED | CLOSED>(dirty, list, count, tile0 + threadIdx.x);
        }
    }
    if (!FRESH && !whole) return; // uniform
    __syncthreads();
    const unsigned int ok = FRESH ? s_seeds : 0u;
    for (int i0 = threadIdx.x; i0 < nw; i0 += 4 * 256) { // four word pairs in flight per lane
        unsigned long long cv[4], rv[4], bm[4];
        int64_t wi[4];
        int tx[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * 256;
            const int tz = i / per_z, rem = i - tz * per_z, ty = rem / wx;
            tx[u] = rem - ty * wx;
            const int64_t z = tzi * TZ + tz, y = tyi * TY + ty;
            const unsigned int wq = (unsigned int)(whole >> (bk.q * tx[u])) & qm;
            wi[u] = (i < nw && (FRESH || wq) && z < t.dz && y < t.dy) ? (z * t.dy + y) * t.wx + tx[u] : -1;
            bm[u] = wq ? block_mask(bk, wq) : 0ull;
            cv[u] = (wi[u] >= 0 && wq) ? cand[wi[u]] : 0ull;
            rv[u] = (!FRESH && wi[u] >= 0) ? reached[wi[u]] : 0ull;
            if (FRESH && wi[u] >= 0 && ok) { // the accepted seeds of this word
                const int64_t z2 = tzi * TZ + tz, y2 = tyi * TY + ty;
                for (int n = 0; n < sp.n; n++)
                    if ((ok >> n & 1u) && sp.xyz[n][2] == z2 && sp.xyz[n][1] == y2 && (sp.xyz[n][0] >> 6) == tx[u])
                        rv[u] |= 1ull << (sp.xyz[n][0] & 63);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (wi[u] < 0) continue;
            const unsigned long long nr = rv[u] | (cv[u] & bm[u]);
            if (FRESH) {
                reached[wi[u]] = nr;
                if (bm[u]) s_chg[tx[u]] = 1u;
            } else if (nr != rv[u]) { // the tile gained voxels: its neighbours (and its own open part) must look again
                reached[wi[u]] = nr;
                s_chg[tx[u]] = 1u;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 27 * wx; i += 256) {
        const int txi = i / 27, d = i - txi * 27;
        if (!s_chg[txi]) continue;
        const int64_t nz = tzi + d / 9 - 1, ny = tyi + (d / 3) % 3 - 1, nx = txi + d % 3 - 1;
        if (nz < 0 || nz >= t.ntz || ny < 0 || ny >= t.nty || nx < 0 || nx >= t.wx) continue;
        const unsigned int ex = block_exist(t, bk, nx);
        const unsigned int wn = (unsigned int)(rowW[nz * t.nty + ny] >> (bk.q * nx)) & ex;
        if (wn == ex) continue; // wholly reached: nothing to gain
        if (!s_all[txi]) {
            // The tile's news is the whole blocks it gained: an unreached candidate next to one of their voxels lies in a
            // block that is not wholly reached and touches a whole block of this tile (face, edge or corner, whatever the
            // structuring element: one tile too many at worst).  Only a neighbour that holds such a block is woken -- on
            // the bench volume 1 140 tiles instead of 1 662, against 1 131 that hold such a candidate (tools/sim_flood.py).
            // (A block is as high and as deep as a tile, TY x TZ: the blocks of a neighbour tile differ from this tile's
            // only in their place along x, which the dilation of the row word covers.)
            const unsigned long long wt = (unsigned long long)((unsigned int)(whole >> (bk.q * txi)) & qm) << (bk.q * txi);
            if (!((unsigned int)((wt | (wt << 1) | (wt >> 1)) >> (bk.q * nx)) & ex & ~wn)) continue;
        }
        enlist_tile<ENLISTED, ENLISTED | CLOSED>(dirty, list, count, (nz * t.nty + ny) * t.wx + nx);
    }
}

// ---- floodfill_auto_threshold: edge planes --------------------------------------------------------------------
// floodfill_py.rs:32-35: a voxel of value v lets the flood step to a 6-neighbour whose value lies in
// [ceil(v * (1 - p)), floor(v * (1 + p))], both f32 products cast to i16 the way Rust's `as` does (saturating, NaN -> 0),
// provided that neighbour's `out` byte is not `fill` yet.  One lane per 8 source voxels -> one byte in each of the six
// planes (+x, -x, +y, -y, +z, -z; bit = SOURCE voxel).
__device__ __forceinline__ int sat_i16(float f) {
    if (f != f) return 0;
    if (f <= -32768.0f) return -32768;
    if (f >= 32767.0f) return 32767;
    return (int)f;
}
__global__ __launch_bounds__(256) void k_flood_edges_auto(const int16_t *__restrict__ data, const uint8_t *__restrict__ out,
                                                          Tiles t, float p, uint8_t fill, uint8_t *__restrict__ edges) {
    const int64_t bpr = t.wx * 8, rows = t.dz * t.dy, total = rows * bpr;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const float lo_f = 1.0f - p, hi_f = 1.0f + p;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t row = i / bpr, q = i - row * bpr;
        const int64_t z = row / t.dy, y = row - z * t.dy;
        unsigned m[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        const int64_t base = row * t.dx;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int64_t x = q * 8 + e;
            if (x >= t.dx) break;
            const float val = (float)data[base + x];
            const int t0 = sat_i16(ceilf(val * lo_f)), t1 = sat_i16(floorf(val * hi_f));
            const int64_t off[6] = {1, -1, t.dx, -t.dx, t.dy * t.dx, -t.dy * t.dx};
            const bool ok[6] = {x + 1 < t.dx, x > 0, y + 1 < t.dy, y > 0, z + 1 < t.dz, z > 0};
#pragma unroll
            for (int d = 0; d < 6; d++) {
                if (!ok[d]) continue;
                const int64_t n = base + x + off[d];
                const int nv = data[n];
                if (out[n] != fill && nv >= t0 && nv <= t1) m[d] |= 1u << e;
            }
        }
        const int64_t plane = total;
#pragma unroll
        for (int d = 0; d < 6; d++) edges[d * plane + i] = (uint8_t)m[d];
    }
}

// seeds whose bits are set no matter what the data says (floodfill.rs:21, floodfill_py.rs:30: `out[seed] = fill` and the
// seed is expanded unconditionally); `cand` may be NULL (directed floods have no candidate plane)
__global__ void k_flood_seed_forced(Tiles t, const int64_t *__restrict__ seeds, int64_t nseeds,
                                    unsigned long long *__restrict__ cand, unsigned long long *__restrict__ reached,
                                    uint8_t *__restrict__ dirty) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= nseeds) return;
    const int64_t x = seeds[3 * n], y = seeds[3 * n + 1], z = seeds[3 * n + 2];
    const int64_t w = (z * t.dy + y) * t.wx + (x >> 6);
    const unsigned long long bit = 1ull << (x & 63);
    if (cand) atomicOr(&cand[w], bit);
    atomicOr(&reached[w], bit);
    mark_tile_nbhd(t, dirty, z / TZ, y / TY, x >> 6);
}

// ---- apply: out[v] = fill where reached ---------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_flood_apply(Tiles t, const uint8_t *__restrict__ reached, T *__restrict__ out,
                                                     T fill) {
    const int64_t bpr = t.wx * 8;
    const int64_t total = t.dz * t.dy * bpr;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const bool aligned8 = ((uintptr_t)out & 7) == 0 && (t.dx & 7) == 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const unsigned m = reached[i];
        if (!m) continue;
        const int64_t row = i / bpr, q = i - row * bpr;
        T *o = out + row * t.dx + q * 8;
        if (sizeof(T) == 1 && m == 0xffu && aligned8) { // inside a filled region: one 8-byte store
            *reinterpret_cast<unsigned long long *>(o) = 0x0101010101010101ull * (unsigned long long)(uint8_t)fill;
            continue;
        }
#pragma unroll
        for (int e = 0; e < 8; e++)
            if (m >> e & 1u) o[e] = fill; // reached bits never exist beyond dx
    }
}

// byte targets with dx % 64 == 0 (rows are whole words, the bit volume is one flat array): one lane = 16 voxels =
// two bytes of reached bits -> one 16-byte store (a read-modify-write of the lane's own 16 bytes on a partial chunk)
__global__ __launch_bounds__(256) void k_flood_apply16(const uint16_t *__restrict__ reached, int64_t nchunks,
                                                       uint4 *__restrict__ out, uint8_t fill) {
    const int64_t stride = (int64_t)gridDim.x * 1024;
    const unsigned int f4 = 0x01010101u * fill;
    // four chunks per lane, 256 apart: the four bit loads (and the loads of the partial chunks' bytes) are in flight
    // together, and every store instruction of a wave writes 1 KB of consecutive bytes
    for (int64_t i0 = (int64_t)blockIdx.x * 1024 + threadIdx.x; i0 < nchunks; i0 += stride) {
        unsigned int m[4];
        uint4 o[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t i = i0 + u * 256;
            m[u] = i < nchunks ? reached[i] : 0u;
            o[u] = make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (m[u] && m[u] != 0xffffu) o[u] = out[i0 + u * 256];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!m[u]) continue;
            uint4 v = make_uint4(f4, f4, f4, f4);
            if (m[u] != 0xffffu) {
                // bit e of m -> byte e: spread 4 bits to 4 byte masks
                auto blend = [&](unsigned int old, unsigned int bits4) {
                    const unsigned int sel = ((bits4 & 1u) * 0xffu) | ((bits4 >> 1 & 1u) * 0xff00u) |
                                             ((bits4 >> 2 & 1u) * 0xff0000u) | ((bits4 >> 3 & 1u) * 0xff000000u);
                    return (old & ~sel) | (f4 & sel);
                };
                v.x = blend(o[u].x, m[u] & 15u);
                v.y = blend(o[u].y, m[u] >> 4 & 15u);
                v.z = blend(o[u].z, m[u] >> 8 & 15u);
                v.w = blend(o[u].w, m[u] >> 12 & 15u);
            }
            out[i0 + u * 256] = v;
        }
    }
}

// k_flood_apply16 for a mask whose bytes are KNOWN: v_in where `inside` (same layout as `reached`) has a bit, 0 elsewhere.  Every
// byte of a chunk with a reached bit is then a function of the two bit fields -- v_sel where reached, else v_in where inside,
// else 0 -- so the lane loads both fields together and stores; no byte of `out` is read (k_flood_apply16 loads a partial
// chunk's 16 bytes after its bits have arrived: a second, dependent round trip).  Chunks without a reached bit are not written
// -- unless ALL: then `out` holds nothing yet (a plane-only threshold) and every chunk is written, `reached` may be NULL (no
// bit), and a wave's four stores are 1 KiB contiguous each.
// WHEN (ivx::ApplyWhen, levels_write.h, with the body both this kernel and marching cubes' k_mc_count_write run): the launch
// was queued before the flood's end was known and goes ahead only if the next round's list is empty.
template <bool ALL>
__global__ __launch_bounds__(256) void k_flood_apply_levels16(const uint16_t *__restrict__ reached, const uint16_t *__restrict__ inside,
                                                              int64_t nchunks, uint4 *__restrict__ out, uint8_t v_in, uint8_t v_sel,
                                                              ApplyWhen when) {
    if (ivx::apply_when_skips(when)) return;
    const int64_t stride = (int64_t)gridDim.x * 1024;
    const unsigned int in4 = 0x01010101u * v_in, sel4 = 0x01010101u * v_sel;
    for (int64_t i0 = (int64_t)blockIdx.x * 1024 + threadIdx.x; i0 < nchunks; i0 += stride) {
        ivx::LevelsWords w;
        ivx::levels_load<ALL>(reached, inside, nchunks, i0, w);
        ivx::levels_store<ALL>(w, nchunks, i0, out, in4, sel4);
    }
}

// out[v] = fill AND mask[v] = select where reached: floodfill_threshold's `out` plus the caller's
// `mask[out_mask.astype(bool)] = 254` (styles.py:3214) in one pass over the reached bits
__global__ __launch_bounds__(256) void k_flood_apply2(Tiles t, const uint8_t *__restrict__ reached, uint8_t *__restrict__ out,
                                                      uint8_t fill, uint8_t *__restrict__ mask, uint8_t select) {
    const int64_t bpr = t.wx * 8;
    const int64_t total = t.dz * t.dy * bpr;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const bool aligned8 = (((uintptr_t)out | (uintptr_t)mask) & 7) == 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const unsigned m = reached[i];
        if (!m) continue;
        const int64_t row = i / bpr, q = i - row * bpr;
        const int64_t base = row * t.dx + q * 8;
        if (m == 0xffu && ((t.dx & 7) == 0) && aligned8) { // inside a filled region: two 8-byte stores
            *reinterpret_cast<unsigned long long *>(out + base) = 0x0101010101010101ull * fill;
            *reinterpret_cast<unsigned long long *>(mask + base) = 0x0101010101010101ull * select;
            continue;
        }
#pragma unroll
        for (int e = 0; e < 8; e++)
            if (m >> e & 1u) {
                out[base + e] = fill;
                mask[base + e] = select;
            }
    }
}

__global__ __launch_bounds__(256) void k_flood_count(const unsigned long long *__restrict__ bits, int64_t nwords,
                                                     unsigned long long *__restrict__ total) {
    unsigned long long s = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += stride) s += __popcll(bits[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
}

static inline int grid_for(int64_t n) {
    const int64_t b = ivx::cdiv(n, 256);
    return (int)(b < 1 ? 1 : (b < 32768 ? b : 32768));
}

template <typename T>
static int run_candidates(const Tiles &t, const void *data, double t0, double t1, const uint8_t *bar, int bar_mode,
                          double fill, uint8_t *cand, hipStream_t st) {
    const int64_t total = t.dz * t.dy * t.wx * 8;
    if (!total) return IVX_OK;
    if (sizeof(T) == 2 && t.dx % 64 == 0 && (((uintptr_t)data | (uintptr_t)bar | (uintptr_t)cand) & 15) == 0) {
        // rows are whole words, so the bit volume is one flat array of 16-voxel chunks
        const int64_t nchunks = t.dz * t.dy * t.dx / 16;
        const int64_t blocks = ivx::cdiv(nchunks, 256);
        const int gg = (int)(blocks < 16384 ? blocks : 16384);
        const short8_t *d8 = (const short8_t *)data;
        const uint4 *b4 = (const uint4 *)bar;
        uint16_t *c16 = (uint16_t *)cand;
        if (bar_mode == 0) hipLaunchKernelGGL((k_flood_candidates16<T, 0>), dim3(gg), dim3(256), 0, st, d8, b4, nchunks, t0, t1, fill, c16);
        else if (bar_mode == 1) hipLaunchKernelGGL((k_flood_candidates16<T, 1>), dim3(gg), dim3(256), 0, st, d8, b4, nchunks, t0, t1, fill, c16);
        else hipLaunchKernelGGL((k_flood_candidates16<T, 2>), dim3(gg), dim3(256), 0, st, d8, b4, nchunks, t0, t1, fill, c16);
        IVX_LAUNCH_CHECK();
        return IVX_OK;
    }
    const int g = grid_for(total);
    if (bar_mode == 0)
        hipLaunchKernelGGL((k_flood_candidates<T, 0>), dim3(g), dim3(256), 0, st, (const T *)data, bar, t, t0, t1, fill, cand);
    else if (bar_mode == 1)
        hipLaunchKernelGGL((k_flood_candidates<T, 1>), dim3(g), dim3(256), 0, st, (const T *)data, bar, t, t0, t1, fill, cand);
    else
        hipLaunchKernelGGL((k_flood_candidates<T, 2>), dim3(g), dim3(256), 0, st, (const T *)data, bar, t, t0, t1, fill, cand);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

} // namespace

extern "C" int ivx_flood_bits_bytes(const ivx_flood_plan *p, size_t *nbytes) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    *nbytes = al256((size_t)(t.dz * t.dy * t.wx) * 8);
    return IVX_OK;
}

extern "C" int ivx_flood_scratch_bytes(const ivx_flood_plan *p, size_t *nbytes) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    *nbytes = make_fscratch(t).total;
    return IVX_OK;
}

// strct (sshape dims <= 3 each, centre offset dim/2: floodfill.rs:108-110) -> 27-bit mask in 3x3x3 offset space
extern "C" int ivx_flood_strct_bits(const uint8_t *strct, const int64_t sshape[3], uint32_t *bits) {
    IVX_REQUIRE(strct && sshape, IVX_EINVAL, "flood: strct is NULL");
    uint32_t b = 0;
    for (int a = 0; a < 3; a++)
        IVX_REQUIRE(sshape[a] >= 1 && sshape[a] <= 3, IVX_EINVAL, "flood: structuring element dims must be 1..3 (got %lld)",
                    (long long)sshape[a]);
    const int64_t oz = sshape[0] / 2, oy = sshape[1] / 2, ox = sshape[2] / 2;
    for (int64_t kk = 0; kk < sshape[0]; kk++)
        for (int64_t jj = 0; jj < sshape[1]; jj++)
            for (int64_t ii = 0; ii < sshape[2]; ii++)
                if (strct[(kk * sshape[1] + jj) * sshape[2] + ii]) {
                    const int64_t dz = kk - oz + 1, dy = jj - oy + 1, dx = ii - ox + 1;
                    b |= 1u << (dz * 9 + dy * 3 + dx);
                }
    *bits = b;
    return IVX_OK;
}

extern "C" int ivx_dev_flood_candidates(const ivx_flood_plan *p, int dtype, const void *data, double t0, double t1,
                                        const uint8_t *barrier, int barrier_mode, double fill, uint64_t *cand,
                                        void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    IVX_REQUIRE(barrier_mode >= 0 && barrier_mode <= 2, IVX_EINVAL, "flood: barrier_mode");
    IVX_REQUIRE(barrier_mode != 1 || barrier, IVX_EINVAL, "flood: barrier array missing");
    hipStream_t st = ivx::S(stream);
    switch (dtype) {
    case IVX_I16: return run_candidates<int16_t>(t, data, t0, t1, barrier, barrier_mode, fill, (uint8_t *)cand, st);
    case IVX_U8: return run_candidates<uint8_t>(t, data, t0, t1, barrier, barrier_mode, fill, (uint8_t *)cand, st);
    case IVX_U16: return run_candidates<uint16_t>(t, data, t0, t1, barrier, barrier_mode, fill, (uint8_t *)cand, st);
    case IVX_F64: return run_candidates<double>(t, data, t0, t1, barrier, barrier_mode, fill, (uint8_t *)cand, st);
    }
    ivx::set_error("flood: unsupported dtype %d", dtype);
    return IVX_EINVAL;
}

extern "C" int ivx_dev_flood_candidates_ranges(const ivx_flood_plan *p, const int16_t *data, double t0, double t1,
                                               const uint8_t *barrier, int barrier_mode, double fill,
                                               const uint32_t *ranges, uint64_t *cand, void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    IVX_REQUIRE(barrier_mode == 0 || barrier_mode == 1, IVX_EINVAL, "flood: candidates_ranges: barrier_mode 0 or 1");
    IVX_REQUIRE(barrier_mode != 1 || barrier, IVX_EINVAL, "flood: barrier array missing");
    IVX_REQUIRE(t.dx % 64 == 0 && (((uintptr_t)data | (uintptr_t)barrier | (uintptr_t)cand) & 15) == 0 && ((uintptr_t)ranges & 3) == 0,
                IVX_EINVAL, "flood: candidates_ranges needs dx %% 64 == 0, 16-byte aligned buffers and 4-byte aligned records "
                            "(use ivx_dev_flood_candidates)");
    const int64_t nchunks = t.dz * t.dy * t.dx / 16;
    if (!nchunks) return IVX_OK;
    IVX_REQUIRE(data && ranges && cand, IVX_EINVAL, "flood: candidates_ranges: null argument");
    const int64_t blocks = ivx::cdiv(nchunks, 256);
    const int gg = (int)(blocks < 16384 ? blocks : 16384);
    hipStream_t st = ivx::S(stream);
    if (barrier_mode == 0)
        hipLaunchKernelGGL(k_flood_candidates_words, dim3(words_grid(nchunks / 4)), dim3(WORDS_PER_WG), 0, st, (const short8_t *)data,
                           (const unsigned *)ranges, nchunks / 4, t0, t1, (unsigned long long *)cand);
    else
        hipLaunchKernelGGL(k_flood_candidates16_ranges, dim3(gg), dim3(256), 0, st, (const short8_t *)data, (const uint4 *)barrier,
                           (const unsigned *)ranges, nchunks, t0, t1, fill, (uint16_t *)cand);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_flood_seed(const ivx_flood_plan *p, int dtype, const void *data, double t0, double t1,
                                  const int64_t *seeds_xyz, int64_t nseeds, uint64_t *cand, uint64_t *reached,
                                  void *scratch_, void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    for (int64_t n = 0; n < nseeds; n++) {
        const int64_t x = seeds_xyz[3 * n], y = seeds_xyz[3 * n + 1], z = seeds_xyz[3 * n + 2];
        IVX_REQUIRE(x >= 0 && y >= 0 && z >= 0 && x < t.dx && y < t.dy && z < t.dz, IVX_ERANGE,
                    "flood: seed (%lld,%lld,%lld) outside volume (%lld,%lld,%lld) [x,y,z]", (long long)x, (long long)y,
                    (long long)z, (long long)t.dx, (long long)t.dy, (long long)t.dz);
    }
    const FScratch s = make_fscratch(t);
    char *scr = (char *)scratch_;
    hipStream_t st = ivx::S(stream);
    ivx::ccl_invalidate(scratch_); // a seed may add a bit to the candidate plane
    if (nseeds <= 16) { // the usual case (one click = one seed): seeds travel as kernel arguments, no staging, no sync
        SeedPack sp;
        sp.n = (int)nseeds;
        for (int64_t n = 0; n < nseeds; n++)
            for (int q = 0; q < 3; q++) sp.xyz[n][q] = seeds_xyz[3 * n + q];
        unsigned long long *c = (unsigned long long *)cand, *r = (unsigned long long *)reached;
        uint8_t *dirty = (uint8_t *)(scr + s.off_dirty0);
        if (nseeds == 0) return IVX_OK;
        switch (dtype) {
        case IVX_I16: hipLaunchKernelGGL(k_flood_seed_args<int16_t>, dim3(1), dim3(64), 0, st, (const int16_t *)data, t, t0, t1, sp, c, r, dirty); break;
        case IVX_U8: hipLaunchKernelGGL(k_flood_seed_args<uint8_t>, dim3(1), dim3(64), 0, st, (const uint8_t *)data, t, t0, t1, sp, c, r, dirty); break;
        case IVX_U16: hipLaunchKernelGGL(k_flood_seed_args<uint16_t>, dim3(1), dim3(64), 0, st, (const uint16_t *)data, t, t0, t1, sp, c, r, dirty); break;
        case IVX_F64: hipLaunchKernelGGL(k_flood_seed_args<double>, dim3(1), dim3(64), 0, st, (const double *)data, t, t0, t1, sp, c, r, dirty); break;
        default: ivx::set_error("flood: unsupported dtype %d", dtype); return IVX_EINVAL;
        }
        IVX_LAUNCH_CHECK();
        return IVX_OK;
    }
    int64_t *d_seeds = (int64_t *)(scr + s.off_seeds);
    for (int64_t b = 0; b < nseeds; b += (int64_t)SEED_CHUNK) {
        const int64_t m = nseeds - b < (int64_t)SEED_CHUNK ? nseeds - b : (int64_t)SEED_CHUNK;
        IVX_HIP(hipMemcpyAsync(d_seeds, seeds_xyz + 3 * b, (size_t)m * 24, hipMemcpyHostToDevice, st));
        const int g = (int)ivx::cdiv(m, 256);
        unsigned long long *c = (unsigned long long *)cand, *r = (unsigned long long *)reached;
        uint8_t *dirty = (uint8_t *)(scr + s.off_dirty0);
        switch (dtype) {
        case IVX_I16: hipLaunchKernelGGL(k_flood_seed<int16_t>, dim3(g), dim3(256), 0, st, (const int16_t *)data, t, t0, t1, d_seeds, m, c, r, dirty); break;
        case IVX_U8: hipLaunchKernelGGL(k_flood_seed<uint8_t>, dim3(g), dim3(256), 0, st, (const uint8_t *)data, t, t0, t1, d_seeds, m, c, r, dirty); break;
        case IVX_U16: hipLaunchKernelGGL(k_flood_seed<uint16_t>, dim3(g), dim3(256), 0, st, (const uint16_t *)data, t, t0, t1, d_seeds, m, c, r, dirty); break;
        case IVX_F64: hipLaunchKernelGGL(k_flood_seed<double>, dim3(g), dim3(256), 0, st, (const double *)data, t, t0, t1, d_seeds, m, c, r, dirty); break;
        default: ivx::set_error("flood: unsupported dtype %d", dtype); return IVX_EINVAL;
        }
        IVX_LAUNCH_CHECK();
        IVX_HIP(hipStreamSynchronize(st)); // d_seeds is reused by the next chunk; seeds_xyz is pageable host memory
    }
    return IVX_OK;
}

// one launch instead of two memsets: reached plane = 0, scratch head (dirty flags, counters) = 0
__global__ __launch_bounds__(256) void k_flood_clear(uint4 *__restrict__ reached, int64_t n16, uint4 *__restrict__ head,
                                                     int64_t h16) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16 + h16; i += stride) {
        if (i < n16) reached[i] = z;
        else head[i - n16] = z;
    }
}

extern "C" int ivx_dev_flood_clear(const ivx_flood_plan *p, uint64_t *reached, void *scratch, void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    const FScratch s = make_fscratch(t);
    const size_t nb = (size_t)(t.dz * t.dy * t.wx) * 8;
    if ((nb | s.off_seeds | (uintptr_t)reached | (uintptr_t)scratch) & 15) { // odd sizes: plain memsets
        IVX_HIP(hipMemsetAsync(reached, 0, nb, ivx::S(stream)));
        IVX_HIP(hipMemsetAsync(scratch, 0, s.off_seeds, ivx::S(stream)));
    } else {
        const int64_t total = (int64_t)((nb + s.off_seeds) / 16);
        const int64_t blocks = ivx::cdiv(total, 256);
        hipLaunchKernelGGL(k_flood_clear, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, ivx::S(stream),
                           (uint4 *)reached, (int64_t)(nb / 16), (uint4 *)scratch, (int64_t)(s.off_seeds / 16));
        IVX_LAUNCH_CHECK();
    }
    ivx::ccl_invalidate(scratch);
    return IVX_OK;
}

// ---- gate: background work that should start once the flood's busy rounds are over --------------------------------------
// ivx_dev_flood_arm_gate(scratch, word, value, below): in the next flood on `scratch` the first round that starts with
// fewer than `below` tiles stores `value` to the device word `word` (and so does the end of the flood, if no round did).  ivx_dev_gate_wait(word, value, timeout, stream) parks `stream` behind a one-wave
// kernel that polls the word (bounded: it gives up after `timeout_us`).  Together: work queued on a second, low-priority
// stream runs under the latency-bound tail of the flood instead of competing with its throughput-bound head.
struct GateArm {
    unsigned int *word;
    unsigned int value, below;
};
static std::map<const void *, GateArm> g_gates;
static std::mutex g_gates_mu;

__global__ void k_gate_wait(const unsigned int *word, unsigned int value, unsigned long long timeout_ticks) {
    if (threadIdx.x) return;
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != value) {
        if (wall_clock64() - t0 > timeout_ticks) break; // never hang: start late rather than never
        __builtin_amdgcn_s_sleep(32);
    }
}
__global__ void k_gate_set(unsigned int *word, unsigned int value) {
    if (threadIdx.x == 0) __hip_atomic_store(word, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// mode (ivx::FloodMode, ivx_internal.h): FLOOD_DIRECTED -- `cand` = the six edge planes of ivx_dev_flood_edges_auto;
// FLOOD_LINEAR -- the three arc planes of a cost level (k_costlevels.hip).  Both run on the rounds engine only: the coarse
// pass and the union-find escape rely on symmetric lattice adjacency.
// `fresh` (may be NULL): the flood starts from these seeds on a plane whose old contents are dead (ivx_dev_flood_grow) --
// the coarse pass then does the clearing and the seeding as well
struct Fresh {
    int dtype;
    const void *data;
    double t0, t1;
    SeedPack sp;
};
// IVX_FLOOD_MODE: "rounds" (default, and what any other value means) = tile frontier, one launch per round, with an escape
// to the union-find path when a flood needs more than CCL_ESCAPE_ROUNDS rounds (serpentine / maze-like regions); "ccl" =
// run-based union-find from the start (k_ccl.hip; no frontier, flat cost).  Measured at 512^3 on the bench blob (20
// rounds): rounds 0.74 ms, ccl 0.86 ms (and 1.4 ms, with 2.7x more tile visits, for a single launch that pulled tiles from a
// device-side ticket queue: removed).
static bool flood_mode_ccl() {
    static const bool ccl = [] {
        const char *e = getenv("IVX_FLOOD_MODE");
        return e && !strcmp(e, "ccl");
    }();
    return ccl;
}
static bool coarse_ok(const Tiles &t, ivx::FloodMode mode) {
    static const bool coarse_on = [] {
        const char *e = getenv("IVX_FLOOD_COARSE");
        return !(e && e[0] == '0');
    }();
    // standard structures only, tile grid small enough for one workgroup's LDS
    return coarse_on && mode == ivx::FLOOD_SYMMETRIC && t.conn != 0 && t.wx <= 64 && (t.nty + 2) * (t.ntz + 2) <= CROWS_MAX &&
           t.nty * t.ntz <= (int64_t)CT * CRP;
}
// the block width of the coarse graph for this tile grid (see Blocks)
static Blocks coarse_blocks(const Tiles &t) {
    static const int bxs_env = [] {
        const char *e = getenv("IVX_FLOOD_BLOCK"); // 16 / 32 / 64: force a coarser block (A/B measurements)
        return e ? atoi(e) : 0;
    }();
    Blocks bk;
    bk.bxs = 16;
    while (bk.bxs < 64 && ((64 / bk.bxs) * t.wx > 64 || bk.bxs < bxs_env)) bk.bxs *= 2;
    bk.q = 64 / bk.bxs;
    return bk;
}
// lanes of k_flood_coarse's one workgroup: one row of tiles per lane up to 1024 lanes, then up to CRP rows per lane
// (128..1024 lanes measured equal)
static int coarse_lanes(const Tiles &t) {
    int ct = 64;
    while (ct < CT && ct < t.nty * t.ntz) ct *= 2;
    return ct;
}
// The coarse pass's three launches (see k_flood_coarse): blocks of 16 / 32 / 64 x 16 x 16 voxels, the finest whose row fits
// one word.  FRESH: the clearing and the seeding of `f` ride along; otherwise `f` carries no seeds.
template <bool FRESH>
static int coarse_pass(const Tiles &t, const FScratch &s, char *scr, const uint64_t *cand, uint64_t *reached, const Fresh &f,
                       int ncnt, hipStream_t st) {
    const Blocks bk = coarse_blocks(t);
    uint8_t *dirty0 = (uint8_t *)(scr + s.off_dirty0), *dirty1 = (uint8_t *)(scr + s.off_dirty1);
    unsigned int *cnt = (unsigned int *)(scr + s.off_cnt), *list0 = (unsigned int *)(scr + s.off_list0);
    unsigned long long *rowF = (unsigned long long *)(scr + s.off_full), *rowW = (unsigned long long *)(scr + s.off_whole);
    unsigned int *seed_ok = (unsigned int *)(scr + s.off_status) + 8;
    const unsigned groups = (unsigned)(t.nty * t.ntz);
    const int ct = coarse_lanes(t);
    hipLaunchKernelGGL(k_flood_block_flags<FRESH>, dim3(groups), dim3(256), 0, st, t, bk, (unsigned long long *)cand,
                       (const unsigned long long *)reached, dirty0, dirty1, rowF, rowW, cnt, ncnt, f.sp, f.dtype, f.data, f.t0,
                       f.t1, seed_ok);
    IVX_LAUNCH_CHECK();
    auto coarse = t.conn == 26 ? k_flood_coarse<26, FRESH> : t.conn == 18 ? k_flood_coarse<18, FRESH> : k_flood_coarse<6, FRESH>;
    hipLaunchKernelGGL(coarse, dim3(1), dim3(ct), 0, st, t, bk, (const unsigned long long *)rowF, rowW, f.sp,
                       (const unsigned int *)seed_ok);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_flood_block_apply<FRESH>, dim3(groups), dim3(256), 0, st, t, bk, (const unsigned long long *)cand,
                       (unsigned long long *)reached, (const unsigned long long *)rowW, dirty0, list0, cnt, f.sp,
                       (const unsigned int *)seed_ok);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}
// the most workgroups a round is launched with: 6 workgroups per CU are resident (80 VGPRs)
static unsigned round_grid_cap(const Tiles &t) { return (unsigned)(t.ntiles < 1536 ? t.ntiles : 1536); }
// Spin on the first word of a pinned progress line until `done(word)`, at most `spins` polls; then take the safe path once:
// synchronise the stream and look again.  `never`: the error when even that word does not satisfy `done`.
template <typename Done>
static int poll_line(volatile unsigned long long *line, long spins, hipStream_t st, Done done, const char *never,
                     unsigned long long *word) {
    for (long n = 0; n < spins; n++) {
        *word = __atomic_load_n((const unsigned long long *)line, __ATOMIC_ACQUIRE);
        if (done(*word)) return IVX_OK;
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    IVX_HIP(hipStreamSynchronize(st));
    *word = __atomic_load_n((const unsigned long long *)line, __ATOMIC_ACQUIRE);
    IVX_REQUIRE(done(*word), IVX_EHIP, "%s", never);
    return IVX_OK;
}
// k_flood_apply_levels16's launch for ivx_dev_flood_apply_levels (ALL false), ivx_dev_mask_from_planes (ALL true) and the
// flood's own early launch of either; levels_check() is the argument check of the two
static int levels_check(const Tiles &t, const uint64_t *reached, const uint64_t *inside_bits, const uint8_t *mask, int v_in, int v_sel,
                        bool all) {
    if (all) {
        IVX_REQUIRE(inside_bits && mask, IVX_EINVAL, "mask_from_planes: null plane or mask");
        IVX_REQUIRE(t.dx % 64 == 0 && ((uintptr_t)mask & 15) == 0 && (((uintptr_t)inside_bits | (uintptr_t)reached) & 7) == 0, IVX_EINVAL,
                    "mask_from_planes: rows of whole 64-voxel words, a 16-byte aligned mask and 8-byte aligned planes only");
        IVX_REQUIRE(v_in >= 0 && v_in <= 255 && v_sel >= 0 && v_sel <= 255, IVX_EINVAL, "mask_from_planes: levels are bytes");
    } else {
        IVX_REQUIRE(reached && inside_bits && mask, IVX_EINVAL, "flood_apply_levels: null plane or mask");
        IVX_REQUIRE(t.dx % 64 == 0 && ((uintptr_t)mask & 15) == 0, IVX_EINVAL,
                    "flood_apply_levels: rows of whole 64-voxel words and a 16-byte aligned mask only");
        IVX_REQUIRE(v_in >= 0 && v_in <= 255 && v_sel >= 0 && v_sel <= 255, IVX_EINVAL, "flood_apply_levels: levels are bytes");
    }
    return IVX_OK;
}
// `ride`: the launch is marching cubes' k_mc_count_write, which does this write and the count of the piece `ride->p`
struct McRide {
    const ivx_mc_params *p;
    void *scratch;
};
static int launch_levels(const Tiles &t, const uint64_t *reached, const uint64_t *inside, uint8_t *mask, int v_in, int v_sel, bool all,
                         const ApplyWhen &when, hipStream_t st, const McRide *ride = nullptr) {
    const int64_t nchunks = t.dz * t.dy * t.dx / 16;
    if (!nchunks) return IVX_OK;
    if (ride) return ivx::mc_ride_launch(ride->p, ride->scratch, reached, inside, nchunks, mask, v_in, v_sel, all, when, st);
    const int64_t blocks = ivx::cdiv(nchunks, 1024);
    auto k = all ? k_flood_apply_levels16<true> : k_flood_apply_levels16<false>;
    hipLaunchKernelGGL(k, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, (const uint16_t *)reached,
                       (const uint16_t *)inside, nchunks, (uint4 *)mask, (uint8_t)v_in, (uint8_t)v_sel, when);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}
// The default look-ahead: how many rounds the host keeps queued beyond the newest one it has seen start, by that round's
// list length.  Every round queued ahead when the first empty one reports is a launch for nothing, so the fewer the better
// -- as long as the host can queue the next round before the one it has just seen start is over.  A round of
// AHEAD_LONG_LIST tiles or more runs longer than the host's way from the poll to the next launch, so nothing needs to be
// queued behind it yet; behind a shorter one (the flood's tail: a few microseconds each) one round waits ready.
// profiles/flood_end_ab.md has the measurements of the fixed values 0 .. 3 against this.
constexpr unsigned AHEAD_LONG_LIST = 384u;
static int default_look_ahead(unsigned n_list) { return n_list >= AHEAD_LONG_LIST ? 0 : 1; }
// The write ivx_dev_flood_grow_select wants behind the flood.  Between the start of the first empty round and the start of a
// kernel the host launches on seeing it lie ~15 us (the report's way to the host, the launch's way to the GPU), whatever
// the host does in between; the rounds queued ahead only fill that time.  So when the lists are running out -- the round
// just seen has fewer than EARLY_BELOW tiles and at most half of the one seen before -- the flood queues the write itself,
// behind the rounds already in the stream, as a launch that looks at the next round's list length on the device
// (ApplyWhen): empty, and the write runs where the first idle round would have; not empty, and it costs ~3 us.  One such
// launch is outstanding at a time and at most EARLY_TRIES per flood, so a flood whose lists shrink and recover pays
// ~6 us at most.  `written` comes back true when such a launch went ahead: the caller then has nothing left to queue.
// `ride`: every launch of the write for this flood carries the count (McRide), so the one that goes ahead counts.  `plain`
// comes back true when the flood took the union-find path instead of ending on its rounds: the write is then queued as
// before, and nothing of marching cubes behind it.
struct EarlyWrite {
    const ivx_flood_write *w;
    bool written;
    const McRide *ride = nullptr;
    bool plain = false;
};
constexpr unsigned EARLY_BELOW = 96u;
constexpr int EARLY_TRIES = 2;
// `look_ahead` < 0: default_look_ahead() of every round seen; IVX_FLOOD_BATCH (0 .. BATCH), if set, overrides either
static int flood_run_impl(const ivx_flood_plan *p, const uint64_t *cand, ivx::FloodMode mode, uint64_t *reached, void *scratch_,
                          int *rounds, void *stream, const Fresh *fresh = nullptr, int look_ahead = -1, EarlyWrite *early = nullptr) {
    const bool sym = mode == ivx::FLOOD_SYMMETRIC;
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    if (rounds) *rounds = 0;
    hipStream_t st = ivx::S(stream);
    GateArm arm = {nullptr, 0u, 0u};
    {
        std::lock_guard<std::mutex> lk(g_gates_mu);
        auto it = g_gates.find(scratch_);
        if (it != g_gates.end()) {
            arm = it->second;
            g_gates.erase(it);
        }
    }
    // whatever path the flood takes, the gate opens at the latest when it returns
    struct GateGuard {
        GateArm &a;
        hipStream_t st;
        ~GateGuard() {
            if (a.word) hipLaunchKernelGGL(k_gate_set, dim3(1), dim3(64), 0, st, a.word, a.value);
        }
    } gate_guard = {arm, st};
    if (t.ntiles == 0) return IVX_OK;
    const FScratch s = make_fscratch(t);
    char *scr = (char *)scratch_;
    uint8_t *dirty[2] = {(uint8_t *)(scr + s.off_dirty0), (uint8_t *)(scr + s.off_dirty1)};
    unsigned int *cnt = (unsigned int *)(scr + s.off_cnt);
    constexpr int CCL_ESCAPE_ROUNDS = 48;
    if (sym && flood_mode_ccl() && ivx::ccl_supported(p->strct_bits)) {
        if (rounds) *rounds = 1;
        // the dirty-tile list is not used by this path; keep it empty so a later frontier run starts clean
        IVX_HIP(hipMemsetAsync(dirty[0], 0, (size_t)t.ntiles, st));
        if (early) early->plain = true;
        return ivx::ccl_run(p, cand, reached, scratch_, st);
    }
    int total_rounds = 0;
    unsigned int *list[2] = {(unsigned int *)(scr + s.off_list0), (unsigned int *)(scr + s.off_list1)};
    // Counters live in a ring of RING dwords indexed by the round number: round r reads cnt[r % RING] (entries of its
    // list), appends to cnt[(r+1) % RING] and clears cnt[(r+2) % RING] for the round after -- no host-side resets, so
    // rounds can be queued back to back.  Every round reports the length of its list to a pinned progress line as it
    // starts; the host keeps `ahead` rounds queued beyond the newest round it has seen start (waiting for a round's END
    // before launching the next would leave the GPU idle for 35-45 us) and stops at the first round that starts empty.
    // `ahead` may be 0: the next round is then queued while the one just seen runs.  The `ahead` rounds queued behind
    // the first empty one find empty lists too: ~4.4 us each that the step's next kernel waits behind, which is why
    // the look-ahead is kept as short as the host's reaction allows (default_look_ahead).
    constexpr int RING = 2 * BATCH;
    static const int env_ahead = [] { // IVX_FLOOD_BATCH: a fixed look-ahead for every flood, 0 .. BATCH (A/B measurements)
        const char *e = getenv("IVX_FLOOD_BATCH");
        if (!e || !*e) return -1;
        const int v = atoi(e);
        return v < 0 ? 0 : (v > BATCH ? BATCH : v);
    }();
    const int fixed_ahead = env_ahead >= 0 ? env_ahead : (look_ahead > BATCH ? BATCH : look_ahead);
    // before any round has reported its length is not known: one round waits behind the first
    int ahead = fixed_ahead >= 0 ? fixed_ahead : 1;
    if (coarse_ok(t, mode)) {
        static const Fresh no_seeds = {0, nullptr, 0.0, 0.0, {{}, 0}};
        rc = fresh ? coarse_pass<true>(t, s, scr, cand, reached, *fresh, CNT_CLEARED, st)
                   : coarse_pass<false>(t, s, scr, cand, reached, no_seeds, CNT_CLEARED, st);
        if (rc) return rc;
    } else {
        IVX_REQUIRE(!fresh, IVX_EINVAL, "flood: the fused start needs the coarse pass");
        IVX_HIP(hipMemsetAsync(cnt, 0, CNT_CLEARED * 4, st));
        hipLaunchKernelGGL(k_flood_build_list, dim3((unsigned)ivx::cdiv(t.ntiles, 256)), dim3(256), 0, st, t, dirty[0], list[0], cnt);
        IVX_LAUNCH_CHECK();
    }
    volatile unsigned long long *line = nullptr;
    uint32_t tag = 0;
    if ((rc = ivx::progress_line(st, &line, &tag))) return rc;
    const unsigned grid_max = round_grid_cap(t);
    // The rounds queued ahead are sized by the newest list length the host has seen: the lists shrink towards the end, and
    // dispatching 1536 workgroups that find nothing costs ~3 us more per round than dispatching 128 (a list that turns out
    // longer than the grid is still served: workgroups stride over it).
    unsigned grid = grid_max;
    int64_t queued = 0; // rounds launched so far
    auto round_kernel = mode == ivx::FLOOD_LINEAR ? k_flood_round_list<2> : mode == ivx::FLOOD_DIRECTED ? k_flood_round_list<1> : k_flood_round_list<0>;
    auto queue_round = [&]() -> int {
        const int r = (int)(queued % RING), cur = (int)(queued & 1);
        const unsigned int tr = (unsigned int)(tag << 24) | (unsigned int)((queued + 1) & 0xffffff);
        // every round carries the gate (arm.word): the first one with a short list opens it
        hipLaunchKernelGGL(round_kernel, dim3(grid), dim3(NT), 0, st, t, (const unsigned long long *)cand,
                           (unsigned long long *)reached, (const unsigned int *)list[cur], (const unsigned int *)(cnt + r), dirty[cur],
                           dirty[cur ^ 1], list[cur ^ 1], cnt + (r + 1) % RING, cnt + (r + 2) % RING, cnt,
                           (unsigned long long *)line, tr,
                           arm.word, arm.value, arm.below);
        IVX_LAUNCH_CHECK();
        queued++;
        return IVX_OK;
    };
    static const bool trace = getenv("IVX_FLOOD_TRACE") != nullptr;
    // the early write (EarlyWrite): the two kinds that are one launch of k_flood_apply_levels16 with arguments it accepts
    static const bool early_on = [] { // IVX_FLOOD_EARLY=0: the write only after the host has seen the end (A/B)
        const char *e = getenv("IVX_FLOOD_EARLY");
        return !(e && e[0] == '0');
    }();
    const bool early_all = early && early->w->kind == IVX_FLOOD_WRITE_MASK_FROM_PLANES;
    int early_left = 0;
    if (early_on && early && (early_all || early->w->kind == IVX_FLOOD_WRITE_APPLY_LEVELS) &&
        levels_check(t, reached, early->w->inside_bits, early->w->mask, early->w->v_in, early->w->v_sel, early_all) == IVX_OK)
        early_left = EARLY_TRIES;
    if (early_left) __atomic_store_n((unsigned long long *)line + 2, 0ull, __ATOMIC_RELEASE); // (a report of this tag's last turn)
    int64_t early_at = -1; // rounds in the stream in front of the outstanding early write, -1: none outstanding
    unsigned long long early_report = 0;
    bool early_seen = false; // its report has arrived
    unsigned int prev_list = 0xffffffffu;
    int64_t seen = 0; // rounds seen starting
    for (;;) {
        while (queued < seen + 1 + ahead)
            if ((rc = queue_round())) return rc;
        // wait for a round beyond `seen` to report; a few hundred ms without news: the safe path once
        unsigned long long v = 0;
        rc = poll_line(line, 20000000L, st,
                       [&](unsigned long long w) {
                           if (early_at >= 0 && __atomic_load_n((const unsigned long long *)line + 2, __ATOMIC_ACQUIRE) == early_report)
                               return early_seen = true;
                           return (uint32_t)(w >> 56) == tag && (int64_t)((w >> 32) & 0xffffffull) > seen;
                       },
                       "flood: the queued rounds never reported", &v);
        if (rc) return rc;
        if (early_seen) { // the early write is running: every round in front of it is complete, and the flood with them
            const unsigned long long u = __atomic_load_n((const unsigned long long *)line + 1, __ATOMIC_ACQUIRE);
            total_rounds = (uint32_t)(u >> 56) == tag ? (int)((u >> 32) & 0xffffffull) : 0;
            early->written = true;
            if (trace) fprintf(stderr, "ivx flood: the write behind round %lld went ahead (%d rounds with work)\n", (long long)early_at, total_rounds);
            break;
        }
        seen = (int64_t)((v >> 32) & 0xffffffull);
        const unsigned int n_list = (unsigned int)(v & 0xffffffffull);
        if (trace) fprintf(stderr, "ivx flood: round %lld starts with %u of %lld tiles (%lld queued)\n", (long long)seen, n_list,
                           (long long)t.ntiles, (long long)queued);
        if (n_list < arm.below) arm.word = nullptr; // that round has opened the gate: nothing left for the guard to do
        grid = n_list >= 384u ? grid_max : (n_list >= 96u ? (grid_max < 512u ? grid_max : 512u) : (grid_max < 128u ? grid_max : 128u));
        if (fixed_ahead < 0) ahead = default_look_ahead(n_list);
        if (n_list == 0) { // converged: word 1 holds the last round that had work (if any, and if it is ours)
            const unsigned long long u = __atomic_load_n((const unsigned long long *)line + 1, __ATOMIC_ACQUIRE);
            total_rounds = (uint32_t)(u >> 56) == tag ? (int)((u >> 32) & 0xffffffull) : 0;
            // an early write behind rounds that include the last one with work finds the next list empty: it goes (or went) ahead
            if (early_at >= 0 && total_rounds <= early_at) early->written = true;
            break;
        }
        if (early_at >= 0 && seen > early_at) early_at = -1; // the round behind it has work: it has returned at once
        if (early_left > 0 && early_at < 0 && n_list < EARLY_BELOW && n_list <= prev_list / 2u) {
            early_at = queued;
            early_left--;
            early_report = ((unsigned long long)tag << 56) | ((unsigned long long)(queued & 0xffffff) << 32) | 1ull;
            if (trace) fprintf(stderr, "ivx flood: write queued behind round %lld\n", (long long)queued);
            rc = launch_levels(t, reached, early->w->inside_bits, early->w->mask, early->w->v_in, early->w->v_sel, early_all,
                               ApplyWhen{cnt + queued % RING, (unsigned long long *)line, early_report}, st, early->ride);
            if (rc) return rc;
        }
        prev_list = n_list;
        total_rounds = (int)seen;
        if (sym && total_rounds >= CCL_ESCAPE_ROUNDS && ivx::ccl_supported(p->strct_bits)) {
            // long, thin region: stop paying one launch per tile hop -- every reached bit so far is correct, the
            // union-find path completes the components they belong to in one flat pass (the rounds already queued
            // keep flooding until then, which is harmless)
            IVX_HIP(hipMemsetAsync(dirty[0], 0, (size_t)t.ntiles, st));
            IVX_HIP(hipMemsetAsync(dirty[1], 0, (size_t)t.ntiles, st));
            if ((rc = ivx::ccl_run(p, cand, reached, scratch_, st))) return rc;
            total_rounds += 1;
            if (early) early->plain = true;
            break;
        }
        IVX_REQUIRE(total_rounds < (1 << 24) - 64, IVX_EHIP, "flood: did not converge");
    }
    if (rounds) *rounds = total_rounds;
    return IVX_OK;
}

// The entry points from before ivx_dev_flood_grow_select keep three rounds queued ahead, as every flood did until the
// default followed the list length: the watershed's cost levels run one short flood per level, each on the heels of the
// last, and the sharded step's floods are resumed round by round; both measured slower with the step's default
// (profiles/flood_end_ab.md section 6), which pays only together with the early write.
constexpr int AHEAD_CHAINED = 3;
int ivx::flood_run(const ivx_flood_plan *p, const uint64_t *planes, ivx::FloodMode mode, uint64_t *reached, void *scratch,
                   int *rounds, void *stream) {
    return flood_run_impl(p, planes, mode, reached, scratch, rounds, stream, nullptr, AHEAD_CHAINED);
}

extern "C" int ivx_dev_flood_run(const ivx_flood_plan *p, const uint64_t *cand, uint64_t *reached, void *scratch_,
                                 int *rounds, void *stream) {
    return flood_run_impl(p, cand, ivx::FLOOD_SYMMETRIC, reached, scratch_, rounds, stream, nullptr, AHEAD_CHAINED);
}
// does a flood of `nseeds` seeds take the fused start (clear and seed inside the coarse pass)?
static bool fused_start(const Tiles &t, int64_t nseeds) {
    static const bool fused_on = [] {
        const char *e = getenv("IVX_FLOOD_FUSED");
        return !(e && e[0] == '0');
    }();
    return fused_on && nseeds >= 1 && nseeds <= 16 && t.ntiles > 0 && !flood_mode_ccl() && coarse_ok(t, ivx::FLOOD_SYMMETRIC);
}
// clear + seed + run in one call: the flood of `seeds` over `cand` into a plane whose old contents are dead.  With at most
// 16 seeds and a standard structuring element the clearing and the seeding ride on the coarse pass (three launches before
// the rounds instead of five, no separate pass over the plane); otherwise the three calls run one after the other.
static int flood_grow_impl(const ivx_flood_plan *p, int dtype, const void *data, double t0, double t1, const int64_t *seeds_xyz,
                           int64_t nseeds, uint64_t *cand, uint64_t *reached, void *scratch_, int *rounds, void *stream,
                           int look_ahead, EarlyWrite *early = nullptr) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    IVX_REQUIRE(ivx::dtype_size(dtype), IVX_EINVAL, "flood: unsupported dtype %d", dtype);
    for (int64_t n = 0; n < nseeds; n++) {
        const int64_t x = seeds_xyz[3 * n], y = seeds_xyz[3 * n + 1], z = seeds_xyz[3 * n + 2];
        IVX_REQUIRE(x >= 0 && y >= 0 && z >= 0 && x < t.dx && y < t.dy && z < t.dz, IVX_ERANGE,
                    "flood: seed (%lld,%lld,%lld) outside volume (%lld,%lld,%lld) [x,y,z]", (long long)x, (long long)y,
                    (long long)z, (long long)t.dx, (long long)t.dy, (long long)t.dz);
    }
    if (!fused_start(t, nseeds)) {
        if ((rc = ivx_dev_flood_clear(p, reached, scratch_, stream))) return rc;
        if ((rc = ivx_dev_flood_seed(p, dtype, data, t0, t1, seeds_xyz, nseeds, cand, reached, scratch_, stream))) return rc;
        return flood_run_impl(p, cand, ivx::FLOOD_SYMMETRIC, reached, scratch_, rounds, stream, nullptr, look_ahead, early);
    }
    ivx::ccl_invalidate(scratch_);
    Fresh f;
    f.dtype = dtype;
    f.data = data;
    f.t0 = t0;
    f.t1 = t1;
    f.sp.n = (int)nseeds;
    for (int64_t n = 0; n < nseeds; n++)
        for (int q = 0; q < 3; q++) f.sp.xyz[n][q] = seeds_xyz[3 * n + q];
    return flood_run_impl(p, cand, ivx::FLOOD_SYMMETRIC, reached, scratch_, rounds, stream, &f, look_ahead, early);
}
extern "C" int ivx_dev_flood_grow(const ivx_flood_plan *p, int dtype, const void *data, double t0, double t1,
                                  const int64_t *seeds_xyz, int64_t nseeds, uint64_t *cand, uint64_t *reached, void *scratch_,
                                  int *rounds, void *stream) {
    return flood_grow_impl(p, dtype, data, t0, t1, seeds_xyz, nseeds, cand, reached, scratch_, rounds, stream, AHEAD_CHAINED);
}
// host only, for tests: default_look_ahead() of a round that starts with `n_list` tiles
extern "C" int ivx_flood_look_ahead(int64_t n_list, int32_t *look_ahead) {
    IVX_REQUIRE(look_ahead && n_list >= 0, IVX_EINVAL, "flood_look_ahead: NULL or negative argument");
    *look_ahead = default_look_ahead(n_list > 0xffffffffll ? 0xffffffffu : (unsigned)n_list);
    return IVX_OK;
}
extern "C" int ivx_dev_flood_visits(const ivx_flood_plan *p, const void *scratch_, uint32_t out[2], void *stream) {
    IVX_REQUIRE(scratch_ && out, IVX_EINVAL, "flood_visits: NULL argument");
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    out[0] = out[1] = 0u;
    if (t.ntiles == 0) return IVX_OK;
    const FScratch s = make_fscratch(t);
    hipStream_t st = ivx::S(stream);
    unsigned int w[CNT_CLEARED - STATS_AT];
    IVX_HIP(hipMemcpyAsync(w, (const char *)scratch_ + s.off_cnt + STATS_AT * 4, sizeof w, hipMemcpyDeviceToHost, st));
    IVX_HIP(hipStreamSynchronize(st));
    out[0] = w[0];
    for (int k = 0; k < HIST; k++) out[0] += w[HIST_AT - STATS_AT + k];
    out[1] = w[HIST_AT - STATS_AT];
    return IVX_OK;
}
// host only, for tests: the path ivx_dev_flood_grow takes for this plan and seed count, by the very functions that size
// its launches (no device call)
extern "C" int ivx_flood_describe(const ivx_flood_plan *p, int64_t nseeds, int32_t out[8]) {
    IVX_REQUIRE(out, IVX_EINVAL, "flood_describe: NULL argument");
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    for (int i = 0; i < 8; i++) out[i] = 0;
    if (coarse_ok(t, ivx::FLOOD_SYMMETRIC)) {
        const Blocks bk = coarse_blocks(t);
        const int ct = coarse_lanes(t);
        out[0] = 1;
        out[1] = bk.bxs;
        out[2] = bk.q;
        out[3] = ct;
        out[4] = (int32_t)ivx::cdiv(t.nty * t.ntz, (int64_t)ct);
    }
    out[5] = fused_start(t, nseeds) ? 1 : 0;
    out[6] = (int32_t)round_grid_cap(t);
    out[7] = (int32_t)t.ntiles;
    return IVX_OK;
}

extern "C" int ivx_dev_flood_run_edges(const ivx_flood_plan *p, const uint64_t *edges, uint64_t *reached, void *scratch_,
                                       int *rounds, void *stream) {
    return flood_run_impl(p, edges, ivx::FLOOD_DIRECTED, reached, scratch_, rounds, stream, nullptr, AHEAD_CHAINED);
}

extern "C" int ivx_flood_edges_bytes(const ivx_flood_plan *p, size_t *nbytes) {
    size_t one;
    int rc = ivx_flood_bits_bytes(p, &one);
    if (rc) return rc;
    *nbytes = 6 * one;
    return IVX_OK;
}

extern "C" int ivx_dev_flood_edges_auto(const ivx_flood_plan *p, const int16_t *data, const uint8_t *out, float pfrac, int fill,
                                        uint64_t *edges, void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    IVX_REQUIRE(data && out && edges, IVX_EINVAL, "flood_edges_auto: NULL argument");
    const int64_t total = t.dz * t.dy * t.wx * 8;
    if (!total) return IVX_OK;
    // the six planes are packed back to back, dz * dy * wx words each (ivx_flood_edges_bytes leaves room for that)
    hipLaunchKernelGGL(k_flood_edges_auto, dim3((unsigned)grid_for(total)), dim3(256), 0, ivx::S(stream), data, out, t, pfrac,
                       (uint8_t)fill, (uint8_t *)edges);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_flood_seed_forced(const ivx_flood_plan *p, const int64_t *seeds_xyz, int64_t nseeds, uint64_t *cand,
                                         uint64_t *reached, void *scratch_, void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    for (int64_t n = 0; n < nseeds; n++) {
        const int64_t x = seeds_xyz[3 * n], y = seeds_xyz[3 * n + 1], z = seeds_xyz[3 * n + 2];
        IVX_REQUIRE(x >= 0 && y >= 0 && z >= 0 && x < t.dx && y < t.dy && z < t.dz, IVX_ERANGE,
                    "flood: seed (%lld,%lld,%lld) outside volume (%lld,%lld,%lld) [x,y,z]", (long long)x, (long long)y,
                    (long long)z, (long long)t.dx, (long long)t.dy, (long long)t.dz);
    }
    if (nseeds == 0) return IVX_OK;
    const FScratch s = make_fscratch(t);
    char *scr = (char *)scratch_;
    hipStream_t st = ivx::S(stream);
    ivx::ccl_invalidate(scratch_);
    int64_t *d_seeds = (int64_t *)(scr + s.off_seeds);
    for (int64_t b = 0; b < nseeds; b += (int64_t)SEED_CHUNK) {
        const int64_t m = nseeds - b < (int64_t)SEED_CHUNK ? nseeds - b : (int64_t)SEED_CHUNK;
        IVX_HIP(hipMemcpyAsync(d_seeds, seeds_xyz + 3 * b, (size_t)m * 24, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_flood_seed_forced, dim3((unsigned)ivx::cdiv(m, 256)), dim3(256), 0, st, t, d_seeds, m,
                           (unsigned long long *)cand, (unsigned long long *)reached, (uint8_t *)(scr + s.off_dirty0));
        IVX_LAUNCH_CHECK();
        IVX_HIP(hipStreamSynchronize(st)); // d_seeds is reused by the next chunk; seeds_xyz is pageable host memory
    }
    return IVX_OK;
}

extern "C" int ivx_dev_flood_arm_gate(const void *scratch, uint32_t *word, uint32_t value, uint32_t below_tiles) {
    IVX_REQUIRE(scratch && word, IVX_EINVAL, "flood_arm_gate: NULL argument");
    std::lock_guard<std::mutex> lk(g_gates_mu);
    g_gates[scratch] = GateArm{word, value, below_tiles};
    return IVX_OK;
}
// forget an arm that no flood consumed (the gate was opened by hand, or the buffers are about to be freed): the entry is
// keyed by the scratch ADDRESS, and a later allocation may get the same one
extern "C" int ivx_dev_flood_disarm_gate(const void *scratch) {
    std::lock_guard<std::mutex> lk(g_gates_mu);
    g_gates.erase(scratch);
    return IVX_OK;
}
extern "C" int ivx_dev_gate_open(uint32_t *word, uint32_t value, void *stream) {
    IVX_REQUIRE(word, IVX_EINVAL, "gate_open: NULL argument");
    hipLaunchKernelGGL(k_gate_set, dim3(1), dim3(64), 0, ivx::S(stream), word, value);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}
extern "C" int ivx_dev_gate_wait(const uint32_t *word, uint32_t value, uint32_t timeout_us, void *stream) {
    IVX_REQUIRE(word, IVX_EINVAL, "gate_wait: NULL argument");
    hipLaunchKernelGGL(k_gate_wait, dim3(1), dim3(64), 0, ivx::S(stream), word, value, (unsigned long long)timeout_us * 100ull);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_flood_mark_slab(const ivx_flood_plan *p, void *scratch_, int64_t z0, int64_t z1, void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    if (z0 < 0) z0 = 0;
    if (z1 > t.dz) z1 = t.dz;
    if (z1 <= z0 || t.ntiles == 0) return IVX_OK;
    const FScratch s = make_fscratch(t);
    const int64_t tz0 = z0 / TZ, tz1 = ivx::cdiv(z1, TZ);
    const int64_t n = (tz1 - tz0) * t.nty * t.wx;
    hipLaunchKernelGGL(k_flood_mark, dim3((unsigned)ivx::cdiv(n, 256)), dim3(256), 0, ivx::S(stream), t, tz0, tz1,
                       (uint8_t *)((char *)scratch_ + s.off_dirty0));
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_flood_apply(const ivx_flood_plan *p, const uint64_t *reached, int dtype, void *target,
                                   double fill, void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    const int64_t total = t.dz * t.dy * t.wx * 8;
    if (!total) return IVX_OK;
    const int g = grid_for(total);
    hipStream_t st = ivx::S(stream);
    const uint8_t *r = (const uint8_t *)reached;
    if (dtype == IVX_U8 && t.dx % 64 == 0 && ((uintptr_t)target & 15) == 0) {
        const int64_t nchunks = t.dz * t.dy * t.dx / 16;
        const int64_t blocks = ivx::cdiv(nchunks, 1024);
        hipLaunchKernelGGL(k_flood_apply16, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st,
                           (const uint16_t *)reached, nchunks, (uint4 *)target, (uint8_t)fill);
        IVX_LAUNCH_CHECK();
        return IVX_OK;
    }
    switch (dtype) {
    case IVX_U8: hipLaunchKernelGGL(k_flood_apply<uint8_t>, dim3(g), dim3(256), 0, st, t, r, (uint8_t *)target, (uint8_t)fill); break;
    case IVX_I16: hipLaunchKernelGGL(k_flood_apply<int16_t>, dim3(g), dim3(256), 0, st, t, r, (int16_t *)target, (int16_t)fill); break;
    case IVX_U16: hipLaunchKernelGGL(k_flood_apply<uint16_t>, dim3(g), dim3(256), 0, st, t, r, (uint16_t *)target, (uint16_t)fill); break;
    case IVX_F64: hipLaunchKernelGGL(k_flood_apply<double>, dim3(g), dim3(256), 0, st, t, r, (double *)target, fill); break;
    default: ivx::set_error("flood: unsupported dtype %d", dtype); return IVX_EINVAL;
    }
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

// mask[reached] = v_sel for a uint8 mask that is known to be v_in inside the plane `inside_bits` and 0 outside it (a fused
// threshold's mask and plane): the same bytes as ivx_dev_flood_apply(..., IVX_U8, mask, v_sel, ...) without reading the mask
extern "C" int ivx_dev_flood_apply_levels(const ivx_flood_plan *p, const uint64_t *reached, const uint64_t *inside_bits, uint8_t *mask,
                                          int v_in, int v_sel, void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    if ((rc = levels_check(t, reached, inside_bits, mask, v_in, v_sel, false))) return rc;
    return launch_levels(t, reached, inside_bits, mask, v_in, v_sel, false, ApplyWhen{nullptr, nullptr, 0ull}, ivx::S(stream));
}

// the whole mask from its planes: v_sel where reached (NULL: nowhere), else v_in where inside, else 0 -- every byte is written
extern "C" int ivx_dev_mask_from_planes(const ivx_flood_plan *p, const uint64_t *inside_bits, const uint64_t *reached, uint8_t *mask,
                                        int v_in, int v_sel, void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    if ((rc = levels_check(t, reached, inside_bits, mask, v_in, v_sel, true))) return rc;
    return launch_levels(t, reached, inside_bits, mask, v_in, v_sel, true, ApplyWhen{nullptr, nullptr, 0ull}, ivx::S(stream));
}

// ivx_dev_flood_grow and the write of its result in one call.  The two writes from the bit planes are queued by the flood
// itself while its lists run out (EarlyWrite); where that launch did not go ahead, or for another kind of write, the
// write's kernel is queued as soon as the host has seen the flood end (the first round that starts empty, or whatever
// path the flood took instead), without the way back to the caller in between, through the entry point it names.
static int grow_select_impl(const ivx_flood_plan *p, int dtype, const void *data, double t0, double t1, const int64_t *seeds_xyz,
                            int64_t nseeds, uint64_t *cand, uint64_t *reached, void *scratch_, int *rounds, const ivx_flood_write *write,
                            int look_ahead, const ivx_mc_params *mc, void *mc_scratch, int *counted, void *stream) {
    IVX_REQUIRE(write && write->kind >= IVX_FLOOD_WRITE_NONE && write->kind <= IVX_FLOOD_WRITE_APPLY_U8, IVX_EINVAL,
                "flood_grow_select: no write description, or one of an unknown kind");
    IVX_REQUIRE(write->kind == IVX_FLOOD_WRITE_NONE || write->mask, IVX_EINVAL, "flood_grow_select: the write has no mask");
    if (counted) *counted = 0;
    EarlyWrite early = {write, false};
    const bool all = write->kind == IVX_FLOOD_WRITE_MASK_FROM_PLANES;
    const McRide ride = {mc, mc_scratch};
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    if (mc && counted && (all || write->kind == IVX_FLOOD_WRITE_APPLY_LEVELS) &&
        levels_check(t, reached, write->inside_bits, write->mask, write->v_in, write->v_sel, all) == IVX_OK &&
        ivx::mc_ride_ok(mc, mc_scratch, t.dz, t.dy, t.dx)) {
        early.ride = &ride;
        ivx::mc_ride_begin(mc_scratch, write->inside_bits); // (the count reads the write's inside plane in place)
    }
    rc = flood_grow_impl(p, dtype, data, t0, t1, seeds_xyz, nseeds, cand, reached, scratch_, rounds, stream, look_ahead, &early);
    if (rc) return rc;
    const bool fused = early.ride && !early.plain;
    if (!early.written) {
        switch (write->kind) {
        case IVX_FLOOD_WRITE_MASK_FROM_PLANES:
        case IVX_FLOOD_WRITE_APPLY_LEVELS:
            if (fused)
                rc = launch_levels(t, reached, write->inside_bits, write->mask, write->v_in, write->v_sel, all, ApplyWhen{nullptr, nullptr, 0ull},
                                   ivx::S(stream), &ride);
            else if (all)
                rc = ivx_dev_mask_from_planes(p, write->inside_bits, reached, write->mask, write->v_in, write->v_sel, stream);
            else
                rc = ivx_dev_flood_apply_levels(p, reached, write->inside_bits, write->mask, write->v_in, write->v_sel, stream);
            break;
        case IVX_FLOOD_WRITE_APPLY_U8: rc = ivx_dev_flood_apply(p, reached, IVX_U8, write->mask, (double)write->v_sel, stream); break;
        default: break;
        }
        if (rc) return rc;
    }
    if (fused) { // the launch that went ahead has counted: the scan behind it, and the caller has a counted piece
        if ((rc = ivx::mc_ride_scan(mc, mc_scratch, ivx::S(stream)))) return rc;
        *counted = 1;
    }
    return IVX_OK;
}
extern "C" int ivx_dev_flood_grow_select(const ivx_flood_plan *p, int dtype, const void *data, double t0, double t1,
                                         const int64_t *seeds_xyz, int64_t nseeds, uint64_t *cand, uint64_t *reached,
                                         void *scratch_, int *rounds, const ivx_flood_write *write, int look_ahead, void *stream) {
    return grow_select_impl(p, dtype, data, t0, t1, seeds_xyz, nseeds, cand, reached, scratch_, rounds, write, look_ahead, nullptr, nullptr,
                            nullptr, stream);
}
// ivx_dev_flood_grow_select for a flood that a surface call follows: where the write is one of the two from the bit planes,
// every launch of it is marching cubes' count of the piece `mc` from the write's inside plane in the same kernel
// (k_mc_count_write, k_mc.hip), with the scan queued behind the launch that went ahead; *counted = 1 then, and the piece in
// `mc_scratch` is what ivx_dev_mc_count_bits_async(mc, write->inside_bits, mc_scratch, stream) would have left.  Every other
// write kind, a piece the plane does not fit, the union-find escape and IVX_FLOOD_MODE=ccl: the write as
// ivx_dev_flood_grow_select queues it, *counted = 0 and nothing of marching cubes in the stream.
extern "C" int ivx_dev_flood_grow_select_count(const ivx_flood_plan *p, int dtype, const void *data, double t0, double t1,
                                               const int64_t *seeds_xyz, int64_t nseeds, uint64_t *cand, uint64_t *reached,
                                               void *scratch_, int *rounds, const ivx_flood_write *write, int look_ahead,
                                               const ivx_mc_params *mc, void *mc_scratch, int *counted, void *stream) {
    IVX_REQUIRE(mc && mc_scratch && counted, IVX_EINVAL, "flood_grow_select_count: null piece, scratch or result");
    return grow_select_impl(p, dtype, data, t0, t1, seeds_xyz, nseeds, cand, reached, scratch_, rounds, write, look_ahead, mc, mc_scratch,
                            counted, stream);
}

extern "C" int ivx_dev_flood_apply2(const ivx_flood_plan *p, const uint64_t *reached, uint8_t *out, int fill,
                                    uint8_t *mask, int select, void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    const int64_t total = t.dz * t.dy * t.wx * 8;
    if (!total) return IVX_OK;
    hipLaunchKernelGGL(k_flood_apply2, dim3(grid_for(total)), dim3(256), 0, ivx::S(stream), t, (const uint8_t *)reached, out,
                       (uint8_t)fill, mask, (uint8_t)select);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_flood_count(const ivx_flood_plan *p, const uint64_t *reached, int64_t *count, void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    *count = 0;
    const int64_t nw = t.dz * t.dy * t.wx;
    if (!nw) return IVX_OK;
    void *d_tot;
    if ((rc = ivx::ws_get_s(ivx::WS_SMALL, ivx::S(stream), 64, &d_tot))) return rc;
    hipStream_t st = ivx::S(stream);
    IVX_HIP(hipMemsetAsync(d_tot, 0, 8, st));
    hipLaunchKernelGGL(k_flood_count, dim3(grid_for(nw)), dim3(256), 0, st, (const unsigned long long *)reached, nw,
                       (unsigned long long *)d_tot);
    IVX_LAUNCH_CHECK();
    unsigned long long h = 0;
    IVX_HIP(hipMemcpyAsync(&h, d_tot, 8, hipMemcpyDeviceToHost, st));
    IVX_HIP(hipStreamSynchronize(st));
    *count = (int64_t)h;
    return IVX_OK;
}

// ---- multi-GPU halo: OR a neighbour's reached plane into slice z; counts words that gained bits -------------
// MARK: the tile of every word that gained bits is flagged dirty by the kernel itself (instead of the host marking the
// whole tile layer of z after reading the count back)
template <bool MARK>
__global__ __launch_bounds__(256) void k_flood_or_plane(unsigned long long *__restrict__ dst,
                                                        const unsigned long long *__restrict__ src,
                                                        const unsigned long long *__restrict__ cand, int64_t nwords,
                                                        unsigned int *__restrict__ changed, Tiles t, int64_t z,
                                                        uint8_t *__restrict__ dirty) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwords) return;
    const unsigned long long add = src[i] & cand[i] & ~dst[i];
    if (add) {
        dst[i] |= add;
        atomicAdd(changed, 1u);
        if (MARK) {
            const int64_t y = i / t.wx, txi = i - y * t.wx;
            mark_tile_nbhd(t, dirty, z / TZ, y / TY, txi);
        }
    }
}

__global__ __launch_bounds__(256) void k_bits_combine(unsigned long long *__restrict__ dst,
                                                      const unsigned long long *__restrict__ src, int64_t n, int op) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dst[i] = op == 0 ? (dst[i] | src[i]) : (dst[i] & ~src[i]);
}
// whole-plane dst |= src (op 0) or dst &= ~src (op 1): keeps a derived inside plane in step with `mask[reached] = v`
extern "C" int ivx_dev_bits_combine(uint64_t *dst, const uint64_t *src, int64_t nwords, int op, void *stream) {
    IVX_REQUIRE(nwords >= 0 && (op == 0 || op == 1), IVX_EINVAL, "bits_combine: bad arguments");
    if (nwords == 0) return IVX_OK;
    const int64_t blocks = ivx::cdiv(nwords, 256);
    hipLaunchKernelGGL(k_bits_combine, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, ivx::S(stream),
                       (unsigned long long *)dst, (const unsigned long long *)src, nwords, op);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_flood_or_plane(const ivx_flood_plan *p, const uint64_t *cand, uint64_t *reached, int64_t z,
                                      const uint64_t *plane, void *scratch_, int *changed, void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    IVX_REQUIRE(z >= 0 && z < t.dz, IVX_ERANGE, "flood: plane %lld outside slab", (long long)z);
    const FScratch s = make_fscratch(t);
    const int64_t nw = t.dy * t.wx;
    *changed = 0;
    if (!nw) return IVX_OK;
    hipStream_t st = ivx::S(stream);
    unsigned int *d_chg = (unsigned int *)((char *)scratch_ + s.off_status);
    IVX_HIP(hipMemsetAsync(d_chg, 0, 4, st));
    hipLaunchKernelGGL(k_flood_or_plane<false>, dim3((unsigned)ivx::cdiv(nw, 256)), dim3(256), 0, st,
                       (unsigned long long *)reached + z * nw, (const unsigned long long *)plane,
                       (const unsigned long long *)cand + z * nw, nw, d_chg, t, z, (uint8_t *)nullptr);
    IVX_LAUNCH_CHECK();
    unsigned int h = 0;
    IVX_HIP(hipMemcpyAsync(&h, d_chg, 4, hipMemcpyDeviceToHost, st));
    IVX_HIP(hipStreamSynchronize(st));
    *changed = (int)h;
    if (h) return ivx_dev_flood_mark_slab(p, scratch_, z - TZ, z + 1 + TZ, stream); // the layers that can see slice z
    return IVX_OK;
}

// The same, without any read-back: the number of words that gained bits is left in the caller's DEVICE word (overwritten),
// where the next exchange's all-reduce picks it up (ivx_comm_exchange_vote): a sharded region-growing round is
// enqueue-only up to its single host read.
static int or_planes_dev_impl(const ivx_flood_plan *p, const uint64_t *cand, uint64_t *reached, int64_t z_a, const uint64_t *plane_a,
                              int64_t z_b, const uint64_t *plane_b, void *scratch_, uint32_t *changed_dev, void *stream, bool zero);
extern "C" int ivx_dev_flood_or_planes_dev(const ivx_flood_plan *p, const uint64_t *cand, uint64_t *reached, int64_t z_a,
                                           const uint64_t *plane_a, int64_t z_b, const uint64_t *plane_b, void *scratch_,
                                           uint32_t *changed_dev, void *stream) {
    return or_planes_dev_impl(p, cand, reached, z_a, plane_a, z_b, plane_b, scratch_, changed_dev, stream, true);
}
// ... ADDED to the caller's device word (which ivx_dev_vote_read left at zero): no 4-byte fill in front of every round
extern "C" int ivx_dev_flood_or_planes_acc(const ivx_flood_plan *p, const uint64_t *cand, uint64_t *reached, int64_t z_a,
                                           const uint64_t *plane_a, int64_t z_b, const uint64_t *plane_b, void *scratch_,
                                           uint32_t *changed_dev, void *stream) {
    return or_planes_dev_impl(p, cand, reached, z_a, plane_a, z_b, plane_b, scratch_, changed_dev, stream, false);
}
static int or_planes_dev_impl(const ivx_flood_plan *p, const uint64_t *cand, uint64_t *reached, int64_t z_a, const uint64_t *plane_a,
                              int64_t z_b, const uint64_t *plane_b, void *scratch_, uint32_t *changed_dev, void *stream, bool zero) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    const FScratch s = make_fscratch(t);
    const int64_t nw = t.dy * t.wx;
    IVX_REQUIRE(changed_dev, IVX_EINVAL, "flood: null counter");
    const int64_t zs[2] = {z_a, z_b};
    const uint64_t *pl[2] = {plane_a, plane_b};
    // both slices are checked before anything is queued: a refused call leaves the plane and the caller's word as they were
    for (int q = 0; q < 2; q++)
        IVX_REQUIRE(!pl[q] || (zs[q] >= 0 && zs[q] < t.dz), IVX_ERANGE, "flood: plane %lld outside slab", (long long)zs[q]);
    hipStream_t st = ivx::S(stream);
    if (zero) IVX_HIP(hipMemsetAsync(changed_dev, 0, 4, st));
    if (!nw || (!plane_a && !plane_b)) return IVX_OK;
    uint8_t *dirty = (uint8_t *)((char *)scratch_ + s.off_dirty0);
    for (int q = 0; q < 2; q++) {
        if (!pl[q]) continue;
        hipLaunchKernelGGL(k_flood_or_plane<true>, dim3((unsigned)ivx::cdiv(nw, 256)), dim3(256), 0, st,
                           (unsigned long long *)reached + zs[q] * nw, (const unsigned long long *)pl[q],
                           (const unsigned long long *)cand + zs[q] * nw, nw, (unsigned int *)changed_dev, t, zs[q], dirty);
        IVX_LAUNCH_CHECK();
    }
    return IVX_OK;
}

// Both halo planes of a slab in one call (either may be NULL): reached[z] |= plane & cand[z] for each, the tiles of the
// words that gained bits are marked dirty on the device, and ONE read-back returns the number of such words.
extern "C" int ivx_dev_flood_or_planes(const ivx_flood_plan *p, const uint64_t *cand, uint64_t *reached, int64_t z_a,
                                       const uint64_t *plane_a, int64_t z_b, const uint64_t *plane_b, void *scratch_,
                                       int *changed, void *stream) {
    Tiles t;
    int rc = make_tiles(p, &t);
    if (rc) return rc;
    const FScratch s = make_fscratch(t);
    const int64_t nw = t.dy * t.wx;
    *changed = 0;
    const int64_t zs[2] = {z_a, z_b};
    const uint64_t *pl[2] = {plane_a, plane_b};
    for (int q = 0; q < 2; q++) // (before anything is queued: a refused call changes nothing)
        IVX_REQUIRE(!pl[q] || (zs[q] >= 0 && zs[q] < t.dz), IVX_ERANGE, "flood: plane %lld outside slab", (long long)zs[q]);
    if (!nw || (!plane_a && !plane_b)) return IVX_OK;
    hipStream_t st = ivx::S(stream);
    unsigned int *d_chg = (unsigned int *)((char *)scratch_ + s.off_status);
    uint8_t *dirty = (uint8_t *)((char *)scratch_ + s.off_dirty0);
    IVX_HIP(hipMemsetAsync(d_chg, 0, 4, st));
    for (int q = 0; q < 2; q++) {
        if (!pl[q]) continue;
        hipLaunchKernelGGL(k_flood_or_plane<true>, dim3((unsigned)ivx::cdiv(nw, 256)), dim3(256), 0, st,
                           (unsigned long long *)reached + zs[q] * nw, (const unsigned long long *)pl[q],
                           (const unsigned long long *)cand + zs[q] * nw, nw, d_chg, t, zs[q], dirty);
        IVX_LAUNCH_CHECK();
    }
    uint32_t seq, h = 0;
    if ((rc = ivx::mailbox_publish(d_chg, 1, st, &seq))) return rc;
    if ((rc = ivx::mailbox_wait(seq, st, &h, 1))) return rc;
    *changed = (int)h;
    return IVX_OK;
}

// ---- host forms -----------------------------------------------------------------------------------
static int flood_host(int dtype, void *data, const int64_t shape[3], const int64_t strides[3], const int64_t *seeds,
                      int64_t nseeds, double t0, double t1, double fill, const uint8_t *strct, const int64_t sshape[3],
                      uint8_t *out, const int64_t ostrides[3], int inplace) {
    using namespace ivx;
    const size_t isz = dtype_size(dtype);
    IVX_REQUIRE(isz, IVX_EINVAL, "floodfill: unsupported dtype %d", dtype);
    ivx_flood_plan plan;
    plan.dz = shape[0]; plan.dy = shape[1]; plan.dx = shape[2];
    plan.wx = cdiv(shape[2], 64);
    int rc;
    if ((rc = ivx_flood_strct_bits(strct, sshape, &plan.strct_bits))) return rc;
    // seed bounds are checked before anything is touched (the reference panics on an out-of-bounds seed)
    for (int64_t n = 0; n < nseeds; n++) {
        const int64_t x = seeds[3 * n], y = seeds[3 * n + 1], z = seeds[3 * n + 2];
        IVX_REQUIRE(x >= 0 && y >= 0 && z >= 0 && x < shape[2] && y < shape[1] && z < shape[0], IVX_ERANGE,
                    "floodfill: seed (%lld,%lld,%lld) outside volume", (long long)x, (long long)y, (long long)z);
    }
    const size_t n = (size_t)shape[0] * shape[1] * shape[2];
    if (n == 0 || nseeds == 0) return IVX_OK;
    size_t bb, sb;
    if ((rc = ivx_flood_bits_bytes(&plan, &bb))) return rc;
    if ((rc = ivx_flood_scratch_bytes(&plan, &sb))) return rc;
    void *d_data, *d_out = nullptr, *d_cand, *d_reach, *d_scr;
    if ((rc = ws_get(WS_IN, n * isz, &d_data))) return rc;
    if ((rc = ws_get(WS_AUX0, bb, &d_cand))) return rc;
    if ((rc = ws_get(WS_AUX1, bb, &d_reach))) return rc;
    if ((rc = ws_get(WS_AUX2, sb, &d_scr))) return rc;
    if ((rc = upload_strided(d_data, data, shape, strides, isz, WS_IN))) return rc;
    if (!inplace) {
        if ((rc = ws_get(WS_OUT, n, &d_out))) return rc;
        if ((rc = upload_strided(d_out, out, shape, ostrides, 1, WS_OUT))) return rc;
    }
    if ((rc = ivx_dev_flood_candidates(&plan, dtype, d_data, t0, t1, (const uint8_t *)d_out, inplace ? 2 : 1, fill,
                                       (uint64_t *)d_cand, nullptr)))
        return rc;
    if ((rc = ivx_dev_flood_grow(&plan, dtype, d_data, t0, t1, seeds, nseeds, (uint64_t *)d_cand, (uint64_t *)d_reach, d_scr,
                                 nullptr, nullptr)))
        return rc;
    if (inplace) {
        if ((rc = ivx_dev_flood_apply(&plan, (const uint64_t *)d_reach, dtype, d_data, fill, nullptr))) return rc;
        IVX_HIP(hipDeviceSynchronize());
        return download_strided(data, shape, strides, d_data, isz, WS_IN);
    }
    if ((rc = ivx_dev_flood_apply(&plan, (const uint64_t *)d_reach, IVX_U8, d_out, fill, nullptr))) return rc;
    IVX_HIP(hipDeviceSynchronize());
    return download_strided(out, shape, ostrides, d_out, 1, WS_OUT);
}

extern "C" int ivx_floodfill_threshold(int dtype, const void *data, const int64_t shape[3], const int64_t strides[3],
                                       const int64_t *seeds_xyz, int64_t nseeds, double t0, double t1, int fill,
                                       const uint8_t *strct, const int64_t sshape[3], uint8_t *out,
                                       const int64_t out_strides[3]) {
    ivx::HostCallGuard host_guard__;
    return flood_host(dtype, (void *)data, shape, strides, seeds_xyz, nseeds, t0, t1, (double)(uint8_t)fill, strct,
                      sshape, out, out_strides, 0);
}

extern "C" int ivx_floodfill_threshold_inplace(int dtype, void *data, const int64_t shape[3], const int64_t strides[3],
                                               const int64_t *seeds_xyz, int64_t nseeds, double t0, double t1,
                                               double fill, const uint8_t *strct, const int64_t sshape[3]) {
    ivx::HostCallGuard host_guard__;
    return flood_host(dtype, data, shape, strides, seeds_xyz, nseeds, t0, t1, fill, strct, sshape, nullptr, strides, 1);
}

// floodfill_internal (floodfill.rs:5-49): 6-neighbour component of `data == v` around (x, y, z); the seed itself is
// filled and expanded whatever its value; voxels whose `out` byte already equals `fill` are barriers.
extern "C" int ivx_floodfill(int dtype, const void *data, const int64_t shape[3], const int64_t strides[3], int64_t x,
                             int64_t y, int64_t z, double v, int fill, uint8_t *out, const int64_t out_strides[3]) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    const size_t isz = dtype_size(dtype);
    IVX_REQUIRE(isz, IVX_EINVAL, "floodfill: unsupported dtype %d", dtype);
    IVX_REQUIRE(x >= 0 && y >= 0 && z >= 0 && x < shape[2] && y < shape[1] && z < shape[0], IVX_ERANGE,
                "floodfill: seed (%lld,%lld,%lld) outside volume", (long long)x, (long long)y, (long long)z);
    ivx_flood_plan plan;
    plan.dz = shape[0]; plan.dy = shape[1]; plan.dx = shape[2];
    plan.wx = cdiv(shape[2], 64);
    plan.strct_bits = (1u << 4) | (1u << 10) | (1u << 12) | (1u << 13) | (1u << 14) | (1u << 16) | (1u << 22); // 6 faces
    const size_t n = (size_t)shape[0] * shape[1] * shape[2];
    size_t bb, sb;
    int rc;
    if ((rc = ivx_flood_bits_bytes(&plan, &bb))) return rc;
    if ((rc = ivx_flood_scratch_bytes(&plan, &sb))) return rc;
    void *d_data, *d_out, *d_cand, *d_reach, *d_scr;
    if ((rc = ws_get(WS_IN, n * isz, &d_data))) return rc;
    if ((rc = ws_get(WS_OUT, n, &d_out))) return rc;
    if ((rc = ws_get(WS_AUX0, bb, &d_cand))) return rc;
    if ((rc = ws_get(WS_AUX1, bb, &d_reach))) return rc;
    if ((rc = ws_get(WS_AUX2, sb, &d_scr))) return rc;
    if ((rc = upload_strided(d_data, data, shape, strides, isz, WS_IN))) return rc;
    if ((rc = upload_strided(d_out, out, shape, out_strides, 1, WS_OUT))) return rc;
    const double fl = (double)(uint8_t)fill;
    const int64_t seed[3] = {x, y, z};
    if ((rc = ivx_dev_flood_clear(&plan, (uint64_t *)d_reach, d_scr, nullptr))) return rc;
    if ((rc = ivx_dev_flood_candidates(&plan, dtype, d_data, v, v, (const uint8_t *)d_out, 1, fl, (uint64_t *)d_cand, nullptr)))
        return rc;
    if ((rc = ivx_dev_flood_seed_forced(&plan, seed, 1, (uint64_t *)d_cand, (uint64_t *)d_reach, d_scr, nullptr))) return rc;
    if ((rc = ivx_dev_flood_run(&plan, (const uint64_t *)d_cand, (uint64_t *)d_reach, d_scr, nullptr, nullptr))) return rc;
    if ((rc = ivx_dev_flood_apply(&plan, (const uint64_t *)d_reach, IVX_U8, d_out, fl, nullptr))) return rc;
    IVX_HIP(hipDeviceSynchronize());
    return download_strided(out, shape, out_strides, d_out, 1, WS_OUT);
}

// floodfill_auto_threshold (floodfill_py.rs:12-85): int16 data, uint8 out; every seed is filled and expanded
// unconditionally, a step from a voxel of value v reaches 6-neighbours in [ceil(v(1-p)), floor(v(1+p))] (f32, as i16).
extern "C" int ivx_floodfill_auto_threshold(const int16_t *data, const int64_t shape[3], const int64_t strides[3],
                                            const int64_t *seeds_xyz, int64_t nseeds, float pfrac, int fill, uint8_t *out,
                                            const int64_t out_strides[3]) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    ivx_flood_plan plan;
    plan.dz = shape[0]; plan.dy = shape[1]; plan.dx = shape[2];
    plan.wx = cdiv(shape[2], 64);
    plan.strct_bits = (1u << 4) | (1u << 10) | (1u << 12) | (1u << 13) | (1u << 14) | (1u << 16) | (1u << 22);
    for (int64_t n = 0; n < nseeds; n++) {
        const int64_t x = seeds_xyz[3 * n], y = seeds_xyz[3 * n + 1], z = seeds_xyz[3 * n + 2];
        IVX_REQUIRE(x >= 0 && y >= 0 && z >= 0 && x < shape[2] && y < shape[1] && z < shape[0], IVX_ERANGE,
                    "floodfill_auto_threshold: seed (%lld,%lld,%lld) outside volume", (long long)x, (long long)y, (long long)z);
    }
    const size_t n = (size_t)shape[0] * shape[1] * shape[2];
    if (n == 0 || nseeds == 0) return IVX_OK;
    size_t bb, eb, sb;
    int rc;
    if ((rc = ivx_flood_bits_bytes(&plan, &bb))) return rc;
    if ((rc = ivx_flood_edges_bytes(&plan, &eb))) return rc;
    if ((rc = ivx_flood_scratch_bytes(&plan, &sb))) return rc;
    void *d_data, *d_out, *d_edges, *d_reach, *d_scr;
    if ((rc = ws_get(WS_IN, n * 2, &d_data))) return rc;
    if ((rc = ws_get(WS_OUT, n, &d_out))) return rc;
    if ((rc = ws_get(WS_AUX0, eb, &d_edges))) return rc;
    if ((rc = ws_get(WS_AUX1, bb, &d_reach))) return rc;
    if ((rc = ws_get(WS_AUX2, sb, &d_scr))) return rc;
    if ((rc = upload_strided(d_data, data, shape, strides, 2, WS_IN))) return rc;
    if ((rc = upload_strided(d_out, out, shape, out_strides, 1, WS_OUT))) return rc;
    if ((rc = ivx_dev_flood_clear(&plan, (uint64_t *)d_reach, d_scr, nullptr))) return rc;
    if ((rc = ivx_dev_flood_edges_auto(&plan, (const int16_t *)d_data, (const uint8_t *)d_out, pfrac, fill, (uint64_t *)d_edges,
                                       nullptr)))
        return rc;
    if ((rc = ivx_dev_flood_seed_forced(&plan, seeds_xyz, nseeds, nullptr, (uint64_t *)d_reach, d_scr, nullptr))) return rc;
    if ((rc = ivx_dev_flood_run_edges(&plan, (const uint64_t *)d_edges, (uint64_t *)d_reach, d_scr, nullptr, nullptr))) return rc;
    if ((rc = ivx_dev_flood_apply(&plan, (const uint64_t *)d_reach, IVX_U8, d_out, (double)(uint8_t)fill, nullptr))) return rc;
    IVX_HIP(hipDeviceSynchronize());
    return download_strided(out, shape, out_strides, d_out, 1, WS_OUT);
}
