// flood_tiles.h -- the tile grid and the scratch layout of the region-growing engine (k_flood.hip), for the units that
// prepare a flood on the device themselves: they mark dirty tiles and read counters inside the engine's scratch block.
// Included by the translation units that need it (contents live in each unit's anonymous namespace).
#pragma once
#include <stdlib.h>

#include "ivx_internal.h"

namespace {

constexpr int TY_LOG = 4, TY = 1 << TY_LOG, TZ = 16; // tile rows / slices (tile is one 64-voxel word wide)

struct Tiles {
    int64_t dz, dy, dx, wx;
    int64_t nty, ntz, ntiles;
    uint32_t strct;
    int itcap; // local iterations per tile visit before the tile re-enlists itself
    int conn; // 6 / 18 / 26 when strct is exactly scipy's generate_binary_structure(3, 1|2|3), else 0 (generic path)
};

static int make_tiles(const ivx_flood_plan *p, Tiles *t) {
    IVX_REQUIRE(p && p->dz >= 0 && p->dy >= 0 && p->dx >= 0, IVX_EINVAL, "flood: bad shape");
    IVX_REQUIRE(p->wx == ivx::cdiv(p->dx, 64), IVX_EINVAL, "flood: plan.wx must be ceil(dx/64)");
    t->dz = p->dz; t->dy = p->dy; t->dx = p->dx; t->wx = p->wx;
    t->nty = ivx::cdiv(p->dy, TY); t->ntz = ivx::cdiv(p->dz, TZ);
    t->ntiles = t->wx * t->nty * t->ntz;
    t->strct = p->strct_bits & ~(1u << 13); // the centre never matters
    {
        uint32_t m6 = 0, m18 = 0, m26 = 0;
        for (int k = 0; k < 27; k++) {
            const int nzc = (k / 9 != 1) + ((k / 3) % 3 != 1) + (k % 3 != 1);
            if (nzc <= 1) m6 |= 1u << k;
            if (nzc <= 2) m18 |= 1u << k;
            m26 |= 1u << k;
        }
        const uint32_t sb = p->strct_bits | (1u << 13);
        t->conn = sb == m26 ? 26 : sb == m18 ? 18 : sb == m6 ? 6 : 0;
    }
    // One tile crossing (TY = TZ = 16 rows) per visit: a tile that is still changing after that re-enlists itself and
    // carries on in the next round, when its neighbours have already started on what it has published so far -- the
    // rounds pipeline instead of waiting for the slowest tile's local fix-point (measured 0.240 -> 0.232 ms on the bench
    // volume; below 16 a straight crossing needs two visits and the round count doubles).
    static const int itcap = [] {
        const char *e = getenv("IVX_FLOOD_ITCAP");
        const int v = e ? atoi(e) : TY + TY / 2; // (round 6: 24 instead of 16 -- 9 rounds instead of 10 on the bench volume, 0.1916 -> 0.1871 ms; 20 .. 64 measure alike)
        return v < 1 ? 1 : v;
    }();
    t->itcap = itcap;
    IVX_REQUIRE(t->ntiles < 0x7fffffffll, IVX_EINVAL, "flood: too many tiles");
    return IVX_OK;
}

// scratch: dirty[2][ntiles] u8 | counter ring | seed staging | status words | round lists | coarse-pass row words
constexpr size_t SEED_CHUNK = 4096;
// the counter block: counter ring, four reserved dwords, the rounds' list lengths (k_flood.hip)
constexpr int FLOOD_CNT_DWORDS = 128;
static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
struct FScratch {
    size_t off_dirty0, off_dirty1, off_cnt, off_seeds, off_status, off_list0, off_list1;
    size_t off_full, off_whole, total;
};
static FScratch make_fscratch(const Tiles &t) {
    FScratch s;
    s.off_dirty0 = 0;
    s.off_dirty1 = al256((size_t)t.ntiles);
    s.off_cnt = al256(s.off_dirty1 + (size_t)t.ntiles);
    s.off_seeds = al256(s.off_cnt + FLOOD_CNT_DWORDS * 4); // everything before off_seeds is zeroed by flood_clear
    s.off_status = al256(s.off_seeds + SEED_CHUNK * 3 * 8);
    s.off_list0 = al256(s.off_status + 64);
    s.off_list1 = al256(s.off_list0 + (size_t)t.ntiles * 4);
    s.off_full = al256(s.off_list1 + (size_t)t.ntiles * 4); // coarse pass: one word per row of tiles, all-candidate / wholly reached
    s.off_whole = al256(s.off_full + (size_t)(t.nty * t.ntz) * 8);
    s.total = al256(s.off_whole + (size_t)(t.nty * t.ntz) * 8);
    return s;
}

// Bits that enter `reached` from OUTSIDE a tile visit (seeds, a neighbour slab's plane OR-ed into a halo slice) are news
// nobody has reported: a visit only tells its neighbours about the faces IT changed.  Wake the word's own tile and every
// tile that can see the word.
__device__ __forceinline__ void mark_tile_nbhd(const Tiles &t, uint8_t *__restrict__ dirty, int64_t tz, int64_t ty, int64_t tx) {
    for (int64_t az = tz - 1; az <= tz + 1; az++)
        for (int64_t ay = ty - 1; ay <= ty + 1; ay++)
            for (int64_t ax = tx - 1; ax <= tx + 1; ax++)
                if (az >= 0 && az < t.ntz && ay >= 0 && ay < t.nty && ax >= 0 && ax < t.wx)
                    dirty[(az * t.nty + ay) * t.wx + ax] = 1;
}

} // namespace
