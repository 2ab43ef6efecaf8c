// mc_common.h -- what the two marching-cubes translation units share: k_mc.hip (inside planes, count, scan, triangle list and
// emit: the triangle soup) and k_mci.hip (the indexed mesh and the cross-slab stitch, which read the planes, the counts and the
// list of the same piece).  The piece's geometry, the scratch layout, the known-levels form of a mask, the device helpers both
// sides use, and the host launchers that k_mc.hip defines and k_mci.hip calls.
#pragma once
#include "ivx_internal.h"
#include "mc_piece.h"

namespace ivx {

// Division of a 32-bit number by a divisor that is fixed for a launch (words per cell row, cell rows per slice), without a
// division: Granlund & Montgomery, "Division by invariant integers using multiplication" (PLDI 1994), figure 4.1 with N = 32.
// With l = ceil(log2 d), mul = floor(2^32 (2^l - d) / d) + 1, s1 = min(l, 1), s2 = max(l - 1, 0):
//   t = floor(mul * n / 2^32),  n / d = (t + ((n - t) >> s1)) >> s2      for EVERY n < 2^32 and every 1 <= d < 2^32
// (2^32 + mul = floor(2^(32+l) / d) + 1 is a 33-bit multiplier whose error stays below one part in 2^32; t <= n, so n - t does not
// wrap, and t + ((n - t) >> s1) <= n.)  Cell-word ids are below 2^32 (checked where the kernels are queued), so both
// divisions of a word id are exact; tests/test_gpu_mc_front_end.py checks the constants against integer division on the host.
struct McDiv {
    uint32_t d, mul, s1, s2;
};
static inline McDiv mc_div_make(uint32_t d) {
    if (d == 0) d = 1; // (an empty grid: nothing is divided)
    uint32_t l = 0;
    while (l < 32 && (1ull << l) < d) l++;
    McDiv m;
    m.d = d;
    m.mul = (uint32_t)((((1ull << l) - d) << 32) / d + 1ull);
    m.s1 = l < 1 ? l : 1;
    m.s2 = l > 0 ? l - 1 : 0;
    return m;
}
__host__ __device__ __forceinline__ uint32_t mc_div(uint32_t n, const McDiv &m) {
    const uint32_t t = (uint32_t)(((uint64_t)m.mul * n) >> 32);
    return (t + ((n - t) >> m.s1)) >> m.s2;
}

struct Geom {
    int64_t nz, ny, nx;  // piece
    int64_t NZ, NY, NX;  // padded grid points
    int64_t ws;          // uint64 words per SOURCE row = ceil(nx/64)
    int64_t WX;          // uint64 words per padded point row
    int64_t WC;          // uint64 words per cell row  (NX-1 cells)
    int64_t nrows;       // (NZ-1)*(NY-1) cell rows
    int pxy, pb;
    double padv;
    double sx, sy, sz;
    int64_t yoff, zoff;
    McDiv div_wc, div_rows; // by WC and by NY - 1: cell-word id -> (slice, row, word in the row)
};
// cell word `wid` (< nwords < 2^32) -> slice k, cell row j, word w of the row
__host__ __device__ __forceinline__ void mc_split_wid(const Geom &g, uint32_t wid, uint32_t &k, uint32_t &j, uint32_t &w) {
    const uint32_t row = mc_div(wid, g.div_wc);
    w = wid - row * g.div_wc.d;
    k = mc_div(row, g.div_rows);
    j = row - k * g.div_rows.d;
}

static int make_geom(const ivx_mc_params *p, Geom *g) {
    IVX_REQUIRE(p && p->nz >= 0 && p->ny >= 0 && p->nx >= 0, IVX_EINVAL, "mc: bad shape");
    IVX_REQUIRE(p->niso >= 1 && p->niso <= 2, IVX_EINVAL, "mc: niso must be 1 or 2");
    IVX_REQUIRE(p->dtype == IVX_U8 || p->dtype == IVX_I16 || p->dtype == IVX_U16, IVX_EINVAL, "mc: dtype");
    g->nz = p->nz; g->ny = p->ny; g->nx = p->nx;
    g->pxy = p->pad_xy ? 1 : 0; g->pb = p->pad_bottom ? 1 : 0;
    g->NZ = p->nz + g->pb + (p->pad_top ? 1 : 0);
    g->NY = p->ny + 2 * g->pxy; g->NX = p->nx + 2 * g->pxy;
    g->ws = ivx::cdiv(g->nx, 64);
    g->WX = ivx::cdiv(g->NX, 64);
    g->WC = g->NX > 1 ? ivx::cdiv(g->NX - 1, 64) : 0;
    g->nrows = (g->NZ > 1 && g->NY > 1) ? (g->NZ - 1) * (g->NY - 1) : 0;
    // (the triangle list names a cell word by 16-bit slice, 16-bit row and 15-bit word-in-row)
    IVX_REQUIRE(g->NZ <= 65536 && g->NY <= 65536 && g->WC <= 32768, IVX_EINVAL, "mc: piece too large (at most 65 535 cells along z and y, 2^21 along x)");
    g->padv = p->pad_value;
    g->sx = p->spacing[0]; g->sy = p->spacing[1]; g->sz = p->spacing[2];
    g->yoff = g->NY - 1 - g->pxy;
    g->zoff = p->roi_start - p->vtk_pz;
    g->div_wc = mc_div_make((uint32_t)g->WC);
    g->div_rows = mc_div_make((uint32_t)(g->NY > 1 ? g->NY - 1 : 1));
    return IVX_OK;
}

// scratch layout (all 256-B aligned): bits[niso][nz*ny*ws] u64 | counts[niso][nwords] u16 |
// blocksum[niso*nblocks] u32 | blockoff[niso*nblocks+1] u64
struct Scratch {
    size_t bits_words, nwords, nblocks;
    size_t off_bits, off_counts, off_bsum, off_boff, total;
};
static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static Scratch make_scratch(const Geom &g, int niso) {
    Scratch s;
    s.bits_words = (size_t)(g.nz * g.ny * g.ws);
    s.nwords = (size_t)(g.nrows * g.WC);
    s.nblocks = (s.nwords + 255) / 256;
    s.off_bits = 0;
    s.off_counts = al256(s.off_bits + (size_t)niso * s.bits_words * 8 + 16);
    s.off_bsum = al256(s.off_counts + (size_t)niso * s.nwords * 2);
    s.off_boff = al256(s.off_bsum + (size_t)niso * s.nblocks * 4);
    s.total = al256(s.off_boff + ((size_t)niso * s.nblocks + 1) * 8);
    return s;
}

template <typename T>
__device__ __forceinline__ double mc_at(const T *a, const Geom &g, int64_t k, int64_t jf, int64_t i) {
    const int64_t ja = (g.NY - 1 - jf) - g.pxy, ia = i - g.pxy, ka = k - g.pb;
    if (ia < 0 || ia >= g.nx || ja < 0 || ja >= g.ny || ka < 0 || ka >= g.nz) return g.padv;
    return (double)a[(ka * g.ny + ja) * g.nx + ia];
}

// edge e -> (axis, low corner, low-corner offset) without tables: edges 0-3 run along x with (dy,dz) = (e&1, e>>1&1),
// 4-7 along y with (dx,dz), 8-11 along z with (dx,dy)  (tools/gen_mc_tables.py conventions).
__device__ __forceinline__ void edge_decode(int e, int &ax, int &bx, int &by, int &bz) {
    ax = e >> 2;
    const int a = e & 1, b = (e >> 1) & 1;
    bx = ax == 0 ? 0 : a;
    by = ax == 0 ? a : (ax == 1 ? 0 : b);
    bz = ax == 2 ? 0 : b;
}

// LEVELS: the voxel values are not gathered but derived -- the piece is a mask known to hold v_out outside the inside plane, v_sel
// where `sel` has a bit and v_in elsewhere inside (a resident pipeline's threshold + region-growing result).  Which end of
// an edge is inside is in the case index already, so a triangle costs three bit look-ups in a 16 MiB plane instead of six
// byte gathers from the mask; the interpolation then runs on the same numbers and gives the same bits.
struct McLevels {
    const uint64_t *sel; // source-coordinate plane, rows of g.ws words
    double v_out, v_in, v_sel;
    // (iso - s0) / (s1 - s0) for the four (which end is inside, which inside level) combinations, divided once on the host:
    // IEEE double division gives the same bits there as three divisions per triangle give here
    double tt[4]; // [in0 * 2 + sel]
};
static inline McLevels make_levels(const uint64_t *sel, double iso, double v_out, double v_in, double v_sel) {
    McLevels lv{sel, v_out, v_in, v_sel, {0.0, 0.0, 0.0, 0.0}};
    for (int in0 = 0; in0 < 2; in0++)
        for (int q = 0; q < 2; q++) {
            const double vin = q ? v_sel : v_in, s0 = in0 ? vin : v_out, s1 = in0 ? v_out : vin;
            lv.tt[in0 * 2 + q] = (iso - s0) / (s1 - s0);
        }
    return lv;
}

static inline uint64_t pad_bits(const ivx_mc_params *p, int q) { return p->pad_value >= p->iso[q] ? ~0ull : 0ull; }

// the inside plane of iso-value `q` of the piece counted into `scratch`: the caller's own (ivx_dev_mc_count_bits), else the scratch's
static inline const uint64_t *mc_bits_ptr(const void *scratch, const Scratch &s, int q) {
    if (const uint64_t *ext = mc_pieces().ext_plane(scratch, q)) return ext;
    return (const uint64_t *)((const char *)scratch + s.off_bits) + (size_t)q * s.bits_words;
}

// f<T>(...) for the voxel type T of the piece (make_geom has refused every other dtype)
#define MC_BY_DTYPE(dtype, f, ...) \
    ((dtype) == IVX_U8 ? f<uint8_t>(__VA_ARGS__) : (dtype) == IVX_I16 ? f<int16_t>(__VA_ARGS__) : f<uint16_t>(__VA_ARGS__))

// ---- host launchers (k_mc.hip) ---------------------------------------------------------------------------------------
// The prologue of every entry point: parameters -> geometry and scratch layout, and the limits of the passes (one workgroup
// per 256 cell words in one grid, 32-bit cell-word ids).  *empty: the piece has no cell, there is nothing to queue.
int mc_piece_layout(const ivx_mc_params *p, Geom *g, Scratch *s, bool *empty);
// the planes "value >= iso0" (and, for a two-iso piece, ">= iso1" s.bits_words words behind it) of the voxels `a` -> dst
int mc_inside_planes(const ivx_mc_params *p, const Geom &g, const Scratch &s, const void *a, void *dst, double iso0, double iso1,
                     hipStream_t st);
// the triangle list of the piece counted into `scratch` -> d_list, clipped to max_tris entries
int mc_queue_list(const ivx_mc_params *p, const Geom &g, const Scratch &s, const void *scratch, void *d_list, int64_t max_tris,
                  hipStream_t st);
// host forms: the strided piece `a` into the library's input block, and a scratch block for it
int mc_upload_piece(const ivx_mc_params *p, const void *a, const int64_t strides[3], void **d_a, void **d_scr);

} // namespace ivx
