// words_from_records.h -- the in-range plane of an int16 image from its per-word (min, max) records, one plane word per lane.
// Included by k_threshold.hip (k_threshold16_plane_use) and k_flood.hip (k_flood_candidates_words).
//
// A lane owns one word: 64 x-voxels, one 128-byte image line, one record, 8 bytes of plane.  A wave reads 256 contiguous
// bytes of records and stores 512 contiguous bytes of plane; there is no loop over words, the grid covers them.  The record
// decides the word where it can (wholly inside: ~0, wholly outside: 0; the image is not looked at there).  The wave's mixed
// words are then served eight at a time: in pass p lane l loads segment l & 7 (16 bytes, 8 voxels) of the wave's
// (8 p + (l >> 3))-th mixed word, so one load instruction fetches eight whole lines.  The 8 lanes of a word OR their bytes
// together (two quad steps, one half-row mirror) and the word's owner lane pulls the result.
// The passes of a wave are one straight-line body per pass count (1, 2, 3, 4, 6 or 8 passes: a wave with 5 or 7 runs the
// next one up and loads its last line again), so that every load is issued before the first is consumed.  In the gfx950 ISA
// (hipcc -O3 -S) each body is its NP global_load_dwordx4 in a row with no s_waitcnt vmcnt between them, then vmcnt(NP-1),
// vmcnt(NP-2), ... vmcnt(0) in front of the passes' arithmetic; 52 VGPRs, 8 waves per SIMD.  With the passes in one unrolled
// loop under `if (8 p < nmix)` instead, the register allocator copied a loaded register right behind the second load and the
// compiler put vmcnt(0) there: that is why the bodies are separate.
// Measured at 512^3 on the bench volume (profiles/threshold_words_ab.md): 14.4 us for 59 MB; the loop with a lane per 16-voxel
// chunk that this replaces took 30.2 us.  Records and stores alone take 6.2 us, the arithmetic 0.7 us, and a wait behind
// every pass's load costs 2.3 us: the kernel was bound by its dependent waits, not by the rate of sparse lines.
#pragma once
#include "ivx_internal.h"

typedef short short8_t __attribute__((ext_vector_type(8)));

namespace {

__device__ __forceinline__ int quad_xor1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, true); } // quad_perm [1,0,3,2]
__device__ __forceinline__ int quad_xor2(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, true); } // quad_perm [2,3,0,1]
__device__ __forceinline__ int half_mirror(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, true); } // lane i <- lane i ^ 7

constexpr int WORDS_PER_WG = 256; // the kernels that call words_from_records run 256 lanes: four waves of 64 words

static inline unsigned words_grid(int64_t nwords) { return (unsigned)ivx::cdiv(nwords, WORDS_PER_WG); }

// NP passes over the wave's nmix mixed words (nmix <= 8 NP).  owner_of: lane r holds the lane that owns the r-th mixed word;
// line0: the wave's first image line + this lane's segment; rank: of this lane's word among the mixed ones.  Every lane of the
// wave runs this; a group past the last mixed word loads that word's line again and its result is not pulled by anyone.
template <int NP>
__device__ __forceinline__ void words_mixed_passes(const short8_t *__restrict__ line0, int owner_of, int nmix, int rank, bool mixed,
                                                   int lo, int hi, unsigned &w_lo, unsigned &w_hi) {
    const int lane = threadIdx.x & 63, grp = lane >> 3, seg = lane & 7;
    short8_t d[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const int k = min(8 * p + grp, nmix - 1);
        const int src = __builtin_amdgcn_ds_bpermute(k << 2, owner_of);
        d[p] = __builtin_nontemporal_load(&line0[src * 8]);
    }
    const int from = (rank & 7) << 5; // the first lane of the group that serves this lane's word in pass rank >> 3
#pragma unroll
    for (int p = 0; p < NP; p++) {
        unsigned b = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) b |= ((int)d[p][i] >= lo && (int)d[p][i] <= hi ? 1u : 0u) << i;
        int x = (int)(b << (8 * (seg & 3))); // the lane's byte in its half of the word
        x |= quad_xor1(x);
        x |= quad_xor2(x);            // every lane of a quad: the quad's half (segments 0..3 low, 4..7 high)
        const int y = half_mirror(x); // the other quad's half
        const int t_lo = __builtin_amdgcn_ds_bpermute(from, seg < 4 ? x : y);
        const int t_hi = __builtin_amdgcn_ds_bpermute(from, seg < 4 ? y : x);
        if (mixed && (rank >> 3) == p) {
            w_lo = (unsigned)t_lo;
            w_hi = (unsigned)t_hi;
        }
    }
}

// plane[w] = bits of (v >= lo && v <= hi) over the 64 voxels of word w, for every w < nwords.  Call from all 256 lanes.
__device__ __forceinline__ void words_from_records(const short8_t *__restrict__ img, const unsigned *__restrict__ ranges,
                                                   int64_t nwords, int lo, int hi, unsigned long long *__restrict__ plane) {
    const int lane = threadIdx.x & 63;
    const int64_t wbase = (int64_t)blockIdx.x * WORDS_PER_WG + __builtin_amdgcn_readfirstlane((int)(threadIdx.x & 192u));
    const int64_t w = wbase + lane;
    const bool valid = w < nwords;
    unsigned rec = 0;
    if (valid) rec = ranges[w];
    const int mn = (int)(short)(rec & 0xffffu), mx = (int)(short)(rec >> 16);
    const bool inside = mn >= lo && mx <= hi;
    const bool mixed = valid && !inside && !(mx < lo || mn > hi);
    unsigned w_lo = inside ? ~0u : 0u, w_hi = w_lo;
    const unsigned long long mk = __ballot(mixed);
    if (mk) { // (wave-uniform from here on: every lane takes part in the permutes)
        const int nmix = __popcll(mk);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
        // lane r learns which lane owns the wave's r-th mixed word: the mixed lanes push their number to their rank, the
        // others to the places behind (a permutation, so no two lanes push to one place)
        const int owner_of = __builtin_amdgcn_ds_permute((mixed ? rank : nmix + lane - rank) << 2, lane);
        const short8_t *line0 = img + wbase * 8 + (lane & 7);
        if (nmix <= 8) words_mixed_passes<1>(line0, owner_of, nmix, rank, mixed, lo, hi, w_lo, w_hi);
        else if (nmix <= 16) words_mixed_passes<2>(line0, owner_of, nmix, rank, mixed, lo, hi, w_lo, w_hi);
        else if (nmix <= 24) words_mixed_passes<3>(line0, owner_of, nmix, rank, mixed, lo, hi, w_lo, w_hi);
        else if (nmix <= 32) words_mixed_passes<4>(line0, owner_of, nmix, rank, mixed, lo, hi, w_lo, w_hi);
        else if (nmix <= 48) words_mixed_passes<6>(line0, owner_of, nmix, rank, mixed, lo, hi, w_lo, w_hi);
        else words_mixed_passes<8>(line0, owner_of, nmix, rank, mixed, lo, hi, w_lo, w_hi);
    }
    if (valid) plane[w] = ((unsigned long long)w_hi << 32) | w_lo;
}

} // namespace
