// mesh_weld_math.h -- the numbers of the surface import's weld: which corners of a triangle soup are the same
// point, where a point's key starts its walk through the hash table, how large that table is, and where the floats of a
// binary STL record lie.  Plain C++ without a GPU construct, so that the very text k_meshweld.hip runs can also be compiled
// for the host and compared with the Python restatement where there is no GPU (tests/mesh_weld_host_emu.cpp,
// tests/test_surface_import_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IVX_MW_HD __host__ __device__
#else
#define IVX_MW_HD
#endif

namespace ivx_mesh_weld_math {

constexpr uint32_t EMPTY = 0xffffffffu;        // a table slot nobody claimed
constexpr int64_t MAX_CORNERS = 2147483647ll;  // 3 T <= 2^31 - 1: corner indices are uint32 below EMPTY and int32 face ids
constexpr int64_t STL_HEADER = 84;             // 80 bytes of text + the little-endian uint32 count
constexpr int64_t STL_RECORD = 50;             // 12 bytes of normal, 9 float32, 2 attribute bytes
constexpr int64_t STL_RECORD_VERTS = 12;       // the 9 floats start here inside a record

// Two corners are one point when their float32 coordinates compare equal as numbers: -0.0 == +0.0, everything else by its
// bits (a soup with a NaN or an infinity is refused, so no NaN != NaN question arises).  The key is the three words after this.
IVX_MW_HD inline uint32_t canon(uint32_t bits) { return bits == 0x80000000u ? 0u : bits; }

IVX_MW_HD inline bool non_finite(uint32_t bits) { return (bits & 0x7f800000u) == 0x7f800000u; }

IVX_MW_HD inline uint64_t fmix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

// 96 key bits -> 32 hash bits (the finaliser of k_meshtail.hip's edge hash, twice); the home slot is hash & (slots - 1)
IVX_MW_HD inline uint32_t hash(uint32_t kx, uint32_t ky, uint32_t kz) {
    uint64_t k = fmix64(((uint64_t)ky << 32) | (uint64_t)kx);
    k ^= (uint64_t)kz * 0x9e3779b97f4a7c15ULL;
    return (uint32_t)fmix64(k);
}

// slots = the power of two >= 2 * corners (load <= 1/2), no floor beyond 2: small soups get small tables.
// 0 for a corner count outside [0, MAX_CORNERS].
IVX_MW_HD inline uint64_t slots(int64_t n_corners) {
    if (n_corners < 0 || n_corners > MAX_CORNERS) return 0;
    uint64_t s = 2;
    while (s < 2ull * (uint64_t)n_corners) s <<= 1;
    return s;
}

// bucket of the probe-length histogram: 0 extra slots -> 0, then 1, 2-3, 4-7, ... (the last bucket, 15, is open-ended)
IVX_MW_HD inline int probe_bucket(uint64_t extra) {
    int b = 0;
    while (extra) {
        b++;
        extra >>= 1;
    }
    return b < 15 ? b : 15;
}

// byte offset, in the file, of float k (0..8: vertex k / 3, coordinate k % 3) of record t.  Always even, a multiple of 4 only
// for even t.
IVX_MW_HD inline int64_t stl_float_offset(int64_t t, int k) { return STL_HEADER + STL_RECORD * t + STL_RECORD_VERTS + 4 * (int64_t)k; }

IVX_MW_HD inline int64_t stl_file_bytes(int64_t ntris) { return STL_HEADER + STL_RECORD * ntris; }

} // namespace ivx_mesh_weld_math
