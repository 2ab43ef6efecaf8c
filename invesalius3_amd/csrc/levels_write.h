// levels_write.h -- the mask's bytes from two bit planes, 1 KiB stretches of four chunks per lane: the body of
// k_flood_apply_levels16 (k_flood.hip), shared with the marching-cubes count that carries the same write in its own launch
// (k_mc_count_write, k_mc.hip).
//
// A chunk is 16 voxels: one 16-bit word of each plane in, one uint4 of mask bytes out -- v_sel where `reached` has a bit, else
// v_in where `inside` has one, else 0.  Lane `tid` of the workgroup that owns the stretch starting at chunk `i0 - tid` handles
// chunks i0, i0 + 256, i0 + 512 and i0 + 768, so each of a wave's four store instructions covers 1 KiB in a row.
// Chunks without a reached bit are not written -- unless ALL: then every chunk is, and `reached` may be NULL (no bit).
// The two halves are separate so that a caller can have other loads in flight between them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ivx {

// WHEN a launch that was queued before the flood's end was known goes ahead (flood_run_impl): only if the list of the round
// that would run next is empty -- the flood is over, `reached` is final -- and then it says so in word 2 of the progress line
// as it starts; otherwise every workgroup returns at once.  `next_len` NULL: unconditional.
struct ApplyWhen {
    const unsigned int *next_len;
    unsigned long long *line;
    unsigned long long report;
};
// true: leave at once.  Otherwise the first lane of the grid has reported (when there is somebody to report to).
__device__ __forceinline__ bool apply_when_skips(const ApplyWhen &when) {
    if (when.next_len) {
        if (*when.next_len != 0u) return true; // (nothing in the stream writes the counter while this kernel runs)
        if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(&when.line[2], when.report, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return false;
}

struct LevelsWords {
    unsigned int m[4], b[4]; // reached / inside words of the lane's four chunks
};

template <bool ALL>
__device__ __forceinline__ void levels_load(const uint16_t *__restrict__ reached, const uint16_t *__restrict__ inside, int64_t nchunks,
                                            int64_t i0, LevelsWords &w) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int64_t i = i0 + u * 256;
        w.m[u] = i < nchunks && (!ALL || reached) ? reached[i] : 0u;
        w.b[u] = i < nchunks ? inside[i] : 0u;
    }
}

template <bool ALL>
__device__ __forceinline__ void levels_store(const LevelsWords &w, int64_t nchunks, int64_t i0, uint4 *__restrict__ out, unsigned int in4,
                                             unsigned int sel4) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (ALL ? i0 + u * 256 >= nchunks : !w.m[u]) continue;
        // bit e of four -> 0xff in byte e (the products' bits e + 7 k are all different: no carries)
        auto bytes = [](unsigned int bits4) { return ((bits4 * 0x00204081u) & 0x01010101u) * 0xffu; };
        auto word = [&](unsigned int r4, unsigned int i4) {
            const unsigned int rs = bytes(r4);
            return (sel4 & rs) | (in4 & bytes(i4) & ~rs);
        };
        out[i0 + u * 256] = make_uint4(word(w.m[u] & 15u, w.b[u] & 15u), word(w.m[u] >> 4 & 15u, w.b[u] >> 4 & 15u),
                                       word(w.m[u] >> 8 & 15u, w.b[u] >> 8 & 15u), word(w.m[u] >> 12 & 15u, w.b[u] >> 12 & 15u));
    }
}

} // namespace ivx
