// partition_u32.h -- stable many-way partition of n items by a uint32 key < nkeys: the stable order (item indices grouped by key,
// original order inside a key) and offsets[nkeys + 1] (offsets[k] = number of items with a key below k).
// Hand-written LSD radix sort of (key, item) pairs, 8 bits per pass, ceil(bits(nkeys - 1) / 8) passes (at least one); a pass is
//   k_part_hist     digit histogram per workgroup of PART_BLOCK_ITEMS items, stored digit-major: hist[digit * nblocks + block]
//   scan_u32        exclusive scan of that table = first output slot of every (digit, block)
//   k_part_scatter  the workgroup walks its items again, 256 at a time; a lane's slot = the (digit, block) base + the items
//                   of its digit in earlier chunks + those in earlier waves of the chunk (LDS) + those in lower lanes of its
//                   wave (wave64 ballot match)
// Every count is aggregated per wave before it touches LDS (one add / store per distinct digit per wave): on a real surface
// ~80 % of the keys are ONE region, the hazard k_mesh_tricount pre-aggregates for.  Histogram and scatter take an item's
// index and digit from the same two inline functions, and every scatter store is bounded by n, so the two kernels cannot
// disagree into memory outside the buffers.  No atomics on global memory, integer arithmetic only: deterministic.
// Streams 16 bytes per item and pass (key + item read, key + item written) plus 4 for the histogram's read of the key.
// Included by the translation units that need it (kernels live in each unit's anonymous namespace); needs scan_u32.h.
#pragma once
#include "ivx_internal.h"
#include "scan_u32.h"

namespace {

constexpr int PART_DIGIT_BITS = 8;
constexpr int PART_DIGITS = 1 << PART_DIGIT_BITS; // == the workgroup size: lane d owns digit d's LDS words
constexpr int PART_CHUNKS = 8;
constexpr int PART_BLOCK_ITEMS = 256 * PART_CHUNKS;

__device__ __forceinline__ uint32_t part_digit(uint32_t key, int shift) { return (key >> shift) & (uint32_t)(PART_DIGITS - 1); }
__device__ __forceinline__ int64_t part_item(uint32_t block, int chunk, uint32_t tid) {
    return (int64_t)block * PART_BLOCK_ITEMS + (int64_t)chunk * 256 + tid;
}
// the lanes of this wave that hold an item (`ok`) with the same digit as this lane's; meaningless in a lane without an item.
// Must be reached by all 64 lanes.
__device__ __forceinline__ unsigned long long part_peers(uint32_t digit, bool ok) {
    unsigned long long peers = __ballot(ok);
#pragma unroll
    for (int b = 0; b < PART_DIGIT_BITS; b++) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long m = __ballot(ok && bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

__global__ __launch_bounds__(256) void k_part_hist(const uint32_t *__restrict__ keys, int64_t n, int shift, uint32_t nblocks,
                                                   uint32_t *__restrict__ hist) {
    __shared__ uint32_t s_h[PART_DIGITS];
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int c = 0; c < PART_CHUNKS; c++) {
        const int64_t i = part_item(blockIdx.x, c, threadIdx.x);
        const bool ok = i < n;
        const uint32_t d = ok ? part_digit(keys[i], shift) : 0u;
        const unsigned long long peers = part_peers(d, ok);
        if (ok && lane == __builtin_ctzll(peers)) atomicAdd(&s_h[d], (uint32_t)__popcll(peers));
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * nblocks + blockIdx.x] = s_h[threadIdx.x];
}

// vals == nullptr: the items are numbered 0 .. n - 1 (the first pass)
__global__ __launch_bounds__(256) void k_part_scatter(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, int64_t n,
                                                      int shift, uint32_t nblocks, const uint32_t *__restrict__ hist,
                                                      uint32_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out) {
    __shared__ uint32_t s_base[PART_DIGITS];
    __shared__ uint32_t s_wave[4][PART_DIGITS];
    s_base[threadIdx.x] = hist[(size_t)threadIdx.x * nblocks + blockIdx.x];
#pragma unroll
    for (int w = 0; w < 4; w++) s_wave[w][threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int c = 0; c < PART_CHUNKS; c++) {
        const int64_t i = part_item(blockIdx.x, c, threadIdx.x);
        const bool ok = i < n;
        const uint32_t key = ok ? keys[i] : 0u;
        const uint32_t d = ok ? part_digit(key, shift) : 0u;
        const unsigned long long peers = part_peers(d, ok);
        if (ok && lane == __builtin_ctzll(peers)) s_wave[wv][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (ok) {
            uint32_t dst = s_base[d] + (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
            for (int w = 0; w < wv; w++) dst += s_wave[w][d];
            if ((int64_t)dst < n) {
                keys_out[dst] = key;
                vals_out[dst] = vals ? vals[i] : (uint32_t)i;
            }
        }
        __syncthreads();
        s_base[threadIdx.x] += (s_wave[0][threadIdx.x] + s_wave[1][threadIdx.x]) + (s_wave[2][threadIdx.x] + s_wave[3][threadIdx.x]);
#pragma unroll
        for (int w = 0; w < 4; w++) s_wave[w][threadIdx.x] = 0u;
        __syncthreads();
    }
}

// offsets[k] = number of items with a key < k, k = 0 .. nkeys, from the sorted keys: position i closes every key between its
// left neighbour's (exclusive) and its own (inclusive); each entry is written by exactly one lane
__global__ __launch_bounds__(256) void k_part_offsets(const uint32_t *__restrict__ sorted, int64_t n, uint32_t nkeys,
                                                      uint32_t *__restrict__ offsets) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const int64_t prev = i == 0 ? -1 : (int64_t)sorted[i - 1];
    int64_t cur = i == n ? (int64_t)nkeys : (int64_t)sorted[i];
    if (cur > (int64_t)nkeys) cur = nkeys;
    for (int64_t k = prev + 1; k <= cur; k++) offsets[k] = (uint32_t)i;
}

static inline int partition_u32_passes(uint32_t nkeys) {
    int bits = 0;
    while (bits < 32 && ((uint64_t)1 << bits) < (uint64_t)nkeys) bits++; // bits(nkeys - 1)
    const int p = (bits + PART_DIGIT_BITS - 1) / PART_DIGIT_BITS;
    return p > 0 ? p : 1;
}
static inline int64_t partition_u32_blocks(int64_t n) { return ivx::cdiv(n, PART_BLOCK_ITEMS); }
// words of scratch behind `hist`: the digit-major table, then the scan's block sums and its total
static inline size_t partition_u32_hist_words(int64_t n) {
    const int64_t tbl = partition_u32_blocks(n) * PART_DIGITS;
    return (size_t)tbl + (size_t)scan_u32_blocks(tbl) + 16;
}

// keys[0] holds the n keys (all < nkeys) on entry; keys[1], vals[0], vals[1] are n words of scratch each, hist
// partition_u32_hist_words(n) words.  On return *order points at the stable order (into vals[]), *sorted at the sorted keys
// (into keys[]), and offsets[0 .. nkeys] is filled.  n >= 1, n < 2^31.
static inline int partition_u32(uint32_t *const keys[2], uint32_t *const vals[2], int64_t n, uint32_t nkeys, uint32_t *hist,
                                uint32_t *offsets, const uint32_t **order, const uint32_t **sorted, hipStream_t st) {
    const int passes = partition_u32_passes(nkeys);
    const uint32_t nb = (uint32_t)partition_u32_blocks(n);
    const int64_t tbl = (int64_t)nb * PART_DIGITS;
    uint32_t *bsum = hist + tbl, *total = bsum + scan_u32_blocks(tbl) + 8;
    int rc;
    for (int p = 0; p < passes; p++) {
        const uint32_t *kin = keys[p & 1], *vin = p ? vals[p & 1] : nullptr;
        hipLaunchKernelGGL(k_part_hist, dim3(nb), dim3(256), 0, st, kin, n, p * PART_DIGIT_BITS, nb, hist);
        IVX_LAUNCH_CHECK();
        if ((rc = scan_u32_exclusive(hist, tbl, bsum, total, st))) return rc;
        hipLaunchKernelGGL(k_part_scatter, dim3(nb), dim3(256), 0, st, kin, vin, n, p * PART_DIGIT_BITS, nb, (const uint32_t *)hist,
                           keys[(p + 1) & 1], vals[(p + 1) & 1]);
        IVX_LAUNCH_CHECK();
    }
    *order = vals[passes & 1];
    *sorted = keys[passes & 1];
    hipLaunchKernelGGL(k_part_offsets, dim3((unsigned)ivx::cdiv(n + 1, 256)), dim3(256), 0, st, *sorted, n, nkeys, offsets);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

} // namespace
