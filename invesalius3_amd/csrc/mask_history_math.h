// mask_history_math.h -- the format arithmetic of the mask edit history's volume snapshots: the `blocks64`
// layout of a dense byte stream, where a block's bit and its literal bytes live, and the plane an offset falls into.
// Plain C++ without a GPU construct, so that the very text k_maskhist.hip runs can also be compiled for the host and
// compared with the numpy restatement where there is no GPU (tests/mask_history_host_emu.cpp, tests/test_history_host.py).
//
//   n bytes -> B = cdiv(n, 64) blocks of 64 bytes -> W = cdiv(B, 64) words of 64 blocks
//   header: value[B] u8 (the block's first byte), padded to 8 bytes | literal[W] u64 | base[W] u32
//   pool:   the literal blocks in stream order, 64 bytes each, bytes past n stored as 0
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IVX_MH_HD __host__ __device__
#else
#define IVX_MH_HD
#endif

namespace ivx_mask_history {

constexpr int BLOCK = 64;       // bytes per block
constexpr int WORD_BLOCKS = 64; // blocks per bitmap word (one wave's ballot)

IVX_MH_HD inline int64_t blocks_of(int64_t n) { return (n + BLOCK - 1) / BLOCK; }
IVX_MH_HD inline int64_t words_of(int64_t n) { return (blocks_of(n) + WORD_BLOCKS - 1) / WORD_BLOCKS; }

// byte offsets of the three header arrays and the header's size: a pure function of n
IVX_MH_HD inline int64_t literal_offset(int64_t n) { return (blocks_of(n) + 7) / 8 * 8; }
IVX_MH_HD inline int64_t base_offset(int64_t n) { return literal_offset(n) + 8 * words_of(n); }
IVX_MH_HD inline int64_t header_bytes(int64_t n) { return base_offset(n) + 4 * words_of(n); }

IVX_MH_HD inline int64_t block_word(int64_t block) { return block >> 6; }
IVX_MH_HD inline int block_bit(int64_t block) { return (int)(block & 63); }
IVX_MH_HD inline int64_t block_of_offset(int64_t offset) { return offset / BLOCK; }
// the bits of a word that stand for the blocks before bit `bit`
IVX_MH_HD inline uint64_t below(int bit) { return ((uint64_t)1 << bit) - 1; }
IVX_MH_HD inline int popcount64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}
// a literal block's place in the pool (in blocks; its byte offset is 64 times that)
IVX_MH_HD inline int64_t pool_slot(uint32_t base_w, uint64_t literal_w, int bit) { return (int64_t)base_w + popcount64(literal_w & below(bit)); }
IVX_MH_HD inline int64_t pool_offset(uint32_t base_w, uint64_t literal_w, int bit) { return BLOCK * pool_slot(base_w, literal_w, bit); }
// valid bytes of a block (the last one may be short)
IVX_MH_HD inline int block_len(int64_t block, int64_t n) {
    const int64_t left = n - block * BLOCK;
    return left >= BLOCK ? BLOCK : (left > 0 ? (int)left : 0);
}
IVX_MH_HD inline int64_t plane_of(int64_t offset, int64_t plane_bytes) { return offset / plane_bytes; }
// the planes the bytes [offset, offset + len) touch: first and last
IVX_MH_HD inline void planes_of_range(int64_t offset, int64_t len, int64_t plane_bytes, int64_t *first, int64_t *last) {
    *first = plane_of(offset, plane_bytes);
    *last = plane_of(offset + (len > 0 ? len - 1 : 0), plane_bytes);
}

} // namespace ivx_mask_history
