// k_maskhist.hip -- volume snapshots of the mask edit history: a dense byte stream encoded as `blocks64`
// (mask_history_math.h has the layout), packed, and restored in place with a flag for every plane that changed.
//
// All three kernels share one geometry: a wave owns one bitmap word = 64 blocks = 4096 bytes of the stream and walks it
// in four loads of 16 bytes per lane, so that one load instruction of the wave covers 1 KB of contiguous bytes; four
// neighbouring lanes hold one block.  Every access goes through one bounds rule: byte `off + q` of the stream is read or
// written only when off + q < n.
#include <algorithm>
#include <vector>

#include "ivx_internal.h"
#include "mask_history_math.h"
#include "scan_u32.h"

namespace mh = ivx_mask_history;

namespace {

struct Chunk {
    union {
        uint4 q;
        uint32_t w[4];
        uint8_t b[16];
    };
    int len; // valid bytes: those of [off, off + 16) below n
};

__device__ __forceinline__ int chunk_len(int64_t off, int64_t n) {
    const int64_t left = n - off;
    return left >= 16 ? 16 : (left > 0 ? (int)left : 0);
}

// 16 bytes of the stream at `off`, the ones at and past n as 0 (never loaded)
template <bool ALIGNED> __device__ __forceinline__ Chunk load_chunk(const uint8_t *__restrict__ p, int64_t off, int64_t n) {
    Chunk c;
    c.len = chunk_len(off, n);
    if (ALIGNED && c.len == 16) {
        c.q = *reinterpret_cast<const uint4 *>(p + off);
    } else {
        c.q = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int q = 0; q < 16; q++)
            if (q < c.len) c.b[q] = p[off + q];
    }
    return c;
}

// bit q set <=> byte q (q < len) of a and b differ
__device__ __forceinline__ uint32_t differing_bytes(const Chunk &a, const Chunk &b, int len) {
    if ((a.w[0] ^ b.w[0]) == 0 && (a.w[1] ^ b.w[1]) == 0 && (a.w[2] ^ b.w[2]) == 0 && (a.w[3] ^ b.w[3]) == 0) return 0u;
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 16; q++)
        if (q < len && a.b[q] != b.b[q]) m |= 1u << q;
    return m;
}

constexpr int64_t WAVE_BYTES = mh::BLOCK * mh::WORD_BLOCKS; // 4096

// One pass over the stream: value[], literal[] and the words' popcounts (into base[], scanned afterwards)
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_mh_scan(const uint8_t *__restrict__ src, int64_t n, int64_t B, int64_t W, uint8_t *__restrict__ value,
                                                 uint64_t *__restrict__ literal, uint32_t *__restrict__ base) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= W) return; // (the whole wave: the shuffles and ballots below see all 64 lanes)
    uint64_t word = 0;
    uint32_t my_value = 0; // the first byte of block `lane` of this word
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t off = w * WAVE_BYTES + j * 1024 + lane * 16;
        const Chunk c = load_chunk<ALIGNED>(src, off, n);
        const uint32_t head = c.b[0];
        const uint32_t first = __shfl(head, lane & ~3, 64); // the block's first byte sits in the first of its four lanes
        bool differs;
        if (c.len == 16) {
            const uint32_t vv = first * 0x01010101u;
            differs = ((c.w[0] ^ vv) | (c.w[1] ^ vv) | (c.w[2] ^ vv) | (c.w[3] ^ vv)) != 0;
        } else {
            differs = false;
#pragma unroll
            for (int q = 0; q < 16; q++)
                if (q < c.len && c.b[q] != first) differs = true;
        }
        uint64_t t = __ballot(differs); // four bits per block
        t |= t >> 1;
        t |= t >> 2;
        t &= 0x1111111111111111ull;
        uint32_t bits = 0;
#pragma unroll
        for (int q = 0; q < 16; q++) bits |= (uint32_t)((t >> (4 * q)) & 1) << q;
        word |= (uint64_t)bits << (16 * j);
        const uint32_t v = __shfl(head, (lane & 15) * 4, 64);
        if ((lane >> 4) == j) my_value = v;
    }
    const int64_t blk = w * mh::WORD_BLOCKS + lane;
    if (blk < B) value[blk] = (uint8_t)my_value;
    if (lane == 0) {
        literal[w] = word;
        base[w] = (uint32_t)mh::popcount64(word);
    }
}

// literal block i of the stream -> pool + 64 * (base[w] + popcount(literal[w] & below(bit)))
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_mh_pack(const uint8_t *__restrict__ src, int64_t n, int64_t W, const uint64_t *__restrict__ literal,
                                                 const uint32_t *__restrict__ base, uint8_t *__restrict__ pool, int64_t L) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= W) return;
    const uint64_t word = literal[w];
    if (word == 0) return;
    const uint32_t b0 = base[w];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int bit = j * 16 + (lane >> 2);
        if (!((word >> bit) & 1)) continue;
        const int64_t slot = mh::pool_slot(b0, word, bit);
        if (slot >= L) continue; // (a header that does not belong to this pool: nothing is written outside it)
        const Chunk c = load_chunk<ALIGNED>(src, w * WAVE_BYTES + j * 1024 + lane * 16, n);
        *reinterpret_cast<uint4 *>(pool + slot * mh::BLOCK + (lane & 3) * 16) = c.q;
    }
}

// decode -> dst.  COMPARE: only chunks that hold a differing byte are stored, and the planes of the differing bytes flagged
template <bool ALIGNED, bool COMPARE>
__global__ __launch_bounds__(256) void k_mh_restore(uint8_t *__restrict__ dst, int64_t n, int64_t W, const uint8_t *__restrict__ value,
                                                    const uint64_t *__restrict__ literal, const uint32_t *__restrict__ base,
                                                    const uint8_t *__restrict__ pool, int64_t L, int64_t plane_bytes,
                                                    uint8_t *__restrict__ plane_flags) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= W) return;
    const uint64_t word = literal[w];
    const uint32_t b0 = base[w];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t off = w * WAVE_BYTES + j * 1024 + lane * 16;
        const int len = chunk_len(off, n);
        if (len == 0) continue;
        const int bit = j * 16 + (lane >> 2);
        Chunk want;
        want.len = len;
        if ((word >> bit) & 1) {
            const int64_t slot = mh::pool_slot(b0, word, bit);
            if (slot >= L) continue;
            want.q = *reinterpret_cast<const uint4 *>(pool + slot * mh::BLOCK + (lane & 3) * 16);
        } else {
            const uint32_t vv = (uint32_t)value[w * mh::WORD_BLOCKS + bit] * 0x01010101u;
            want.q = make_uint4(vv, vv, vv, vv);
        }
        uint32_t differ = (1u << len) - 1;
        if (COMPARE) {
            Chunk have = load_chunk<ALIGNED>(dst, off, n);
            if (len < 16) // (bytes past n: zero in `have`, whatever the header says in `want`)
                for (int q = len; q < 16; q++) want.b[q] = 0;
            differ = differing_bytes(want, have, len);
            if (!differ) continue;
        }
        if (ALIGNED && len == 16) {
            *reinterpret_cast<uint4 *>(dst + off) = want.q;
        } else {
#pragma unroll
            for (int q = 0; q < 16; q++)
                if (q < len) dst[off + q] = want.b[q];
        }
        if (COMPARE && plane_flags) {
            const int64_t p0 = mh::plane_of(off, plane_bytes);
            if ((p0 + 1) * plane_bytes - off >= len) {
                plane_flags[p0] = 1; // the whole chunk lies in one plane
            } else {
                for (int q = 0; q < len; q++)
                    if ((differ >> q) & 1) plane_flags[mh::plane_of(off + q, plane_bytes)] = 1;
            }
        }
    }
}

struct Header {
    uint8_t *value;
    uint64_t *literal;
    uint32_t *base;
};
inline Header header_of(void *header, int64_t n) {
    Header h;
    h.value = (uint8_t *)header;
    h.literal = (uint64_t *)((uint8_t *)header + mh::literal_offset(n));
    h.base = (uint32_t *)((uint8_t *)header + mh::base_offset(n));
    return h;
}
inline bool grid_ok(int64_t n, unsigned *grid) {
    const int64_t g = ivx::cdiv(mh::words_of(n), 4);
    if (g <= 0 || g >= ((int64_t)1 << 31)) return false;
    *grid = (unsigned)g;
    return true;
}

} // namespace

extern "C" int ivx_mask_snapshot_header_bytes(int64_t n, size_t *nbytes) {
    IVX_REQUIRE(n >= 0 && nbytes, IVX_EINVAL, "mask_snapshot_header_bytes: negative size or null");
    *nbytes = (size_t)mh::header_bytes(n);
    return IVX_OK;
}

extern "C" int ivx_dev_mask_snapshot_scan(const uint8_t *src, int64_t n, void *header, int64_t *literal_blocks, void *stream) {
    IVX_REQUIRE(n >= 0 && literal_blocks, IVX_EINVAL, "mask_snapshot_scan: negative size or null");
    *literal_blocks = 0;
    if (n == 0) return IVX_OK;
    IVX_REQUIRE(src && header && (uintptr_t)header % 8 == 0, IVX_EINVAL, "mask_snapshot_scan: null or misaligned header");
    unsigned grid;
    IVX_REQUIRE(grid_ok(n, &grid), IVX_EINVAL, "mask_snapshot_scan: %lld bytes", (long long)n);
    hipStream_t st = ivx::S(stream);
    const int64_t B = mh::blocks_of(n), W = mh::words_of(n);
    const Header h = header_of(header, n);
    if (mh::literal_offset(n) > B) IVX_HIP(hipMemsetAsync(h.value + B, 0, (size_t)(mh::literal_offset(n) - B), st)); // the padding
    if (((uintptr_t)src & 15) == 0) hipLaunchKernelGGL(k_mh_scan<true>, dim3(grid), dim3(256), 0, st, src, n, B, W, h.value, h.literal, h.base);
    else
        hipLaunchKernelGGL(k_mh_scan<false>, dim3(grid), dim3(256), 0, st, src, n, B, W, h.value, h.literal, h.base);
    IVX_LAUNCH_CHECK();
    void *ws;
    int rc;
    const int64_t nsb = scan_u32_blocks(W);
    if ((rc = ivx::ws_get_s(ivx::WS_SMALL, st, (size_t)(nsb + 2) * 4 + 64, &ws))) return rc;
    uint32_t *bsum = (uint32_t *)ws, *total = bsum + nsb + 1;
    if ((rc = scan_u32_exclusive(h.base, W, bsum, total, st))) return rc;
    uint32_t L = 0;
    IVX_HIP(hipMemcpyAsync(&L, total, 4, hipMemcpyDeviceToHost, st));
    IVX_HIP(hipStreamSynchronize(st)); // the one wait of a snapshot: the pool is sized from L
    *literal_blocks = (int64_t)L;
    return IVX_OK;
}

extern "C" int ivx_dev_mask_snapshot_pack(const uint8_t *src, int64_t n, const void *header, void *pool, int64_t literal_blocks,
                                          void *stream) {
    IVX_REQUIRE(n >= 0 && literal_blocks >= 0, IVX_EINVAL, "mask_snapshot_pack: negative size");
    if (n == 0 || literal_blocks == 0) return IVX_OK;
    IVX_REQUIRE(src && header && pool && (uintptr_t)header % 8 == 0 && (uintptr_t)pool % 16 == 0, IVX_EINVAL,
                "mask_snapshot_pack: null or misaligned block");
    IVX_REQUIRE(literal_blocks <= mh::blocks_of(n), IVX_EINVAL, "mask_snapshot_pack: %lld literal blocks of %lld", (long long)literal_blocks,
                (long long)mh::blocks_of(n));
    unsigned grid;
    IVX_REQUIRE(grid_ok(n, &grid), IVX_EINVAL, "mask_snapshot_pack: %lld bytes", (long long)n);
    const Header h = header_of(const_cast<void *>(header), n);
    const int64_t W = mh::words_of(n);
    if (((uintptr_t)src & 15) == 0)
        hipLaunchKernelGGL(k_mh_pack<true>, dim3(grid), dim3(256), 0, ivx::S(stream), src, n, W, (const uint64_t *)h.literal,
                           (const uint32_t *)h.base, (uint8_t *)pool, literal_blocks);
    else
        hipLaunchKernelGGL(k_mh_pack<false>, dim3(grid), dim3(256), 0, ivx::S(stream), src, n, W, (const uint64_t *)h.literal,
                           (const uint32_t *)h.base, (uint8_t *)pool, literal_blocks);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

namespace {
template <bool COMPARE>
int restore_launch(uint8_t *dst, int64_t n, const void *header, const void *pool, int64_t L, int64_t plane_bytes, uint8_t *flags,
                   hipStream_t st) {
    unsigned grid;
    IVX_REQUIRE(grid_ok(n, &grid), IVX_EINVAL, "mask_snapshot_restore: %lld bytes", (long long)n);
    const Header h = header_of(const_cast<void *>(header), n);
    const int64_t W = mh::words_of(n);
    if (((uintptr_t)dst & 15) == 0)
        hipLaunchKernelGGL((k_mh_restore<true, COMPARE>), dim3(grid), dim3(256), 0, st, dst, n, W, (const uint8_t *)h.value,
                           (const uint64_t *)h.literal, (const uint32_t *)h.base, (const uint8_t *)pool, L, plane_bytes, flags);
    else
        hipLaunchKernelGGL((k_mh_restore<false, COMPARE>), dim3(grid), dim3(256), 0, st, dst, n, W, (const uint8_t *)h.value,
                           (const uint64_t *)h.literal, (const uint32_t *)h.base, (const uint8_t *)pool, L, plane_bytes, flags);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}
int restore_check(const char *what, const void *dst, int64_t n, const void *header, const void *pool, int64_t L) {
    IVX_REQUIRE(n >= 0 && L >= 0 && L <= mh::blocks_of(n), IVX_EINVAL, "%s: %lld bytes, %lld literal blocks", what, (long long)n, (long long)L);
    if (n == 0) return IVX_OK;
    IVX_REQUIRE(dst && header && (uintptr_t)header % 8 == 0 && (pool || !L) && (uintptr_t)pool % 16 == 0, IVX_EINVAL,
                "%s: null or misaligned block", what);
    return IVX_OK;
}
} // namespace

extern "C" int ivx_dev_mask_snapshot_restore(uint8_t *dst, int64_t n, const void *header, const void *pool, int64_t literal_blocks,
                                             int64_t plane_bytes, uint8_t *plane_flags, void *stream) {
    int rc = restore_check("mask_snapshot_restore", dst, n, header, pool, literal_blocks);
    if (rc || n == 0) return rc;
    IVX_REQUIRE(!plane_flags || plane_bytes >= 1, IVX_EINVAL, "mask_snapshot_restore: planes of %lld bytes", (long long)plane_bytes);
    return restore_launch<true>(dst, n, header, pool, literal_blocks, plane_flags ? plane_bytes : 1, plane_flags, ivx::S(stream));
}

// ---- host forms ---------------------------------------------------------------------------------------------------------------
extern "C" int ivx_mask_snapshot(const uint8_t *matrix, size_t nbytes, void **header_out, void **pool_out, int64_t *literal_blocks) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(matrix && nbytes && header_out && pool_out && literal_blocks, IVX_EINVAL, "mask_snapshot: null or empty");
    IVX_REQUIRE(nbytes < ((size_t)1 << 46), IVX_EINVAL, "mask_snapshot: %zu bytes", nbytes);
    *header_out = *pool_out = nullptr;
    *literal_blocks = 0;
    const int64_t n = (int64_t)nbytes;
    int rc;
    MirrorHold *hold;
    void *src;
    if ((rc = mirror_acquire(matrix, nbytes, true, &hold, &src))) return rc;
    if (!src) { // not registered: staged once
        if ((rc = ws_get(WS_IN, nbytes, &src))) return rc;
        if ((rc = copy_h2d(src, matrix, nbytes))) return rc;
    }
    void *hdr = nullptr, *pool = nullptr;
    int64_t L = 0;
    hipError_t e = hipMalloc(&hdr, (size_t)mh::header_bytes(n));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("mask_snapshot: no device memory for a header of %lld bytes", (long long)mh::header_bytes(n));
        rc = IVX_ENOMEM;
    }
    if (!rc) rc = ivx_dev_mask_snapshot_scan((const uint8_t *)src, n, hdr, &L, nullptr);
    if (!rc) {
        e = hipMalloc(&pool, L ? (size_t)L * mh::BLOCK : 16);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("mask_snapshot: no device memory for a pool of %lld blocks", (long long)L);
            rc = IVX_ENOMEM;
        }
    }
    if (!rc) rc = ivx_dev_mask_snapshot_pack((const uint8_t *)src, n, hdr, pool, L, nullptr);
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) {
        set_error("mask_snapshot: the pack did not complete");
        rc = IVX_EHIP;
    }
    mirror_release(hold, 0);
    if (rc) {
        if (hdr) (void)hipFree(hdr);
        if (pool) (void)hipFree(pool);
        return rc;
    }
    *header_out = hdr;
    *pool_out = pool;
    *literal_blocks = L;
    return IVX_OK;
}

extern "C" int ivx_mask_snapshot_restore(uint8_t *matrix, size_t nbytes, const void *header, const void *pool, int64_t literal_blocks,
                                         size_t plane_bytes, int64_t *planes_written) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(matrix && nbytes && plane_bytes, IVX_EINVAL, "mask_snapshot_restore: null or empty");
    IVX_REQUIRE(nbytes < ((size_t)1 << 46), IVX_EINVAL, "mask_snapshot_restore: %zu bytes", nbytes);
    const int64_t n = (int64_t)nbytes, pb = (int64_t)plane_bytes, nplanes = cdiv(n, pb);
    int rc;
    if ((rc = restore_check("mask_snapshot_restore", matrix, n, header, pool, literal_blocks))) return rc;
    if (planes_written) *planes_written = 0;
    MirrorHold *hold;
    void *mirror;
    if ((rc = mirror_acquire(matrix, nbytes, true, &hold, &mirror))) return rc;
    if (!mirror) { // nothing to compare with: decoded into a workspace block, all of it downloaded
        void *d;
        if ((rc = ws_get(WS_OUT, nbytes, &d))) return rc;
        if ((rc = restore_launch<false>((uint8_t *)d, n, header, pool, literal_blocks, 1, nullptr, nullptr))) return rc;
        IVX_HIP(hipStreamSynchronize(nullptr));
        if ((rc = copy_d2h(matrix, d, nbytes))) return rc;
        if (planes_written) *planes_written = nplanes;
        return IVX_OK;
    }
    // into the mirror, then the planes that changed to the host: host and mirror hold the same bytes afterwards
    std::vector<uint8_t> flags((size_t)nplanes);
    void *d_flags;
    int64_t written = 0;
    rc = ws_get(WS_AUX0, (size_t)nplanes, &d_flags);
    if (!rc && hipMemsetAsync(d_flags, 0, (size_t)nplanes, nullptr) != hipSuccess) rc = IVX_EHIP;
    if (!rc) rc = restore_launch<true>((uint8_t *)mirror, n, header, pool, literal_blocks, pb, (uint8_t *)d_flags, nullptr);
    if (!rc && hipMemcpy(flags.data(), d_flags, (size_t)nplanes, hipMemcpyDeviceToHost) != hipSuccess) rc = IVX_EHIP; // (small, like seeds)
    if (rc == IVX_EHIP) set_error("mask_snapshot_restore: the restore did not complete (%s)", hipGetErrorString(hipGetLastError()));
    for (int64_t p = 0; !rc && p < nplanes;) {
        if (!flags[(size_t)p]) {
            p++;
            continue;
        }
        int64_t q = p;
        while (q < nplanes && flags[(size_t)q]) q++;
        const int64_t lo = p * pb, hi = std::min(q * pb, n);
        rc = mirror_fetch(hold, matrix + lo, (const uint8_t *)mirror + lo, (size_t)(hi - lo));
        written += q - p;
        p = q;
    }
    mirror_release(hold, (size_t)std::min(written * pb, n));
    if (!rc && planes_written) *planes_written = written;
    return rc;
}
