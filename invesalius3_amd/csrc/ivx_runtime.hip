// ivx_runtime.hip -- runtime plumbing of libivx.so: errors, device memory, streams, events,
// cached workspaces and the strided host<->dense device staging used by the host-level entry points.
#include <execinfo.h>
#include <signal.h>
#include <stdarg.h>
#include <stdlib.h>
#include <sys/mman.h>
#include <unistd.h>

#include <atomic>
#include <map>
#include <vector>
#include <mutex>
#include <thread>
#include <vector>

#include "ivx_internal.h"
#include "mailbox_slot.h"
#include "resident_ranges.h"

namespace ivx {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

bool trace_enabled() {
    static const bool on = getenv("IVX_TRACE") != nullptr;
    return on;
}

struct Slot {
    void *p = nullptr;
    size_t n = 0;
};
static Slot g_ws[WS_COUNT];
static Slot g_hs[WS_COUNT];
static std::mutex g_mu;

int ws_get(int slot, size_t nbytes, void **dptr) {
    std::lock_guard<std::mutex> lk(g_mu);
    Slot &s = g_ws[slot];
    if (nbytes == 0) nbytes = 16;
    if (s.n < nbytes) {
        if (s.p) IVX_HIP(hipFree(s.p));
        s.p = nullptr;
        s.n = 0;
        size_t want = nbytes + (nbytes >> 3) + 4096; // a little slack so growing volumes do not thrash
        IVX_HIP(hipMalloc(&s.p, want));
        s.n = want;
    }
    *dptr = s.p;
    return IVX_OK;
}

static std::map<std::pair<int, hipStream_t>, Slot> g_ws_stream;

int ws_get_s(int slot, hipStream_t stream, size_t nbytes, void **dptr) {
    if (stream == nullptr) return ws_get(slot, nbytes, dptr);
    std::lock_guard<std::mutex> lk(g_mu);
    Slot &s = g_ws_stream[std::make_pair(slot, stream)];
    if (nbytes == 0) nbytes = 16;
    if (s.n < nbytes) {
        if (s.p) IVX_HIP(hipFree(s.p)); // synchronises the device: nothing can still be using the old block
        s.p = nullptr;
        s.n = 0;
        size_t want = nbytes + (nbytes >> 3) + 4096;
        IVX_HIP(hipMalloc(&s.p, want));
        s.n = want;
    }
    *dptr = s.p;
    return IVX_OK;
}

// give a stream's slot back when it holds more than `keep_below` bytes (big, rarely needed blocks: the IFT flood's link records)
int ws_release_s(int slot, hipStream_t stream, size_t keep_below) {
    std::lock_guard<std::mutex> lk(g_mu);
    Slot *s = nullptr;
    if (stream == nullptr) {
        s = &g_ws[slot];
    } else {
        auto it = g_ws_stream.find(std::make_pair(slot, stream));
        if (it == g_ws_stream.end()) return IVX_OK;
        s = &it->second;
    }
    if (s->p && s->n > keep_below) {
        IVX_HIP(hipFree(s->p));
        s->p = nullptr;
        s->n = 0;
    }
    return IVX_OK;
}

static std::recursive_mutex g_host_mu;
static int g_host_depth = 0;       // nesting of host-level entry points (they call each other)
static uint64_t g_host_epoch = 1;  // one per OUTERMOST host call: what upload_strided staged stays valid inside it
static void ivx_bt_handler(int sig);
HostCallGuard::HostCallGuard() {
    g_host_mu.lock();
    if (g_host_depth++ == 0) g_host_epoch++;
    static const bool bt = getenv("IVX_BACKTRACE") != nullptr;
    if (bt) { // re-arm on every host call: test runners install their own handlers after the library is loaded
        signal(SIGABRT, ivx_bt_handler);
        signal(SIGSEGV, ivx_bt_handler);
    }
}
uint64_t host_epoch() { return g_host_epoch; } // (the number of the running outermost host call)
HostCallGuard::~HostCallGuard() {
    g_host_depth--;
    g_host_mu.unlock();
}

int hs_get(int slot, size_t nbytes, void **hptr) {
    std::lock_guard<std::mutex> lk(g_mu);
    Slot &s = g_hs[slot];
    if (nbytes == 0) nbytes = 16;
    if (s.n < nbytes) {
        if (s.p) IVX_HIP(hipHostFree(s.p));
        s.p = nullptr;
        s.n = 0;
        size_t want = nbytes + (nbytes >> 3) + 4096;
        IVX_HIP(hipHostMalloc(&s.p, want, hipHostMallocDefault));
        s.n = want;
    }
    *hptr = s.p;
    return IVX_OK;
}

// ---- pageable host memory at (nearly) the link's rate ----------------------------------------------------------------
// The reference hands np.memmap / plain numpy arrays over (invesalius/data/mask.py:422-431, slice_.py:192): pageable memory.
// What that costs was measured per direction (see copy_h2d / copy_d2h below): a warm pageable upload already runs at the
// link's rate (the runtime locks the user pages), a download into pages that were never touched -- the np.empty result array
// of every call -- does not: one thread takes every page fault and the copy crawls at 25 GB/s.  For that case a copy of
// >= 4 MB is cut into chunks that a few host threads ("lanes") move through their own page-locked double buffers on their own
// streams: while the DMA engine carries chunk k of a lane, the lane's thread unpacks chunk k - lanes, so the page faults of the
// fresh array are spread over the lanes (46 GB/s).  A pointer that is already page-locked (ivx_host_alloc, hipHostRegister)
// goes straight to hipMemcpy.  Synchronous like hipMemcpy: the bytes are in place on return.
namespace {
constexpr size_t STAGE_MIN = 4u << 20;
constexpr int STAGE_MAX_LANES = 16;
static size_t stage_chunk() { // bytes per lane buffer (IVX_STAGE_CHUNK_MB: 1 .. 64, default 4)
    static const size_t n = []() {
        const char *e = getenv("IVX_STAGE_CHUNK_MB");
        long v = e ? atol(e) : 4;
        if (v < 1) v = 1;
        if (v > 64) v = 64;
        return (size_t)v << 20;
    }();
    return n;
}
struct StageLane {
    void *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t st = nullptr;
};
struct StageCtx {
    int nl = 0;
    StageLane lane[STAGE_MAX_LANES];
};
static std::mutex g_stage_mu; // one staged copy at a time (the lanes are the parallelism)
static std::map<int, StageCtx> g_stage;

static int stage_lanes() {
    static const int n = []() {
        const char *e = getenv("IVX_STAGE_THREADS");
        int v = e ? atoi(e) : 0;
        if (!e) {
            const unsigned hc = std::thread::hardware_concurrency();
            v = hc >= 16 ? 8 : hc >= 8 ? 4 : hc >= 4 ? 2 : 0;
        }
        return v < 0 ? 0 : v > STAGE_MAX_LANES ? STAGE_MAX_LANES : v;
    }();
    return n;
}

static bool host_is_pinned(const void *p) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError(); // unregistered memory: the query fails, and that failure must not linger
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

static int stage_ctx(int dev, StageCtx **out) {
    StageCtx &c = g_stage[dev];
    const int want = stage_lanes();
    while (c.nl < want) {
        StageLane &l = c.lane[c.nl];
        IVX_HIP(hipStreamCreateWithFlags(&l.st, hipStreamNonBlocking));
        for (int q = 0; q < 2; q++) {
            IVX_HIP(hipHostMalloc(&l.buf[q], stage_chunk(), hipHostMallocDefault));
            IVX_HIP(hipEventCreateWithFlags(&l.ev[q], hipEventDisableTiming));
        }
        c.nl++;
    }
    *out = &c;
    return IVX_OK;
}

// to_device: dev <- host, else host <- dev
static int staged_copy(void *dev_p, void *host_p, size_t n, bool to_device) {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    int dev = 0;
    IVX_HIP(hipGetDevice(&dev));
    StageCtx *c;
    int rc = stage_ctx(dev, &c);
    if (rc) return rc;
    IVX_HIP(hipStreamSynchronize(nullptr));
    const size_t STAGE_CHUNK = stage_chunk();
    const size_t nchunks = (n + STAGE_CHUNK - 1) / STAGE_CHUNK;
    const int nl = (size_t)c->nl < nchunks ? c->nl : (int)nchunks;
    std::vector<hipError_t> err((size_t)nl, hipSuccess);
    auto work = [&](int t) {
        hipError_t e = hipSetDevice(dev);
        StageLane &l = c->lane[t];
        char *d = (char *)dev_p, *h = (char *)host_p;
        size_t prev = 0, prev_len = 0;
        int k = 0;
        for (size_t i = (size_t)t; i < nchunks && e == hipSuccess; i += (size_t)nl, k++) {
            const int q = k & 1;
            const size_t off = i * STAGE_CHUNK, len = n - off < STAGE_CHUNK ? n - off : STAGE_CHUNK;
            if (to_device) {
                if (k >= 2) e = hipEventSynchronize(l.ev[q]); // the DMA that last read this buffer
                if (e != hipSuccess) break;
                memcpy(l.buf[q], h + off, len);
                e = hipMemcpyAsync(d + off, l.buf[q], len, hipMemcpyHostToDevice, l.st);
                if (e == hipSuccess) e = hipEventRecord(l.ev[q], l.st);
            } else {
                e = hipMemcpyAsync(l.buf[q], d + off, len, hipMemcpyDeviceToHost, l.st);
                if (e == hipSuccess) e = hipEventRecord(l.ev[q], l.st);
                if (k >= 1 && e == hipSuccess) { // unpack the previous chunk while this one is in flight
                    e = hipEventSynchronize(l.ev[q ^ 1]);
                    if (e == hipSuccess) memcpy(h + prev, l.buf[q ^ 1], prev_len);
                }
                prev = off;
                prev_len = len;
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(l.st);
        if (!to_device && e == hipSuccess && k >= 1) memcpy(h + prev, l.buf[(k - 1) & 1], prev_len);
        err[(size_t)t] = e;
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nl; t++) th.emplace_back(work, t);
    work(0);
    for (auto &t : th) t.join();
    for (int t = 0; t < nl; t++)
        if (err[(size_t)t] != hipSuccess) {
            set_error("staged %s copy of %zu bytes: %s", to_device ? "host-to-device" : "device-to-host", n, hipGetErrorString(err[(size_t)t]));
            return err[(size_t)t] == hipErrorOutOfMemory ? IVX_ENOMEM : IVX_EHIP;
        }
    return IVX_OK;
}
} // namespace

// fraction of a sample of the range's pages that are not resident yet (a fresh np.empty / a new memmap): writing into such a
// range is bound by its page faults, which the lanes take in parallel
static bool mostly_untouched(const void *p, size_t n) {
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE);
    const uintptr_t a0 = ((uintptr_t)p + pg - 1) & ~(uintptr_t)(pg - 1), a1 = ((uintptr_t)p + n) & ~(uintptr_t)(pg - 1);
    if (a1 <= a0 + 32 * pg) return false;
    const size_t npages = (a1 - a0) / pg;
    int missing = 0;
    constexpr int SAMPLES = 32;
    for (int q = 0; q < SAMPLES; q++) {
        unsigned char v = 0;
        const uintptr_t a = a0 + (npages - 1) * (size_t)q / (SAMPLES - 1) * pg;
        if (mincore((void *)a, pg, &v) != 0) return false;
        missing += !(v & 1);
    }
    return missing * 2 > SAMPLES;
}

// Measured on the MI355X box (tools/bench_stage.py, profiles/r04_stage_copies.txt; 630 MB of one bench step):
//   host -> device, pageable, warm: hipMemcpy 55.7 GB/s (the runtime locks the user pages itself), lanes 22 - 50 GB/s  -> hipMemcpy
//   device -> host into pages never touched (np.empty): hipMemcpy 24.9 GB/s (faults taken by one thread), lanes 46 GB/s -> lanes
//   device -> host into touched pages: hipMemcpy 55 GB/s, lanes 47 GB/s                                                 -> hipMemcpy
// IVX_STAGE_THREADS=0 never uses the lanes; IVX_STAGE_UP=1 sends uploads through them as well (A/B).
// (bytes the helpers of this file really moved across the link, ivx_transfer_stats: [0] host -> device, [1] device -> host,
// [2] host -> device for the stale check alone (not in [0]), [3] served device -> device from a resident mirror)
static std::atomic<uint64_t> g_xfer[4];
static int raw_h2d(void *dst_dev, const void *src, size_t n) {
    if (!n) return IVX_OK;
    g_xfer[0].fetch_add(n, std::memory_order_relaxed);
    static const bool up = []() { const char *e = getenv("IVX_STAGE_UP"); return e && e[0] == '1'; }();
    if (up && n >= STAGE_MIN && stage_lanes() > 0 && !host_is_pinned(src)) return staged_copy(dst_dev, const_cast<void *>(src), n, true);
    IVX_HIP(hipMemcpy(dst_dev, src, n, hipMemcpyHostToDevice));
    return IVX_OK;
}
static int raw_d2h(void *dst, const void *src_dev, size_t n) {
    if (!n) return IVX_OK;
    g_xfer[1].fetch_add(n, std::memory_order_relaxed);
    // IVX_D2H_LANES (read per call: A/B runs flip it inside one process): 1 = every pageable destination through the lanes,
    // 0 = never, unset = where the destination's pages are mostly not resident yet
    const char *force = getenv("IVX_D2H_LANES");
    const bool lanes_ok = n >= STAGE_MIN && stage_lanes() > 0 && !(force && force[0] == '0');
    if (lanes_ok && ((force && force[0] == '1') || mostly_untouched(dst, n)) && !host_is_pinned(dst))
        return staged_copy(const_cast<void *>(src_dev), dst, n, false);
    IVX_HIP(hipMemcpy(dst, src_dev, n, hipMemcpyDeviceToHost));
    return IVX_OK;
}

static inline bool dense3(const int64_t shape[3], const int64_t st[3], size_t isz) {
    return st[2] == (int64_t)isz && st[1] == shape[2] * (int64_t)isz && st[0] == shape[1] * shape[2] * (int64_t)isz;
}

// ---- strided host views at PCIe speed ------------------------------------------------------------------------
// The views the GUI passes -- `mask.matrix[1:, 1:, 1:]` of the (d+1, h+1, w+1) memmap, axis-sliced slabs -- are
// sub-boxes of a C-contiguous parent: contiguous rows, constant pitches.  Such a view lies inside ONE contiguous byte
// span of the parent that is barely larger than the view itself, so it travels as one dense copy each way and the
// re-pitching is a device kernel (TB/s) instead of a host memcpy per row (the round-1 path: 65 ms for a 512^3 mask).
// On the way back the span is first fetched (unless this very call uploaded it), the kernel scatters the result into
// the view's bytes, and the whole span returns: the parent's pad / flag cells between the rows come back unchanged.
struct SpanSlot {
    void *d = nullptr;
    size_t cap = 0;
    const void *host = nullptr;
    size_t nbytes = 0;
    uint64_t epoch = 0;
};
static SpanSlot g_span[WS_COUNT];

static bool span_of(const int64_t shape[3], const int64_t st[3], size_t isz, size_t *span) {
    const int64_t row = shape[2] * (int64_t)isz;
    if (st[2] != (int64_t)isz || st[1] < row || st[0] < st[1] * shape[1]) return false;
    const size_t n = (size_t)shape[0] * shape[1] * row;
    const size_t sp = (size_t)(shape[0] - 1) * st[0] + (size_t)(shape[1] - 1) * st[1] + row;
    if (sp > n + n / 4 + 65536) return false; // a thin slice of a big parent: not worth moving the parent
    *span = sp;
    return true;
}

// dense (rows packed) <-> pitched, 16 bytes of the dense side per lane; TO_PITCHED: dense -> pitched
template <bool TO_PITCHED>
__global__ __launch_bounds__(256) void k_repitch(uint8_t *__restrict__ pitched, int64_t p0, int64_t p1, uint8_t *__restrict__ dense,
                                                 int64_t nz, int64_t ny, int64_t row) {
    const int64_t chunks = (row + 15) / 16;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nz * ny * chunks) return;
    const int64_t c = i % chunks, r = i / chunks, y = r % ny, z = r / ny;
    const int64_t off = c * 16, len = row - off < 16 ? row - off : 16;
    uint8_t *pp = pitched + z * p0 + y * p1 + off;
    uint8_t *dp = dense + (z * ny + y) * row + off;
    uint8_t v[16];
    if (TO_PITCHED) {
        if (len == 16 && ((uintptr_t)dp & 15) == 0) *reinterpret_cast<uint4 *>(v) = *reinterpret_cast<const uint4 *>(dp);
        else
            for (int q = 0; q < len; q++) v[q] = dp[q];
        if (len == 16 && ((uintptr_t)pp & 15) == 0) *reinterpret_cast<uint4 *>(pp) = *reinterpret_cast<const uint4 *>(v);
        else
            for (int q = 0; q < len; q++) pp[q] = v[q];
    } else {
        if (len == 16 && ((uintptr_t)pp & 15) == 0) *reinterpret_cast<uint4 *>(v) = *reinterpret_cast<const uint4 *>(pp);
        else
            for (int q = 0; q < len; q++) v[q] = pp[q];
        if (len == 16 && ((uintptr_t)dp & 15) == 0) *reinterpret_cast<uint4 *>(dp) = *reinterpret_cast<const uint4 *>(v);
        else
            for (int q = 0; q < len; q++) dp[q] = v[q];
    }
}

static int span_buffer(int hslot, size_t span, SpanSlot **out) {
    SpanSlot &sp = g_span[hslot];
    if (sp.cap < span) {
        if (sp.d) IVX_HIP(hipFree(sp.d));
        sp.d = nullptr;
        sp.cap = 0;
        const size_t want = span + (span >> 3) + 4096;
        IVX_HIP(hipMalloc(&sp.d, want));
        sp.cap = want;
        sp.epoch = 0;
    }
    *out = &sp;
    return IVX_OK;
}

// ---- resident host arrays -----------------------------------------------------------------------------
// A caller declares once that a host byte range is the project's image or mask matrix (ivx_host_register): the range gets
// a mirror in HBM, and every copy helper of this file that is handed memory inside it serves an upload from the mirror
// (device -> device) and writes a download through to it, the host copy staying the authoritative one.  The range
// arithmetic and the table are resident_ranges.h; here are the mirror, the kernels and the lock.  Every device operation
// on a mirror runs on the null stream under g_res_mu and is synchronised before the lock is dropped, so a mirror is at
// rest whenever the lock is free (a release therefore waits for a copy in flight) and every served copy is complete when
// the helper returns, like the hipMemcpy it replaces.  g_res_count == 0 skips all of it.
static std::mutex g_res_mu;
static resident::Registry g_res;
static std::atomic<size_t> g_res_count{0};
static std::atomic<int> g_res_check{-1}; // ivx_host_set_check; -1: IVX_RESIDENT_CHECK decides
static std::map<int, void *> g_res_chk;  // per device: staging block of the stale check and the packed refresh + the check's result word
constexpr size_t RES_CHK_CHUNK = 16u << 20;

static bool res_check_on() {
    int v = g_res_check.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("IVX_RESIDENT_CHECK");
        v = e && e[0] == '1';
        g_res_check.store(v, std::memory_order_relaxed);
    }
    return v != 0;
}

// Any 3-D view <-> dense, one element (or 16 bytes of the dense side) per lane.  Consecutive lanes walk the dense side's
// innermost index, so the dense side is always coalesced; the view side is whatever the strides make it.  `view` points at
// element [0][0][0], strides are signed bytes.  VEC: the dense rows are whole 16-byte chunks of an aligned block.
template <typename T, bool SCATTER, bool VEC>
static __device__ __forceinline__ void view_xfer_lane(uint8_t *__restrict__ view, int64_t s0, int64_t s1, int64_t s2, T *__restrict__ dense,
                                                      int64_t n0, int64_t n1, int64_t n2) {
    constexpr int E = VEC ? 16 / (int)sizeof(T) : 1;
    const int64_t per_row = n2 / E;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n0 * n1 * per_row) return;
    const int64_t c = i % per_row, r = i / per_row, y = r % n1, z = r / n1;
    uint8_t *vp = view + z * s0 + y * s1 + c * E * s2;
    T *dp = dense + r * n2 + c * E;
    if (VEC) {
        union {
            uint4 q;
            T e[E];
        } u;
        if (SCATTER) {
            u.q = *reinterpret_cast<const uint4 *>(dp);
#pragma unroll
            for (int k = 0; k < E; k++) *reinterpret_cast<T *>(vp + k * s2) = u.e[k];
        } else {
#pragma unroll
            for (int k = 0; k < E; k++) u.e[k] = *reinterpret_cast<const T *>(vp + k * s2);
            *reinterpret_cast<uint4 *>(dp) = u.q;
        }
    } else {
        if (SCATTER) *reinterpret_cast<T *>(vp) = *dp;
        else
            *dp = *reinterpret_cast<const T *>(vp);
    }
}
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_view_gather(uint8_t *__restrict__ view, int64_t s0, int64_t s1, int64_t s2, T *__restrict__ dense,
                                                     int64_t n0, int64_t n1, int64_t n2) {
    view_xfer_lane<T, false, VEC>(view, s0, s1, s2, dense, n0, n1, n2);
}
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_view_scatter(uint8_t *__restrict__ view, int64_t s0, int64_t s1, int64_t s2, T *__restrict__ dense,
                                                      int64_t n0, int64_t n1, int64_t n2) {
    view_xfer_lane<T, true, VEC>(view, s0, s1, s2, dense, n0, n1, n2);
}

template <typename T, bool SCATTER, bool VEC>
static int view_xfer_launch(uint8_t *view, const int64_t st[3], void *dense, const int64_t shape[3]) {
    const int64_t E = VEC ? 16 / (int64_t)sizeof(T) : 1;
    const int64_t blocks = cdiv(shape[0] * shape[1] * (shape[2] / E), 256);
    IVX_REQUIRE(blocks > 0 && blocks < ((int64_t)1 << 31), IVX_EINVAL, "view copy: %lld workgroups", (long long)blocks);
    if (SCATTER)
        hipLaunchKernelGGL((k_view_scatter<T, VEC>), dim3((unsigned)blocks), dim3(256), 0, 0, view, st[0], st[1], st[2], (T *)dense, shape[0],
                           shape[1], shape[2]);
    else
        hipLaunchKernelGGL((k_view_gather<T, VEC>), dim3((unsigned)blocks), dim3(256), 0, 0, view, st[0], st[1], st[2], (T *)dense, shape[0],
                           shape[1], shape[2]);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}
template <bool SCATTER> static int view_xfer(uint8_t *view, const int64_t st[3], void *dense, const int64_t shape[3], size_t isz) {
    const bool vec = (shape[2] * (int64_t)isz) % 16 == 0 && ((uintptr_t)dense & 15) == 0;
    switch (isz) {
    case 1: return vec ? view_xfer_launch<uint8_t, SCATTER, true>(view, st, dense, shape) : view_xfer_launch<uint8_t, SCATTER, false>(view, st, dense, shape);
    case 2: return vec ? view_xfer_launch<uint16_t, SCATTER, true>(view, st, dense, shape) : view_xfer_launch<uint16_t, SCATTER, false>(view, st, dense, shape);
    case 4: return vec ? view_xfer_launch<uint32_t, SCATTER, true>(view, st, dense, shape) : view_xfer_launch<uint32_t, SCATTER, false>(view, st, dense, shape);
    case 8: return vec ? view_xfer_launch<uint64_t, SCATTER, true>(view, st, dense, shape) : view_xfer_launch<uint64_t, SCATTER, false>(view, st, dense, shape);
    }
    set_error("view copy: item size %zu (1, 2, 4 or 8)", isz);
    return IVX_EINVAL;
}

// *first = min(*first, off0 + offset of the first byte where a and b differ); a, b 16-byte aligned, 16 bytes per lane
__global__ __launch_bounds__(256) void k_bytes_differ(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, size_t n,
                                                      unsigned long long off0, unsigned long long *first) {
    __shared__ unsigned long long s[256];
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
    unsigned long long mine = ~0ull;
    if (i < n) {
        const int len = n - i < 16 ? (int)(n - i) : 16;
        alignas(16) uint8_t x[16], y[16];
        if (len == 16) {
            *reinterpret_cast<uint4 *>(x) = *reinterpret_cast<const uint4 *>(a + i);
            *reinterpret_cast<uint4 *>(y) = *reinterpret_cast<const uint4 *>(b + i);
        } else
            for (int q = 0; q < len; q++) x[q] = a[i + q], y[q] = b[i + q];
        for (int q = len - 1; q >= 0; q--)
            if (x[q] != y[q]) mine = off0 + i + (unsigned)q;
    }
    s[threadIdx.x] = mine;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w && s[threadIdx.x + w] < s[threadIdx.x]) s[threadIdx.x] = s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0 && s[0] != ~0ull) atomicMin(first, s[0]);
}

// mirror[dst + i] = block[src + i] for the intervals of `tab` (dst, src, len triples at the head of the block): one
// workgroup per interval -- the many small pending writes of a registration (flag cells) in one upload and one launch
__global__ __launch_bounds__(256) void k_patch(uint8_t *__restrict__ mirror, const uint8_t *__restrict__ block) {
    const unsigned long long *tab = reinterpret_cast<const unsigned long long *>(block) + 3 * (size_t)blockIdx.x;
    const unsigned long long dst = tab[0], src = tab[1], len = tab[2];
    for (unsigned long long i = threadIdx.x; i < len; i += 256) mirror[dst + i] = block[src + i];
}

static int res_scratch(int dev, void **blk) { // per device: RES_CHK_CHUNK bytes + the stale check's result word
    void *&b = g_res_chk[dev];
    if (!b) IVX_HIP(hipMalloc(&b, RES_CHK_CHUNK + 16));
    *blk = b;
    return IVX_OK;
}

// the host's pending writes into the mirror, exactly those bytes
static int res_refresh(resident::Range *r) {
    const size_t ni = r->pending.v.size(), nb = r->pending.bytes();
    if (ni > 4 && ni * 24 + nb <= (1u << 20)) { // many small ones: packed behind a table, one copy, one launch
        std::vector<uint8_t> pack(ni * 24 + nb);
        unsigned long long *tab = reinterpret_cast<unsigned long long *>(pack.data());
        size_t at = ni * 24;
        for (size_t k = 0; k < ni; k++) {
            const resident::Interval &iv = r->pending.v[k];
            tab[3 * k] = iv.lo, tab[3 * k + 1] = at, tab[3 * k + 2] = iv.hi - iv.lo;
            memcpy(pack.data() + at, (const char *)r->base + iv.lo, iv.hi - iv.lo);
            at += iv.hi - iv.lo;
        }
        void *blk;
        int rc = res_scratch(r->device, &blk);
        if (rc || (rc = raw_h2d(blk, pack.data(), pack.size()))) return rc;
        hipLaunchKernelGGL(k_patch, dim3((unsigned)ni), dim3(256), 0, 0, (uint8_t *)r->mirror, (const uint8_t *)blk);
        IVX_LAUNCH_CHECK();
        IVX_HIP(hipStreamSynchronize(nullptr));
        r->stats[resident::ST_REFRESHES] += ni;
        r->stats[resident::ST_REFRESH_BYTES] += nb;
        r->pending.clear();
        return IVX_OK;
    }
    for (const resident::Interval &iv : r->pending.v) {
        int rc = raw_h2d((char *)r->mirror + iv.lo, (const char *)r->base + iv.lo, iv.hi - iv.lo);
        if (rc) return rc;
        r->stats[resident::ST_REFRESHES]++;
        r->stats[resident::ST_REFRESH_BYTES] += iv.hi - iv.lo;
    }
    r->pending.clear();
    return IVX_OK;
}

// IVX_RESIDENT_CHECK: host bytes [off, off + n) of the registration against the mirror (costs the upload the mirror saves)
static int res_check(resident::Range *r, size_t off, size_t n) {
    void *blk;
    int rc = res_scratch(r->device, &blk);
    if (rc) return rc;
    unsigned long long *first = (unsigned long long *)((char *)blk + RES_CHK_CHUNK), none = ~0ull, got = ~0ull;
    IVX_HIP(hipMemcpy(first, &none, 8, hipMemcpyHostToDevice));
    const size_t lo = off & ~(size_t)15, hi = off + n; // (down to a 16-byte boundary of the mirror: still inside the range)
    for (size_t at = lo; at < hi; at += RES_CHK_CHUNK) {
        const size_t len = hi - at < RES_CHK_CHUNK ? hi - at : RES_CHK_CHUNK;
        IVX_HIP(hipMemcpy(blk, (const char *)r->base + at, len, hipMemcpyHostToDevice));
        g_xfer[2].fetch_add(len, std::memory_order_relaxed);
        hipLaunchKernelGGL(k_bytes_differ, dim3((unsigned)cdiv((int64_t)cdiv((int64_t)len, 16), 256)), dim3(256), 0, 0,
                           (const uint8_t *)blk, (const uint8_t *)r->mirror + at, len, (unsigned long long)at, first);
        IVX_LAUNCH_CHECK();
        IVX_HIP(hipStreamSynchronize(nullptr)); // the next chunk overwrites the block
    }
    IVX_HIP(hipMemcpy(&got, first, 8, hipMemcpyDeviceToHost));
    if (got != ~0ull) {
        set_error("IVX_ESTALE: the registered host array at %p (%zu bytes) differs from its device mirror, first at byte offset %llu: "
                  "the host wrote it without ivx_host_touch", (void *)r->base, r->nbytes, got);
        return IVX_ESTALE;
    }
    return IVX_OK;
}

// The registration of the current device that holds all of [lo, hi), with the registry lock held in `lk` for as long as the
// caller works on the mirror; *out stays nullptr (and the lock is dropped) on a miss.  The host's pending writes are brought
// in first; `reads`: the caller is going to read mirror bytes, so the stale check (when on) runs over them.
static int res_acquire(uintptr_t lo, uintptr_t hi, bool reads, std::unique_lock<std::mutex> &lk, resident::Range **out) {
    *out = nullptr;
    lk = std::unique_lock<std::mutex>(g_res_mu);
    int dev = 0;
    IVX_HIP(hipGetDevice(&dev));
    resident::Range *r = g_res.find_containing(lo, hi, dev);
    if (!r) {
        lk.unlock();
        return IVX_OK;
    }
    int rc = res_refresh(r);
    if (!rc && reads && res_check_on()) rc = res_check(r, lo - r->base, hi - lo);
    if (rc) return rc;
    *out = r;
    return IVX_OK;
}

// the library wrote host bytes [lo, hi) that no mirror received: the registrations they overlap are stale there
static void res_invalidate(uintptr_t lo, uintptr_t hi) {
    std::lock_guard<std::mutex> lk(g_res_mu);
    g_res.invalidate(lo, hi);
}

static bool res_aligned(const resident::Range *r, const void *p, const int64_t st[3], size_t isz) {
    const int64_t m = (int64_t)isz;
    return ((uintptr_t)p - r->base) % isz == 0 && st[0] % m == 0 && st[1] % m == 0 && st[2] % m == 0;
}

int copy_h2d(void *dst_dev, const void *src, size_t n) {
    if (!n) return IVX_OK;
    if (g_res_count.load(std::memory_order_acquire)) {
        std::unique_lock<std::mutex> lk;
        resident::Range *r;
        int rc = res_acquire((uintptr_t)src, (uintptr_t)src + n, true, lk, &r);
        if (rc) return rc;
        if (r) {
            IVX_HIP(hipMemcpyAsync(dst_dev, (const char *)r->mirror + ((uintptr_t)src - r->base), n, hipMemcpyDeviceToDevice, nullptr));
            IVX_HIP(hipStreamSynchronize(nullptr));
            r->stats[resident::ST_HITS]++;
            r->stats[resident::ST_HIT_BYTES] += n;
            g_xfer[3].fetch_add(n, std::memory_order_relaxed);
            return IVX_OK;
        }
    }
    return raw_h2d(dst_dev, src, n);
}

int copy_d2h(void *dst, const void *src_dev, size_t n) {
    if (!n) return IVX_OK;
    int rc = raw_d2h(dst, src_dev, n); // the host copy is the authoritative one, whatever happens to the mirror
    if (rc || !g_res_count.load(std::memory_order_acquire)) return rc;
    std::unique_lock<std::mutex> lk;
    resident::Range *r;
    if ((rc = res_acquire((uintptr_t)dst, (uintptr_t)dst + n, false, lk, &r))) return rc;
    if (!r) {
        res_invalidate((uintptr_t)dst, (uintptr_t)dst + n);
        return IVX_OK;
    }
    IVX_HIP(hipMemcpyAsync((char *)r->mirror + ((uintptr_t)dst - r->base), src_dev, n, hipMemcpyDeviceToDevice, nullptr));
    IVX_HIP(hipStreamSynchronize(nullptr));
    r->stats[resident::ST_WRITES]++;
    r->stats[resident::ST_WRITE_BYTES] += n;
    return IVX_OK;
}

// upload_strided from a registered view: k_repitch for rows of 16 bytes and more, the general gather for everything else
static int res_upload_view(void *dst_dev, const void *src, const int64_t shape[3], const int64_t st[3], size_t isz, bool *served) {
    *served = false;
    uintptr_t lo, hi;
    if (!resident::view_extent((uintptr_t)src, shape, st, 3, isz, &lo, &hi)) return IVX_OK;
    std::unique_lock<std::mutex> lk;
    resident::Range *r;
    int rc = res_acquire(lo, hi, true, lk, &r);
    if (rc || !r) return rc;
    if (!res_aligned(r, src, st, isz)) return IVX_OK;
    uint8_t *m = (uint8_t *)r->mirror + ((uintptr_t)src - r->base);
    const int64_t row = shape[2] * (int64_t)isz;
    if (st[2] == (int64_t)isz && row >= 16) {
        const int64_t chunks = (row + 15) / 16;
        hipLaunchKernelGGL(k_repitch<false>, dim3((unsigned)cdiv(shape[0] * shape[1] * chunks, 256)), dim3(256), 0, 0, m, st[0], st[1],
                           (uint8_t *)dst_dev, shape[0], shape[1], row);
        IVX_LAUNCH_CHECK();
    } else if ((rc = view_xfer<false>(m, st, dst_dev, shape, isz)))
        return rc;
    IVX_HIP(hipStreamSynchronize(nullptr));
    const size_t n = (size_t)shape[0] * shape[1] * row;
    r->stats[resident::ST_HITS]++;
    r->stats[resident::ST_HIT_BYTES] += n;
    g_xfer[3].fetch_add(n, std::memory_order_relaxed);
    *served = true;
    return IVX_OK;
}

// download_strided's span path into a registered parent: the result is scattered into the mirror itself (which holds the
// bytes between the view's rows, so nothing is fetched from the host) and the span goes to the host from there
static int res_download_span(void *dst, const int64_t shape[3], const int64_t st[3], const void *src_dev, size_t isz, size_t span, bool *served) {
    *served = false;
    std::unique_lock<std::mutex> lk;
    resident::Range *r;
    int rc = res_acquire((uintptr_t)dst, (uintptr_t)dst + span, true, lk, &r);
    if (rc || !r) return rc;
    uint8_t *m = (uint8_t *)r->mirror + ((uintptr_t)dst - r->base);
    const int64_t row = shape[2] * (int64_t)isz, chunks = (row + 15) / 16;
    hipLaunchKernelGGL(k_repitch<true>, dim3((unsigned)cdiv(shape[0] * shape[1] * chunks, 256)), dim3(256), 0, 0, m, st[0], st[1],
                       (uint8_t *)const_cast<void *>(src_dev), shape[0], shape[1], row);
    IVX_LAUNCH_CHECK();
    IVX_HIP(hipStreamSynchronize(nullptr));
    if ((rc = raw_d2h(dst, m, span))) return rc;
    r->stats[resident::ST_WRITES]++;
    r->stats[resident::ST_WRITE_BYTES] += (size_t)shape[0] * shape[1] * row;
    *served = true;
    return IVX_OK;
}

// after download_strided's host scatter: the same bytes into the mirror (general scatter), or the overlap marked stale
static int res_after_view_write(void *dst, const int64_t shape[3], const int64_t st[3], const void *src_dev, size_t isz) {
    uintptr_t lo, hi;
    if (!resident::view_extent((uintptr_t)dst, shape, st, 3, isz, &lo, &hi)) return IVX_OK;
    std::unique_lock<std::mutex> lk;
    resident::Range *r;
    int rc = res_acquire(lo, hi, false, lk, &r);
    if (rc) return rc;
    if (r && res_aligned(r, dst, st, isz)) {
        if ((rc = view_xfer<true>((uint8_t *)r->mirror + ((uintptr_t)dst - r->base), st, const_cast<void *>(src_dev), shape, isz))) return rc;
        IVX_HIP(hipStreamSynchronize(nullptr));
        r->stats[resident::ST_WRITES]++;
        r->stats[resident::ST_WRITE_BYTES] += (size_t)shape[0] * shape[1] * shape[2] * isz;
        return IVX_OK;
    }
    if (r) g_res.invalidate(lo, hi); // (a misaligned view: the lock is still held)
    else
        res_invalidate(lo, hi);
    return IVX_OK;
}

// rows gathered / scattered by a few host threads (views that are not sub-boxes of a contiguous parent)
template <typename F> static void rows_parallel(int64_t nrows, F f) {
    const int nt = nrows > 4096 ? 4 : 1;
    if (nt == 1) { f(0, nrows); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back(f, nrows * t / nt, nrows * (t + 1) / nt);
    for (auto &t : th) t.join();
}

// a view gathered row by row on the host into page-locked staging, then one copy (views that are not sub-boxes of a
// contiguous parent; short rows)
static int upload_rows(void *dst_dev, const void *src, const int64_t shape[3], const int64_t st[3], size_t isz, int hslot) {
    const size_t n = (size_t)shape[0] * shape[1] * shape[2] * isz;
    void *h;
    int rc = hs_get(hslot, n, &h);
    if (rc) return rc;
    char *d = (char *)h;
    const char *s = (const char *)src;
    const size_t row = (size_t)shape[2] * isz;
    const int64_t ny = shape[1], nx = shape[2];
    rows_parallel(shape[0] * shape[1], [=](int64_t r0, int64_t r1) {
        for (int64_t r = r0; r < r1; r++) {
            const int64_t z = r / ny, y = r - z * ny;
            const char *sp = s + z * st[0] + y * st[1];
            char *dp = d + (size_t)r * row;
            if (st[2] == (int64_t)isz) memcpy(dp, sp, row);
            else
                for (int64_t x = 0; x < nx; x++) memcpy(dp + x * isz, sp + x * st[2], isz);
        }
    });
    IVX_HIP(hipMemcpy(dst_dev, h, n, hipMemcpyHostToDevice));
    g_xfer[0].fetch_add(n, std::memory_order_relaxed);
    return IVX_OK;
}

int upload_strided(void *dst_dev, const void *src, const int64_t shape[3], const int64_t st[3], size_t isz,
                   int hslot) {
    const size_t n = (size_t)shape[0] * shape[1] * shape[2] * isz;
    if (n == 0) return IVX_OK;
    if (dense3(shape, st, isz)) return copy_h2d(dst_dev, src, n);
    if (g_res_count.load(std::memory_order_acquire)) {
        bool served = false;
        int rc = res_upload_view(dst_dev, src, shape, st, isz, &served);
        if (rc || served) return rc;
    }
    size_t span = 0;
    if (hslot >= 0 && hslot < WS_COUNT && span_of(shape, st, isz, &span)) {
        SpanSlot *sp;
        int rc = span_buffer(hslot, span, &sp);
        if (rc) return rc;
        if ((rc = raw_h2d(sp->d, src, span))) return rc;
        sp->host = src;
        sp->nbytes = span;
        sp->epoch = g_host_depth > 0 ? g_host_epoch : 0;
        const int64_t row = shape[2] * (int64_t)isz, chunks = (row + 15) / 16;
        hipLaunchKernelGGL(k_repitch<false>, dim3((unsigned)cdiv(shape[0] * shape[1] * chunks, 256)), dim3(256), 0, 0,
                           (uint8_t *)sp->d, st[0], st[1], (uint8_t *)dst_dev, shape[0], shape[1], row);
        IVX_LAUNCH_CHECK();
        return IVX_OK;
    }
    return upload_rows(dst_dev, src, shape, st, isz, hslot);
}

// The library wrote the host view itself with the CPU (flag cells): the same values into the mirror, when there is one --
// gathered from the host, uploaded (exactly the view's bytes) into the caller's `d_scratch` and scattered from there.
int mirror_host_view(const void *view, const int64_t shape[3], const int64_t st[3], size_t isz, void *d_scratch, int hslot) {
    if (!g_res_count.load(std::memory_order_acquire) || shape[0] * shape[1] * shape[2] == 0) return IVX_OK;
    {
        uintptr_t lo, hi;
        if (!resident::view_extent((uintptr_t)view, shape, st, 3, isz, &lo, &hi)) return IVX_OK;
        std::lock_guard<std::mutex> lk(g_res_mu);
        int dev = 0;
        IVX_HIP(hipGetDevice(&dev));
        if (!g_res.find_containing(lo, hi, dev)) { // nothing to keep in step, or only an overlap: stale there
            g_res.invalidate(lo, hi);
            return IVX_OK;
        }
    }
    int rc = upload_rows(d_scratch, view, shape, st, isz, hslot);
    if (rc) return rc;
    return res_after_view_write(const_cast<void *>(view), shape, st, d_scratch, isz);
}

int download_strided(void *dst, const int64_t shape[3], const int64_t st[3], const void *src_dev, size_t isz,
                     int hslot) {
    const size_t n = (size_t)shape[0] * shape[1] * shape[2] * isz;
    if (n == 0) return IVX_OK;
    if (dense3(shape, st, isz)) return copy_d2h(dst, src_dev, n);
    const bool res = g_res_count.load(std::memory_order_acquire) != 0;
    size_t span = 0;
    if (hslot >= 0 && hslot < WS_COUNT && span_of(shape, st, isz, &span)) {
        if (res) {
            bool served = false;
            int rc = res_download_span(dst, shape, st, src_dev, isz, span, &served);
            if (rc || served) return rc;
        }
        SpanSlot *sp;
        int rc = span_buffer(hslot, span, &sp);
        if (rc) return rc;
        const bool fresh = sp->host == dst && sp->nbytes == span && sp->epoch != 0 && sp->epoch == g_host_epoch && g_host_depth > 0;
        if (!fresh && (rc = raw_h2d(sp->d, dst, span))) return rc; // the bytes between the view's rows
        const int64_t row = shape[2] * (int64_t)isz, chunks = (row + 15) / 16;
        hipLaunchKernelGGL(k_repitch<true>, dim3((unsigned)cdiv(shape[0] * shape[1] * chunks, 256)), dim3(256), 0, 0,
                           (uint8_t *)sp->d, st[0], st[1], (uint8_t *)const_cast<void *>(src_dev), shape[0], shape[1], row);
        IVX_LAUNCH_CHECK();
        IVX_HIP(hipStreamSynchronize(nullptr)); // (the kernel above runs on the null stream; the staged copy on its own streams)
        if ((rc = copy_d2h(dst, sp->d, span))) return rc;
        sp->epoch = 0; // the host copy is the truth again
        return IVX_OK;
    }
    void *h;
    int rc = hs_get(hslot, n, &h);
    if (rc) return rc;
    IVX_HIP(hipMemcpy(h, src_dev, n, hipMemcpyDeviceToHost));
    g_xfer[1].fetch_add(n, std::memory_order_relaxed);
    const char *s = (const char *)h;
    char *d = (char *)dst;
    const size_t row = (size_t)shape[2] * isz;
    const int64_t ny = shape[1], nx = shape[2];
    rows_parallel(shape[0] * shape[1], [=](int64_t r0, int64_t r1) {
        for (int64_t r = r0; r < r1; r++) {
            const int64_t z = r / ny, y = r - z * ny;
            char *dp = d + z * st[0] + y * st[1];
            const char *sp = s + (size_t)r * row;
            if (st[2] == (int64_t)isz) memcpy(dp, sp, row);
            else
                for (int64_t x = 0; x < nx; x++) memcpy(dp + x * st[2], sp + x * isz, isz);
        }
    });
    if (res) return res_after_view_write(dst, shape, st, src_dev, isz);
    return IVX_OK;
}

int download_strided2(void *dst, const int64_t shape[2], const int64_t st[2], const void *src_dev, size_t isz,
                      int hslot) {
    const int64_t sh3[3] = {1, shape[0], shape[1]};
    const int64_t st3[3] = {0, st[0], st[1]};
    if (st[1] == (int64_t)isz && st[0] == shape[1] * (int64_t)isz) {
        const size_t n = (size_t)shape[0] * shape[1] * isz;
        return copy_d2h(dst, src_dev, n);
    }
    return download_strided(dst, sh3, st3, src_dev, isz, hslot);
}

// ---- a mirror handed to a host-level entry point (ivx_internal.h) ----
struct MirrorHold {
    std::unique_lock<std::mutex> lk;
    resident::Range *r = nullptr;
};
int mirror_acquire(const void *p, size_t n, bool reads, MirrorHold **hold, void **mirror) {
    *hold = nullptr;
    *mirror = nullptr;
    if (!n || !g_res_count.load(std::memory_order_acquire)) return IVX_OK;
    MirrorHold *h = new MirrorHold();
    int rc = res_acquire((uintptr_t)p, (uintptr_t)p + n, reads, h->lk, &h->r);
    if (rc || !h->r) {
        delete h; // (drops the lock when the stale check failed with it held)
        return rc;
    }
    *hold = h;
    *mirror = (char *)h->r->mirror + ((uintptr_t)p - h->r->base);
    if (reads) {
        h->r->stats[resident::ST_HITS]++;
        h->r->stats[resident::ST_HIT_BYTES] += n;
    }
    return IVX_OK;
}
int mirror_fetch(MirrorHold *hold, void *host, const void *mirror, size_t n) {
    (void)hold; // (the lock it holds is what keeps the mirror at rest)
    return raw_d2h(host, mirror, n);
}
void mirror_release(MirrorHold *hold, size_t written) {
    if (!hold) return;
    if (written) {
        hold->r->stats[resident::ST_WRITES]++;
        hold->r->stats[resident::ST_WRITE_BYTES] += written;
    }
    delete hold;
}

// ---- mailbox ------------------------------------------------------------------------------------------------
static uint32_t *g_mb = nullptr; // pinned host memory, 64 dwords per slot x 64 slots (ring)
static uint32_t g_mb_seq = 0;     // the newest sequence number handed out (mailbox_slot.h has the ring's arithmetic)

// the next sequence number (g_mu held); the first call makes the ring
static int mailbox_hand_out(uint32_t *seq_out) {
    if (!g_mb) {
        void *p = nullptr;
        IVX_HIP(hipHostMalloc(&p, MAILBOX_SLOTS * 64 * 4, hipHostMallocMapped | hipHostMallocCoherent));
        memset(p, 0, MAILBOX_SLOTS * 64 * 4);
        g_mb = (uint32_t *)p;
    }
    *seq_out = g_mb_seq = mailbox_next_seq(g_mb_seq);
    return IVX_OK;
}

__global__ void k_mailbox_publish(const uint32_t *__restrict__ src, int n, uint32_t *mb, uint32_t seq) {
    if (threadIdx.x || blockIdx.x) return;
    for (int i = 0; i < n; i++) mb[i] = src[i];
    __threadfence_system();
    __hip_atomic_store(&mb[63], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int mailbox_publish(const void *dsrc, int ndwords, hipStream_t st, uint32_t *seq_out) {
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (int rc = mailbox_hand_out(seq_out)) return rc;
    }
    IVX_REQUIRE(ndwords >= 0 && ndwords <= 32, IVX_EINVAL, "mailbox: too many words");
    uint32_t *slot = g_mb + (size_t)mailbox_slot_of(*seq_out) * 64;
    hipLaunchKernelGGL(k_mailbox_publish, dim3(1), dim3(64), 0, st, (const uint32_t *)dsrc, ndwords, slot, *seq_out);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

// a slot and a sequence number for a kernel that publishes by itself (dwords 0 .. n-1, a system-scope fence, then the sequence
// number into dword 63 with release semantics at system scope -- what k_mailbox_publish does): saves the publishing launch
int mailbox_reserve(uint32_t **slot_out, uint32_t *seq_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = mailbox_hand_out(seq_out)) return rc;
    *slot_out = g_mb + (size_t)mailbox_slot_of(*seq_out) * 64;
    return IVX_OK;
}

// the sharded flood's vote (parallel.py, slab_region_grow): two device words { everybody's votes of the last round, my new count }.
// Setting them and reading them used to be two memsets, a 4-byte device copy and a synchronising 8-byte download per round --
// 16 us each as copy-engine calls; here: one-thread kernels and the mailbox (no stream synchronisation).
__global__ void k_vote_set(int32_t *v, int32_t a, int32_t b) {
    v[0] = a;
    v[1] = b;
}
// publish both words, then stage the next round's vote (votes[0] <- my count: the next exchange all-reduces it in place)
__global__ void k_vote_publish(int32_t *v, uint32_t *mb, uint32_t seq) {
    if (threadIdx.x || blockIdx.x) return;
    const int32_t a = v[0], b = v[1];
    mb[0] = (uint32_t)a;
    mb[1] = (uint32_t)b;
    v[0] = b;
    v[1] = 0; // (ivx_dev_flood_or_planes_acc adds the next round's gains to it)
    __threadfence_system();
    __hip_atomic_store(&mb[63], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int vote_publish(int32_t *votes, hipStream_t st, uint32_t *seq_out) {
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (int rc = mailbox_hand_out(seq_out)) return rc;
    }
    uint32_t *slot = g_mb + (size_t)mailbox_slot_of(*seq_out) * 64;
    hipLaunchKernelGGL(k_vote_publish, dim3(1), dim3(64), 0, st, votes, slot, *seq_out);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

int mailbox_wait(uint32_t seq, hipStream_t st, uint32_t *out, int ndwords) {
    volatile uint32_t *slot = g_mb + (size_t)mailbox_slot_of(seq) * 64;
    bool ok = false;
    for (long spins = 0; spins < 20000000L; spins++) { // ~ a few hundred ms worst case, then the safe path
        if (__atomic_load_n(&slot[63], __ATOMIC_ACQUIRE) == seq) { ok = true; break; }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    if (!ok) {
        IVX_HIP(hipStreamSynchronize(st));
        IVX_REQUIRE(__atomic_load_n(&slot[63], __ATOMIC_ACQUIRE) == seq, IVX_EHIP, "mailbox: GPU never published sequence %u", seq);
    }
    for (int i = 0; i < ndwords; i++) out[i] = slot[i];
    return IVX_OK;
}

// mailbox_wait for a number handed out by mailbox_reserve a while ago, whose slot may have gone to a later number since
// (64 slots): `*got` = 0, with nothing read, when it has -- before the wait, during it, or under the read.  Launches nothing.
int mailbox_wait_reserved(uint32_t seq, hipStream_t st, uint32_t *out, int ndwords, int *got) {
    *got = 0;
    auto in_slot = [seq]() {
        std::lock_guard<std::mutex> lk(g_mu);
        return g_mb != nullptr && mailbox_seq_in_slot(seq, g_mb_seq);
    };
    if (!in_slot()) return IVX_OK;
    volatile uint32_t *slot = g_mb + (size_t)mailbox_slot_of(seq) * 64;
    bool ok = false;
    for (long spins = 0; spins < 20000000L; spins++) {
        if (__atomic_load_n(&slot[63], __ATOMIC_ACQUIRE) == seq) { ok = true; break; }
        if ((spins & 4095) == 4095 && !in_slot()) return IVX_OK; // (another thread's messages went round the ring meanwhile)
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    if (!ok) {
        IVX_HIP(hipStreamSynchronize(st));
        if (__atomic_load_n(&slot[63], __ATOMIC_ACQUIRE) != seq) {
            IVX_REQUIRE(!in_slot(), IVX_EHIP, "mailbox: GPU never published sequence %u", seq);
            return IVX_OK;
        }
    }
    uint32_t w[32];
    for (int i = 0; i < ndwords; i++) w[i] = slot[i];
    // the words are `seq`'s only if the slot's next owner was not even handed out when they had been read
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (slot[63] != seq || !in_slot()) return IVX_OK;
    for (int i = 0; i < ndwords; i++) out[i] = w[i];
    *got = 1;
    return IVX_OK;
}

// ---- progress lines ----------------------------------------------------------------------------------------
// one 64-B line per stream, carved from pinned chunks of 64 lines; a line is handed back when its stream is destroyed
struct ProgressLine {
    unsigned long long *p;
    uint8_t tag;
};
static std::map<hipStream_t, ProgressLine> g_pl;
static std::vector<unsigned long long *> g_pl_free;

int progress_line(hipStream_t st, volatile unsigned long long **line, uint32_t *tag) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_pl.find(st);
    if (it == g_pl.end()) {
        if (g_pl_free.empty()) {
            void *p = nullptr;
            IVX_HIP(hipHostMalloc(&p, 64 * 64, hipHostMallocMapped | hipHostMallocCoherent));
            memset(p, 0, 64 * 64);
            for (int i = 63; i >= 0; i--) g_pl_free.push_back((unsigned long long *)p + (size_t)i * 8);
        }
        ProgressLine l = {g_pl_free.back(), 0};
        g_pl_free.pop_back();
        it = g_pl.insert(std::make_pair(st, l)).first;
    }
    if (++it->second.tag == 0) it->second.tag = 1;
    *tag = it->second.tag;
    *line = it->second.p;
    return IVX_OK;
}

void progress_forget_stream(void *stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_pl.find((hipStream_t)stream);
    if (it == g_pl.end()) return;
    // the stream has been synchronised by the caller: nothing can still write to the line.  The next owner starts from
    // a clean line, so the tag may start over.
    memset(it->second.p, 0, 64);
    g_pl_free.push_back(it->second.p);
    g_pl.erase(it);
}

} // namespace ivx

using namespace ivx;

// IVX_BACKTRACE=1: print a native backtrace on SIGABRT / SIGSEGV (diagnostic aid; off by default)
static void ivx::ivx_bt_handler(int sig) {
    void *frames[64];
    const int n = backtrace(frames, 64);
    const char msg[] = "ivx: fatal signal, native backtrace:\n";
    (void)!write(2, msg, sizeof(msg) - 1);
    backtrace_symbols_fd(frames, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}
__attribute__((constructor)) static void ivx_install_bt() {
    if (getenv("IVX_BACKTRACE")) {
        signal(SIGABRT, ivx_bt_handler);
        signal(SIGSEGV, ivx_bt_handler);
    }
}

extern "C" {

int ivx_version(void) { return 100; }
const char *ivx_last_error(void) { return g_err; }

int ivx_device_count(int *count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        n = 0;
        (void)hipGetLastError();
    }
    *count = n;
    return IVX_OK;
}
int ivx_set_device(int device) {
    IVX_HIP(hipSetDevice(device));
    return IVX_OK;
}
int ivx_device_synchronize(void) {
    IVX_HIP(hipDeviceSynchronize());
    return IVX_OK;
}
int ivx_device_name(char *buf, size_t buflen) {
    int dev = 0;
    IVX_HIP(hipGetDevice(&dev));
    hipDeviceProp_t p;
    IVX_HIP(hipGetDeviceProperties(&p, dev));
    snprintf(buf, buflen, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
    return IVX_OK;
}
int ivx_malloc(void **dptr, size_t nbytes) {
    IVX_HIP(hipMalloc(dptr, nbytes ? nbytes : 16));
    return IVX_OK;
}
int ivx_free(void *dptr) {
    if (dptr) IVX_HIP(hipFree(dptr));
    return IVX_OK;
}
int ivx_memset(void *dptr, int value, size_t nbytes, void *stream) {
    if (nbytes) IVX_HIP(hipMemsetAsync(dptr, value, nbytes, S(stream)));
    return IVX_OK;
}
// (pageable host memory of >= 4 MB travels through the page-locked lane buffers above; IVX_STAGE_THREADS=0: plain hipMemcpy)
int ivx_memcpy_h2d(void *dst, const void *src, size_t nbytes) { return copy_h2d(dst, src, nbytes); }
int ivx_memcpy_d2h(void *dst, const void *src, size_t nbytes) { return copy_d2h(dst, src, nbytes); }
// a 3-D host view (signed byte strides) <-> a dense device block: what every host-level entry point does with its arrays
int ivx_upload_strided(void *dst, const void *src, const int64_t shape[3], const int64_t strides[3], size_t itemsize) {
    IVX_REQUIRE(dst && src && shape && strides, IVX_EINVAL, "ivx_upload_strided: null");
    IVX_REQUIRE(itemsize == 1 || itemsize == 2 || itemsize == 4 || itemsize == 8, IVX_EINVAL, "ivx_upload_strided: item size %zu", itemsize);
    IVX_REQUIRE(shape[0] >= 0 && shape[1] >= 0 && shape[2] >= 0, IVX_EINVAL, "ivx_upload_strided: negative shape");
    HostCallGuard g; // (the staging blocks are the host-level entry points')
    int rc = upload_strided(dst, src, shape, strides, itemsize, WS_IN);
    if (rc) return rc;
    // upload_strided leaves a sub-box's re-pitch kernel on the null stream, which is enough for the host-level entry points (they
    // go on working there); this call's users launch on their own non-blocking streams next, so the block must be complete now
    IVX_HIP(hipStreamSynchronize(nullptr));
    return IVX_OK;
}
int ivx_download_strided(void *dst, const int64_t shape[3], const int64_t strides[3], const void *src, size_t itemsize) {
    IVX_REQUIRE(dst && src && shape && strides, IVX_EINVAL, "ivx_download_strided: null");
    IVX_REQUIRE(itemsize == 1 || itemsize == 2 || itemsize == 4 || itemsize == 8, IVX_EINVAL, "ivx_download_strided: item size %zu", itemsize);
    IVX_REQUIRE(shape[0] >= 0 && shape[1] >= 0 && shape[2] >= 0, IVX_EINVAL, "ivx_download_strided: negative shape");
    HostCallGuard g;
    return download_strided(dst, shape, strides, src, itemsize, WS_OUT);
}

// ---- resident host arrays: the registry's public face (include/ivx.h) ----
int ivx_host_register(const void *base, size_t nbytes, uint64_t *handle) {
    IVX_REQUIRE(base && nbytes && handle, IVX_EINVAL, "ivx_host_register: null or empty range");
    std::lock_guard<std::mutex> lk(g_res_mu);
    int dev = 0;
    IVX_HIP(hipGetDevice(&dev));
    uint64_t h = 0;
    IVX_REQUIRE(g_res.add((uintptr_t)base, nbytes, dev, &h) == resident::RES_OK, IVX_EINVAL,
                "ivx_host_register: [%p, +%zu) overlaps a registered range", base, nbytes);
    resident::Range *r = g_res.get(h);
    hipError_t e = hipMalloc(&r->mirror, nbytes);
    int rc = IVX_OK;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("ivx_host_register: no device memory for a mirror of %zu bytes (%s)", nbytes, hipGetErrorString(e));
        rc = e == hipErrorOutOfMemory ? IVX_ENOMEM : IVX_EHIP;
    } else if ((rc = raw_h2d(r->mirror, base, nbytes)))
        (void)hipFree(r->mirror);
    if (rc) {
        g_res.release(h);
        return rc;
    }
    g_res_count.store(g_res.count(), std::memory_order_release);
    *handle = h;
    return IVX_OK;
}
// a registration whose mirror starts as zeros: nothing is uploaded (the new arrays of a swap, which a host form fills next)
int ivx_host_register_zero(const void *base, size_t nbytes, uint64_t *handle) {
    IVX_REQUIRE(base && nbytes && handle, IVX_EINVAL, "ivx_host_register_zero: null or empty range");
    std::lock_guard<std::mutex> lk(g_res_mu);
    int dev = 0;
    IVX_HIP(hipGetDevice(&dev));
    uint64_t h = 0;
    IVX_REQUIRE(g_res.add((uintptr_t)base, nbytes, dev, &h) == resident::RES_OK, IVX_EINVAL,
                "ivx_host_register_zero: [%p, +%zu) overlaps a registered range", base, nbytes);
    resident::Range *r = g_res.get(h);
    hipError_t e = hipMalloc(&r->mirror, nbytes);
    if (e == hipSuccess) {
        e = hipMemsetAsync(r->mirror, 0, nbytes, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) (void)hipFree(r->mirror);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("ivx_host_register_zero: no zeroed mirror of %zu bytes (%s)", nbytes, hipGetErrorString(e));
        g_res.release(h);
        return e == hipErrorOutOfMemory ? IVX_ENOMEM : IVX_EHIP;
    }
    g_res_count.store(g_res.count(), std::memory_order_release);
    *handle = h;
    return IVX_OK;
}
// zeros on the host and, where the bytes are registered, in the mirror: nothing crosses the link
int ivx_host_zero(void *p, size_t nbytes) {
    IVX_REQUIRE(p || !nbytes, IVX_EINVAL, "ivx_host_zero: null");
    if (!nbytes) return IVX_OK;
    memset(p, 0, nbytes);
    if (!g_res_count.load(std::memory_order_acquire)) return IVX_OK;
    std::unique_lock<std::mutex> lk;
    resident::Range *r;
    int rc = res_acquire((uintptr_t)p, (uintptr_t)p + nbytes, false, lk, &r);
    if (rc) return rc;
    if (!r) {
        res_invalidate((uintptr_t)p, (uintptr_t)p + nbytes);
        return IVX_OK;
    }
    IVX_HIP(hipMemsetAsync((char *)r->mirror + ((uintptr_t)p - r->base), 0, nbytes, nullptr));
    IVX_HIP(hipStreamSynchronize(nullptr));
    r->stats[resident::ST_WRITES]++;
    r->stats[resident::ST_WRITE_BYTES] += nbytes;
    return IVX_OK;
}
int ivx_host_touch_range(uint64_t handle, size_t offset, size_t nbytes) {
    std::lock_guard<std::mutex> lk(g_res_mu);
    IVX_REQUIRE(g_res.get(handle), IVX_EINVAL, "ivx_host_touch: handle %llu is released or was never given out", (unsigned long long)handle);
    IVX_REQUIRE(g_res.touch(handle, offset, nbytes) == resident::RES_OK, IVX_EINVAL,
                "ivx_host_touch: [%zu, +%zu) leaves the registered range of %zu bytes", offset, nbytes, g_res.get(handle)->nbytes);
    return IVX_OK;
}
int ivx_host_touch(uint64_t handle) {
    size_t n = 0;
    {
        std::lock_guard<std::mutex> lk(g_res_mu);
        resident::Range *r = g_res.get(handle);
        IVX_REQUIRE(r, IVX_EINVAL, "ivx_host_touch: handle %llu is released or was never given out", (unsigned long long)handle);
        n = r->nbytes;
    }
    return ivx_host_touch_range(handle, 0, n);
}
int ivx_host_release(uint64_t handle) {
    std::lock_guard<std::mutex> lk(g_res_mu); // (held by every copy that uses a mirror: this waits for it)
    resident::Range *r = g_res.get(handle);
    IVX_REQUIRE(r, IVX_EINVAL, "ivx_host_release: handle %llu is released or was never given out", (unsigned long long)handle);
    if (r->mirror) (void)hipFree(r->mirror);
    g_res.release(handle);
    g_res_count.store(g_res.count(), std::memory_order_release);
    return IVX_OK;
}
int ivx_host_stats(uint64_t handle, uint64_t out[8]) {
    std::lock_guard<std::mutex> lk(g_res_mu);
    resident::Range *r = g_res.get(handle);
    IVX_REQUIRE(r && out, IVX_EINVAL, "ivx_host_stats: handle %llu is released or was never given out", (unsigned long long)handle);
    for (int i = 0; i < 8; i++) out[i] = r->stats[i];
    return IVX_OK;
}
int ivx_host_count(uint64_t *count) {
    IVX_REQUIRE(count, IVX_EINVAL, "ivx_host_count: null");
    std::lock_guard<std::mutex> lk(g_res_mu);
    *count = g_res.count();
    return IVX_OK;
}
int ivx_host_set_check(int on) {
    g_res_check.store(on ? 1 : 0, std::memory_order_relaxed);
    return IVX_OK;
}
int ivx_transfer_stats(uint64_t out[4]) {
    IVX_REQUIRE(out, IVX_EINVAL, "ivx_transfer_stats: null");
    for (int i = 0; i < 4; i++) out[i] = g_xfer[i].load(std::memory_order_relaxed);
    return IVX_OK;
}
// Page-locked host memory for callers that keep their arrays where the DMA engines can reach them directly: a pageable
// numpy array crosses PCIe through the runtime's bounce buffers (~25-40 GB/s here), a pinned one at the link's rate.
int ivx_host_alloc(void **hptr, size_t nbytes) {
    IVX_REQUIRE(hptr, IVX_EINVAL, "ivx_host_alloc: null");
    IVX_HIP(hipHostMalloc(hptr, nbytes ? nbytes : 16, hipHostMallocDefault));
    return IVX_OK;
}
int ivx_host_free(void *hptr) {
    if (hptr) IVX_HIP(hipHostFree(hptr));
    return IVX_OK;
}
int ivx_memcpy_d2d(void *dst, const void *src, size_t nbytes, void *stream) {
    if (nbytes) IVX_HIP(hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToDevice, S(stream)));
    return IVX_OK;
}
int ivx_dev_vote_set(int32_t *votes, int32_t v0, int32_t v1, void *stream) {
    IVX_REQUIRE(votes, IVX_EINVAL, "ivx_dev_vote_set: null");
    hipLaunchKernelGGL(ivx::k_vote_set, dim3(1), dim3(1), 0, S(stream), votes, v0, v1);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}
int ivx_dev_vote_read(int32_t *votes, int32_t out[2], void *stream) {
    IVX_REQUIRE(votes && out, IVX_EINVAL, "ivx_dev_vote_read: null");
    uint32_t seq = 0, w[2] = {0, 0};
    int rc = ivx::vote_publish(votes, S(stream), &seq);
    if (rc != IVX_OK) return rc;
    rc = ivx::mailbox_wait(seq, S(stream), w, 2);
    if (rc != IVX_OK) return rc;
    out[0] = (int32_t)w[0];
    out[1] = (int32_t)w[1];
    return IVX_OK;
}
int ivx_stream_create(void **stream) {
    hipStream_t s;
    IVX_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void *)s;
    return IVX_OK;
}
// a stream whose work yields to the default-priority streams' when both have workgroups waiting (background work that
// should fill idle CUs without slowing the main stream down)
int ivx_stream_create_low_priority(void **stream) {
    int least = 0, greatest = 0;
    IVX_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    hipStream_t s;
    IVX_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least));
    *stream = (void *)s;
    return IVX_OK;
}
int ivx_stream_destroy(void *stream) {
    if (!stream) return IVX_OK;
    IVX_HIP(hipStreamSynchronize(S(stream)));
    { // the stream's private workspaces go with it (a later stream may be handed the same handle value)
        std::lock_guard<std::mutex> lk(g_mu);
        for (auto it = g_ws_stream.begin(); it != g_ws_stream.end();) {
            if (it->first.second == S(stream)) {
                if (it->second.p) (void)hipFree(it->second.p);
                it = g_ws_stream.erase(it);
            } else {
                ++it;
            }
        }
    }
    ccl_forget_stream(stream);
    progress_forget_stream(stream);
    IVX_HIP(hipStreamDestroy(S(stream)));
    return IVX_OK;
}
int ivx_stream_synchronize(void *stream) {
    IVX_HIP(hipStreamSynchronize(S(stream)));
    return IVX_OK;
}
int ivx_event_create(void **event) {
    hipEvent_t e;
    // timing events between kernels of one stream: no system-scope fence when the event fires (a default event drains
    // the caches to host visibility and leaves a ~5 us bubble in the stream every time it is recorded)
    IVX_HIP(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    *event = (void *)e;
    return IVX_OK;
}
// an event for ORDERING streams (ivx_event_record + ivx_stream_wait_event), not for timing: full fence, no timestamps
int ivx_event_create_sync(void **event) {
    hipEvent_t e;
    IVX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *event = (void *)e;
    return IVX_OK;
}
int ivx_event_destroy(void *event) {
    if (event) IVX_HIP(hipEventDestroy((hipEvent_t)event));
    return IVX_OK;
}
int ivx_event_record(void *event, void *stream) {
    IVX_HIP(hipEventRecord((hipEvent_t)event, S(stream)));
    return IVX_OK;
}
int ivx_stream_wait_event(void *stream, void *event) {
    IVX_HIP(hipStreamWaitEvent(S(stream), (hipEvent_t)event, 0));
    return IVX_OK;
}
int ivx_event_elapsed_ms(void *start, void *stop, float *ms) {
    IVX_HIP(hipEventSynchronize((hipEvent_t)stop));
    IVX_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return IVX_OK;
}
int ivx_release_workspace(void) {
    {
        std::lock_guard<std::mutex> rk(g_res_mu); // the stale check's staging blocks (the mirrors stay: they are not workspace)
        for (auto &kv : g_res_chk)
            if (kv.second) (void)hipFree(kv.second);
        g_res_chk.clear();
    }
    std::lock_guard<std::mutex> lk(g_mu);
    for (int i = 0; i < WS_COUNT; i++) {
        if (g_ws[i].p) (void)hipFree(g_ws[i].p);
        g_ws[i] = Slot();
        if (g_hs[i].p) (void)hipHostFree(g_hs[i].p);
        g_hs[i] = Slot();
        if (ivx::g_span[i].d) (void)hipFree(ivx::g_span[i].d);
        ivx::g_span[i] = ivx::SpanSlot();
    }
    for (auto &kv : g_ws_stream)
        if (kv.second.p) (void)hipFree(kv.second.p);
    g_ws_stream.clear();
    return IVX_OK;
}

} // extern "C"
