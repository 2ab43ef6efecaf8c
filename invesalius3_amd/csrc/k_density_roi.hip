// k_density_roi.hip -- the density measures: CircleDensityMeasure.calc_density and PolygonDensityMeasure.calc_density
// (invesalius/data/measures.py:2019-2107, 2229-2319) for a batch of R regions of interest in one launch.
//
// Which pixels a region selects is stated in density_roi_math.h (rule E, the reference's ellipse bit for bit; rule P, the
// project's statement of the wx fill, DESIGN 7o says what is unpinned).  The statistics follow k_density (k_misc.hip): count,
// sum and sum of squares as exact 64-bit integers, min and max, reduced per wave by shuffles, per workgroup through LDS and
// per region by one set of atomics per workgroup.
//
// MI355X design: a measure reads one slice's bounding box -- 3.7 KB for an ellipse of radius 20 px, 325 KB for one of radius
// 200 px -- so a call is bound by the launch and the download, not by HBM, and a panel of measures is a batch of such small
// reductions.  One launch serves all of them: every region's clipped box is cut into chunks of 1024 pixels, one workgroup per
// chunk, and a workgroup finds its region by a binary search over the chunks' prefix sums.  Consecutive lanes take consecutive
// pixels of a box row, so an axial or coronal box reads whole lines; a sagittal view has one element per 64-byte line (its
// element stride is the volume's row pitch), which is why the box is kept tight: the line count is the pixel count.  A
// polygon's points sit in LDS (16 B each, IVX_ROI_MAX_POINTS of them are 32 KB).  The records start as zeros from ONE memset;
// min and max travel as 32768 - v and v + 32769 under atomicMax, so that zero means "no pixel yet", and the workgroup that
// arrives last at a region -- counted in the upper bits of the record's first word, behind an agent-scope release -- reads
// the record back with returning atomics and stores its plain form: cnt, s1, s2, lo, hi.  Every load is inside the box, the
// box inside the slice (clipped by the host from the parameters, never taken from the caller).
#include <algorithm>
#include <cmath>
#include <vector>

#include "density_roi_math.h"
#include "ivx_internal.h"

namespace dr = ivx_density_roi_math;

namespace {

constexpr int CHUNK = 1024;           // pixels per workgroup, four per lane
constexpr int TICKET_SHIFT = 40;      // record word 0 while the launch runs: arrivals << 40 | count
constexpr int64_t MAX_BOX = (int64_t)1 << 33;

__global__ __launch_bounds__(256) void k_roi_density(const ivx_roi *__restrict__ rois, int64_t n_rois, const double *__restrict__ points,
                                                     unsigned long long *__restrict__ records) {
    __shared__ double s_pts[2 * IVX_ROI_MAX_POINTS];
    __shared__ long long sh[4][3];
    __shared__ int shm[4][2];
    // the last region whose first chunk is not behind this workgroup's (regions without chunks share their successor's)
    const int64_t b = blockIdx.x;
    int64_t lo_r = 0, hi_r = n_rois - 1;
    while (lo_r < hi_r) {
        const int64_t mid = (lo_r + hi_r + 1) >> 1;
        if (rois[mid].first_block <= b) lo_r = mid;
        else
            hi_r = mid - 1;
    }
    const ivx_roi &q = rois[lo_r];
    const int64_t chunk = b - q.first_block;
    if (chunk < 0 || chunk >= q.n_blocks) return; // (cannot happen with the host's prefix sums)
    const int64_t bw = q.x1 - q.x0, total = bw * (q.y1 - q.y0);
    const int np = q.kind == dr::KIND_POLYGON ? q.n_points : 0;
    if (np > 0) {
        const double *src = points + 2 * q.first_point;
        for (int i = threadIdx.x; i < 2 * np; i += 256) s_pts[i] = src[i];
        __syncthreads();
    }
    long long cnt = 0, s = 0, s2 = 0;
    int lo = 32767, hi = -32768;
    const uint8_t *img = reinterpret_cast<const uint8_t *>(q.image);
#pragma unroll
    for (int k = 0; k < CHUNK / 256; k++) {
        const int64_t idx = chunk * CHUNK + k * 256 + threadIdx.x;
        if (idx >= total) continue;
        const int64_t r = idx / bw, y = q.y0 + r, x = q.x0 + (idx - r * bw);
        if (x < 0 || x >= q.w || y < 0 || y >= q.h) continue;
        const bool in = q.kind == dr::KIND_POLYGON ? dr::polygon_selects(s_pts, np, x, y) : dr::ellipse_selects(x, y, q.sx, q.sy, q.cx, q.cy, q.a2, q.b2);
        if (!in) continue;
        const int v = *reinterpret_cast<const int16_t *>(img + y * q.row_stride + x * q.elem_stride);
        cnt++;
        s += v;
        s2 += (long long)v * v;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        s += __shfl_xor(s, o, 64);
        s2 += __shfl_xor(s2, o, 64);
        const int l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        sh[threadIdx.x >> 6][0] = cnt;
        sh[threadIdx.x >> 6][1] = s;
        sh[threadIdx.x >> 6][2] = s2;
        shm[threadIdx.x >> 6][0] = lo;
        shm[threadIdx.x >> 6][1] = hi;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const long long c4 = sh[0][0] + sh[1][0] + sh[2][0] + sh[3][0];
    unsigned long long *rec = records + 5 * lo_r;
    if (c4) {
        atomicAdd(&rec[1], (unsigned long long)(sh[0][1] + sh[1][1] + sh[2][1] + sh[3][1])); // two's complement sum
        atomicAdd(&rec[2], (unsigned long long)(sh[0][2] + sh[1][2] + sh[2][2] + sh[3][2]));
        const int l4 = std::min(std::min(shm[0][0], shm[1][0]), std::min(shm[2][0], shm[3][0]));
        const int h4 = std::max(std::max(shm[0][1], shm[1][1]), std::max(shm[2][1], shm[3][1]));
        atomicMax(&rec[3], (unsigned long long)(32768 - l4));
        atomicMax(&rec[4], (unsigned long long)(h4 + 32769));
    }
    // arrive: the adds above are released before the ticket, and the last arrival acquires every other workgroup's
    const unsigned long long old = __hip_atomic_fetch_add(&rec[0], ((unsigned long long)1 << TICKET_SHIFT) + (unsigned long long)c4, __ATOMIC_ACQ_REL,
                                                          __HIP_MEMORY_SCOPE_AGENT);
    if ((long long)(old >> TICKET_SHIFT) + 1 != q.n_blocks) return;
    const unsigned long long count = (old & (((unsigned long long)1 << TICKET_SHIFT) - 1)) + (unsigned long long)c4;
    const unsigned long long le = atomicMax(&rec[3], 0ull), he = atomicMax(&rec[4], 0ull); // (returning atomics: read where the adds went)
    atomicExch(&rec[0], count); // (atomics again: the words were last written by atomics of other workgroups)
    atomicExch(&rec[3], count ? (unsigned long long)(32768 - (long long)le) : 0ull);
    atomicExch(&rec[4], count ? (unsigned long long)((long long)he - 32769) : 0ull);
}

// clamp(v, 0, n) of a double that may be anything but nan
static int64_t clamp_index(double v, int64_t n) { return v <= 0.0 ? 0 : (v >= (double)n ? n : (int64_t)v); }

// [*p0, *p1) of an axis of n pixels: the pixels that can lie in [lo, hi] (pixel units), one more on either side
static void axis_box(double lo, double hi, int64_t n, int64_t *p0, int64_t *p1) {
    if (!std::isfinite(lo) || !std::isfinite(hi)) { // no usable bound: the whole axis, the predicate decides
        *p0 = 0, *p1 = n;
        return;
    }
    *p0 = clamp_index(std::floor(lo) - 1.0, n);
    *p1 = clamp_index(std::ceil(hi) + 2.0, n);
    if (*p1 < *p0) *p1 = *p0;
}

// checks the caller's descriptors and fills what the library owns: the clipped box and the chunks' prefix sums
static int prepare(const ivx_roi *rois, int64_t n_rois, const double *points_host, int64_t n_points, std::vector<ivx_roi> &out, int64_t *blocks) {
    IVX_REQUIRE(n_rois >= 0 && n_points >= 0, IVX_EINVAL, "roi_density: negative count");
    IVX_REQUIRE(n_rois == 0 || rois, IVX_EINVAL, "roi_density: no descriptors");
    out.assign(rois, rois + n_rois);
    int64_t at = 0;
    for (int64_t r = 0; r < n_rois; r++) {
        ivx_roi &q = out[(size_t)r];
        IVX_REQUIRE(q.h >= 0 && q.w >= 0, IVX_EINVAL, "roi_density: region %lld: negative size", (long long)r);
        IVX_REQUIRE(q.kind == dr::KIND_ELLIPSE || q.kind == dr::KIND_POLYGON, IVX_EINVAL, "roi_density: region %lld: kind %d", (long long)r, q.kind);
        q.x0 = q.y0 = 0, q.x1 = q.w, q.y1 = q.h;
        if (q.kind == dr::KIND_ELLIPSE) {
            q.n_points = 0, q.first_point = 0;
            const double a = std::sqrt(q.a2), bb = std::sqrt(q.b2);
            if (q.sx > 0.0) axis_box((q.cx - a) / q.sx, (q.cx + a) / q.sx, q.w, &q.x0, &q.x1);
            if (q.sy > 0.0) axis_box((q.cy - bb) / q.sy, (q.cy + bb) / q.sy, q.h, &q.y0, &q.y1);
        } else {
            IVX_REQUIRE(q.n_points >= 0 && q.n_points <= IVX_ROI_MAX_POINTS, IVX_EINVAL, "roi_density: region %lld: a polygon of %d points (at most %d)",
                        (long long)r, q.n_points, (int)IVX_ROI_MAX_POINTS);
            IVX_REQUIRE(q.first_point >= 0 && q.first_point + q.n_points <= n_points, IVX_EINVAL,
                        "roi_density: region %lld: points [%lld, %lld) of %lld", (long long)r, (long long)q.first_point,
                        (long long)(q.first_point + q.n_points), (long long)n_points);
            if (q.n_points < 3) q.x1 = q.x0, q.y1 = q.y0; // selects nothing
            else if (points_host) {
                double lx = INFINITY, hx = -INFINITY, ly = INFINITY, hy = -INFINITY;
                bool finite = true;
                for (int k = 0; k < q.n_points; k++) {
                    const double x = points_host[2 * (q.first_point + k)], y = points_host[2 * (q.first_point + k) + 1];
                    finite = finite && std::isfinite(x) && std::isfinite(y);
                    lx = std::min(lx, x), hx = std::max(hx, x), ly = std::min(ly, y), hy = std::max(hy, y);
                }
                if (finite) { // a pixel's centre is i + 0.5
                    axis_box(lx - 0.5, hx - 0.5, q.w, &q.x0, &q.x1);
                    axis_box(ly - 0.5, hy - 0.5, q.h, &q.y0, &q.y1);
                }
            }
        }
        const int64_t bw = q.x1 - q.x0, bh = q.y1 - q.y0;
        IVX_REQUIRE(bw == 0 || bh < MAX_BOX / bw, IVX_EINVAL, "roi_density: region %lld: a box of %lld x %lld pixels", (long long)r, (long long)bh, (long long)bw);
        IVX_REQUIRE(bw * bh == 0 || q.image, IVX_EINVAL, "roi_density: region %lld: no image", (long long)r);
        IVX_REQUIRE(((q.row_stride | q.elem_stride) & 1) == 0 && (((uintptr_t)q.image) & 1) == 0, IVX_EINVAL,
                    "roi_density: region %lld: the int16 view is not aligned to its elements", (long long)r);
        q.first_block = at;
        q.n_blocks = ivx::cdiv(bw * bh, CHUNK);
        at += q.n_blocks;
        IVX_REQUIRE(at < ((int64_t)1 << 31), IVX_EINVAL, "roi_density: %lld workgroups", (long long)at);
    }
    *blocks = at;
    return IVX_OK;
}

// prepared descriptors (device image pointers) -> device, one memset, one launch
static int enqueue(const std::vector<ivx_roi> &q, int64_t blocks, const double *points_dev, int64_t *records_dev, hipStream_t st) {
    const size_t R = q.size();
    if (!R) return IVX_OK;
    IVX_HIP(hipMemsetAsync(records_dev, 0, R * IVX_ROI_RECORD_BYTES, st));
    if (!blocks) return IVX_OK;
    void *d_q;
    int rc;
    if ((rc = ivx::ws_get_s(ivx::WS_SMALL, st, R * sizeof(ivx_roi), &d_q))) return rc;
    IVX_HIP(hipMemcpyAsync(d_q, q.data(), R * sizeof(ivx_roi), hipMemcpyHostToDevice, st)); // (pageable: staged before the call returns)
    hipLaunchKernelGGL(k_roi_density, dim3((unsigned)blocks), dim3(256), 0, st, (const ivx_roi *)d_q, (int64_t)R, points_dev,
                       (unsigned long long *)records_dev);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

} // namespace

extern "C" int ivx_dev_roi_density(const ivx_roi *rois, int64_t n_rois, const double *points_host, const double *points_dev, int64_t n_points,
                                   int64_t *records, void *stream) {
    std::vector<ivx_roi> q;
    int64_t blocks = 0;
    int rc;
    if ((rc = prepare(rois, n_rois, points_host, n_points, q, &blocks))) return rc;
    IVX_REQUIRE(n_rois == 0 || records, IVX_EINVAL, "roi_density: no records block");
    IVX_REQUIRE((((uintptr_t)records) & 7) == 0, IVX_EINVAL, "roi_density: the records block is not 8-byte aligned");
    IVX_REQUIRE(n_points == 0 || (points_dev && (((uintptr_t)points_dev) & 7) == 0), IVX_EINVAL, "roi_density: the points block is missing or unaligned");
    return enqueue(q, blocks, points_dev, records, ivx::S(stream));
}

// host form: when every region's box lies in one registered array the kernel reads its mirror in place -- only descriptors
// and points go up; otherwise the boxes alone are staged dense (upload_strided serves those of a registered array from its
// mirror all the same).  R records of 40 bytes come back in one copy.
extern "C" int ivx_roi_density(const ivx_roi *rois, int64_t n_rois, const double *points, int64_t n_points, int64_t *records) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    std::vector<ivx_roi> q;
    int64_t blocks = 0;
    int rc;
    if ((rc = prepare(rois, n_rois, points, n_points, q, &blocks))) return rc;
    IVX_REQUIRE(n_points == 0 || points, IVX_EINVAL, "roi_density: no points");
    if (n_rois == 0) return IVX_OK;
    IVX_REQUIRE(records, IVX_EINVAL, "roi_density: no records block");
    const size_t R = (size_t)n_rois;
    void *d_rec, *d_pts = nullptr;
    if ((rc = ws_get(WS_OUT, R * IVX_ROI_RECORD_BYTES, &d_rec))) return rc;
    if (n_points) {
        if ((rc = ws_get(WS_AUX0, (size_t)n_points * 16, &d_pts))) return rc;
        if ((rc = copy_h2d(d_pts, points, (size_t)n_points * 16))) return rc;
    }
    // the bytes the boxes span, all regions together
    uintptr_t lo = UINTPTR_MAX, hi = 0;
    size_t box_bytes = 0;
    for (const ivx_roi &r : q) {
        if (!r.n_blocks) continue;
        for (int c = 0; c < 4; c++) {
            const int64_t y = (c & 1) ? r.y1 - 1 : r.y0, x = (c & 2) ? r.x1 - 1 : r.x0;
            const uintptr_t p = (uintptr_t)r.image + (uintptr_t)(y * r.row_stride + x * r.elem_stride);
            lo = std::min(lo, p), hi = std::max(hi, p + 2);
        }
        box_bytes += (size_t)((r.x1 - r.x0) * (r.y1 - r.y0)) * 2 + 16;
    }
    MirrorHold *hold = nullptr;
    void *mirror = nullptr;
    if (blocks && (rc = mirror_acquire((const void *)lo, hi - lo, true, &hold, &mirror))) return rc;
    if (mirror && (((uintptr_t)mirror - lo) & 1)) { // (a mirror that shifts the elements off their alignment: staged instead)
        mirror_release(hold, 0);
        hold = nullptr, mirror = nullptr;
    }
    if (mirror) {
        for (ivx_roi &r : q)
            if (r.n_blocks) r.image = (const void *)((uintptr_t)mirror + ((uintptr_t)r.image - lo));
    } else if (blocks) {
        void *d_box;
        if ((rc = ws_get(WS_IN, box_bytes, &d_box))) return rc;
        uintptr_t at = (uintptr_t)d_box;
        for (ivx_roi &r : q) {
            if (!r.n_blocks) continue;
            const int64_t bw = r.x1 - r.x0, bh = r.y1 - r.y0;
            const int64_t sh[3] = {1, bh, bw}, st[3] = {r.row_stride * bh, r.row_stride, r.elem_stride};
            const void *first = (const void *)((uintptr_t)r.image + (uintptr_t)(r.y0 * r.row_stride + r.x0 * r.elem_stride));
            if ((rc = upload_strided((void *)at, first, sh, st, 2, WS_IN))) return rc;
            // the dense box stands for rows y0.., columns x0.. of a view whose element [0][0] lies before it (never read)
            r.image = (const void *)(at - (uintptr_t)((r.y0 * bw + r.x0) * 2));
            r.row_stride = bw * 2, r.elem_stride = 2;
            at += ((size_t)(bw * bh) * 2 + 15) & ~(size_t)15;
        }
    }
    rc = enqueue(q, blocks, (const double *)d_pts, (int64_t *)d_rec, nullptr);
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) {
        set_error("roi_density: the launch did not complete (%s)", hipGetErrorString(hipGetLastError()));
        rc = IVX_EHIP;
    }
    mirror_release(hold, 0);
    if (rc) return rc;
    return copy_d2h(records, d_rec, R * IVX_ROI_RECORD_BYTES);
}
