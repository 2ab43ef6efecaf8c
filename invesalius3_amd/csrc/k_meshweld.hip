// k_meshweld.hip -- surface import: a triangle soup, as an STL file holds it, to the indexed mesh every surface
// kernel of the library works on.  Replaces vtkSTLReader's merge (vtkMergePoints::InsertUniquePoint per corner in file order;
// Surface.CreateSurfaceFromFile, invesalius/data/surface.py:625-845) and the vtkTransformPolyDataFilter of
// ConvertPolydataToInv (surface.py:850-870).
//
//   stl unpack   the file's bytes are on the device; records start at byte 84 with a stride of 50, so every second record is
//                only 2-byte aligned.  A workgroup loads the 16-byte aligned span of its 128 records into LDS with uint4 loads
//                (bytes past the file's end, in the last chunk alone, one by one) and the lanes put the floats together from
//                16-bit halves there: no unaligned global load, coalesced float stores.  Raises the non-finite flag.
//   insert       one lane per corner j; open addressing with linear probing over uint32 slots holding CORNER INDICES, EMPTY =
//                0xffffffff.  At slot s: cur = atomicCAS(&tab[s], EMPTY, j); empty, or key(cur) == key(j) -> atomicMin(&tab[s],
//                j), slot_of[j] = s, done; otherwise the next slot, wrapping.  Every index ever stored in one slot carries the
//                slot's key (the CAS winner fixes it, only equal keys lower it), a key never occupies two slots (slots are never
//                emptied, so the first slot of its walk that is not another key's is the same for every lane), hence after the
//                kernel tab[slot_of[j]] is the first occurrence of j's point whatever order the waves ran in.  The walk is
//                bounded by the slot count: an overrun (impossible at load <= 1/2) sets a status word, it never spins.
//   flags, scan  rep[j] = tab[slot_of[j]]; flag[j] = rep[j] == j; scan_u32_exclusive -> new ids in first-occurrence order.
//   vertices     representatives copy their ORIGINAL bits (a first -0.0 stays -0.0).
//   faces        newid[rep[3 t + c]] and a keep flag (three different ids); a second scan; compaction in order.
//   counts       32 uint32 words on the device (IVX_WELD_*): V, kept, dropped, overrun, non-finite, longest walk, log2(slots),
//                and the walk-length histogram in words 8..23 (mesh_weld_math.h probe_bucket).  One small download.
//   transform    out = float32(((m0 x + m1 y) + m2 z) + m3) per row in float64, one lane per point (no contraction: the
//                library is built with -ffp-contract=off).
// Only vector loads, stores and atomics; plain C++.
#include <algorithm>

#include "ivx_internal.h"
#include "mesh_weld_math.h"
#include "scan_u32.h"

namespace {

namespace mw = ivx_mesh_weld_math;

constexpr int UNPACK_RECORDS = 128;                                                     // records per workgroup
constexpr int UNPACK_CHUNKS = (15 + UNPACK_RECORDS * (int)mw::STL_RECORD + 15) / 16 + 1; // 16-byte chunks of its span

__global__ __launch_bounds__(256) void k_stl_unpack(const uint8_t *__restrict__ bytes, int64_t nbytes, int64_t ntris,
                                                    uint32_t *__restrict__ soup, uint32_t *__restrict__ flag) {
    __shared__ uint4 s_span[UNPACK_CHUNKS];
    const int64_t t0 = (int64_t)blockIdx.x * UNPACK_RECORDS;
    const int nrec = ntris - t0 < UNPACK_RECORDS ? (int)(ntris - t0) : UNPACK_RECORDS;
    const int64_t start = mw::STL_HEADER + mw::STL_RECORD * t0;
    const int64_t a0 = start & ~(int64_t)15;
    const int head = (int)(start - a0);
    const int nchunks = (head + nrec * (int)mw::STL_RECORD + 15) / 16;
    for (int c = threadIdx.x; c < nchunks; c += 256) {
        const int64_t a = a0 + 16 * (int64_t)c;
        uint4 v;
        if (a + 16 <= nbytes) {
            v = *reinterpret_cast<const uint4 *>(bytes + a);
        } else { // the file's last chunk: only the bytes that exist
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            for (int q = 0; q < 16; q++)
                if (a + q < nbytes) w[q >> 2] |= (uint32_t)bytes[a + q] << (8 * (q & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        s_span[c] = v;
    }
    __syncthreads();
    const uint16_t *s16 = reinterpret_cast<const uint16_t *>(s_span);
    bool bad = false;
    for (int q = threadIdx.x; q < 9 * nrec; q += 256) {
        const int rec = q / 9, k = q - rec * 9;
        const int off = (head + rec * (int)mw::STL_RECORD + (int)mw::STL_RECORD_VERTS + 4 * k) >> 1;
        const uint32_t b = (uint32_t)s16[off] | ((uint32_t)s16[off + 1] << 16);
        bad |= mw::non_finite(b);
        soup[t0 * 9 + q] = b;
    }
    if (bad) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(256) void k_weld_insert(const uint32_t *__restrict__ soup, int64_t n, uint32_t *tab, uint32_t mask,
                                                     uint32_t *__restrict__ slot_of, uint32_t *counts) {
    __shared__ uint32_t s_hist[16];
    __shared__ uint32_t s_max;
    if (threadIdx.x < 16) s_hist[threadIdx.x] = 0;
    if (threadIdx.x == 16) s_max = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) {
        const uint32_t x = soup[3 * j], y = soup[3 * j + 1], z = soup[3 * j + 2];
        if (mw::non_finite(x) || mw::non_finite(y) || mw::non_finite(z)) atomicOr(&counts[IVX_WELD_NONFINITE], 1u);
        const uint32_t kx = mw::canon(x), ky = mw::canon(y), kz = mw::canon(z);
        uint32_t s = mw::hash(kx, ky, kz) & mask;
        const uint64_t nslots = (uint64_t)mask + 1;
        uint64_t extra = 0;
        bool done = false;
        for (; extra < nslots; extra++) {
            const uint32_t cur = atomicCAS(&tab[s], mw::EMPTY, (uint32_t)j);
            bool mine = cur == mw::EMPTY || cur == (uint32_t)j;
            if (!mine) {
                const size_t c3 = 3 * (size_t)cur;
                mine = mw::canon(soup[c3]) == kx && mw::canon(soup[c3 + 1]) == ky && mw::canon(soup[c3 + 2]) == kz;
            }
            if (mine) {
                atomicMin(&tab[s], (uint32_t)j);
                slot_of[j] = s;
                done = true;
                break;
            }
            s = (s + 1) & mask;
        }
        if (!done) {
            atomicOr(&counts[IVX_WELD_OVERRUN], 1u);
            slot_of[j] = s; // (every slot was taken: any of them holds a corner index; the host raises anyway)
        } else {
            atomicAdd(&s_hist[mw::probe_bucket(extra)], 1u);
            if (extra) atomicMax(&s_max, extra < 0xffffffffull ? (uint32_t)extra : 0xffffffffu);
        }
    }
    __syncthreads();
    if (threadIdx.x < 16 && s_hist[threadIdx.x]) atomicAdd(&counts[IVX_WELD_HIST + threadIdx.x], s_hist[threadIdx.x]);
    if (threadIdx.x == 16 && s_max) atomicMax(&counts[IVX_WELD_MAX_PROBE], s_max);
}

// slot_of[j] -> rep[j] in place (every lane reads and writes its own word); flag[j] = j is its point's first occurrence
__global__ __launch_bounds__(256) void k_weld_flags(const uint32_t *__restrict__ tab, uint32_t *__restrict__ rep,
                                                    uint32_t *__restrict__ flag, int64_t n) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = tab[rep[j]];
    rep[j] = r;
    flag[j] = r == (uint32_t)j ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_weld_vertices(const uint32_t *__restrict__ soup, const uint32_t *__restrict__ rep,
                                                       const uint32_t *__restrict__ newid, uint32_t *__restrict__ verts, int64_t n) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n || rep[j] != (uint32_t)j) return;
    const size_t o = 3 * (size_t)newid[j]; // newid[j] <= j < n: inside the 3 T points of room
    verts[o] = soup[3 * j];
    verts[o + 1] = soup[3 * j + 1];
    verts[o + 2] = soup[3 * j + 2];
}

__global__ __launch_bounds__(256) void k_weld_faces(const uint32_t *__restrict__ rep, const uint32_t *__restrict__ newid,
                                                    int32_t *__restrict__ tmp, uint32_t *__restrict__ keep, int64_t ntris) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ntris) return;
    const uint32_t a = newid[rep[3 * t]], b = newid[rep[3 * t + 1]], c = newid[rep[3 * t + 2]];
    tmp[3 * t] = (int32_t)a;
    tmp[3 * t + 1] = (int32_t)b;
    tmp[3 * t + 2] = (int32_t)c;
    keep[t] = (a != b && b != c && a != c) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_weld_compact_faces(const int32_t *__restrict__ tmp, const uint32_t *__restrict__ pos,
                                                            int32_t *__restrict__ faces, int64_t ntris, uint32_t *counts) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) counts[IVX_WELD_DROPPED] = (uint32_t)ntris - counts[IVX_WELD_KEPT]; // (the scan's total is there already)
    if (t >= ntris) return;
    const int32_t a = tmp[3 * t], b = tmp[3 * t + 1], c = tmp[3 * t + 2];
    if (a == b || b == c || a == c) return;
    const size_t o = 3 * (size_t)pos[t]; // pos[t] <= t < ntris
    faces[o] = a;
    faces[o + 1] = b;
    faces[o + 2] = c;
}

struct Affine {
    double m[16];
};

__global__ __launch_bounds__(256) void k_mesh_transform_points(const float *verts, int64_t n, Affine a, float *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = (double)verts[3 * i], y = (double)verts[3 * i + 1], z = (double)verts[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double p0 = a.m[4 * r] * x, p1 = a.m[4 * r + 1] * y, p2 = a.m[4 * r + 2] * z;
        out[3 * i + r] = (float)(((p0 + p1) + p2) + a.m[4 * r + 3]);
    }
}

static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct WeldLayout {
    uint64_t slots;
    size_t off_tab, off_rep, off_newid, off_tmp, off_keep, off_bsum, total;
};

static bool weld_layout(int64_t ntris, WeldLayout *w) {
    if (ntris < 0 || ntris > mw::MAX_CORNERS / 3) return false;
    const int64_t n = 3 * ntris;
    w->slots = mw::slots(n);
    size_t o = 0;
    w->off_tab = o, o += up256((size_t)w->slots * 4);
    w->off_rep = o, o += up256((size_t)n * 4 + 4);
    w->off_newid = o, o += up256((size_t)n * 4 + 4);
    w->off_tmp = o, o += up256((size_t)n * 4 + 4);
    w->off_keep = o, o += up256((size_t)ntris * 4 + 4);
    w->off_bsum = o, o += up256(((size_t)scan_u32_blocks(n) + 2) * 4);
    w->total = o;
    return true;
}

static int check_counts(const uint32_t *got, int64_t *counts) {
    if (counts)
        for (int q = 0; q < IVX_WELD_COUNT_WORDS; q++) counts[q] = (int64_t)got[q];
    IVX_REQUIRE(!got[IVX_WELD_OVERRUN], IVX_EINTERNAL, "mesh weld: a probe walked the whole table (internal error)");
    IVX_REQUIRE(!got[IVX_WELD_NONFINITE], IVX_EDOM, "mesh weld: the soup holds a coordinate that is not finite");
    return IVX_OK;
}

} // namespace

extern "C" int ivx_mesh_weld_slots(int64_t n_corners, uint64_t *slots) {
    IVX_REQUIRE(slots != nullptr, IVX_EINVAL, "mesh weld: null argument");
    IVX_REQUIRE(n_corners >= 0 && n_corners <= mw::MAX_CORNERS, IVX_EDOM, "mesh weld: %lld corners, at most 2^31 - 1",
                (long long)n_corners);
    *slots = mw::slots(n_corners);
    return IVX_OK;
}

extern "C" int ivx_mesh_weld_bytes(int64_t ntris, size_t *bytes) {
    WeldLayout w;
    IVX_REQUIRE(bytes != nullptr, IVX_EINVAL, "mesh weld: null argument");
    IVX_REQUIRE(weld_layout(ntris, &w), IVX_EDOM, "mesh weld: %lld triangles, at most (2^31 - 1) / 3", (long long)ntris);
    *bytes = w.total;
    return IVX_OK;
}

extern "C" int ivx_dev_stl_unpack(const uint8_t *bytes, int64_t ntris, float *soup_out, uint32_t *flag, void *stream) {
    IVX_REQUIRE(ntris >= 0 && ntris <= mw::MAX_CORNERS / 3, IVX_EDOM, "stl unpack: %lld triangles, at most (2^31 - 1) / 3",
                (long long)ntris);
    IVX_REQUIRE(((uintptr_t)bytes & 15) == 0, IVX_EINVAL, "stl unpack: the file's bytes must start at a 16-byte aligned address");
    if (ntris == 0) return IVX_OK;
    hipLaunchKernelGGL(k_stl_unpack, dim3((unsigned)ivx::cdiv(ntris, UNPACK_RECORDS)), dim3(256), 0, ivx::S(stream), bytes,
                       mw::stl_file_bytes(ntris), ntris, (uint32_t *)soup_out, flag);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_mesh_weld(const float *soup, int64_t ntris, void *scratch, float *verts_out, int32_t *faces_out,
                                 uint32_t *counts_out, void *stream) {
    WeldLayout w;
    IVX_REQUIRE(weld_layout(ntris, &w), IVX_EDOM, "mesh weld: %lld triangles, at most (2^31 - 1) / 3", (long long)ntris);
    hipStream_t st = ivx::S(stream);
    IVX_HIP(hipMemsetAsync(counts_out, 0, IVX_WELD_COUNT_WORDS * 4, st));
    if (ntris == 0) return IVX_OK;
    const int64_t n = 3 * ntris;
    char *base = (char *)scratch;
    uint32_t *tab = (uint32_t *)(base + w.off_tab), *rep = (uint32_t *)(base + w.off_rep);
    uint32_t *newid = (uint32_t *)(base + w.off_newid), *keep = (uint32_t *)(base + w.off_keep);
    uint32_t *bsum = (uint32_t *)(base + w.off_bsum);
    int32_t *tmp = (int32_t *)(base + w.off_tmp);
    const uint32_t *bits = (const uint32_t *)soup;
    int rc, lg = 0;
    while ((1ull << lg) < w.slots) lg++;
    IVX_HIP(hipMemsetAsync(tab, 0xff, (size_t)w.slots * 4, st));
    IVX_HIP(hipMemsetAsync(counts_out + IVX_WELD_LOG2_SLOTS, lg, 1, st)); // (one byte of a zeroed little-endian word)
    const unsigned gn = (unsigned)ivx::cdiv(n, 256), gt = (unsigned)ivx::cdiv(ntris, 256);
    hipLaunchKernelGGL(k_weld_insert, dim3(gn), dim3(256), 0, st, bits, n, tab, (uint32_t)(w.slots - 1), rep, counts_out);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_weld_flags, dim3(gn), dim3(256), 0, st, tab, rep, newid, n);
    IVX_LAUNCH_CHECK();
    if ((rc = scan_u32_exclusive(newid, n, bsum, counts_out + IVX_WELD_VERTS, st))) return rc;
    hipLaunchKernelGGL(k_weld_vertices, dim3(gn), dim3(256), 0, st, bits, rep, newid, (uint32_t *)verts_out, n);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_weld_faces, dim3(gt), dim3(256), 0, st, rep, newid, tmp, keep, ntris);
    IVX_LAUNCH_CHECK();
    if ((rc = scan_u32_exclusive(keep, ntris, bsum, counts_out + IVX_WELD_KEPT, st))) return rc;
    hipLaunchKernelGGL(k_weld_compact_faces, dim3(gt), dim3(256), 0, st, tmp, keep, faces_out, ntris, counts_out);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_mesh_transform_points(const float *verts, int64_t nverts, const double *m16, float *out, void *stream) {
    IVX_REQUIRE(nverts >= 0 && m16 != nullptr, IVX_EINVAL, "mesh transform: bad argument");
    if (nverts == 0) return IVX_OK;
    Affine a;
    for (int q = 0; q < 16; q++) a.m[q] = m16[q];
    hipLaunchKernelGGL(k_mesh_transform_points, dim3((unsigned)ivx::cdiv(nverts, 256)), dim3(256), 0, ivx::S(stream), verts, nverts,
                       a, out);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

// ---- host forms -----------------------------------------------------------------------------------------------------
namespace {

// weld of the soup in d_soup (device), results to the host arrays (room for 3 T points and T facets)
static int weld_to_host(const float *d_soup, int64_t ntris, float *verts_out, int32_t *faces_out, int64_t *counts) {
    using namespace ivx;
    size_t nb;
    int rc;
    if ((rc = ivx_mesh_weld_bytes(ntris, &nb))) return rc;
    void *d_ws, *d_v, *d_f, *d_c;
    if ((rc = ws_get(WS_MESH, nb + 16, &d_ws))) return rc;
    if ((rc = ws_get(WS_OUT, (size_t)ntris * 36 + 16, &d_v))) return rc;
    if ((rc = ws_get(WS_AUX1, (size_t)ntris * 12 + 16, &d_f))) return rc;
    if ((rc = ws_get(WS_SMALL, IVX_WELD_COUNT_WORDS * 4, &d_c))) return rc;
    if ((rc = ivx_dev_mesh_weld(d_soup, ntris, d_ws, (float *)d_v, (int32_t *)d_f, (uint32_t *)d_c, nullptr))) return rc;
    uint32_t got[IVX_WELD_COUNT_WORDS];
    IVX_HIP(hipMemcpy(got, d_c, sizeof got, hipMemcpyDeviceToHost));
    if ((rc = check_counts(got, counts))) return rc;
    if (verts_out && got[IVX_WELD_VERTS]) IVX_HIP(hipMemcpy(verts_out, d_v, (size_t)got[IVX_WELD_VERTS] * 12, hipMemcpyDeviceToHost));
    if (faces_out && got[IVX_WELD_KEPT]) IVX_HIP(hipMemcpy(faces_out, d_f, (size_t)got[IVX_WELD_KEPT] * 12, hipMemcpyDeviceToHost));
    return IVX_OK;
}

} // namespace

extern "C" int ivx_mesh_weld(const float *soup, int64_t ntris, float *verts_out, int32_t *faces_out, int64_t *counts) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(ntris >= 0 && ntris <= mw::MAX_CORNERS / 3, IVX_EDOM, "mesh weld: %lld triangles, at most (2^31 - 1) / 3",
                (long long)ntris);
    if (counts)
        for (int q = 0; q < IVX_WELD_COUNT_WORDS; q++) counts[q] = 0;
    if (ntris == 0) return IVX_OK;
    void *d_s;
    int rc;
    if ((rc = ws_get(WS_IN, (size_t)ntris * 36 + 16, &d_s))) return rc;
    if ((rc = copy_h2d(d_s, soup, (size_t)ntris * 36))) return rc;
    return weld_to_host((const float *)d_s, ntris, verts_out, faces_out, counts);
}

extern "C" int ivx_mesh_stl_weld(const uint8_t *file_bytes, size_t nbytes, float *verts_out, int32_t *faces_out, int64_t *counts) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(file_bytes != nullptr && nbytes >= (size_t)mw::STL_HEADER, IVX_EDOM, "stl: shorter than a binary header");
    uint32_t cnt;
    memcpy(&cnt, file_bytes + 80, 4);
    const int64_t ntris = (int64_t)cnt;
    IVX_REQUIRE((uint64_t)nbytes == (uint64_t)mw::STL_HEADER + (uint64_t)mw::STL_RECORD * cnt, IVX_EDOM,
                "stl: %zu bytes are not 84 + 50 * %u", nbytes, cnt);
    IVX_REQUIRE(ntris <= mw::MAX_CORNERS / 3, IVX_EDOM, "mesh weld: %lld triangles, at most (2^31 - 1) / 3", (long long)ntris);
    if (counts)
        for (int q = 0; q < IVX_WELD_COUNT_WORDS; q++) counts[q] = 0;
    if (ntris == 0) return IVX_OK;
    void *d_b, *d_s, *d_c;
    int rc;
    if ((rc = ws_get(WS_AUX0, nbytes + 16, &d_b))) return rc;
    if ((rc = ws_get(WS_IN, (size_t)ntris * 36 + 16, &d_s))) return rc;
    if ((rc = ws_get(WS_SMALL, IVX_WELD_COUNT_WORDS * 4, &d_c))) return rc;
    if ((rc = copy_h2d(d_b, file_bytes, nbytes))) return rc;
    IVX_HIP(hipMemsetAsync(d_c, 0, 4, nullptr));
    if ((rc = ivx_dev_stl_unpack((const uint8_t *)d_b, ntris, (float *)d_s, (uint32_t *)d_c, nullptr))) return rc;
    return weld_to_host((const float *)d_s, ntris, verts_out, faces_out, counts); // (the weld raises the same flag again)
}

extern "C" int ivx_mesh_transform_points(const float *verts, int64_t nverts, const double *m16, float *out) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(nverts >= 0 && m16 != nullptr, IVX_EINVAL, "mesh transform: bad argument");
    if (nverts == 0) return IVX_OK;
    void *d_v;
    int rc;
    if ((rc = ws_get(WS_IN, (size_t)nverts * 12 + 16, &d_v))) return rc;
    if ((rc = copy_h2d(d_v, verts, (size_t)nverts * 12))) return rc;
    if ((rc = ivx_dev_mesh_transform_points((const float *)d_v, nverts, m16, (float *)d_v, nullptr))) return rc;
    IVX_HIP(hipDeviceSynchronize());
    return copy_d2h(out, d_v, (size_t)nverts * 12);
}
