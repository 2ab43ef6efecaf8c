// k_mask3d.hip -- the 3-D mask editor: polygon cuts and 3-D brush strokes in place on the padded mask matrix.
//
// Reference semantics (byte-exact; the per-voxel rules are mask3d_math.h, float64 in the reference's order):
//   screen filter  Mask3DEditorState.get_filters + CutMaskFromPolygons:196-200 (invesalius/data/mask3d_editor_state.py):
//                  OR of polygon2mask_rs over the polygons, transposed, inverted in include mode
//   cut            mask_cut (invesalius_rs/src/mask_cut.rs:7-61) on matrix[1:, 1:, 1:]
//   brush stroke   brush_mask_rs (brush_mask.rs:5-71) once per dab of a drag
//   equal          the np.array_equal of start_brush_stroke:293-296
//
// MI355X design.  The matrix is (d+1, h+1, w+1) bytes with one plane of slice flags in front of every axis; the voxels are
// the interior [1:, 1:, 1:], whose rows start at odd addresses.  The cut therefore does not walk rows: it walks the matrix
// as one stream of 16-byte chunks aligned in memory (one chunk per lane and step, 1 KB per wave and load), finds each
// byte's padded coordinates by counting on from the chunk's first, and takes a byte for a voxel only when all three are
// >= 1.  The bytes in front of the first aligned address and behind the last whole chunk go one per lane through the same
// rule.  A chunk is stored whole only when none of its bytes is padding; otherwise its changed bytes are stored one by one,
// so a flag byte is never written.  The float64 projection runs only for voxels > 127.  The stroke is launched over the
// 16 x 4 x 4 tiles of the union of its dabs' boxes; a workgroup first lists, in LDS, the dabs whose box meets its tile.
#include <algorithm>
#include <vector>

#include "ivx_internal.h"
#include "mask3d_math.h"

namespace m3 = ivx_mask3d_math;

namespace {

union Chunk16 {
    uint4 q;
    uint8_t b[16];
};

// ---- screen filter ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_m3e_boxes(const double *__restrict__ pts, const int64_t *__restrict__ offsets, int64_t K, int64_t w,
                                                  int64_t h, m3::PolyBox *__restrict__ boxes) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    const int64_t n = offsets[k + 1] - offsets[k];
    m3::PolyBox b = {0, 0, 0, 0};
    if (n > 0) b = m3::poly_box(pts + 2 * offsets[k], n, w, h);
    boxes[k] = b;
}

__global__ __launch_bounds__(256) void k_m3e_filter(uint8_t *__restrict__ out, int64_t h, int64_t w, const double *__restrict__ pts,
                                                    const int64_t *__restrict__ offsets, const m3::PolyBox *__restrict__ boxes, int64_t K,
                                                    int edit_mode) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= h * w) return;
    const int64_t y = i / w, x = i - y * w;
    out[i] = m3::filter_cell(pts, offsets, boxes, K, y, x, edit_mode) ? 1 : 0;
}

// ---- cut -------------------------------------------------------------------------------------------------------------------
struct CutArgs {
    int64_t n;          // bytes of the padded matrix
    int64_t head;       // bytes in front of the first 16-byte boundary (0 .. 15, <= n)
    int64_t nchunks;    // whole aligned chunks after the head
    int64_t ph, pw;     // padded rows per plane, padded bytes per row
    int64_t pad;        // 1: the padded matrix; 0: a dense block of voxels alone (a DeviceVolume's mask)
    double sx, sy, sz, max_depth;
    int64_t mh, mw;
    int edit_mode;
};

// byte `at` of the padded matrix, one voxel or none
__device__ __forceinline__ void cut_byte(uint8_t *__restrict__ mat, int64_t at, const CutArgs &a, const uint8_t *__restrict__ filter,
                                         const m3::Mat4 &m, const m3::Mat4 &mv, uint8_t *__restrict__ plane_flags) {
    if (!(mat[at] > 127)) return;
    const int64_t px = at % a.pw, r = at / a.pw, py = r % a.ph, pz = r / a.ph;
    if (px < a.pad || py < a.pad || pz < a.pad) return; // a slice flag, not a voxel
    if (m3::cut_voxel(px - a.pad, py - a.pad, pz - a.pad, a.sx, a.sy, a.sz, a.max_depth, filter, a.mh, a.mw, m, mv, a.edit_mode)) {
        mat[at] = 0;
        plane_flags[pz] = 1;
    }
}

__global__ __launch_bounds__(256) void k_m3e_cut(uint8_t *__restrict__ mat, CutArgs a, const uint8_t *__restrict__ filter, m3::Mat4 m,
                                                 m3::Mat4 mv, uint8_t *__restrict__ plane_flags) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t c = t; c < a.nchunks; c += stride) {
        const int64_t off = a.head + c * 16; // off + 16 <= n
        Chunk16 v;
        v.q = *reinterpret_cast<const uint4 *>(mat + off);
        bool any = false;
#pragma unroll
        for (int i = 0; i < 16; i++) any |= v.b[i] > 127;
        if (!any) continue;
        int64_t px = off % a.pw, r = off / a.pw, py = r % a.ph, pz = r / a.ph;
        uint32_t changed = 0;
        bool padding = false;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const bool voxel = px >= a.pad && py >= a.pad && pz >= a.pad;
            padding |= !voxel;
            if (voxel && v.b[i] > 127 &&
                m3::cut_voxel(px - a.pad, py - a.pad, pz - a.pad, a.sx, a.sy, a.sz, a.max_depth, filter, a.mh, a.mw, m, mv, a.edit_mode)) {
                v.b[i] = 0;
                changed |= 1u << i;
                plane_flags[pz] = 1;
            }
            if (++px == a.pw) {
                px = 0;
                if (++py == a.ph) {
                    py = 0;
                    pz++;
                }
            }
        }
        if (!changed) continue;
        if (!padding) {
            *reinterpret_cast<uint4 *>(mat + off) = v.q;
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++)
                if ((changed >> i) & 1) mat[off + i] = 0;
        }
    }
    // the bytes in front of the first chunk and behind the last one: at most 15 each
    const int64_t tail0 = a.head + a.nchunks * 16;
    const int64_t loose = a.head + (a.n - tail0);
    for (int64_t i = t; i < loose; i += stride) cut_byte(mat, i < a.head ? i : tail0 + (i - a.head), a, filter, m, mv, plane_flags);
}

// ---- brush stroke ----------------------------------------------------------------------------------------------------------
constexpr int STROKE_CAP = 256; // centres of one launch (LDS: 24 B of centre, 24 B of box, 2 B of list each)
constexpr int TX = 16, TY = 4, TZ = 4;

struct StrokeArgs {
    int64_t d, h, w;          // interior
    int64_t ps, rs, pad;      // bytes between planes / rows; 1 for the padded matrix, 0 for a block of voxels alone
    int64_t x0, y0, z0;       // the union box's lower corner (interior coordinates)
    int64_t tx, ty, tz;       // tiles along each axis
    double sx, sy, sz, radius, radius_sq;
    int n;                    // centres of this launch, 1 .. STROKE_CAP
    int edit_mode;            // 0 or 1
};

__global__ __launch_bounds__(256) void k_m3e_stroke(uint8_t *__restrict__ mat, const uint8_t *__restrict__ orig, StrokeArgs a,
                                                    const double *__restrict__ centres, uint8_t *__restrict__ plane_flags) {
    __shared__ double s_c[STROKE_CAP * 3];
    __shared__ int32_t s_box[STROKE_CAP * 6];
    __shared__ uint16_t s_list[STROKE_CAP];
    __shared__ int s_count;
    const int t = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t tix = tile % a.tx, tr = tile / a.tx, tiy = tr % a.ty, tiz = tr / a.ty;
    const int64_t bx0 = a.x0 + tix * TX, by0 = a.y0 + tiy * TY, bz0 = a.z0 + tiz * TZ;
    if (t == 0) s_count = 0;
    __syncthreads();
    for (int k = t; k < a.n; k += 256) {
        const double cx = centres[3 * k], cy = centres[3 * k + 1], cz = centres[3 * k + 2];
        const m3::DabBox b = m3::dab_box(cx, cy, cz, a.radius, a.sx, a.sy, a.sz, a.d, a.h, a.w);
        s_c[3 * k] = cx, s_c[3 * k + 1] = cy, s_c[3 * k + 2] = cz;
        // (the box ends are < 2^31: the entry point admits no longer axis)
        s_box[6 * k] = (int32_t)b.x0, s_box[6 * k + 1] = (int32_t)b.x1, s_box[6 * k + 2] = (int32_t)b.y0;
        s_box[6 * k + 3] = (int32_t)b.y1, s_box[6 * k + 4] = (int32_t)b.z0, s_box[6 * k + 5] = (int32_t)b.z1;
        const bool meets = !m3::box_empty(b) && b.x0 < bx0 + TX && b.x1 >= bx0 && b.y0 < by0 + TY && b.y1 >= by0 && b.z0 < bz0 + TZ &&
                           b.z1 >= bz0;
        if (meets) s_list[atomicAdd(&s_count, 1)] = (uint16_t)k;
    }
    __syncthreads();
    const int count = s_count;
    if (count == 0) return;
    const int64_t x = bx0 + (t % TX), y = by0 + (t / TX) % TY, z = bz0 + t / (TX * TY);
    if (x >= a.w || y >= a.h || z >= a.d) return;
    bool hit = false;
    for (int j = 0; j < count && !hit; j++) {
        const int k = s_list[j];
        const m3::DabBox b = {s_box[6 * k], s_box[6 * k + 1], s_box[6 * k + 2], s_box[6 * k + 3], s_box[6 * k + 4], s_box[6 * k + 5]};
        hit = m3::box_holds(b, x, y, z) && m3::dab_in_sphere(x, y, z, a.sx, a.sy, a.sz, s_c[3 * k], s_c[3 * k + 1], s_c[3 * k + 2], a.radius_sq);
    }
    if (!hit) return;
    const int64_t at = (z + a.pad) * a.ps + (y + a.pad) * a.rs + (x + a.pad);
    const int have = mat[at];
    int o = -1;
    if (a.edit_mode == m3::EDIT_INCLUDE && orig) o = orig[at];
    const int v = m3::dab_value(a.edit_mode, have, o);
    if (v >= 0 && v != have) {
        mat[at] = (uint8_t)v;
        plane_flags[z + a.pad] = 1;
    }
}

// ---- apply: dst[1:, 1:, 1:] = src[1:, 1:, 1:] (update_views) -----------------------------------------------------------------
// Both are padded matrices of the same shape.  One byte per lane and step: src and dst are two different allocations whose
// 16-byte boundaries need not coincide, and the pass is rare (once per tool event, after the kernel that did the work).
__global__ __launch_bounds__(256) void k_m3e_apply(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, int64_t n, int64_t ph,
                                                   int64_t pw, uint8_t *__restrict__ plane_flags) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; at < n; at += stride) {
        const uint8_t v = src[at];
        if (v == dst[at]) continue;
        const int64_t px = at % pw, r = at / pw, py = r % ph, pz = r / ph;
        if (px == 0 || py == 0 || pz == 0) continue;
        dst[at] = v;
        plane_flags[pz] = 1;
    }
}

// ---- Mask.modified(all_volume=True): matrix[0] = matrix[:, 0, :] = matrix[:, :, 0] = 1 ------------------------------------------
__global__ __launch_bounds__(256) void k_m3e_flag_planes(uint8_t *__restrict__ mat, int64_t pd, int64_t ph, int64_t pw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t a = ph * pw, b = pd * pw, c = pd * ph;
    if (i < a) mat[i] = 1;                                                  // [0, y, x]
    else if (i < a + b) mat[((i - a) / pw) * a + (i - a) % pw] = 1;         // [z, 0, x]
    else if (i < a + b + c) mat[((i - a - b) / ph) * a + ((i - a - b) % ph) * pw] = 1; // [z, y, 0]
}

// ---- equal -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_m3e_differ(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int64_t n, int vec,
                                                    int *__restrict__ differ) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool d = false;
    const int64_t nchunks = vec ? n / 16 : 0;
    for (int64_t c = t; c < nchunks; c += stride) {
        const uint4 p = reinterpret_cast<const uint4 *>(a)[c], q = reinterpret_cast<const uint4 *>(b)[c];
        d |= ((p.x ^ q.x) | (p.y ^ q.y) | (p.z ^ q.z) | (p.w ^ q.w)) != 0;
    }
    for (int64_t i = nchunks * 16 + t; i < n; i += stride) d |= a[i] != b[i];
    if (d) *differ = 1; // (every writer stores the same value)
}

static inline unsigned grid_for(int64_t n, int per = 1) {
    const int64_t b = ivx::cdiv(n, (int64_t)256 * per);
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(b, 16384));
}

inline void copy_mat(m3::Mat4 *dst, const double *src) {
    for (int i = 0; i < 16; i++) dst->m[i] = src[i];
}

struct Padded {
    int64_t d, h, w, pad, pd, ph, pw, n;
};
// the padded matrix of a (d, h, w) interior, dense: strides ((h+1)(w+1), w+1, 1); or, with strides (h w, w, 1), the voxels alone
int padded_of(const char *what, const int64_t shape[3], const int64_t st[3], Padded *p) {
    IVX_REQUIRE(shape[0] >= 0 && shape[1] >= 0 && shape[2] >= 0, IVX_EINVAL, "%s: negative shape", what);
    IVX_REQUIRE(shape[0] < ((int64_t)1 << 31) - 1 && shape[1] < ((int64_t)1 << 31) - 1 && shape[2] < ((int64_t)1 << 31) - 1, IVX_EINVAL,
                "%s: an axis of 2^31 voxels or more", what);
    p->d = shape[0], p->h = shape[1], p->w = shape[2];
    p->pad = (st[2] == 1 && st[1] == p->w && st[0] == p->h * p->w) ? 0 : 1;
    p->pd = p->d + p->pad, p->ph = p->h + p->pad, p->pw = p->w + p->pad;
    p->n = p->pd * p->ph * p->pw;
    IVX_REQUIRE(st[2] == 1 && st[1] == p->pw && st[0] == p->ph * p->pw, IVX_EINVAL,
                "%s: the padded matrix must be dense (strides %lld, %lld, %lld for interior %lld x %lld x %lld)", what, (long long)st[0],
                (long long)st[1], (long long)st[2], (long long)p->d, (long long)p->h, (long long)p->w);
    return IVX_OK;
}

} // namespace

extern "C" int ivx_m3e_brush_capacity(void) { return STROKE_CAP; }

extern "C" int ivx_dev_m3e_filter(int64_t w, int64_t h, const double *points_dev, const int64_t *offsets_dev, int64_t n_polygons,
                                  int edit_mode, uint8_t *out, void *stream) {
    IVX_REQUIRE(w >= 0 && h >= 0 && n_polygons >= 0, IVX_EINVAL, "m3e_filter: negative size");
    IVX_REQUIRE(edit_mode == m3::EDIT_INCLUDE || edit_mode == m3::EDIT_EXCLUDE, IVX_EINVAL, "m3e_filter: edit mode %d", edit_mode);
    if (w == 0 || h == 0) return IVX_OK;
    IVX_REQUIRE(out && (n_polygons == 0 || offsets_dev), IVX_EINVAL, "m3e_filter: null block");
    IVX_REQUIRE(ivx::cdiv(w * h, 256) < ((int64_t)1 << 31), IVX_EINVAL, "m3e_filter: a viewport of %lld x %lld", (long long)w, (long long)h);
    hipStream_t st = ivx::S(stream);
    if (n_polygons == 0) {
        IVX_HIP(hipMemsetAsync(out, edit_mode == m3::EDIT_INCLUDE ? 1 : 0, (size_t)(w * h), st));
        return IVX_OK;
    }
    void *boxes;
    int rc;
    if ((rc = ivx::ws_get_s(ivx::WS_SMALL, st, (size_t)n_polygons * sizeof(m3::PolyBox), &boxes))) return rc;
    hipLaunchKernelGGL(k_m3e_boxes, dim3((unsigned)ivx::cdiv(n_polygons, 64)), dim3(64), 0, st, points_dev, offsets_dev, n_polygons, w, h,
                       (m3::PolyBox *)boxes);
    IVX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_m3e_filter, dim3((unsigned)ivx::cdiv(w * h, 256)), dim3(256), 0, st, out, h, w, points_dev, offsets_dev,
                       (const m3::PolyBox *)boxes, n_polygons, edit_mode);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_m3e_cut(uint8_t *matrix, const int64_t shape[3], const int64_t strides[3], const double spacing[3], double max_depth,
                               const uint8_t *filter, int64_t mh, int64_t mw, const double *m, const double *mv, int edit_mode,
                               uint8_t *plane_flags, void *stream) {
    Padded p;
    int rc;
    if ((rc = padded_of("m3e_cut", shape, strides, &p))) return rc;
    IVX_REQUIRE(mh >= 0 && mw >= 0, IVX_EINVAL, "m3e_cut: negative filter shape");
    if (p.d == 0 || p.h == 0 || p.w == 0) return IVX_OK;
    IVX_REQUIRE(matrix && plane_flags && m && mv && (filter || mh * mw == 0), IVX_EINVAL, "m3e_cut: null block");
    CutArgs a;
    a.n = p.n;
    a.head = std::min<int64_t>((int64_t)((16 - ((uintptr_t)matrix & 15)) & 15), p.n);
    a.nchunks = (p.n - a.head) / 16;
    a.ph = p.ph, a.pw = p.pw, a.pad = p.pad;
    a.sx = spacing[0], a.sy = spacing[1], a.sz = spacing[2], a.max_depth = max_depth;
    a.mh = mh, a.mw = mw, a.edit_mode = edit_mode;
    m3::Mat4 A, B;
    copy_mat(&A, m);
    copy_mat(&B, mv);
    hipLaunchKernelGGL(k_m3e_cut, dim3(grid_for(a.nchunks)), dim3(256), 0, ivx::S(stream), matrix, a, filter, A, B,
                       plane_flags);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_m3e_brush_stroke(uint8_t *matrix, const uint8_t *orig, const int64_t shape[3], const int64_t strides[3],
                                        const double spacing[3], const double *centres_host, const double *centres_dev, int64_t n_centres,
                                        double radius, int edit_mode, uint8_t *plane_flags, void *stream) {
    Padded p;
    int rc;
    if ((rc = padded_of("m3e_brush_stroke", shape, strides, &p))) return rc;
    IVX_REQUIRE(n_centres >= 0, IVX_EINVAL, "m3e_brush_stroke: negative count");
    if (p.d == 0 || p.h == 0 || p.w == 0 || n_centres == 0) return IVX_OK;
    if (edit_mode != m3::EDIT_INCLUDE && edit_mode != m3::EDIT_EXCLUDE) return IVX_OK; // the reference touches nothing in any other mode
    IVX_REQUIRE(matrix && plane_flags && centres_host && centres_dev, IVX_EINVAL, "m3e_brush_stroke: null block");
    StrokeArgs a;
    a.d = p.d, a.h = p.h, a.w = p.w, a.ps = p.ph * p.pw, a.rs = p.pw, a.pad = p.pad;
    a.sx = spacing[0], a.sy = spacing[1], a.sz = spacing[2], a.radius = radius, a.radius_sq = radius * radius;
    a.edit_mode = edit_mode;
    for (int64_t first = 0; first < n_centres; first += STROKE_CAP) {
        const int64_t n = std::min<int64_t>(STROKE_CAP, n_centres - first);
        m3::DabBox u = {INT64_MAX, -1, INT64_MAX, -1, INT64_MAX, -1};
        for (int64_t k = first; k < first + n; k++) {
            const m3::DabBox b = m3::dab_box(centres_host[3 * k], centres_host[3 * k + 1], centres_host[3 * k + 2], radius, a.sx, a.sy, a.sz, p.d,
                                             p.h, p.w);
            if (m3::box_empty(b)) continue;
            u.x0 = std::min(u.x0, b.x0), u.x1 = std::max(u.x1, b.x1);
            u.y0 = std::min(u.y0, b.y0), u.y1 = std::max(u.y1, b.y1);
            u.z0 = std::min(u.z0, b.z0), u.z1 = std::max(u.z1, b.z1);
        }
        if (m3::box_empty(u)) continue; // no dab of this launch reaches the volume
        a.x0 = u.x0, a.y0 = u.y0, a.z0 = u.z0;
        a.tx = ivx::cdiv(u.x1 - u.x0 + 1, TX), a.ty = ivx::cdiv(u.y1 - u.y0 + 1, TY), a.tz = ivx::cdiv(u.z1 - u.z0 + 1, TZ);
        a.n = (int)n;
        const int64_t tiles = a.tx * a.ty * a.tz;
        IVX_REQUIRE(tiles < ((int64_t)1 << 31), IVX_EINVAL, "m3e_brush_stroke: %lld tiles", (long long)tiles);
        hipLaunchKernelGGL(k_m3e_stroke, dim3((unsigned)tiles), dim3(256), 0, ivx::S(stream), matrix, orig, a, centres_dev + 3 * first,
                           plane_flags);
        IVX_LAUNCH_CHECK();
    }
    return IVX_OK;
}

extern "C" int ivx_dev_m3e_apply(uint8_t *matrix, const uint8_t *src, const int64_t shape[3], const int64_t strides[3],
                                 uint8_t *plane_flags, void *stream) {
    Padded p;
    int rc;
    if ((rc = padded_of("m3e_apply", shape, strides, &p))) return rc;
    IVX_REQUIRE(p.pad == 1, IVX_EINVAL, "m3e_apply: the padded matrix");
    if (p.d == 0 || p.h == 0 || p.w == 0) return IVX_OK;
    IVX_REQUIRE(matrix && src && plane_flags, IVX_EINVAL, "m3e_apply: null block");
    hipLaunchKernelGGL(k_m3e_apply, dim3(grid_for(p.n, 4)), dim3(256), 0, ivx::S(stream), matrix, src, p.n, p.ph, p.pw, plane_flags);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_m3e_equal(const uint8_t *a, const uint8_t *b, int64_t n, int *equal, void *stream) {
    IVX_REQUIRE(n >= 0 && equal, IVX_EINVAL, "m3e_equal: negative size or null");
    *equal = 1;
    if (n == 0) return IVX_OK;
    IVX_REQUIRE(a && b, IVX_EINVAL, "m3e_equal: null block");
    hipStream_t st = ivx::S(stream);
    void *d;
    int rc;
    if ((rc = ivx::ws_get_s(ivx::WS_SMALL, st, 64, &d))) return rc;
    IVX_HIP(hipMemsetAsync(d, 0, 4, st));
    const int vec = ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0;
    hipLaunchKernelGGL(k_m3e_differ, dim3(grid_for(n, 16)), dim3(256), 0, st, a, b, n, vec, (int *)d);
    IVX_LAUNCH_CHECK();
    int differ = 0;
    IVX_HIP(hipMemcpyAsync(&differ, d, 4, hipMemcpyDeviceToHost, st));
    IVX_HIP(hipStreamSynchronize(st));
    *equal = differ ? 0 : 1;
    return IVX_OK;
}

// ---- host forms ---------------------------------------------------------------------------------------------------------------
namespace {

// polygons -> device: points and offsets in one block of `slot`
int upload_polygons(int slot, const double *points, const int64_t *offsets, int64_t K, const double **d_pts, const int64_t **d_off) {
    using namespace ivx;
    *d_pts = nullptr, *d_off = nullptr;
    if (K == 0) return IVX_OK;
    IVX_REQUIRE(offsets && offsets[0] == 0, IVX_EINVAL, "m3e: the polygons' offsets start at 0");
    for (int64_t k = 0; k < K; k++) IVX_REQUIRE(offsets[k + 1] >= offsets[k], IVX_EINVAL, "m3e: the polygons' offsets decrease");
    const int64_t npts = offsets[K];
    IVX_REQUIRE(npts == 0 || points, IVX_EINVAL, "m3e: null points");
    void *blk;
    int rc;
    const size_t off_bytes = (size_t)(K + 1) * 8, pts_at = (off_bytes + 15) & ~(size_t)15;
    if ((rc = ws_get(slot, pts_at + (size_t)npts * 16 + 16, &blk))) return rc;
    IVX_HIP(hipMemcpy(blk, offsets, off_bytes, hipMemcpyHostToDevice));
    if (npts) IVX_HIP(hipMemcpy((char *)blk + pts_at, points, (size_t)npts * 16, hipMemcpyHostToDevice));
    *d_off = (const int64_t *)blk;
    *d_pts = (const double *)((char *)blk + pts_at);
    return IVX_OK;
}

// What the host forms share: the matrix in device memory (its mirror, or a staged copy), the kernel, the way back.
struct HostEdit {
    ivx::MirrorHold *hold = nullptr;
    void *dev = nullptr; // the padded matrix
    void *flags = nullptr;
    bool bound = false;
    Padded p;
    uint8_t *host = nullptr;
    int64_t st[3];

    int open(const char *what, uint8_t *matrix, const int64_t shape[3], const int64_t strides[3]) {
        using namespace ivx;
        int rc;
        if ((rc = padded_of(what, shape, strides, &p))) return rc;
        IVX_REQUIRE(matrix, IVX_EINVAL, "%s: null matrix", what);
        host = matrix;
        for (int i = 0; i < 3; i++) st[i] = strides[i];
        if ((rc = ws_get(WS_AUX1, (size_t)p.pd + 16, &flags))) return rc;
        IVX_HIP(hipMemsetAsync(flags, 0, (size_t)p.pd, nullptr));
        if ((rc = mirror_acquire(matrix, (size_t)p.n, true, &hold, &dev))) return rc;
        bound = dev != nullptr;
        if (!bound) { // staged once
            const int64_t psh[3] = {p.pd, p.ph, p.pw};
            if ((rc = ws_get(WS_OUT, (size_t)p.n + 16, &dev))) return rc;
            if ((rc = upload_strided(dev, matrix, psh, st, 1, WS_OUT))) return rc;
        }
        return IVX_OK;
    }
    // after the kernels (rc: theirs): the changed planes to the host, the hold released
    int close(int rc, int64_t *planes_written) {
        using namespace ivx;
        std::vector<uint8_t> f((size_t)p.pd);
        if (!rc && hipMemcpy(f.data(), flags, (size_t)p.pd, hipMemcpyDeviceToHost) != hipSuccess) { // (small, like seeds; waits for the kernels)
            set_error("m3e: the edit did not complete (%s)", hipGetErrorString(hipGetLastError()));
            rc = IVX_EHIP;
        }
        const int64_t pb = p.ph * p.pw;
        int64_t written = 0;
        for (int64_t z = 0; !rc && z < p.pd;) {
            if (!f[(size_t)z]) {
                z++;
                continue;
            }
            int64_t q = z;
            while (q < p.pd && f[(size_t)q]) q++;
            if (bound) {
                rc = mirror_fetch(hold, host + z * pb, (const uint8_t *)dev + z * pb, (size_t)((q - z) * pb));
            } else {
                const int64_t psh[3] = {q - z, p.ph, p.pw};
                rc = download_strided(host + z * pb, psh, st, (const uint8_t *)dev + z * pb, 1, WS_OUT);
            }
            written += q - z;
            z = q;
        }
        if (bound) mirror_release(hold, (size_t)(written * pb));
        hold = nullptr;
        if (!rc && planes_written) *planes_written = written;
        return rc;
    }
    void abandon() {
        if (hold) ivx::mirror_release(hold, 0);
        hold = nullptr;
    }
};

} // namespace

extern "C" int ivx_m3e_filter(int64_t w, int64_t h, const double *points, const int64_t *offsets, int64_t n_polygons, int edit_mode,
                              uint8_t *out) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(w >= 0 && h >= 0 && n_polygons >= 0, IVX_EINVAL, "m3e_filter: negative size");
    if (w == 0 || h == 0) return IVX_OK;
    const double *d_pts;
    const int64_t *d_off;
    void *d_out;
    int rc;
    if ((rc = upload_polygons(WS_AUX0, points, offsets, n_polygons, &d_pts, &d_off))) return rc;
    if ((rc = ws_get(WS_AUX2, (size_t)(w * h) + 16, &d_out))) return rc;
    if ((rc = ivx_dev_m3e_filter(w, h, d_pts, d_off, n_polygons, edit_mode, (uint8_t *)d_out, nullptr))) return rc;
    IVX_HIP(hipMemcpy(out, d_out, (size_t)(w * h), hipMemcpyDeviceToHost));
    return IVX_OK;
}

extern "C" int ivx_m3e_cut(uint8_t *matrix, const int64_t shape[3], const int64_t strides[3], const double spacing[3], double max_depth,
                           const uint8_t *filter, int64_t mh, int64_t mw, const double *points, const int64_t *offsets, int64_t n_polygons,
                           const double *m, const double *mv, int edit_mode, int64_t *planes_written) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(mh >= 0 && mw >= 0 && n_polygons >= 0 && m && mv && spacing, IVX_EINVAL, "m3e_cut: negative size or null");
    if (planes_written) *planes_written = 0;
    if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return IVX_OK;
    // the filter first: given as an (mh, mw) byte image, or made on the device from the polygons
    void *d_f = nullptr;
    int rc;
    if ((rc = ws_get(WS_AUX2, (size_t)(mh * mw) + 16, &d_f))) return rc;
    if (filter) {
        if (mh * mw) IVX_HIP(hipMemcpy(d_f, filter, (size_t)(mh * mw), hipMemcpyHostToDevice));
    } else {
        const double *d_pts;
        const int64_t *d_off;
        if ((rc = upload_polygons(WS_AUX0, points, offsets, n_polygons, &d_pts, &d_off))) return rc;
        if ((rc = ivx_dev_m3e_filter(mw, mh, d_pts, d_off, n_polygons, edit_mode, (uint8_t *)d_f, nullptr))) return rc;
    }
    HostEdit e;
    if ((rc = e.open("m3e_cut", matrix, shape, strides))) {
        e.abandon();
        return rc;
    }
    rc = ivx_dev_m3e_cut((uint8_t *)e.dev, shape, strides, spacing, max_depth, (const uint8_t *)d_f, mh, mw, m, mv, edit_mode,
                         (uint8_t *)e.flags, nullptr);
    return e.close(rc, planes_written);
}

extern "C" int ivx_m3e_brush_stroke(uint8_t *matrix, const uint8_t *orig, const int64_t shape[3], const int64_t strides[3],
                                    const double spacing[3], const double *centres, int64_t n_centres, double radius, int edit_mode,
                                    int64_t *planes_written) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    IVX_REQUIRE(n_centres >= 0 && spacing, IVX_EINVAL, "m3e_brush_stroke: negative count or null");
    if (planes_written) *planes_written = 0;
    if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0 || n_centres == 0) return IVX_OK;
    if (edit_mode != m3::EDIT_INCLUDE && edit_mode != m3::EDIT_EXCLUDE) return IVX_OK;
    Padded p;
    int rc;
    if ((rc = padded_of("m3e_brush_stroke", shape, strides, &p))) return rc;
    IVX_REQUIRE(centres, IVX_EINVAL, "m3e_brush_stroke: null centres");
    // the original before the matrix is held: a bound original comes from its own mirror, device to device
    void *d_orig = nullptr, *d_c;
    if (orig && edit_mode == m3::EDIT_INCLUDE) {
        const int64_t psh[3] = {p.pd, p.ph, p.pw};
        if ((rc = ws_get(WS_IN, (size_t)p.n + 16, &d_orig))) return rc;
        if ((rc = upload_strided(d_orig, orig, psh, strides, 1, WS_IN))) return rc;
    }
    if ((rc = ws_get(WS_AUX0, (size_t)n_centres * 24 + 16, &d_c))) return rc;
    IVX_HIP(hipMemcpy(d_c, centres, (size_t)n_centres * 24, hipMemcpyHostToDevice));
    HostEdit e;
    if ((rc = e.open("m3e_brush_stroke", matrix, shape, strides))) {
        e.abandon();
        return rc;
    }
    rc = ivx_dev_m3e_brush_stroke((uint8_t *)e.dev, (const uint8_t *)d_orig, shape, strides, spacing, centres, (const double *)d_c, n_centres,
                                  radius, edit_mode, (uint8_t *)e.flags, nullptr);
    return e.close(rc, planes_written);
}

// matrix[1:, 1:, 1:] = src[1:, 1:, 1:] for a padded device block `src` of the same shape (update_views)
extern "C" int ivx_m3e_apply(uint8_t *matrix, const uint8_t *src_dev, const int64_t shape[3], const int64_t strides[3],
                             int64_t *planes_written) {
    ivx::HostCallGuard host_guard__;
    IVX_REQUIRE(src_dev, IVX_EINVAL, "m3e_apply: null block");
    if (planes_written) *planes_written = 0;
    if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return IVX_OK;
    HostEdit e;
    int rc;
    if ((rc = e.open("m3e_apply", matrix, shape, strides))) {
        e.abandon();
        return rc;
    }
    rc = ivx_dev_m3e_apply((uint8_t *)e.dev, src_dev, shape, strides, (uint8_t *)e.flags, nullptr);
    return e.close(rc, planes_written);
}

// Mask.modified(all_volume=True) (invesalius/data/mask.py:462-466): the three flag planes become 1.  The host's are written
// by the CPU, a registered matrix's mirror by a kernel: no byte crosses the link.
extern "C" int ivx_m3e_flag_planes(uint8_t *matrix, const int64_t shape[3], const int64_t strides[3]) {
    ivx::HostCallGuard host_guard__;
    using namespace ivx;
    Padded p;
    int rc;
    if ((rc = padded_of("m3e_flag_planes", shape, strides, &p))) return rc;
    IVX_REQUIRE(p.pad == 1, IVX_EINVAL, "m3e_flag_planes: the padded matrix");
    IVX_REQUIRE(matrix, IVX_EINVAL, "m3e_flag_planes: null matrix");
    MirrorHold *hold;
    void *mirror;
    if ((rc = mirror_acquire(matrix, (size_t)p.n, true, &hold, &mirror))) return rc;
    const int64_t a = p.ph * p.pw, total = a + p.pd * p.pw + p.pd * p.ph;
    if (mirror) {
        hipLaunchKernelGGL(k_m3e_flag_planes, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, nullptr, (uint8_t *)mirror, p.pd, p.ph, p.pw);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) {
            set_error("m3e_flag_planes: the launch did not complete");
            rc = IVX_EHIP;
        }
    }
    if (!rc) {
        memset(matrix, 1, (size_t)a);
        for (int64_t z = 0; z < p.pd; z++) {
            memset(matrix + z * a, 1, (size_t)p.pw);
            for (int64_t y = 0; y < p.ph; y++) matrix[z * a + y * p.pw] = 1;
        }
    }
    mirror_release(hold, mirror && !rc ? (size_t)total : 0);
    return rc;
}
