// mask3d_math.h -- the per-voxel rules of the 3-D mask editor: the projection and depth test of mask_cut
// (invesalius_rs/src/mask_cut.rs:30-60), the dab box and the sphere test of brush_mask_rs (brush_mask.rs:24-69), the clamped
// bounding box of polygon2mask_rs (polygon_mask.rs:14-36) and the Rust float -> integer casts they go through.  Everything
// is float64 in the reference's operation order; no expression may be contracted into a fused multiply-add (the library is
// built with -ffp-contract=off, and so is the host emulation of the tests).  Plain C++ and compiler builtins only, so that
// the very text k_mask3d.hip runs also compiles for the host (tests/mask3d_host_emu.cpp, tests/test_mask3d_editor_host.py).
#pragma once
#include <stdint.h>

#include "density_roi_math.h"

#if defined(__HIPCC__)
#define IVX_M3_HD __host__ __device__
#else
#define IVX_M3_HD
#endif

namespace ivx_mask3d_math {

enum { EDIT_INCLUDE = 0, EDIT_EXCLUDE = 1 };

struct Mat4 {
    double m[16]; // row-major
};

// row i of (nalgebra) Matrix4 * Vector4: the sum runs left to right over the columns
IVX_M3_HD inline double row_dot(const Mat4 &a, int i, double p0, double p1, double p2, double p3) {
    return ((a.m[4 * i] * p0 + a.m[4 * i + 1] * p1) + a.m[4 * i + 2] * p2) + a.m[4 * i + 3] * p3;
}

// Rust `f64 as usize` / `f64 as isize`: saturating, NaN -> 0
IVX_M3_HD inline uint64_t f2usize(double v) {
    if (!(v > 0.0)) return 0;
    if (v >= 18446744073709551615.0) return UINT64_MAX;
    return (uint64_t)v;
}
IVX_M3_HD inline int64_t f2isize(double v) {
    if (v != v) return 0;
    if (v <= -9223372036854775808.0) return INT64_MIN;
    if (v >= 9223372036854775807.0) return INT64_MAX;
    return (int64_t)v;
}
// Rust f64::max / f64::min: the other operand when one is NaN
IVX_M3_HD inline double rmax(double a, double b) { return a != a ? b : (b != b ? a : (a > b ? a : b)); }
IVX_M3_HD inline double rmin(double a, double b) { return a != a ? b : (b != b ? a : (a < b ? a : b)); }

// ---- the cut ---------------------------------------------------------------------------------------------------------------
enum { CUT_KEEP = 0, CUT_ON_SCREEN = 1, CUT_OFF_SCREEN = 2 };

// What mask_cut does with interior voxel (x, y, z), which the caller has found to be > 127: CUT_KEEP (behind the eye or deeper
// than max_depth), CUT_ON_SCREEN (it falls on filter cell (*fy, *fx) of the (mh, mw) filter and is zeroed iff that cell is
// set) or CUT_OFF_SCREEN (zeroed iff the edit mode is EDIT_INCLUDE).
IVX_M3_HD inline int cut_project(int64_t x, int64_t y, int64_t z, double sx, double sy, double sz, double max_depth, int64_t mh,
                                 int64_t mw, const Mat4 &m, const Mat4 &mv, int64_t *fy, int64_t *fx) {
    const double p0 = (double)x * sx, p1 = (double)y * sy, p2 = (double)z * sz;
    const double q3 = row_dot(m, 3, p0, p1, p2, 1.0);
    if (!(q3 > 0.0)) return CUT_KEEP;
    const double q0 = row_dot(m, 0, p0, p1, p2, 1.0) / q3, q1 = row_dot(m, 1, p0, p1, p2, 1.0) / q3;
    const double c3 = row_dot(mv, 3, p0, p1, p2, 1.0);
    const double c0 = row_dot(mv, 0, p0, p1, p2, 1.0) / c3, c1 = row_dot(mv, 1, p0, p1, p2, 1.0) / c3,
                 c2 = row_dot(mv, 2, p0, p1, p2, 1.0) / c3;
    const double dist = __builtin_sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    if (!(dist <= max_depth)) return CUT_KEEP;
    const double px = (q0 / 2.0 + 0.5) * (double)(mw - 1);
    const double py = (q1 / 2.0 + 0.5) * (double)(mh - 1);
    if (px >= 0.0 && px < (double)mw && py >= 0.0 && py < (double)mh) {
        *fy = (int64_t)f2usize(py);
        *fx = (int64_t)f2usize(px);
        return CUT_ON_SCREEN;
    }
    return CUT_OFF_SCREEN;
}

// true: the voxel becomes 0.  `filter` is the dense (mh, mw) byte image.
IVX_M3_HD inline bool cut_voxel(int64_t x, int64_t y, int64_t z, double sx, double sy, double sz, double max_depth,
                                const uint8_t *filter, int64_t mh, int64_t mw, const Mat4 &m, const Mat4 &mv, int edit_mode) {
    int64_t fy = 0, fx = 0;
    const int r = cut_project(x, y, z, sx, sy, sz, max_depth, mh, mw, m, mv, &fy, &fx);
    if (r == CUT_ON_SCREEN) return filter[fy * mw + fx] != 0;
    return r == CUT_OFF_SCREEN && edit_mode == EDIT_INCLUDE;
}

// ---- the brush -------------------------------------------------------------------------------------------------------------
struct DabBox {
    int64_t x0, x1, y0, y1, z0, z1; // inclusive; empty when some lower end lies above its upper end
};
IVX_M3_HD inline bool box_empty(const DabBox &b) { return b.x0 > b.x1 || b.y0 > b.y1 || b.z0 > b.z1; }
IVX_M3_HD inline bool box_holds(const DabBox &b, int64_t x, int64_t y, int64_t z) {
    return z >= b.z0 && z <= b.z1 && y >= b.y0 && y <= b.y1 && x >= b.x0 && x <= b.x1;
}
IVX_M3_HD inline int64_t box_end(uint64_t v) { return v > (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)v; }

// brush_mask.rs:24-31 for a (d, h, w) volume with d, h, w >= 1
IVX_M3_HD inline DabBox dab_box(double cx, double cy, double cz, double radius, double sx, double sy, double sz, int64_t d, int64_t h,
                                int64_t w) {
    DabBox b;
    b.x0 = box_end(f2usize(rmax(__builtin_floor((cx - radius) / sx), 0.0)));
    b.x1 = box_end(f2usize(rmin(rmax(__builtin_ceil((cx + radius) / sx), 0.0), (double)(w - 1))));
    b.y0 = box_end(f2usize(rmax(__builtin_floor((cy - radius) / sy), 0.0)));
    b.y1 = box_end(f2usize(rmin(rmax(__builtin_ceil((cy + radius) / sy), 0.0), (double)(h - 1))));
    b.z0 = box_end(f2usize(rmax(__builtin_floor((cz - radius) / sz), 0.0)));
    b.z1 = box_end(f2usize(rmin(rmax(__builtin_ceil((cz + radius) / sz), 0.0), (double)(d - 1))));
    return b;
}

// the sphere test of brush_mask.rs:40-45 / :53-58
IVX_M3_HD inline bool dab_in_sphere(int64_t x, int64_t y, int64_t z, double sx, double sy, double sz, double cx, double cy, double cz,
                                    double radius_sq) {
    const double dx = (double)x * sx - cx, dy = (double)y * sy - cy, dz = (double)z * sz - cz;
    const double dist_sq = (dx * dx + dy * dy) + dz * dz;
    return dist_sq <= radius_sq;
}

// The byte one dab leaves in a voxel it hits: -1 = unchanged.  `have` is the voxel, `orig` the same voxel of the original
// mask or -1 when no original was given.  Any other mode than 0 and 1 touches nothing.
IVX_M3_HD inline int dab_value(int edit_mode, int have, int orig) {
    if (edit_mode == EDIT_EXCLUDE) return have > 0 ? 0 : -1;
    if (edit_mode == EDIT_INCLUDE) return orig < 0 ? 255 : (orig > 0 ? orig : -1);
    return -1;
}

// ---- the screen filter -----------------------------------------------------------------------------------------------------
struct PolyBox {
    uint64_t min_x, max_x, min_y, max_y; // rows r (the x of a display point) and columns c that polygon2mask_rs tests at all
};
IVX_M3_HD inline uint64_t poly_lo(double v, int64_t lim) {
    int64_t a = f2isize(__builtin_floor(v));
    a = a == INT64_MIN ? a : a - 1;
    const uint64_t u = (uint64_t)(a > 0 ? a : 0);
    return u > (uint64_t)lim ? (uint64_t)lim : u;
}
IVX_M3_HD inline uint64_t poly_hi(double v, int64_t lim) {
    int64_t a = f2isize(__builtin_ceil(v));
    a = a == INT64_MAX ? a : a + 1;
    const uint64_t u = (uint64_t)(a > 0 ? a : 0);
    return u > (uint64_t)lim ? (uint64_t)lim : u;
}
// polygon_mask.rs:14-36 for n >= 1 points
IVX_M3_HD inline PolyBox poly_box(const double *pts, int64_t n, int64_t w, int64_t h) {
    double min_px = 1.7976931348623157e308, max_px = -1.7976931348623157e308, min_py = min_px, max_py = max_px;
    for (int64_t i = 0; i < n; i++) {
        const double x = pts[2 * i], y = pts[2 * i + 1];
        if (x < min_px) min_px = x;
        if (x > max_px) max_px = x;
        if (y < min_py) min_py = y;
        if (y > max_py) max_py = y;
    }
    PolyBox b;
    b.min_x = poly_lo(min_px, w), b.max_x = poly_hi(max_px, w);
    b.min_y = poly_lo(min_py, h), b.max_y = poly_hi(max_py, h);
    return b;
}
// polygon2mask_rs((w, h), pts)[r, c] for one polygon of n points with its box
IVX_M3_HD inline bool poly_cell(const double *pts, int64_t n, const PolyBox &b, int64_t r, int64_t c) {
    if (n <= 0) return false;
    if (!((uint64_t)r >= b.min_x && (uint64_t)r <= b.max_x && (uint64_t)c >= b.min_y && (uint64_t)c <= b.max_y)) return false;
    return ivx_density_roi_math::polygon_contains(pts, n, (double)r, (double)c);
}
// The filter of CutMaskFromPolygons at row y, column x of the (h, w) image: the OR over the K polygons of
// polygon2mask_rs((w, h), p)[x, y] -- the transposition is this exchange of indices -- inverted in EDIT_INCLUDE.
IVX_M3_HD inline bool filter_cell(const double *pts, const int64_t *offsets, const PolyBox *boxes, int64_t K, int64_t y, int64_t x,
                                  int edit_mode) {
    bool any = false;
    for (int64_t k = 0; k < K && !any; k++)
        any = poly_cell(pts + 2 * offsets[k], offsets[k + 1] - offsets[k], boxes[k], x, y);
    return edit_mode == EDIT_INCLUDE ? !any : any;
}

} // namespace ivx_mask3d_math
