// density_roi_math.h -- which pixels of a slice a density measure selects: rule E, the ellipse of
// CircleDensityMeasure.calc_density (invesalius/data/measures.py:2062-2064), and rule P, the polygon of
// PolygonDensityMeasure.calc_density (measures.py:2258-2276).  Everything is float64; no expression may be contracted into a
// fused multiply-add (the library is built with -ffp-contract=off, and so is the host emulation of the tests).  Plain C++
// without a GPU construct, so that the very text k_density_roi.hip and k_polygon2mask run can also be compiled for the host
// and compared with the numpy restatement where there is no GPU (tests/density_roi_host_emu.cpp, tests/test_density_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IVX_DR_HD __host__ __device__
#else
#define IVX_DR_HD
#endif

namespace ivx_density_roi_math {

enum { KIND_ELLIPSE = 0, KIND_POLYGON = 1 };

// Rule E.  Pixel (row j, column i) stands at (i * sx, j * sy) -- what np.ogrid[0:dy*sy:sy, 0:dx*sx:sx] holds, one rounded
// product each -- and is selected iff (x - cx)^2 / a2 + (y - cy)^2 / b2 <= 1.  a2 and b2 are Python's a ** 2 and b ** 2,
// computed by the caller (pow(a, 2) is not a * a for every double).  a2 == 0 or b2 == 0 gives inf or nan: a comparison with
// nan is false, nothing more is selected, as numpy has it.
IVX_DR_HD inline bool ellipse_selects(int64_t i, int64_t j, double sx, double sy, double cx, double cy, double a2, double b2) {
    const double x = (double)i * sx, y = (double)j * sy;
    const double dx = x - cx, dy = y - cy;
    const double qx = dx * dx, qy = dy * dy;
    const double tx = qx / a2, ty = qy / b2;
    const double s = tx + ty;
    return s <= 1.0;
}

// The crossing test of one edge (xi, yi) - (xj, yj) against the ray from (px, py): the expression of polygon2mask_rs
IVX_DR_HD inline bool edge_crosses(double px, double py, double xi, double yi, double xj, double yj) {
    return ((yi > py) != (yj > py)) && (px < (xj - xi) * (py - yi) / (yj - yi) + xi);
}

// odd-even rule over the n points pts[2 k], pts[2 k + 1] (closed: the last point joins the first)
IVX_DR_HD inline bool polygon_contains(const double *pts, int64_t n, double px, double py) {
    bool inside = false;
    int64_t j = n - 1;
    for (int64_t k = 0; k < n; k++) {
        if (edge_crosses(px, py, pts[2 * k], pts[2 * k + 1], pts[2 * j], pts[2 * j + 1])) inside = !inside;
        j = k;
    }
    return inside;
}

// Rule P.  The vertices are in pixel units (x / sx, y / sy); pixel i covers [i, i + 1), and it is selected iff its centre
// (i + 0.5, j + 0.5) is inside.  Fewer than three points select nothing.  (Rule E puts the pixel at i * sx, rule P at
// i + 0.5: the half pixel between them is the reference's.)
IVX_DR_HD inline bool polygon_selects(const double *pts, int64_t n, int64_t i, int64_t j) {
    if (n < 3) return false;
    return polygon_contains(pts, n, (double)i + 0.5, (double)j + 0.5);
}

} // namespace ivx_density_roi_math
