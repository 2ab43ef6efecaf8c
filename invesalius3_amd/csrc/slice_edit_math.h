// slice_edit_math.h -- the arithmetic of the slice brush: where a dab's footprint window lands on the slice, what
// of it survives the four clips, and the byte a footprint pixel addresses in a strided 2-D view.  It restates the part the
// three edit_mask_pixel bodies of the reference share (invesalius/data/slice_.py:656-715, styles.py:392-455, :2000-2063).
// Plain C++ without a GPU construct, so that the very text k_slice_edit.hip runs can also be compiled for the host and
// compared with the reference's golden vectors where there is no GPU (tests/slice_edit_host_emu.cpp,
// tests/test_editor_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IVX_SE_HD __host__ __device__
#else
#define IVX_SE_HD
#endif

namespace ivx_slice_edit {

// python's int(float): toward zero; saturated far outside any slice so that the window sums below cannot overflow
IVX_SE_HD inline int64_t trunc_i64(double v) {
    if (!(v == v)) return 0;
    if (v >= 1073741824.0) return 1073741824;
    if (v <= -1073741824.0) return -1073741824;
    return (int64_t)v;
}

// (px, py) of a position given as ONE flat integer: ``py = position / W`` is a float division, ``px = position % W``
// python's modulo, the sign of the divisor (slice_.py:677-678)
inline void flat_position(int64_t position, int64_t W, double *px, double *py) {
    int64_t m = position % W;
    if (m != 0 && ((m < 0) != (W < 0))) m += W;
    *px = (double)m;
    *py = (double)position / (double)W;
}

// first column (or row) of the unclipped window: ``c = n / 2 + 1`` (float), ``int(p - n + c)``  (slice_.py:690-695)
IVX_SE_HD inline int64_t window_start(double p, int64_t n) {
    const double c = (double)n / 2.0 + 1.0;
    return trunc_i64((p - (double)n) + c);
}

// One axis of the four clips (slice_.py:697-709): the window [i0, i0 + n) against [0, extent).  `skip` footprint columns are
// trimmed at the low side, `count` are left, the first of them lands on slice column `at`.  A window that misses the slice
// leaves count == 0: the reference then indexes with an empty boolean array and writes nothing.
struct Clip {
    int64_t at, skip, count;
};
IVX_SE_HD inline Clip clip_axis(int64_t i0, int64_t n, int64_t extent) {
    Clip c;
    c.skip = i0 < 0 ? -i0 : 0;
    c.at = i0 < 0 ? 0 : i0;
    int64_t end = i0 + n;
    if (end > extent) end = extent;
    c.count = end - c.at;
    if (c.skip > n) c.skip = n;
    if (c.count < 0) c.count = 0;
    return c;
}

// Footprint pixel (fy, fx) of a dab whose window starts at (xi, yi): its slice pixel, or false when it lies outside the
// h x w slice.  This is the test every store and every image load of the kernel goes through, whatever the host clipped.
IVX_SE_HD inline bool dab_pixel(int64_t xi, int64_t yi, int64_t fy, int64_t fx, int64_t h, int64_t w, int64_t *y, int64_t *x) {
    const int64_t yy = yi + fy, xx = xi + fx;
    if (yy < 0 || yy >= h || xx < 0 || xx >= w) return false;
    *y = yy;
    *x = xx;
    return true;
}

// byte offset of slice pixel (y, x) in a 2-D view with signed byte strides
IVX_SE_HD inline int64_t view_offset(int64_t y, int64_t x, int64_t row_stride, int64_t elem_stride) {
    return y * row_stride + x * elem_stride;
}

// the rule of one operation (invesalius/constants.py:341-346, slice_.py:721-739): the byte to write, or -1 for "leave it"
enum { OP_DRAW = 0, OP_ERASE = 1, OP_THRESH = 2, OP_THRESH_ERASE = 3, OP_THRESH_ADD_ONLY = 4, OP_THRESH_ERASE_ONLY = 5, OP_FILL = 6 };
IVX_SE_HD inline int op_value(int op, int v, int lo, int hi, int fill) {
    const bool in = v >= lo && v <= hi;
    switch (op) {
    case OP_ERASE: return 1;
    case OP_DRAW: return 254;
    case OP_THRESH: return in ? 254 : 1;
    case OP_THRESH_ERASE: return in ? 1 : 254;
    case OP_THRESH_ADD_ONLY: return in ? 254 : -1;
    case OP_THRESH_ERASE_ONLY: return in ? -1 : 1;
    case OP_FILL: return fill & 255;
    }
    return -1;
}
IVX_SE_HD inline bool op_reads_image(int op) { return op >= OP_THRESH && op <= OP_THRESH_ERASE_ONLY; }

} // namespace ivx_slice_edit
