// slice_show_math.h -- the arithmetic of the slice display: rules R1 - R7, the project's statement of what
// Slice.do_ww_wl, do_colour_image, do_colour_mask, do_custom_colour and do_blend (invesalius/data/slice_.py:1656-1695,
// 1771-1873) make VTK compute.  Everything is float64 unless an integer type is named; no expression may be contracted into
// a fused multiply-add (the library is built with -ffp-contract=off).  Plain C++ without a GPU construct, so that the very
// text k_slice_show.hip runs can also be compiled for the host and compared with the numpy restatement where there is no GPU
// (tests/slice_show_host_emu.cpp, tests/test_slice_display_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IVX_SS_HD __host__ __device__
#else
#define IVX_SS_HD
#endif

namespace ivx_slice_show_math {

enum { MODE_OTHER = 0, MODE_PLIST = 1, MODE_WIDGET = 2 };
// the reference's five seams as bits of `stages`
enum { ST_WWWL = 1, ST_COLOUR = 2, ST_MASK = 4, ST_AUX = 8, ST_BLEND = 16, ST_ALL = 31 };
// what the image operand holds; IMG_U8 is a grey picture (one byte per pixel, or the first byte of each RGB pixel)
enum { IMG_I16 = 0, IMG_F64 = 1, IMG_U8 = 2, IMG_RGB8 = 3 };
enum { MAX_NODES = 256, BLEND_OPACITY = 205 }; // 205 == u16(256 * 0.8 + 0.5)

IVX_SS_HD inline double clampd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }
// truncation of a non-negative double to uint8; the rules only ever hand it values in [0, 256)
IVX_SS_HD inline int u8(double x) { return (int)clampd(x, 0.0, 255.0); }
// clamp(trunc(x), 0, n - 1) without leaving the range of int
IVX_SS_HD inline int index_in(double x, int n) {
    if (!(x > 0.0)) return 0;
    if (x >= (double)n) return n - 1;
    return (int)x;
}

// what the host derives once per picture from (ww, wl), the table range and the aux table's size
struct Window {
    double lo, hi;         // R1: v <= lo -> lo_val, v >= hi -> hi_val
    double shift, scale;   // R1: u8((v + shift) * scale)
    int lo_val, hi_val;
    double r2_min, r2_scale; // R2: (g - r2_min) * r2_scale
    int r2_flat;             //     tmax <= tmin
    double r3_lo, r3_scale;  // R3: (v - r3_lo) * r3_scale
    double r6_scale;         // R6: v * r6_scale
    int r6_n;
};

// `float_input`: the MeanIP picture (float64) -- no clamp to int16's range, no truncation
inline Window make_window(double ww, double wl, int float_input, double tmin, double tmax, int aux_max) {
    Window W;
    const double f_lo = wl - ww / 2.0, f_hi = f_lo + ww;
    double lo_c = f_lo, hi_c = f_hi;
    if (!float_input) {
        lo_c = clampd(f_lo, -32768.0, 32767.0);
        hi_c = clampd(f_hi, -32768.0, 32767.0);
        W.lo = (double)(int64_t)lo_c;
        W.hi = (double)(int64_t)hi_c;
    } else {
        W.lo = lo_c;
        W.hi = hi_c;
    }
    W.lo_val = u8(clampd(255.0 * (lo_c - f_lo) / ww, 0.0, 255.0));
    W.hi_val = u8(clampd(255.0 * (hi_c - f_lo) / ww, 0.0, 255.0));
    W.shift = ww / 2.0 - wl;
    W.scale = 255.0 / ww;
    W.r2_min = tmin;
    W.r2_flat = tmax <= tmin;
    W.r2_scale = W.r2_flat ? 0.0 : 256.0 / (tmax - tmin);
    W.r3_lo = wl - ww / 2.0;
    W.r3_scale = 256.0 / ww;
    W.r6_n = aux_max + 1;
    W.r6_scale = aux_max > 0 ? (double)W.r6_n / (double)aux_max : 0.0;
    return W;
}

// R1: window / level to grey
IVX_SS_HD inline int r1_grey(const Window &W, double v) {
    if (v <= W.lo) return W.lo_val;
    if (v >= W.hi) return W.hi_val;
    const double s = v + W.shift;
    return u8(s * W.scale);
}
// R2: grey to the index of the 256-entry HSV table
IVX_SS_HD inline int r2_index(const Window &W, int g) {
    if (W.r2_flat) return (double)g > W.r2_min ? 255 : 0;
    const double d = (double)g - W.r2_min;
    return index_in(d * W.r2_scale, 256);
}
// R3: value to the index of the plist table
IVX_SS_HD inline int r3_index(const Window &W, double v) {
    const double d = v - W.r3_lo;
    return index_in(d * W.r3_scale, 256);
}
// R4: the widget's nodes, sorted by value; colours as c / 255.  out: three bytes
IVX_SS_HD inline void r4_colour(const double *values, const double *colours, int n, double v, int out[3]) {
    if (n <= 0) {
        out[0] = out[1] = out[2] = 0;
        return;
    }
    int k = -1; // the last node with value <= v
    for (int i = 0; i < n; i++)
        if (values[i] <= v) k = i;
    if (k < 0 || k == n - 1) {
        const double *c = colours + 3 * (k < 0 ? 0 : n - 1);
        for (int q = 0; q < 3; q++) out[q] = u8(c[q] * 255.0 + 0.5);
        return;
    }
    const double t = (v - values[k]) / (values[k + 1] - values[k]);
    for (int q = 0; q < 3; q++) {
        const double c0 = colours[3 * k + q], c1 = colours[3 * k + 3 + q];
        const double d = (c1 - c0) * t;
        const double c = c0 + d;
        out[q] = u8(c * 255.0 + 0.5);
    }
}
// R6: the aux byte to the index of the custom table
IVX_SS_HD inline int r6_index(const Window &W, int v) {
    if (W.r6_n <= 1) return 0;
    return index_in((double)v * W.r6_scale, W.r6_n);
}
// R7: one channel of the normal blend at opacity 0.8, in integers
IVX_SS_HD inline int r7_blend(int base, int over, int alpha) {
    const int r = alpha * BLEND_OPACITY, f = 65280 - r;
    return (base * f + over * r) >> 16;
}

} // namespace ivx_slice_show_math
