// imagegeo_math.h -- the arithmetic of the gantry-tilt correction: scipy.ndimage.shift(slice, (s, 0), order 3,
// mode "constant", output int16) as imagedata_utils.FixGantryTilt calls it once per slice (imagedata_utils.py:143-154),
// restated for one image column.  The y axis is prefiltered in float64 with the cubic B-spline pole (gain, exact mirror
// initialisations, causal and anti-causal recursion), an output row reads four taps around its source coordinate with the
// end samples mirrored, and the sum is stored rounded half away from zero and clamped.  The x axis has shift 0: its
// prefilter plus interpolation is the identity to about 2e-11 and is not run.  Plain C++ without a GPU construct, every
// operation written in the reference's order and compiled with -ffp-contract=off, so that the very text k_imagegeo.hip runs
// can be compiled for the host and compared with live scipy where there is no GPU (tests/imagegeo_host_emu.cpp,
// tests/test_imagegeo_host.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define IVX_IG_HD __host__ __device__
#else
#define IVX_IG_HD
#endif

namespace ivx_imagegeo {

constexpr int NO_MIN = 0x7fffffff; // "no value seen": the minimum of nothing

// the one pole of the cubic B-spline, sqrt(3) - 2 (the literal is the double nearest sqrt(3)), and the gain the
// prefilter multiplies every sample by first
IVX_IG_HD inline double pole() { return 1.7320508075688772 - 2.0; }
IVX_IG_HD inline double gain() {
    const double z = pole();
    return (1.0 - z) * (1.0 - 1.0 / z);
}

// pole ** (n - 1) as the reference forms it: the C library's pow.  Host only -- a device pow need not round alike, so the
// kernels are handed this number.
inline double pole_power(int64_t n) { return pow(pole(), (double)(n - 1)); }

// The prefilter of one line of n samples, in[i * is] -> c[i * cs].  A line of one sample is left as it is.
// *imin: the smallest input sample (NO_MIN for an empty line).
IVX_IG_HD inline void prefilter_line(const int16_t *in, int64_t is, double *c, int64_t cs, int64_t n, double zn1, int *imin) {
    int lo = NO_MIN;
    if (n < 2) {
        if (n == 1) {
            c[0] = (double)in[0];
            lo = in[0];
        }
        *imin = lo;
        return;
    }
    const double z = pole(), g = gain();
    // the exact causal initialisation for a signal mirrored about its end samples, over the whole line
    double c0 = (double)in[0] * g + zn1 * ((double)in[(n - 1) * is] * g);
    double zi = z;
    for (int64_t i = 1; i < n - 1; i++) {
        c0 = c0 + zi * ((double)in[i * is] * g + zn1 * ((double)in[(n - 1 - i) * is] * g));
        zi = zi * z;
    }
    c0 = c0 / (1.0 - zn1 * zn1);
    lo = in[0];
    c[0] = c0;
    double prev = c0;
    for (int64_t i = 1; i < n; i++) { // causal
        const int v = in[i * is];
        lo = v < lo ? v : lo;
        prev = (double)v * g + z * prev;
        c[i * cs] = prev;
    }
    // anti-causal initialisation, then the recursion
    double next = (z * c[(n - 2) * cs] + prev) * z / (z * z - 1.0);
    c[(n - 1) * cs] = next;
    for (int64_t i = n - 2; i >= 0; i--) {
        next = z * (next - c[i * cs]);
        c[i * cs] = next;
    }
    *imin = lo;
}

// Source coordinate of output row y: ``cc = y + (-shift)``; false when it falls outside [0, H - 1] -- the whole row is
// `cval` then.  `nshift` is the negated shift, as the reference hands it to its C code.
IVX_IG_HD inline bool row_source(int64_t y, double nshift, int64_t H, double *cc) {
    const double c = (double)y + nshift;
    *cc = c;
    return !(c < 0.0 || c > (double)(H - 1));
}

// the cubic B-spline weights of the four taps floor(cc) - 1 .. floor(cc) + 2
IVX_IG_HD inline void weights(double cc, double w[4]) {
    const double y = cc - floor(cc), z = 1.0 - y;
    w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
    w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = z * z * z / 6.0;
    double last = 1.0;
    for (int k = 0; k < 3; k++) last -= w[k];
    w[3] = last;
}

// a tap index mirrored about the end samples (-1 -> 1, n -> n - 2), any distance; a line of one sample is sample 0
IVX_IG_HD inline int64_t mirror_index(int64_t idx, int64_t n) {
    if (n <= 1) return 0;
    const int64_t s2 = 2 * n - 2;
    if (idx < 0) {
        idx = s2 * (-idx / s2) + idx;
        return idx <= 1 - n ? idx + s2 : -idx;
    }
    if (idx >= n) {
        idx -= s2 * (idx / s2);
        if (idx >= n) idx = s2 - idx;
    }
    return idx;
}

IVX_IG_HD inline double interpolate(const double *c, int64_t cs, int64_t n, double cc) {
    const int64_t start = (int64_t)floor(cc) - 1;
    double w[4];
    weights(cc, w);
    double t = 0.0;
    for (int k = 0; k < 4; k++) t += c[mirror_index(start + k, n) * cs] * w[k];
    return t;
}

// the store into an int16 output: half away from zero, clamped, truncated
IVX_IG_HD inline int16_t round_store_i16(double t) {
    t = t > 0 ? t + 0.5 : t - 0.5;
    if (t > 32767.0) t = 32767.0;
    else if (t < -32768.0)
        t = -32768.0;
    return (int16_t)t;
}

// One column of one slice: img[y * s] for y < H is replaced by the shifted column; rows that fall outside are left as they
// are (the fill pass writes them).  c: H doubles of scratch, stride cs.  *imin: the smallest sample read, *omin: the
// smallest sample written (NO_MIN when no row was).
IVX_IG_HD inline void shift_column(int16_t *img, int64_t s, double *c, int64_t cs, int64_t H, double nshift, double zn1, int *imin,
                                   int *omin) {
    prefilter_line(img, s, c, cs, H, zn1, imin);
    int lo = NO_MIN;
    for (int64_t y = 0; y < H; y++) {
        double cc;
        if (!row_source(y, nshift, H, &cc)) continue;
        const int16_t v = round_store_i16(interpolate(c, cs, H, cc));
        img[y * s] = v;
        lo = v < lo ? v : lo;
    }
    *omin = lo;
}

// does slice with this shift have a row that the fill pass writes?
inline bool has_fill_rows(int64_t H, double nshift) {
    double cc;
    for (int64_t y = 0; y < H; y++)
        if (!row_source(y, nshift, H, &cc)) return true;
    return false;
}

// The chain of fill values: FixGantryTilt takes ``cval = matrix.min()`` anew before every slice, so slice n sees the
// corrected slices before it and the original ones from itself on.  old_min[n]: the minimum of the original slice;
// new_min[n]: of the rows shift_column wrote (NO_MIN: none); fills[n]: the slice has rows to fill.
inline void resolve_cvals(int64_t D, const int *old_min, const int *new_min, const uint8_t *fills, int *cval) {
    int run = NO_MIN;
    for (int64_t n = D - 1; n >= 0; n--) { // cval[n] <- min of the original slices n ..
        run = old_min[n] < run ? old_min[n] : run;
        cval[n] = run;
    }
    run = NO_MIN; // min of the corrected slices .. n - 1
    for (int64_t n = 0; n < D; n++) {
        if (run < cval[n]) cval[n] = run;
        int full = new_min[n];
        if (fills[n] && cval[n] < full) full = cval[n];
        run = full < run ? full : run;
    }
}

} // namespace ivx_imagegeo
