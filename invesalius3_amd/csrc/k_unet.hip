// k_unet.hip -- the deep-learning brain (MRI T1) and trachea (CT) segmentation on the GPU.
//
// Replaces invesalius/segmentation/deep_learning/segment.py:74-191 (gen_patches + segment_torch) and model.py:9-113 (the
// Unet3D both tools share), as run by BrainSegmentProcess / TracheaSegmentProcess, and the mask write of
// SegmentProcess.apply_segment_threshold (segment.py:465-490).  float32 in, float32 accumulate; no library kernels.
//
//   * conv 5^3 pad 2 and ConvTranspose3d k4 s2 p1 are one implicit-GEMM kernel on v_mfma_f32_16x16x4_f32: M = output
//     voxels of a batch of patches (channels-last activations), N = output channels, K = taps x input channels.  A wave
//     owns MT x NT tiles of 16 x 16; A and B come straight from global memory (L1 / L2 hold the 5^3 halo and the weights).
//     The transposed conv is split into its 8 output-parity classes, each a 2^3-tap conv; a wave's tiles are all of one
//     class, so its weight rows are wave-uniform.  Folded BatchNorm + bias + ReLU sit in the epilogue; the decoder's
//     torch.cat((up, skip), 1) is two source pointers, never a copy.
//   * every sum is an ordered MFMA chain or a serial loop: no atomics, two runs give the same bits.
//   * segment pipeline: numpy-exact normalisation (int16 wraps included), patch gather with zero fill, per-voxel in-order
//     accumulation over the cuts that cover it (so the result does not depend on the batch split), count and divide
//     (correctly rounded f32 '/', built without fast-math), threshold into the mask.
#include <math.h>

#include <vector>

#include "ivx_internal.h"

namespace {
using namespace ivx;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NLEV = 4;                 // pooling levels
constexpr int FEAT[5] = {8, 16, 32, 64, 128};
constexpr int TABLE_INTS = 3 * 16384;   // per-axis cover ranges of the segment pipeline (axes up to 16384)
constexpr int MAX_CUT_AXIS = 16384;
constexpr int NLAYERS = 27;             // launches of one forward (ivx_unet3d_layer_times)

struct Layer {       // one conv or transposed conv, device layouts
    int cin, cinpad, cout, coutpad, kind; // kind 0: conv 5^3 + ReLU, 1: ConvTranspose3d (no ReLU)
    float *w;        // conv: [125][cinpad][coutpad]; upconv: [8 class][8 tap][cinpad][coutpad]
    float *b;        // [coutpad]
};

struct Net {
    Layer enc[5][2];  // enc1..enc4, bottleneck
    Layer up[4];      // upconv for level 3..0 (index = level)
    Layer dec[4][2];  // decoder of level 0..3
    float head[9];    // 8 weights + bias of the final 1x1 conv
};

struct ConvArgs {
    const float *src0, *src1;
    int c0, c1, cinpad;
    const float *w, *b;
    float *dst;
    int cout, coutpad;
    int S;           // input edge (conv: = output edge)
    int nvox;        // batch * S^3
    int tiles_per_class, ngroups, relu;
};

// one wave: MT x NT tiles of 16 output voxels x 16 output channels.  Lane l holds A[voxel l&15][k l>>4] and
// B[k l>>4][channel l&15]; C/D: channel = l&15, voxel = 4 (l>>4) + r.
template <int MT, int NT, int KIND>
__global__ __launch_bounds__(256) void k_conv(ConvArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int ngrp = a.ngroups;
    const int cls = KIND == 1 ? wave / (a.tiles_per_class * ngrp) : 0;
    const int rem = KIND == 1 ? wave - cls * a.tiles_per_class * ngrp : wave;
    const int tile = rem / ngrp, grp = rem - tile * ngrp;
    if (KIND == 1 && cls >= 8) return;
    const int m0 = tile * 16 * MT;
    if (m0 >= a.nvox) return; // wave-uniform
    const int row = lane & 15, kq = lane >> 4;
    const int S = a.S, S3 = S * S * S;
    const int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
    int vn[MT], vz[MT], vy[MT], vx[MT];
    bool vm[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        const int m = m0 + mt * 16 + row;
        vm[mt] = m < a.nvox;
        const int mm = vm[mt] ? m : 0;
        vn[mt] = mm / S3;
        int r = mm - vn[mt] * S3;
        vz[mt] = r / (S * S);
        r -= vz[mt] * S * S;
        vy[mt] = r / S;
        vx[mt] = r - vy[mt] * S;
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int cin = a.c0 + a.c1, cinpad = a.cinpad, coutpad = a.coutpad;
    const int ncol0 = grp * NT * 16 + row;
    const int ntaps = KIND == 0 ? 125 : 8;
    const float *wcls = a.w + (size_t)(KIND == 1 ? cls * 8 : 0) * cinpad * coutpad;
    for (int t = 0; t < ntaps; t++) {
        int dz, dy, dx;
        if (KIND == 0) {
            dz = t / 25 - 2;
            dy = (t / 5) % 5 - 2;
            dx = t % 5 - 2;
        } else { // input i = q + p - b per axis
            dz = pz - ((t >> 2) & 1);
            dy = py - ((t >> 1) & 1);
            dx = px - (t & 1);
        }
        int base[MT];
        bool inb[MT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const int z = vz[mt] + dz, y = vy[mt] + dy, x = vx[mt] + dx;
            inb[mt] = vm[mt] && (unsigned)z < (unsigned)S && (unsigned)y < (unsigned)S && (unsigned)x < (unsigned)S;
            base[mt] = inb[mt] ? ((vn[mt] * S + z) * S + y) * S + x : 0;
        }
        const float *wt = wcls + (size_t)t * cinpad * coutpad;
        for (int ci0 = 0; ci0 < cin; ci0 += 4) {
            const int ci = ci0 + kq;
            const bool first = ci0 < a.c0; // a 4-channel step never straddles the two sources (c0 % 4 == 0 or c1 == 0)
            const float *src = first ? a.src0 : a.src1;
            const int C = first ? a.c0 : a.c1;
            const int cc = first ? ci : ci - a.c0;
            float av[MT], bv[NT];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) av[mt] = (inb[mt] && cc < C) ? src[(size_t)base[mt] * C + cc] : 0.f;
            const float *wr = wt + (size_t)ci * coutpad + ncol0; // ci < cinpad: padded rows are zero
#pragma unroll
            for (int nt = 0; nt < NT; nt++) bv[nt] = ncol0 + nt * 16 < coutpad ? wr[nt * 16] : 0.f;
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int nt = 0; nt < NT; nt++)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
        }
    }
    // epilogue: + folded bias, ReLU, channels-last store
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const int j = ncol0 + nt * 16;
        if (j >= a.cout) continue;
        const float bj = a.b[j];
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = m0 + mt * 16 + kq * 4 + r;
                if (m >= a.nvox) continue;
                float v = acc[mt][nt][r] + bj;
                if (a.relu) v = v > 0.f ? v : 0.f;
                size_t o;
                if (KIND == 0) {
                    o = (size_t)m;
                } else {
                    const int n = m / S3;
                    int q = m - n * S3;
                    const int qz = q / (S * S);
                    q -= qz * S * S;
                    const int qy = q / S, qx = q - qy * S, T = 2 * S;
                    o = (((size_t)n * T + 2 * qz + pz) * T + 2 * qy + py) * T + 2 * qx + px;
                }
                a.dst[o * a.cout + j] = v;
            }
    }
}

// MaxPool3d(2), channels-last: in (n, S, S, S, C) -> out (n, S/2, S/2, S/2, C)
__global__ __launch_bounds__(256) void k_pool(const float *__restrict__ in, float *__restrict__ out, int S, int C,
                                              int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int h = S / 2;
    const int c = (int)(i % C);
    int64_t v = i / C;
    const int x = (int)(v % h);
    v /= h;
    const int y = (int)(v % h);
    v /= h;
    const int z = (int)(v % h);
    const int64_t n = v / h;
    float m = -INFINITY;
    for (int dz = 0; dz < 2; dz++)
        for (int dy = 0; dy < 2; dy++)
            for (int dx = 0; dx < 2; dx++) {
                const float e = in[((((n * S + 2 * z + dz) * S + 2 * y + dy) * S) + 2 * x + dx) * C + c];
                m = e > m ? e : m;
            }
    out[i] = m;
}

struct Head {
    float w[9];
};

// Conv3d(8 -> 1, k 1) + sigmoid
__global__ __launch_bounds__(256) void k_head(const float *__restrict__ in, float *__restrict__ out, int64_t nvox, Head h) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nvox) return;
    const float4 *p = (const float4 *)(in + v * 8);
    const float4 a = p[0], b = p[1];
    float s = h.w[8];
    s = fmaf(a.x, h.w[0], s);
    s = fmaf(a.y, h.w[1], s);
    s = fmaf(a.z, h.w[2], s);
    s = fmaf(a.w, h.w[3], s);
    s = fmaf(b.x, h.w[4], s);
    s = fmaf(b.y, h.w[5], s);
    s = fmaf(b.z, h.w[6], s);
    s = fmaf(b.w, h.w[7], s);
    out[v] = 1.0f / (1.0f + expf(-s));
}

// image_normalize(image, 0.0, 1.0, float32) in numpy 2 promotion: (image - imin) wraps in int16, (imax - imin) wraps in
// int16, the scale 1.0 / d and the product are float64, + 0.0, one rounding to float32.  Constant image -> 0.
__global__ __launch_bounds__(256) void k_normalize(const int16_t *__restrict__ img, int64_t n, const float *__restrict__ mm,
                                                   float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int imin = (int)mm[0], imax = (int)mm[1];
    if (imin == imax) {
        out[i] = 0.0f;
        return;
    }
    const int16_t d = (int16_t)(imax - imin);
    const double scale = 1.0 / (double)d;
    const int16_t v = (int16_t)((int)img[i] - imin);
    out[i] = (float)((double)v * scale + 0.0);
}

struct Cuts {
    int nz, ny, nx; // volume
    int cz, cy, cx; // number of starts per axis
    int P;
};

// patches [p0, p0 + nb) of the cut list (itertools.product(z, y, x) order) -> in[b][P^3], zero outside the volume
__global__ __launch_bounds__(256) void k_gather(const float *__restrict__ vol, const int *__restrict__ starts, Cuts c, int p0,
                                                int nb, float *__restrict__ out) {
    const int64_t P3 = (int64_t)c.P * c.P * c.P;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P3 * nb) return;
    const int b = (int)(i / P3);
    int r = (int)(i - (int64_t)b * P3);
    const int k = p0 + b;
    const int xi = k % c.cx, yi = (k / c.cx) % c.cy, zi = k / (c.cx * c.cy);
    const int z = r / (c.P * c.P) + starts[zi];
    r %= c.P * c.P;
    const int y = r / c.P + starts[c.cz + yi], x = r % c.P + starts[c.cz + c.cy + xi];
    out[i] = (z < c.nz && y < c.ny && x < c.nx) ? vol[((int64_t)z * c.ny + y) * c.nx + x] : 0.0f;
}

// prob[v] += out[k][v - start_k] for every cut k in [p0, p0 + nb) covering v, in cut order (float32, as `+=` does)
// rng: per axis and coordinate, first | last << 16 of the covering start indices
__global__ __launch_bounds__(256) void k_accumulate(float *__restrict__ prob, const int *__restrict__ starts,
                                                    const int *__restrict__ rng, Cuts c, int p0, int nb,
                                                    const float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)c.nz * c.ny * c.nx;
    if (i >= n) return;
    const int x = (int)(i % c.nx), y = (int)((i / c.nx) % c.ny), z = (int)(i / ((int64_t)c.nx * c.ny));
    const int rz = rng[z], ry = rng[c.nz + y], rx = rng[c.nz + c.ny + x];
    const int zlo = rz & 0xffff, zhi = rz >> 16, ylo = ry & 0xffff, yhi = ry >> 16, xlo = rx & 0xffff, xhi = rx >> 16;
    const int kfirst = (zlo * c.cy + ylo) * c.cx + xlo, klast = (zhi * c.cy + yhi) * c.cx + xhi;
    if (klast < p0 || kfirst >= p0 + nb) return;
    const int64_t P = c.P;
    float p = prob[i];
    for (int zi = zlo; zi <= zhi; zi++)
        for (int yi = ylo; yi <= yhi; yi++)
            for (int xi = xlo; xi <= xhi; xi++) {
                const int k = (zi * c.cy + yi) * c.cx + xi;
                if (k < p0 || k >= p0 + nb) continue;
                const int64_t lz = z - starts[zi], ly = y - starts[c.cz + yi], lx = x - starts[c.cz + c.cy + xi];
                p += out[(int64_t)(k - p0) * P * P * P + (lz * P + ly) * P + lx];
            }
    prob[i] = p;
}

// probability_array /= sums: sums is the number of covering cuts, an exact float32 integer
__global__ __launch_bounds__(256) void k_divide(float *__restrict__ prob, const int *__restrict__ rng, Cuts c) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)c.nz * c.ny * c.nx;
    if (i >= n) return;
    const int x = (int)(i % c.nx), y = (int)((i / c.nx) % c.ny), z = (int)(i / ((int64_t)c.nx * c.ny));
    const int rz = rng[z], ry = rng[c.nz + y], rx = rng[c.nz + c.ny + x];
    const int cnt = ((rz >> 16) - (rz & 0xffff) + 1) * ((ry >> 16) - (ry & 0xffff) + 1) * ((rx >> 16) - (rx & 0xffff) + 1);
    prob[i] = prob[i] / (float)cnt;
}

// mask[1+z, 1+y, 1+x] = (p >= thr) * 255 (border = 1) or mask[z, y, x] (border = 0, the dense interior)
__global__ __launch_bounds__(256) void k_threshold(const float *__restrict__ prob, int nz, int ny, int nx, float thr,
                                                   uint8_t *__restrict__ mask, int64_t sz, int64_t sy, int64_t sx, int border) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)nz * ny * nx;
    if (i >= n) return;
    const int64_t x = i % nx, y = (i / nx) % ny, z = i / ((int64_t)nx * ny);
    mask[(z + border) * sz + (y + border) * sy + (x + border) * sx] = prob[i] >= thr ? 255 : 0;
}

// mask[:, 0, 0] = mask[0, :, 0] = mask[0, 0, :] = 2 on the (nz + 1, ny + 1, nx + 1) mask
__global__ __launch_bounds__(256) void k_flag_lines(uint8_t *__restrict__ mask, int nz, int ny, int nx, int64_t sz, int64_t sy,
                                                    int64_t sx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= nz) mask[i * sz] = 2;
    if (i <= ny) mask[i * sy] = 2;
    if (i <= nx) mask[i * sx] = 2;
}

inline unsigned nblk(int64_t n) { return (unsigned)cdiv(n, 256); }

template <int MT, int NT, int KIND> int launch_conv(const ConvArgs &a0, hipStream_t st) {
    ConvArgs a = a0;
    const int ntiles = (int)cdiv(a.cout, 16);
    a.ngroups = (int)cdiv(ntiles, NT);
    a.tiles_per_class = (int)cdiv(a.nvox, 16 * MT);
    const int64_t waves = (int64_t)a.tiles_per_class * a.ngroups * (KIND == 1 ? 8 : 1);
    hipLaunchKernelGGL((k_conv<MT, NT, KIND>), dim3((unsigned)cdiv(waves, 4)), dim3(256), 0, st, a);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

// tile shape per layer: the largest MT x NT that still leaves >= 2048 waves (8 per CU); small layers fall to 1 x 1
void pick_tile(int kind, int64_t nvox, int cout, int *mt, int *nt) {
    const int ntiles = (int)cdiv(cout, 16);
    const int64_t mcount = nvox * (kind == 1 ? 8 : 1);
    auto waves = [&](int m, int n) { return cdiv(mcount, 16 * m) * cdiv(ntiles, n); };
    auto set = [&](int m, int n) { *mt = m, *nt = n; };
    if (ntiles >= 4 && waves(4, 4) >= 2048) return set(4, 4);
    if (ntiles >= 2 && waves(4, 2) >= 2048) return set(4, 2);
    if (ntiles == 1 && waves(8, 1) >= 2048) return set(8, 1);
    if (ntiles >= 2 && waves(2, 2) >= 2048) return set(2, 2);
    if (waves(4, 1) >= 2048) return set(4, 1);
    if (waves(2, 1) >= 2048) return set(2, 1);
    return set(1, 1);
}

// the seven instantiated tile shapes; any other pair is an error
template <int KIND> int launch_tile(int mt, int nt, const ConvArgs &a, hipStream_t st) {
    switch (mt * 10 + nt) {
    case 11: return launch_conv<1, 1, KIND>(a, st);
    case 21: return launch_conv<2, 1, KIND>(a, st);
    case 41: return launch_conv<4, 1, KIND>(a, st);
    case 81: return launch_conv<8, 1, KIND>(a, st);
    case 22: return launch_conv<2, 2, KIND>(a, st);
    case 42: return launch_conv<4, 2, KIND>(a, st);
    case 44: return launch_conv<4, 4, KIND>(a, st);
    }
    ivx::set_error("unet3d: no conv kernel of tile shape %d x %d", mt, nt);
    return IVX_EINVAL;
}

template <int KIND> int run_conv(const ConvArgs &a, hipStream_t st) {
    int mt, nt;
    pick_tile(KIND, a.nvox, a.cout, &mt, &nt);
    return launch_tile<KIND>(mt, nt, a, st);
}

ConvArgs conv_args(const Layer &L, const float *s0, int c0, const float *s1, int c1, float *dst, int S, int nb, int relu) {
    ConvArgs a{};
    a.src0 = s0;
    a.src1 = s1;
    a.c0 = c0;
    a.c1 = c1;
    a.cinpad = L.cinpad;
    a.w = L.w;
    a.b = L.b;
    a.dst = dst;
    a.cout = L.cout;
    a.coutpad = L.coutpad;
    a.S = S;
    a.nvox = nb * S * S * S;
    a.relu = relu;
    return a;
}

int conv(const Layer &L, const float *s0, int c0, const float *s1, int c1, float *dst, int S, int nb, hipStream_t st) {
    const ConvArgs a = conv_args(L, s0, c0, s1, c1, dst, S, nb, L.kind == 0);
    return L.kind == 0 ? run_conv<0>(a, st) : run_conv<1>(a, st);
}

int pool(const float *in, float *out, int S, int C, int nb, hipStream_t st) {
    const int64_t total = (int64_t)nb * (S / 2) * (S / 2) * (S / 2) * C;
    hipLaunchKernelGGL(k_pool, dim3(nblk(total)), dim3(256), 0, st, in, out, S, C, total);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

int head(const float *w9, const float *in, float *out, int64_t nvox, hipStream_t st) {
    Head h;
    memcpy(h.w, w9, sizeof h.w);
    hipLaunchKernelGGL(k_head, dim3(nblk(nvox)), dim3(256), 0, st, in, out, nvox, h);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

// activation floats per patch: two ping-pong buffers of 8 P^3 + the four skips
int64_t act_floats(int P) {
    const int64_t P3 = (int64_t)P * P * P;
    int64_t s = 16 * P3;
    for (int l = 0; l < NLEV; l++) s += FEAT[l] * (P3 >> (3 * l));
    return s;
}

struct Timing { // optional per-launch HIP events (ivx_unet3d_layer_times)
    hipEvent_t *ev;
    int k;
};

int rec(Timing *tm, hipStream_t st) {
    if (tm) IVX_HIP(hipEventRecord(tm->ev[tm->k++], st));
    return IVX_OK;
}

// forward of nb patches (in: nb x P^3, out: nb x P^3); ws holds act_floats(P) * nb floats
int forward_batch(const Net &N, const float *in, float *out, int nb, int P, float *ws, hipStream_t st, Timing *tm) {
    const int64_t P3 = (int64_t)P * P * P;
    float *X = ws, *Y = ws + 8 * P3 * nb;
    float *skip[NLEV];
    float *p = ws + 16 * P3 * nb;
    for (int l = 0; l < NLEV; l++) {
        skip[l] = p;
        p += (int64_t)FEAT[l] * (P3 >> (3 * l)) * nb;
    }
    int rc;
    // encoder: conv1 -> X, conv2 -> skip[l], pool -> X
    const float *cur = in;
    int ccur = 1;
    for (int l = 0; l < NLEV; l++) {
        const int S = P >> l;
        if ((rc = conv(N.enc[l][0], cur, ccur, nullptr, 0, Y, S, nb, st)) || (rc = rec(tm, st))) return rc;
        if ((rc = conv(N.enc[l][1], Y, FEAT[l], nullptr, 0, skip[l], S, nb, st)) || (rc = rec(tm, st))) return rc;
        if ((rc = pool(skip[l], X, S, FEAT[l], nb, st)) || (rc = rec(tm, st))) return rc;
        cur = X;
        ccur = FEAT[l];
    }
    const int SB = P >> NLEV;
    if ((rc = conv(N.enc[4][0], X, FEAT[3], nullptr, 0, Y, SB, nb, st)) || (rc = rec(tm, st))) return rc;
    if ((rc = conv(N.enc[4][1], Y, FEAT[4], nullptr, 0, X, SB, nb, st)) || (rc = rec(tm, st))) return rc;
    float *d = X, *o = Y;
    for (int l = NLEV - 1; l >= 0; l--) {
        const int S = P >> l;
        if ((rc = conv(N.up[l], d, FEAT[l + 1], nullptr, 0, o, S / 2, nb, st)) || (rc = rec(tm, st))) return rc;
        // torch.cat((upconv, enc), 1): upsampled channels first
        if ((rc = conv(N.dec[l][0], o, FEAT[l], skip[l], FEAT[l], d, S, nb, st)) || (rc = rec(tm, st))) return rc;
        if ((rc = conv(N.dec[l][1], d, FEAT[l], nullptr, 0, o, S, nb, st)) || (rc = rec(tm, st))) return rc;
        std::swap(d, o);
    }
    if ((rc = head(N.head, d, out, P3 * nb, st))) return rc;
    return rec(tm, st);
}

// gen_patches' starts along one axis (segment.py:78-97)
void axis_starts(int n, int P, int ov, std::vector<int> &s) {
    s.clear();
    const int step = P - ov;
    for (int i = 0; i < n; i += step)
        if (i + P <= n) s.push_back(i);
    if (s.empty())
        s.push_back(0);
    else if (s.back() + P < n)
        s.push_back(n - P);
}

int check_patch(int P) {
    IVX_REQUIRE(P >= 16 && P % 16 == 0 && P <= 512, IVX_EDOM, "unet3d: patch size %d is not a positive multiple of 16 (<= 512)", P);
    return IVX_OK;
}

void free_layer(Layer &L) {
    if (L.w) (void)hipFree(L.w);
    if (L.b) (void)hipFree(L.b);
    L.w = L.b = nullptr;
}

// one layer's host parameters in torch layout (w, then b) -> the device layouts of `Layer`
int pack_layer(Layer &L, const float *p, const float *bias, int cin, int cout, int kind) {
    L.cin = cin;
    L.cinpad = (int)cdiv(cin, 4) * 4;
    L.cout = cout;
    L.coutpad = (int)cdiv(cout, 16) * 16;
    L.kind = kind;
    const int taps = kind == 0 ? 125 : 64;
    std::vector<float> w((size_t)taps * L.cinpad * L.coutpad, 0.f), b(L.coutpad, 0.f);
    if (kind == 0) { // torch (cout, cin, 5, 5, 5) -> [tap][cin][cout]
        for (int co = 0; co < cout; co++)
            for (int c = 0; c < cin; c++)
                for (int t = 0; t < 125; t++) w[((size_t)t * L.cinpad + c) * L.coutpad + co] = p[((size_t)co * cin + c) * 125 + t];
    } else { // torch (cin, cout, 4, 4, 4) -> [class][tap][cin][cout]; kernel index k = (1 - p) + 2 b per axis
        for (int c = 0; c < cin; c++)
            for (int co = 0; co < cout; co++)
                for (int cls = 0; cls < 8; cls++)
                    for (int tap = 0; tap < 8; tap++) {
                        const int kz = (1 - ((cls >> 2) & 1)) + 2 * ((tap >> 2) & 1);
                        const int ky = (1 - ((cls >> 1) & 1)) + 2 * ((tap >> 1) & 1);
                        const int kx = (1 - (cls & 1)) + 2 * (tap & 1);
                        w[(((size_t)cls * 8 + tap) * L.cinpad + c) * L.coutpad + co] =
                            p[((size_t)c * cout + co) * 64 + (kz * 4 + ky) * 4 + kx];
                    }
    }
    for (int co = 0; co < cout; co++) b[co] = bias[co];
    IVX_HIP(hipMalloc(&L.w, w.size() * 4));
    IVX_HIP(hipMalloc(&L.b, b.size() * 4));
    IVX_HIP(hipMemcpy(L.w, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    IVX_HIP(hipMemcpy(L.b, b.data(), b.size() * 4, hipMemcpyHostToDevice));
    return IVX_OK;
}

} // namespace

/* ---------------------------------------------------------------------------------------------- C ABI */

extern "C" int ivx_unet3d_param_count(int64_t *nfloats) {
    IVX_REQUIRE(nfloats, IVX_EINVAL, "unet3d: null argument");
    int64_t s = 0;
    auto conv5 = [&](int ci, int co) { s += (int64_t)co * ci * 125 + co; };
    int ci = 1;
    for (int l = 0; l < 5; l++) {
        conv5(ci, FEAT[l]);
        conv5(FEAT[l], FEAT[l]);
        ci = FEAT[l];
    }
    for (int l = NLEV - 1; l >= 0; l--) {
        s += (int64_t)FEAT[l + 1] * FEAT[l] * 64 + FEAT[l];
        conv5(2 * FEAT[l], FEAT[l]);
        conv5(FEAT[l], FEAT[l]);
    }
    s += 9;
    *nfloats = s;
    return IVX_OK;
}

extern "C" int ivx_unet3d_free(void *net) {
    Net *N = (Net *)net;
    if (!N) return IVX_OK;
    for (auto &e : N->enc) free_layer(e[0]), free_layer(e[1]);
    for (auto &u : N->up) free_layer(u);
    for (auto &e : N->dec) free_layer(e[0]), free_layer(e[1]);
    delete N;
    return IVX_OK;
}

extern "C" int ivx_unet3d_load(const float *blob, int64_t nfloats, void **net_out) {
    IVX_REQUIRE(blob && net_out, IVX_EINVAL, "unet3d: null argument");
    int64_t want = 0;
    ivx_unet3d_param_count(&want);
    IVX_REQUIRE(nfloats == want, IVX_EINVAL, "unet3d: parameter blob has %lld floats, the network needs %lld",
                (long long)nfloats, (long long)want);
    Net *N = new Net();
    const float *p = blob;
    int rc = IVX_OK;
    auto put = [&](Layer &L, int cin, int cout, int kind) -> int {
        const float *w = p;
        p += (size_t)cout * cin * (kind == 0 ? 125 : 64) + cout;
        return pack_layer(L, w, p - cout, cin, cout, kind);
    };
    int ci = 1;
    for (int l = 0; l < 5 && !rc; l++) {
        if (!(rc = put(N->enc[l][0], ci, FEAT[l], 0))) rc = put(N->enc[l][1], FEAT[l], FEAT[l], 0);
        ci = FEAT[l];
    }
    for (int l = NLEV - 1; l >= 0 && !rc; l--) {
        if (!(rc = put(N->up[l], FEAT[l + 1], FEAT[l], 1)) && !(rc = put(N->dec[l][0], 2 * FEAT[l], FEAT[l], 0)))
            rc = put(N->dec[l][1], FEAT[l], FEAT[l], 0);
    }
    if (rc) {
        ivx_unet3d_free(N);
        return rc;
    }
    memcpy(N->head, p, 9 * sizeof(float));
    *net_out = N;
    return IVX_OK;
}

extern "C" int ivx_unet3d_workspace_bytes(const void *net, int patch, int batch, size_t *nbytes) {
    IVX_REQUIRE(net && nbytes, IVX_EINVAL, "unet3d: null argument");
    int rc;
    if ((rc = check_patch(patch))) return rc;
    IVX_REQUIRE(batch >= 1, IVX_EDOM, "unet3d: batch must be >= 1");
    const int64_t P3 = (int64_t)patch * patch * patch;
    *nbytes = (size_t)((act_floats(patch) + 2 * P3) * batch + TABLE_INTS) * 4;
    return IVX_OK;
}

static int forward_all(const void *net, const float *in, int64_t n, int patch, float *out, void *workspace, size_t ws_bytes,
                       void *stream, Timing *tm) {
    IVX_REQUIRE(net && in && out && workspace, IVX_EINVAL, "unet3d: null argument");
    int rc;
    if ((rc = check_patch(patch))) return rc;
    const int64_t per = act_floats(patch) * 4;
    const int64_t P3 = (int64_t)patch * patch * patch;
    const int64_t cap = std::min<int64_t>((int64_t)ws_bytes / per, INT32_MAX / (8 * P3)); // voxel * channel indices fit int
    IVX_REQUIRE(cap >= 1, IVX_EDOM, "unet3d: workspace of %zu bytes holds no %d^3 patch (%lld bytes each)", ws_bytes, patch,
                (long long)per);
    for (int64_t i = 0; i < n; i += cap) {
        const int nb = (int)std::min<int64_t>(cap, n - i);
        if ((rc = forward_batch(*(const Net *)net, in + i * P3, out + i * P3, nb, patch, (float *)workspace, S(stream), tm)))
            return rc;
    }
    return IVX_OK;
}

extern "C" int ivx_dev_unet3d_forward(const void *net, const float *in, int64_t n, int patch, float *out, void *workspace,
                                      size_t ws_bytes, void *stream) {
    return forward_all(net, in, n, patch, out, workspace, ws_bytes, stream, nullptr);
}

extern "C" int ivx_unet3d_layer_times(const void *net, const float *in, int64_t n, int patch, float *out, void *workspace,
                                      size_t ws_bytes, void *stream, float *ms) {
    IVX_REQUIRE(ms, IVX_EINVAL, "unet3d: null argument");
    const int64_t cap = (int64_t)ws_bytes / (act_floats(patch) * 4);
    IVX_REQUIRE(cap >= n, IVX_EDOM, "unet3d: layer times need the whole batch in one workspace");
    hipEvent_t ev[NLAYERS + 1];
    for (auto &e : ev) IVX_HIP(hipEventCreate(&e));
    Timing tm{ev + 1, 0};
    int rc = IVX_OK;
    if (hipEventRecord(ev[0], S(stream)) != hipSuccess) rc = IVX_EHIP;
    if (!rc) rc = forward_all(net, in, n, patch, out, workspace, ws_bytes, stream, &tm);
    if (!rc && hipEventSynchronize(ev[NLAYERS]) != hipSuccess) rc = IVX_EHIP;
    for (int i = 0; i < NLAYERS && !rc; i++)
        if (hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]) != hipSuccess) rc = IVX_EHIP;
    for (auto &e : ev) (void)hipEventDestroy(e);
    if (rc == IVX_EHIP) ivx::set_error("unet3d: event timing failed");
    return rc;
}

extern "C" int ivx_dev_unet3d_normalize(const int16_t *img, int64_t n, float *out, float *minmax2, void *stream) {
    IVX_REQUIRE(img && out && minmax2, IVX_EINVAL, "unet3d: null argument");
    if (n <= 0) return IVX_OK;
    int rc;
    if ((rc = ivx_dev_minmax_f32(IVX_I16, img, n, minmax2, stream))) return rc;
    hipLaunchKernelGGL(k_normalize, dim3(nblk(n)), dim3(256), 0, S(stream), img, n, (const float *)minmax2, out);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_segment_cut_count(const int64_t shape[3], int patch, int overlap, int64_t *ncuts) {
    IVX_REQUIRE(shape && ncuts, IVX_EINVAL, "unet3d: null argument");
    int rc;
    if ((rc = check_patch(patch))) return rc;
    IVX_REQUIRE(overlap >= 0 && overlap < 100, IVX_EDOM, "unet3d: overlap %d outside [0, 100)", overlap);
    const int ov = (int)((int64_t)patch * overlap / 100);
    int64_t c = 1;
    std::vector<int> s;
    for (int a = 0; a < 3; a++) {
        IVX_REQUIRE(shape[a] >= 1 && shape[a] <= MAX_CUT_AXIS, IVX_EDOM, "unet3d: axis of %lld voxels", (long long)shape[a]);
        axis_starts((int)shape[a], patch, ov, s);
        c *= (int64_t)s.size();
    }
    *ncuts = c;
    return IVX_OK;
}

extern "C" int ivx_dev_unet3d_segment(const void *net, const float *vol, const int64_t shape[3], int patch, int overlap,
                                      int batch, float *prob, void *workspace, size_t ws_bytes, float *progress,
                                      void *stream) {
    IVX_REQUIRE(net && vol && shape && prob && workspace, IVX_EINVAL, "unet3d: null argument");
    int64_t ncuts = 0;
    int rc;
    if ((rc = ivx_segment_cut_count(shape, patch, overlap, &ncuts))) return rc;
    size_t need = 0;
    if ((rc = ivx_unet3d_workspace_bytes(net, patch, batch, &need))) return rc;
    IVX_REQUIRE(ws_bytes >= need, IVX_EDOM, "unet3d: workspace of %zu bytes, the batch needs %zu", ws_bytes, need);
    const int ov = (int)((int64_t)patch * overlap / 100);
    std::vector<int> sa[3];
    for (int a = 0; a < 3; a++) axis_starts((int)shape[a], patch, ov, sa[a]);
    const int nz = (int)shape[0], ny = (int)shape[1], nx = (int)shape[2];
    // host tables: starts of the three axes, then per axis and coordinate the first | last covering start index
    std::vector<int> tab;
    for (int a = 0; a < 3; a++) tab.insert(tab.end(), sa[a].begin(), sa[a].end());
    const size_t rng_off = tab.size();
    for (int a = 0; a < 3; a++) {
        const int n = (int)shape[a];
        for (int v = 0; v < n; v++) {
            int lo = -1, hi = -1;
            for (int k = 0; k < (int)sa[a].size(); k++)
                if (sa[a][k] <= v && v < sa[a][k] + patch) {
                    if (lo < 0) lo = k;
                    hi = k;
                }
            tab.push_back(lo | (hi << 16));
        }
    }
    IVX_REQUIRE((int64_t)tab.size() <= TABLE_INTS, IVX_EDOM, "unet3d: volume too large for the cut tables");
    const int64_t P3 = (int64_t)patch * patch * patch;
    float *ws = (float *)workspace;
    float *act = ws, *pin = act + act_floats(patch) * batch, *pout = pin + P3 * batch;
    int *dtab = (int *)(pout + P3 * batch);
    hipStream_t st = S(stream);
    IVX_HIP(hipMemcpyAsync(dtab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
    IVX_HIP(hipStreamSynchronize(st)); // `tab` is pageable and goes out of scope
    Cuts c{nz, ny, nx, (int)sa[0].size(), (int)sa[1].size(), (int)sa[2].size(), patch};
    const int64_t nvol = (int64_t)nz * ny * nx;
    for (int64_t p0 = 0; p0 < ncuts; p0 += batch) {
        const int nb = (int)std::min<int64_t>(batch, ncuts - p0);
        hipLaunchKernelGGL(k_gather, dim3(nblk(P3 * nb)), dim3(256), 0, st, vol, (const int *)dtab, c, (int)p0, nb, pin);
        IVX_LAUNCH_CHECK();
        if ((rc = forward_batch(*(const Net *)net, pin, pout, nb, patch, act, st, nullptr))) return rc;
        hipLaunchKernelGGL(k_accumulate, dim3(nblk(nvol)), dim3(256), 0, st, prob, (const int *)dtab,
                           (const int *)(dtab + rng_off), c, (int)p0, nb, (const float *)pout);
        IVX_LAUNCH_CHECK();
        if (progress) {
            IVX_HIP(hipStreamSynchronize(st));
            *progress = (float)((double)(p0 + nb) / (double)ncuts);
        }
    }
    hipLaunchKernelGGL(k_divide, dim3(nblk(nvol)), dim3(256), 0, st, prob, (const int *)(dtab + rng_off), c);
    IVX_LAUNCH_CHECK();
    return IVX_OK;
}

extern "C" int ivx_dev_segment_threshold(const float *prob, const int64_t shape[3], float threshold, uint8_t *mask,
                                         const int64_t mstrides[3], int border, void *stream) {
    IVX_REQUIRE(prob && shape && mask && mstrides, IVX_EINVAL, "segment threshold: null argument");
    const int64_t n = shape[0] * shape[1] * shape[2];
    if (n > 0) {
        hipLaunchKernelGGL(k_threshold, dim3(nblk(n)), dim3(256), 0, S(stream), prob, (int)shape[0], (int)shape[1],
                           (int)shape[2], threshold, mask, mstrides[0], mstrides[1], mstrides[2], border ? 1 : 0);
        IVX_LAUNCH_CHECK();
    }
    if (border) {
        const int64_t m = std::max(shape[0], std::max(shape[1], shape[2])) + 1;
        hipLaunchKernelGGL(k_flag_lines, dim3(nblk(m)), dim3(256), 0, S(stream), mask, (int)shape[0], (int)shape[1],
                           (int)shape[2], mstrides[0], mstrides[1], mstrides[2]);
        IVX_LAUNCH_CHECK();
    }
    return IVX_OK;
}

// SegmentProcess._run_segmentation + segment_torch in one call: int16 image (any strides) -> [get_LUT_value] ->
// image_normalize -> cuts, batched forward, in-order accumulate onto `prob` (dense float32, read and written), divide
extern "C" int ivx_segment_unet3d(const void *net, const int16_t *img, const int64_t shape[3], const int64_t strides[3],
                                  int apply_wwwl, double window, double level, int patch, int overlap, int batch, float *prob,
                                  float *progress) {
    HostCallGuard guard;
    IVX_REQUIRE(net && img && shape && strides && prob, IVX_EINVAL, "segment: null argument");
    int64_t ncuts = 0;
    int rc;
    if ((rc = ivx_segment_cut_count(shape, patch, overlap, &ncuts))) return rc;
    size_t wsb = 0;
    if ((rc = ivx_unet3d_workspace_bytes(net, patch, batch, &wsb))) return rc;
    const int64_t n = shape[0] * shape[1] * shape[2];
    void *d_img = nullptr, *d_lut = nullptr, *d_norm = nullptr, *d_prob = nullptr, *d_ws = nullptr, *d_mm = nullptr;
    if ((rc = ws_get(WS_IN, (size_t)n * 2, &d_img)) || (rc = ws_get(WS_AUX0, (size_t)n * 2, &d_lut)) ||
        (rc = ws_get(WS_AUX1, (size_t)n * 4, &d_norm)) || (rc = ws_get(WS_OUT, (size_t)n * 4, &d_prob)) ||
        (rc = ws_get(WS_AUX2, wsb, &d_ws)) || (rc = ws_get(WS_SMALL, 64, &d_mm)))
        return rc;
    if ((rc = upload_strided(d_img, img, shape, strides, 2, WS_IN))) return rc;
    const int16_t *src = (const int16_t *)d_img;
    if (apply_wwwl) { // get_LUT_value: np.piecewise keeps int16
        if ((rc = ivx_dev_lut_i16(src, n, window, level, 0, (int16_t *)d_lut, nullptr))) return rc;
        src = (const int16_t *)d_lut;
    }
    if ((rc = ivx_dev_unet3d_normalize(src, n, (float *)d_norm, (float *)d_mm, nullptr))) return rc;
    if ((rc = copy_h2d(d_prob, prob, (size_t)n * 4))) return rc;
    if ((rc = ivx_dev_unet3d_segment(net, (const float *)d_norm, shape, patch, overlap, batch, (float *)d_prob, d_ws, wsb,
                                     progress, nullptr)))
        return rc;
    IVX_HIP(hipDeviceSynchronize());
    return copy_d2h(prob, d_prob, (size_t)n * 4);
}

/* ------------------------------------------------------------------- diagnostic: one layer at a time (tests) */

// one conv (kind 0) or transposed conv (kind 1) through pack_layer and k_conv; (mt, nt) forces the tile shape,
// (0, 0) leaves it to pick_tile.  Every refusal comes before the first device call.
extern "C" int ivx_dev_unet3d_conv_layer(int kind, const float *src0, int c0, const float *src1, int c1, const float *w,
                                         const float *bias, int cout, int S, int nb, int relu, int mt, int nt, float *dst,
                                         int *mt_used, int *nt_used, void *stream) {
    IVX_REQUIRE(src0 && w && bias && dst && mt_used && nt_used, IVX_EINVAL, "unet3d layer: null argument");
    IVX_REQUIRE(kind == 0 || kind == 1, IVX_EINVAL, "unet3d layer: kind %d is neither 0 (conv) nor 1 (transposed conv)", kind);
    IVX_REQUIRE(c0 >= 1 && c1 >= 0 && (c1 > 0) == (src1 != nullptr), IVX_EINVAL,
                "unet3d layer: %d + %d input channels do not match the sources given", c0, c1);
    IVX_REQUIRE(c1 == 0 || c0 % 4 == 0, IVX_EINVAL,
                "unet3d layer: with a second source the first must have a multiple of 4 channels, got %d", c0);
    IVX_REQUIRE(cout >= 1 && S >= 1 && nb >= 1, IVX_EINVAL, "unet3d layer: cout %d, edge %d, %d patches", cout, S, nb);
    const int cin = c0 + c1;
    const int64_t nvox = (int64_t)nb * S * S * S;
    IVX_REQUIRE(nvox * (kind == 1 ? 8 : 1) * std::max(cin, cout) <= INT32_MAX, IVX_EDOM,
                "unet3d layer: voxel * channel indices must fit int");
    if (mt || nt) {
        const int shape = mt * 10 + nt;
        IVX_REQUIRE(mt >= 1 && nt >= 1 && nt <= 4 && (shape == 11 || shape == 21 || shape == 41 || shape == 81 || shape == 22 ||
                                                     shape == 42 || shape == 44),
                    IVX_EINVAL, "unet3d layer: no conv kernel of tile shape %d x %d", mt, nt);
        // what pick_tile can choose: NT columns need NT column tiles, 8 x 1 is for a single column tile
        IVX_REQUIRE((nt == 1 || cout > 16 * (nt - 1)) && (mt != 8 || cout <= 16), IVX_EINVAL,
                    "unet3d layer: tile shape %d x %d is never used for %d output channels", mt, nt, cout);
    } else {
        pick_tile(kind, nvox, cout, &mt, &nt);
    }
    hipStream_t st = (hipStream_t)stream;
    Layer L{};
    int rc = pack_layer(L, w, bias, cin, cout, kind);
    if (!rc) {
        const ConvArgs a = conv_args(L, src0, c0, src1, c1, dst, S, nb, relu ? 1 : 0);
        rc = kind == 0 ? launch_tile<0>(mt, nt, a, st) : launch_tile<1>(mt, nt, a, st);
    }
    if (!rc && hipStreamSynchronize(st) != hipSuccess) { // the weights are freed below
        ivx::set_error("unet3d layer: the kernel failed");
        rc = IVX_EHIP;
    }
    free_layer(L);
    if (!rc) *mt_used = mt, *nt_used = nt;
    return rc;
}

extern "C" int ivx_dev_unet3d_pool_layer(const float *in, float *out, int S, int C, int nb, void *stream) {
    IVX_REQUIRE(in && out, IVX_EINVAL, "unet3d layer: null argument");
    IVX_REQUIRE(S >= 2 && S % 2 == 0 && C >= 1 && nb >= 1, IVX_EINVAL, "unet3d layer: pool of edge %d, %d channels, %d patches",
                S, C, nb);
    return pool(in, out, S, C, nb, (hipStream_t)stream);
}

extern "C" int ivx_dev_unet3d_head_layer(const float *in, const float *w9, int64_t nvox, float *out, void *stream) {
    IVX_REQUIRE(in && w9 && out, IVX_EINVAL, "unet3d layer: null argument");
    IVX_REQUIRE(nvox >= 1, IVX_EINVAL, "unet3d layer: head over %lld voxels", (long long)nvox);
    return head(w9, in, out, nvox, (hipStream_t)stream);
}
