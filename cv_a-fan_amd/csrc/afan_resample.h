// Pillow's separable 8-bit bilinear resampler as device code, shared by the loaders' batch kernels (afan_seg_data.hip: the
// segmentation batch; afan_det_data.hip: the detection batch): the coefficients of one output coordinate, the per-tile tables in
// LDS, and the sampling of one output pixel (the horizontal pass, rounded to uint8, then the vertical pass).
//   * triangle filter of support max(in/out, 1) around (x + 0.5) * in/out, double coefficients summed left to right and normalised,
//     int(+-0.5 + k * 2^22), accumulator 2^21, >> 22, clip; a pass whose size does not change is the identity (one tap of 2^22).
//   * ToTensor on the CPU: the correctly rounded quotient fl(v / 255) (not afan_data.hip's device product).
// seg_data._resize_bilinear restates it in numpy; tests/golden/seg_aug_pillow.npz and det_data_pillow.npz hold Pillow's own output.
#pragma once
#include "afan_common.h"

#include <limits.h>

// the coefficient and coordinate arithmetic below must round operation by operation: 0.5 + k * 2^22 as an fma rounds differently
#pragma clang fp contract(off)

// The tile is the including kernel file's choice: it defines, in the unnamed namespace and before this header, BLOCK (threads per
// workgroup), TW and TH (one workgroup = TH output rows x TW output columns of one sample).
namespace {
static_assert(BLOCK == 256 && TW % 4 == 0 && TW >= 4 && TH >= 1, "the tile of the including file (256 threads fill the 256-entry /255 table)");
constexpr int KMAX = 8;              // taps per axis: ceil(in/out) * 2 + 1 <= 7 for in/out <= 3
constexpr int PREC = 22;             // Pillow's PRECISION_BITS (32 - 8 - 2)
constexpr int MAX_SIDE = 1 << 15;    // a resized side is clamped to this (the reference's largest is 2 x 500)
constexpr double MAX_SHRINK = 3.0;

// ToTensor's scaling as the CPU computes it, torch.from_numpy(u8).float().div(255): a true fp32 division, correctly rounded.
struct Quot255 {
    float v[256];
    constexpr Quot255() : v() {
        for (int i = 0; i < 256; ++i) v[i] = (float)i / 255.0f;
    }
};
__constant__ Quot255 kQuot255 = Quot255();

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> PREC;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for ONE output coordinate x of a resize in -> out (bilinear: support 1).
__device__ void bilinear_taps(int x, int in, int out, int& xmin_o, int& n_o, int (&coef)[KMAX]) {
#pragma unroll
    for (int u = 0; u < KMAX; ++u) coef[u] = 0;
    if (in == out) {                       // the pass is skipped: identity
        xmin_o = x;
        n_o = 1;
        coef[0] = 1 << PREC;
        return;
    }
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    const double center = (x + 0.5) * scale;
    const double ss = 1.0 / fs;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    int n = xmax - xmin;
    n = n < 0 ? 0 : (n > KMAX ? KMAX : n);
    double k[KMAX];
    double ww = 0.0;
#pragma unroll
    for (int u = 0; u < KMAX; ++u) {
        double w = 0.0;
        if (u < n) {
            double t = ((u + xmin) - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            w = t < 1.0 ? 1.0 - t : 0.0;
            ww += w;
        }
        k[u] = w;
    }
#pragma unroll
    for (int u = 0; u < KMAX; ++u) {
        if (u < n) {
            double v = k[u];
            if (ww != 0.0) v /= ww;
            coef[u] = v < 0.0 ? (int)(-0.5 + v * (double)(1 << PREC)) : (int)(0.5 + v * (double)(1 << PREC));
        }
    }
    xmin_o = xmin;
    n_o = n;
}

// One workgroup = one TH x TW tile of ONE sample's output.  Its tables live in LDS: per tile column the horizontal taps (first
// source column, count, KMAX coefficients) and the nearest source column; per tile row the same vertically.  A count of -1 marks a
// row / column of the padding.  (The nearest tables are the segmentation labels'; a kernel without labels leaves them unwritten.)
struct Tables {
    int cmin[TW], cn[TW], ccoef[KMAX][TW], ncol[TW];
    int rmin[TH], rn[TH], rcoef[KMAX][TH], nrow[TH];
};

// the resized image's uint8 pixel behind tile position (ti, tj); false (and 0, 0, 0) in the padding
__device__ __forceinline__ bool sample_rgb(const Tables& s, const uint8_t* __restrict__ img, int w, int ti, int tj, int (&c)[3]) {
    const int rn = s.rn[ti], rmin = s.rmin[ti];
    const int cn = s.cn[tj], cmin = s.cmin[tj];
    if (rn < 0 || cn < 0) {
        c[0] = c[1] = c[2] = 0;
        return false;
    }
    int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
    for (int vv = 0; vv < rn; ++vv) {
        const uint8_t* __restrict__ sp = img + ((int64_t)(rmin + vv) * w + cmin) * 3;
        int h0 = 1 << (PREC - 1), h1 = h0, h2 = h0;
        for (int u = 0; u < cn; ++u) {
            const int cc = s.ccoef[u][tj];
            h0 += (int)sp[3 * u] * cc;
            h1 += (int)sp[3 * u + 1] * cc;
            h2 += (int)sp[3 * u + 2] * cc;
        }
        const int cv = s.rcoef[vv][ti];
        a0 += clip8(h0) * cv;                                     // the horizontal pass is rounded to uint8 before the vertical one
        a1 += clip8(h1) * cv;
        a2 += clip8(h2) * cv;
    }
    c[0] = clip8(a0);
    c[1] = clip8(a1);
    c[2] = clip8(a2);
    return true;
}
}  // namespace
