// The segmentation training batch in one launch (gfx950): gather from a resident, variably sized uint8 split + Pillow's bilinear
// (image) and nearest (label) resize + pad_if_needed + crop + horizontal flip + /255.
// Reference behaviour: Segmentation/args.py:113-121 (ExtRandomScale((0.5, 2.0)), ExtRandomCrop(513, pad_if_needed=True),
// ExtRandomHorizontalFlip, ExtToTensor) applied per image by two DataLoader workers on PIL images; the validation transforms
// (:123-136: ExtResize + ExtCenterCrop, or the image as it is) are the same function with other parameters.  The draws are the
// caller's (seg_data.SegDeviceLoader); the kernel is a pure function of them.
//
// What is reproduced bit for bit (seg_data._augment_numpy restates it; tests/golden/seg_aug_pillow.npz holds Pillow's own output):
//   * bilinear: Pillow's separable 8-bit resampler — triangle filter of support max(in/out, 1) around (x + 0.5) * in/out, double
//     coefficients summed left to right and normalised, int(+-0.5 + k * 2^22), accumulator 2^21, >> 22, clip; the HORIZONTAL pass
//     first, ROUNDED TO uint8, then the vertical pass.  A pass whose size does not change is the identity (one tap of 2^22).
//   * nearest: Pillow's ACCUMULATED source coordinate, xo = a/2; tab[x] = int(xo); xo += a — a serial double sum, not
//     int((x + 0.5) * a), which lands on other pixels.
//   * pad_if_needed (ext_transforms.py:383-390): width short -> ALL FOUR sides by p1, then the padded height short -> all four
//     again by p2; fill 0 for the image and for the label.
//   * ToTensor on the CPU: the correctly rounded quotient fl(v / 255) (not afan_data.hip's device product).
#include "afan_common.h"

namespace {
constexpr int BLOCK = 256;
constexpr int TW = 128;              // tile: TH output rows x TW output columns per workgroup
constexpr int TH = 16;
}  // namespace
#include "afan_resample.h"   // the bilinear taps, the tile tables and sample_rgb (shared with afan_det_data.hip)

using namespace afan;

// the coefficient and coordinate arithmetic below must round operation by operation: 0.5 + k * 2^22 as an fma rounds differently
#pragma clang fp contract(off)

namespace {

// One workgroup = one TH x TW tile of ONE sample's output.  Its tables (afan_resample.h: Tables) live in LDS.  Waves 0-1 build the
// column taps, wave 2 the row taps and then the rows' nearest table, one lane of wave 3 the columns' nearest table (the serial
// accumulated sums, up to the tile's last coordinate).  A count of -1 marks a row / column of the padding.
// An item is 4 consecutive columns of one output row (VEC, out_w % 4 == 0: 16-byte stores) or one pixel.
// The three kernels below (the batch, the colour-jitter statistics, the batch with colour jitter) share the geometry, the tables and
// the sampling as device functions.

// the sample's parameters, clamped (uniform over the workgroup)
struct Geom {
    int h, w, oh, ow, P, top, left;
    int64_t base;                                                 // the image's first pixel in the packed split
    bool fl, valid;
};

__device__ __forceinline__ Geom sample_geom(int64_t b, const int64_t* __restrict__ img_off, const int32_t* __restrict__ hs,
                                            const int32_t* __restrict__ ws, int64_t n_src, int64_t total_pixels,
                                            const int64_t* __restrict__ index, const int64_t* __restrict__ p_oh,
                                            const int64_t* __restrict__ p_ow, const int64_t* __restrict__ p_top,
                                            const int64_t* __restrict__ p_left, const int64_t* __restrict__ p_flip, int out_h, int out_w,
                                            double max_shrink) {
    Geom g;
    int64_t k = index[b];
    k = k < 0 ? 0 : (k >= n_src ? n_src - 1 : k);
    int h = hs[k], w = ws[k];
    const int64_t off = img_off[k];
    int64_t base = off / 3;
    // never read outside the split, whatever the tables say: an entry that does not fit gives an all-padding sample
    const bool valid = h >= 1 && w >= 1 && h <= MAX_SIDE && w <= MAX_SIDE && off >= 0 && base + (int64_t)h * w <= total_pixels;
    if (!valid) { h = 1; w = 1; base = 0; }
    int lo_h = (int)ceil((double)h / max_shrink), lo_w = (int)ceil((double)w / max_shrink);
    lo_h = lo_h < 1 ? 1 : lo_h;
    lo_w = lo_w < 1 ? 1 : lo_w;
    int64_t v = p_oh[b];
    const int oh = (int)(v < lo_h ? lo_h : (v > MAX_SIDE ? MAX_SIDE : v));
    v = p_ow[b];
    const int ow = (int)(v < lo_w ? lo_w : (v > MAX_SIDE ? MAX_SIDE : v));
    const int p1 = ow < out_w ? (1 + out_w - ow) / 2 : 0;         // ext_transforms.py:383-385
    const int ph1 = oh + 2 * p1;
    const int p2 = ph1 < out_h ? (1 + out_h - ph1) / 2 : 0;       // :388-390, on the already padded height
    const int P = p1 + p2;
    const int ph = oh + 2 * P, pw = ow + 2 * P;                   // (>= out_h, out_w)
    v = p_top[b];
    g.top = (int)(v < 0 ? 0 : (v > ph - out_h ? ph - out_h : v));
    v = p_left[b];
    g.left = (int)(v < 0 ? 0 : (v > pw - out_w ? pw - out_w : v));
    g.fl = p_flip[b] != 0;
    g.h = h; g.w = w; g.oh = oh; g.ow = ow; g.P = P; g.base = base; g.valid = valid;
    return g;
}

// the tile's tables (the caller synchronises the workgroup afterwards); LABELS: the nearest tables too
template <bool LABELS>
__device__ __forceinline__ void build_tables(Tables& s, const Geom& g, int tid, int i0, int j0, int out_h, int out_w) {
    static_assert(BLOCK == 256 && TW + TH <= 192, "thread roles below");
    const int h = g.h, w = g.w, oh = g.oh, ow = g.ow, P = g.P, top = g.top, left = g.left;
    const bool fl = g.fl, valid = g.valid;
    if (tid < TW) {
        const int j = j0 + tid;
        const int jj = fl ? out_w - 1 - j : j;
        const int c = left + jj - P;
        int xmin = 0, n = -1, coef[KMAX];
#pragma unroll
        for (int u = 0; u < KMAX; ++u) coef[u] = 0;
        if (j < out_w && c >= 0 && c < ow && valid) bilinear_taps(c, w, ow, xmin, n, coef);
        s.cmin[tid] = xmin;
        s.cn[tid] = n;
#pragma unroll
        for (int u = 0; u < KMAX; ++u) s.ccoef[u][tid] = coef[u];
    } else if (tid < TW + TH) {
        const int t = tid - TW;
        const int r = top + i0 + t - P;
        int xmin = 0, n = -1, coef[KMAX];
#pragma unroll
        for (int u = 0; u < KMAX; ++u) coef[u] = 0;
        if (i0 + t < out_h && r >= 0 && r < oh && valid) bilinear_taps(r, h, oh, xmin, n, coef);
        s.rmin[t] = xmin;
        s.rn[t] = n;
#pragma unroll
        for (int u = 0; u < KMAX; ++u) s.rcoef[u][t] = coef[u];
    }
    if (LABELS && tid == TW + TH) {                               // (wave 2) rows: Pillow's accumulated nearest coordinate
        for (int t = 0; t < TH; ++t) s.nrow[t] = 0;
        const int r_first = top + i0 - P;                         // tile row t <-> resized row r_first + t
        int r_last = r_first + TH - 1;
        r_last = r_last > oh - 1 ? oh - 1 : r_last;
        const double a = (double)h / (double)oh;
        double xo = a * 0.5;
        for (int r = 0; r <= r_last; ++r) {
            if (r >= r_first) {
                int sr = (int)xo;
                s.nrow[r - r_first] = sr > h - 1 ? h - 1 : sr;
            }
            xo += a;
        }
    }
    if (LABELS && tid == 192) {                                   // (wave 3) columns
        for (int t = 0; t < TW; ++t) s.ncol[t] = 0;
        // tile column t <-> resized column c = left + (fl ? out_w - 1 - (j0 + t) : j0 + t) - P
        const int ca = left + (fl ? out_w - 1 - j0 : j0) - P;     // t = 0
        const int cb = fl ? ca - (TW - 1) : ca + (TW - 1);        // t = TW - 1
        const int c_first = ca < cb ? ca : cb;
        int c_last = ca < cb ? cb : ca;
        c_last = c_last > ow - 1 ? ow - 1 : c_last;
        const double a = (double)w / (double)ow;
        double xo = a * 0.5;
        for (int c = 0; c <= c_last; ++c) {
            if (c >= c_first) {
                int sc = (int)xo;
                s.ncol[fl ? ca - c : c - ca] = sc > w - 1 ? w - 1 : sc;
            }
            xo += a;
        }
    }
}
// the tile's pixels: sample, `op` on the uint8 pixel (the padding's too), / 255, store; the label beside it (padding: 0)
template <bool VEC, class Op>
__device__ __forceinline__ void write_tile(const Tables& s, const float* __restrict__ s_quot, const Geom& g,
                                           const uint8_t* __restrict__ images, const uint8_t* __restrict__ labels, int64_t b,
                                           float* __restrict__ out, int64_t* __restrict__ labels_out, int out_h, int out_w, int tid,
                                           int i0, int j0, Op op) {
    const int w = g.w;
    const uint8_t* __restrict__ img = images + 3 * g.base;
    const uint8_t* __restrict__ lab = labels + g.base;
    const int64_t plane = (int64_t)out_h * out_w;
    float* __restrict__ dst = out + b * 3 * plane;
    int64_t* __restrict__ ldst = labels_out + b * plane;
    constexpr int E = VEC ? 4 : 1;
    constexpr int WQ = TW / E;
    for (int it = tid; it < TH * WQ; it += BLOCK) {
        const int ti = it / WQ;
        const int tq = it - ti * WQ;
        const int i = i0 + ti;
        const int jq = j0 + tq * E;
        if (i >= out_h || jq >= out_w) continue;                  // (VEC: out_w % 4 == 0, so the 4 columns are in or out together)
        float px[3][E];
        int64_t lb[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int tj = tq * E + e;
            int c[3];
            const bool inside = sample_rgb(s, img, w, ti, tj, c);                         // padding: 0 for the image AND the label
            lb[e] = inside ? (int64_t)lab[(int64_t)s.nrow[ti] * w + s.ncol[tj]] : 0;
            op(c);
            px[0][e] = s_quot[c[0]];
            px[1][e] = s_quot[c[1]];
            px[2][e] = s_quot[c[2]];
        }
        const int64_t o = (int64_t)i * out_w + jq;
        if (VEC) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float t4[4] = {px[ch][0], px[ch][E > 1 ? 1 : 0], px[ch][E > 2 ? 2 : 0], px[ch][E > 3 ? 3 : 0]};
                Elt<float>::stv(dst + ch * plane + o, t4);
            }
            typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
            const i64x2 l01 = {lb[0], lb[E > 1 ? 1 : 0]}, l23 = {lb[E > 2 ? 2 : 0], lb[E > 3 ? 3 : 0]};
            *reinterpret_cast<i64x2*>(ldst + o) = l01;
            *reinterpret_cast<i64x2*>(ldst + o + 2) = l23;
        } else {
            dst[o] = px[0][0];
            dst[plane + o] = px[1][0];
            dst[2 * plane + o] = px[2][0];
            ldst[o] = lb[0];
        }
    }
}

struct NoOp {
    __device__ __forceinline__ void operator()(int (&)[3]) const {}
};

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void seg_batch_aug_kernel(
    const uint8_t* __restrict__ images, const int64_t* __restrict__ img_off, const uint8_t* __restrict__ labels,
    const int32_t* __restrict__ hs, const int32_t* __restrict__ ws, int64_t n_src, int64_t total_pixels,
    const int64_t* __restrict__ index, const int64_t* __restrict__ p_oh, const int64_t* __restrict__ p_ow,
    const int64_t* __restrict__ p_top, const int64_t* __restrict__ p_left, const int64_t* __restrict__ p_flip,
    float* __restrict__ out, int64_t* __restrict__ labels_out, int out_h, int out_w, double max_shrink, int tiles_x, int tiles_y) {
    __shared__ Tables s;
    __shared__ float s_quot[256];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x;
    const int ty = (blockIdx.x / tiles_x) % tiles_y;
    const int64_t b = blockIdx.x / (tiles_x * tiles_y);
    const int i0 = ty * TH, j0 = tx * TW;
    const Geom g = sample_geom(b, img_off, hs, ws, n_src, total_pixels, index, p_oh, p_ow, p_top, p_left, p_flip, out_h, out_w, max_shrink);
    s_quot[tid] = kQuot255.v[tid];
    build_tables<true>(s, g, tid, i0, j0, out_h, out_w);
    __syncthreads();
    write_tile<VEC>(s, s_quot, g, images, labels, b, out, labels_out, out_h, out_w, tid, i0, j0, NoOp());
}

// ------------------------------------------------------------------------------------ ExtColorJitter(brightness, contrast, saturation)
// torchvision's PIL functional: ImageEnhance.{Brightness, Contrast, Color}(img).enhance(f) = Image.blend(degenerate, img, f), each on
// the uint8 output of the one before, in one of the six orders.  seg_data._jitter_numpy restates it; tests/golden/
// seg_jitter_pillow.npz holds Pillow's own output.
//   * blend, per channel, in fp32 with the product and the sum rounded SEPARATELY (Pillow's C compiles to a multiply and an add;
//     an fma rounds once and lands on the other side of an integer for some inputs): t = d + f * (i - d); 0 <= f <= 1: (uint8)t,
//     else 0 for t <= 0, 255 for t >= 255, (uint8)t between.
//   * degenerate image d: brightness 0; contrast int(S / n + 0.5) in double, S the INTEGER sum of the gray values of the whole
//     crop as it is when contrast's turn comes (padding included); saturation the pixel's own gray value.
//   * gray = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (Pillow's RGB -> L).
constexpr int OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2;
// order code 0..5 -> the three operations in turn (the permutations of (0, 1, 2) in lexicographic order), 2 bits each
__device__ __forceinline__ int order_ops(int64_t code) {
    const int k = (int)(code < 0 ? 0 : (code > 5 ? 5 : code));
    //            (0,1,2)             (0,2,1)             (1,0,2)             (1,2,0)             (2,0,1)             (2,1,0)
    const int packed[6] = {0 | 1 << 2 | 2 << 4, 0 | 2 << 2 | 1 << 4, 1 | 0 << 2 | 2 << 4, 1 | 2 << 2 | 0 << 4, 2 | 0 << 2 | 1 << 4,
                           2 | 1 << 2 | 0 << 4};
    int r = packed[0];
#pragma unroll
    for (int q = 1; q < 6; ++q) r = k == q ? packed[q] : r;
    return r;
}

__device__ __forceinline__ int gray_l(const int (&c)[3]) {
    return (19595 * c[0] + 38470 * c[1] + 7471 * c[2] + 0x8000) >> 16;
}

__device__ __forceinline__ int blend8(int d, int i, float f, bool inside01) {
    const float t = __fadd_rn((float)d, __fmul_rn(f, (float)(i - d)));      // (i - d is exact in fp32: what float(i) - float(d) gives)
    if (inside01) return (int)t;                                            // between d and i: no clip needed
    return !(t > 0.f) ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ void jitter_op(int op, float f, int mean, int (&c)[3]) {
    const bool in01 = f >= 0.f && f <= 1.f;
    const int d = op == OP_BRIGHTNESS ? 0 : (op == OP_CONTRAST ? mean : gray_l(c));
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch] = blend8(d, c[ch], f, in01);
}

// Launch 1 (after the clear): the gray sum contrast needs, over the crop as it is after the operations that come BEFORE contrast in the sample's
// order (they are pointwise, so they are applied on the fly).  Integer sums only: per workgroup one 64-bit atomic add into
// gray_sum[b] — the total does not depend on the order of the adds.  Padding pixels are 0 and stay 0 under brightness and
// saturation, so they add nothing (they do count in n, which the second launch knows).
__global__ __launch_bounds__(BLOCK) void seg_jitter_stats_kernel(
    const uint8_t* __restrict__ images, const int64_t* __restrict__ img_off, const int32_t* __restrict__ hs,
    const int32_t* __restrict__ ws, int64_t n_src, int64_t total_pixels, const int64_t* __restrict__ index,
    const int64_t* __restrict__ p_oh, const int64_t* __restrict__ p_ow, const int64_t* __restrict__ p_top,
    const int64_t* __restrict__ p_left, const int64_t* __restrict__ p_flip, const int64_t* __restrict__ p_order,
    const float* __restrict__ f_bri, const float* __restrict__ f_sat, unsigned long long* __restrict__ gray_sum, int out_h, int out_w,
    double max_shrink, int tiles_x, int tiles_y) {
    __shared__ Tables s;
    __shared__ unsigned s_red[BLOCK / AFAN_WAVE];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x;
    const int ty = (blockIdx.x / tiles_x) % tiles_y;
    const int64_t b = blockIdx.x / (tiles_x * tiles_y);
    const int i0 = ty * TH, j0 = tx * TW;
    const Geom g = sample_geom(b, img_off, hs, ws, n_src, total_pixels, index, p_oh, p_ow, p_top, p_left, p_flip, out_h, out_w, max_shrink);
    const int ops3 = order_ops(p_order[b]);
    const float fb = f_bri[b], fs = f_sat[b];
    build_tables<false>(s, g, tid, i0, j0, out_h, out_w);
    __syncthreads();
    const uint8_t* __restrict__ img = images + 3 * g.base;
    unsigned acc = 0;                                             // <= 255 * TH * TW / BLOCK per thread
    for (int it = tid; it < TH * TW; it += BLOCK) {
        const int ti = it / TW;
        const int tj = it - ti * TW;
        if (i0 + ti >= out_h || j0 + tj >= out_w) continue;
        int c[3];
        if (!sample_rgb(s, img, g.w, ti, tj, c)) continue;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int op = (ops3 >> (2 * q)) & 3;
            if (op == OP_CONTRAST) break;
            jitter_op(op, op == OP_BRIGHTNESS ? fb : fs, 0, c);
        }
        acc += (unsigned)gray_l(c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((tid & (AFAN_WAVE - 1)) == 0) s_red[tid / AFAN_WAVE] = acc;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int q = 0; q < BLOCK / AFAN_WAVE; ++q) t += s_red[q];
        if (t) atomicAdd(gray_sum + b, t);
    }
}

// Launch 0: the sums start at zero.  A kernel, not hipMemsetAsync: the call is made to be captured into a graph and replayed, and every
// replay must clear the sums again — with a captured memset the second replay gave a wrong batch (tests/test_seg_jitter_gpu.py
// replays twice).
__global__ __launch_bounds__(BLOCK) void seg_jitter_clear_kernel(unsigned long long* __restrict__ gray_sum, int64_t m) {
    const int64_t b = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (b < m) gray_sum[b] = 0ull;
}

struct JitterOp {
    int ops3, mean;
    float f[3];
    __device__ __forceinline__ void operator()(int (&c)[3]) const {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int op = (ops3 >> (2 * q)) & 3;
            jitter_op(op, op == OP_BRIGHTNESS ? f[0] : (op == OP_SATURATION ? f[2] : f[1]), mean, c);
        }
    }
};

// Launch 2: the batch kernel with the three operations between the crop and the flip (the flip is a permutation of the columns
// and the operations are pointwise given the mean, so applying them to the mirrored pixel is the same).
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void seg_batch_aug_jitter_kernel(
    const uint8_t* __restrict__ images, const int64_t* __restrict__ img_off, const uint8_t* __restrict__ labels,
    const int32_t* __restrict__ hs, const int32_t* __restrict__ ws, int64_t n_src, int64_t total_pixels,
    const int64_t* __restrict__ index, const int64_t* __restrict__ p_oh, const int64_t* __restrict__ p_ow,
    const int64_t* __restrict__ p_top, const int64_t* __restrict__ p_left, const int64_t* __restrict__ p_flip,
    const int64_t* __restrict__ p_order, const float* __restrict__ f_bri, const float* __restrict__ f_con,
    const float* __restrict__ f_sat, const unsigned long long* __restrict__ gray_sum, float* __restrict__ out,
    int64_t* __restrict__ labels_out, int out_h, int out_w, double max_shrink, int tiles_x, int tiles_y) {
    __shared__ Tables s;
    __shared__ float s_quot[256];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x;
    const int ty = (blockIdx.x / tiles_x) % tiles_y;
    const int64_t b = blockIdx.x / (tiles_x * tiles_y);
    const int i0 = ty * TH, j0 = tx * TW;
    const Geom g = sample_geom(b, img_off, hs, ws, n_src, total_pixels, index, p_oh, p_ow, p_top, p_left, p_flip, out_h, out_w, max_shrink);
    JitterOp op;
    op.ops3 = order_ops(p_order[b]);
    op.f[0] = f_bri[b];
    op.f[1] = f_con[b];
    op.f[2] = f_sat[b];
    // ImageStat's mean and ImageEnhance.Contrast's int(mean + 0.5), in double from the integer sum
    op.mean = (int)((double)gray_sum[b] / (double)((int64_t)out_h * out_w) + 0.5);
    s_quot[tid] = kQuot255.v[tid];
    build_tables<true>(s, g, tid, i0, j0, out_h, out_w);
    __syncthreads();
    write_tile<VEC>(s, s_quot, g, images, labels, b, out, labels_out, out_h, out_w, tid, i0, j0, op);
}
}  // namespace

extern "C" int afan_seg_batch_aug_u8(const uint8_t* images, const int64_t* img_off, const uint8_t* labels, const int32_t* hs,
                                     const int32_t* ws, int64_t n_src, int64_t total_pixels, const int64_t* index,
                                     const int64_t* oh, const int64_t* ow, const int64_t* top, const int64_t* left,
                                     const int64_t* flip, float* out, int64_t* labels_out, int64_t m, int64_t out_h,
                                     int64_t out_w, double max_shrink, afan_stream_t stream) {
    if (m < 0 || out_h < 0 || out_w < 0 || n_src < 0 || total_pixels < 0) return AFAN_ESHAPE;
    if (out_h > (1 << 20) || out_w > (1 << 20)) return AFAN_ESHAPE;
    if (!(max_shrink >= 1.0) || max_shrink > MAX_SHRINK) return AFAN_ESHAPE;   // more than KMAX taps per axis (NaN included)
    const int64_t plane = out_h * out_w;
    if (plane > INT_MAX || (plane > 0 && m > (INT64_MAX / 8) / (3 * plane))) return AFAN_ESHAPE;
    if (m == 0 || plane == 0) return AFAN_OK;
    if (!images || !img_off || !labels || !hs || !ws || !index || !oh || !ow || !top || !left || !flip || !out || !labels_out)
        return AFAN_ENULL;
    if (n_src == 0 || total_pixels == 0) return AFAN_ESHAPE;      // a non-empty batch cannot be gathered from an empty split
    if (!aligned(out, 4) || !aligned(labels_out, 8) || !aligned(img_off, 8) || !aligned(hs, 4) || !aligned(ws, 4) ||
        !aligned(index, 8) || !aligned(oh, 8) || !aligned(ow, 8) || !aligned(top, 8) || !aligned(left, 8) || !aligned(flip, 8))
        return AFAN_EALIGN;
    const int64_t tiles_x = (out_w + TW - 1) / TW, tiles_y = (out_h + TH - 1) / TH;
    if (tiles_x * tiles_y > INT_MAX / m) return AFAN_ESHAPE;
    const bool vec = (out_w % 4 == 0) && aligned(out, 16) && aligned(labels_out, 16);
    hipStream_t st = (hipStream_t)stream;
    // algorithmic bytes per output pixel: 12 (image) + 8 (label) written, ~3 + 1 source bytes read
    AFAN_PROF("seg_batch_aug_kernel", (double)m * (double)plane * 24.0, st);
    const dim3 grid((unsigned)(m * tiles_x * tiles_y));
    if (vec)
        seg_batch_aug_kernel<true><<<grid, BLOCK, 0, st>>>(images, img_off, labels, hs, ws, n_src, total_pixels, index, oh, ow, top, left,
                                                          flip, out, labels_out, (int)out_h, (int)out_w, max_shrink, (int)tiles_x,
                                                          (int)tiles_y);
    else
        seg_batch_aug_kernel<false><<<grid, BLOCK, 0, st>>>(images, img_off, labels, hs, ws, n_src, total_pixels, index, oh, ow, top,
                                                           left, flip, out, labels_out, (int)out_h, (int)out_w, max_shrink, (int)tiles_x,
                                                           (int)tiles_y);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

extern "C" int afan_seg_batch_aug_jitter_u8(const uint8_t* images, const int64_t* img_off, const uint8_t* labels, const int32_t* hs,
                                            const int32_t* ws, int64_t n_src, int64_t total_pixels, const int64_t* index,
                                            const int64_t* oh, const int64_t* ow, const int64_t* top, const int64_t* left,
                                            const int64_t* flip, const int64_t* order, const float* brightness, const float* contrast,
                                            const float* saturation, int64_t* gray_sum, float* out, int64_t* labels_out, int64_t m,
                                            int64_t out_h, int64_t out_w, double max_shrink, afan_stream_t stream) {
    if (m < 0 || out_h < 0 || out_w < 0 || n_src < 0 || total_pixels < 0) return AFAN_ESHAPE;
    if (out_h > (1 << 20) || out_w > (1 << 20)) return AFAN_ESHAPE;
    if (!(max_shrink >= 1.0) || max_shrink > MAX_SHRINK) return AFAN_ESHAPE;   // more than KMAX taps per axis (NaN included)
    const int64_t plane = out_h * out_w;
    if (plane > INT_MAX || (plane > 0 && m > (INT64_MAX / 8) / (3 * plane))) return AFAN_ESHAPE;
    if (m == 0 || plane == 0) return AFAN_OK;
    if (!images || !img_off || !labels || !hs || !ws || !index || !oh || !ow || !top || !left || !flip || !order || !brightness ||
        !contrast || !saturation || !gray_sum || !out || !labels_out)
        return AFAN_ENULL;
    if (n_src == 0 || total_pixels == 0) return AFAN_ESHAPE;      // a non-empty batch cannot be gathered from an empty split
    if (!aligned(out, 4) || !aligned(labels_out, 8) || !aligned(img_off, 8) || !aligned(hs, 4) || !aligned(ws, 4) ||
        !aligned(index, 8) || !aligned(oh, 8) || !aligned(ow, 8) || !aligned(top, 8) || !aligned(left, 8) || !aligned(flip, 8) ||
        !aligned(order, 8) || !aligned(brightness, 4) || !aligned(contrast, 4) || !aligned(saturation, 4) || !aligned(gray_sum, 8))
        return AFAN_EALIGN;
    const int64_t tiles_x = (out_w + TW - 1) / TW, tiles_y = (out_h + TH - 1) / TH;
    if (tiles_x * tiles_y > INT_MAX / m) return AFAN_ESHAPE;
    const bool vec = (out_w % 4 == 0) && aligned(out, 16) && aligned(labels_out, 16);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(m * tiles_x * tiles_y));
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(gray_sum);
    {
        // algorithmic bytes per output pixel: ~3 source bytes read (the m sums are noise)
        AFAN_PROF("seg_jitter_stats_kernel", (double)m * (double)plane * 3.0, st);
        seg_jitter_clear_kernel<<<dim3((unsigned)((m + BLOCK - 1) / BLOCK)), BLOCK, 0, st>>>(sums, m);
        AFAN_LAUNCH_CHECK();
        seg_jitter_stats_kernel<<<grid, BLOCK, 0, st>>>(images, img_off, hs, ws, n_src, total_pixels, index, oh, ow, top, left, flip, order,
                                                        brightness, saturation, sums, (int)out_h, (int)out_w, max_shrink, (int)tiles_x,
                                                        (int)tiles_y);
        AFAN_LAUNCH_CHECK();
    }
    // algorithmic bytes per output pixel: 12 (image) + 8 (label) written, ~3 + 1 source bytes read
    AFAN_PROF("seg_batch_aug_jitter_kernel", (double)m * (double)plane * 24.0, st);
    if (vec)
        seg_batch_aug_jitter_kernel<true><<<grid, BLOCK, 0, st>>>(images, img_off, labels, hs, ws, n_src, total_pixels, index, oh, ow, top,
                                                                 left, flip, order, brightness, contrast, saturation, sums, out, labels_out,
                                                                 (int)out_h, (int)out_w, max_shrink, (int)tiles_x, (int)tiles_y);
    else
        seg_batch_aug_jitter_kernel<false><<<grid, BLOCK, 0, st>>>(images, img_off, labels, hs, ws, n_src, total_pixels, index, oh, ow, top,
                                                                  left, flip, order, brightness, contrast, saturation, sums, out,
                                                                  labels_out, (int)out_h, (int)out_w, max_shrink, (int)tiles_x,
                                                                  (int)tiles_y);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}
