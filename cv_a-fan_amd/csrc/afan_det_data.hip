// The detection training batch in one launch (gfx950): gather from a resident, variably sized uint8 split + mirror + Pillow's
// bilinear resize + zero padding to the right and below + /255, and the sample's ground-truth boxes (mirrored, scaled, padded).
// Reference behaviour: Detection/dataset/voc2007.py:95-116 (ImageOps.mirror and `image.width - bboxes[:, [2, 0]]` with probability
// one half, Base.preprocess, `bboxes *= scale`) and dataset/base.py:75-124 (Resize((round(h * scale), round(w * scale))), ToTensor,
// padding_collate_fn's F.pad to the batch's largest image and zero rows up to its largest box count), per image in eight
// DataLoader workers on PIL images.  The draws are the caller's (det_data.DetDeviceLoader); the kernel is a pure function of them.
//
// What is reproduced bit for bit (det_data._det_batch_numpy restates it; tests/golden/det_data_pillow.npz holds Pillow's and torch's
// own output):
//   * the image: the resampler of afan_resample.h on the MIRRORED source — the mirror comes BEFORE the horizontal pass, so output
//     column c takes the taps of column c over source columns w - 1 - x (Pillow's coefficients are not mirror-symmetric to the last
//     bit, so this is not column ow - 1 - c of the unmirrored resize).  The tile's column table holds the taps already mirrored
//     (first column w - xmin - n, coefficients reversed); the integer sum does not depend on the order, so sample_rgb is used as it is.
//   * the padding: the result at the top-left of the plane, 0 to the right of ow and below oh.
//   * the boxes, in fp32, every operation rounded on its own: l' = fl(w - r), r' = fl(w - l) where mirrored, then fl(x * scale).
#include "afan_common.h"

namespace {
constexpr int BLOCK = 256;
constexpr int TW = 128;              // tile: TH output rows x TW output columns per workgroup
constexpr int TH = 16;
}  // namespace
#include "afan_resample.h"   // the bilinear taps, the tile tables and sample_rgb (shared with afan_seg_data.hip)

using namespace afan;

#pragma clang fp contract(off)

namespace {

// the sample's parameters, clamped (uniform over the workgroup)
struct DetGeom {
    int h, w, oh, ow;
    int64_t base;                                                 // the image's first pixel in the packed split
    int64_t box0, count;                                          // the sample's rows of boxes_src / cls_src
    bool fl, valid;
};

__device__ __forceinline__ DetGeom det_geom(int64_t b, const int64_t* __restrict__ img_off, const int32_t* __restrict__ hs,
                                            const int32_t* __restrict__ ws, int64_t n_src, int64_t total_pixels,
                                            const int64_t* __restrict__ box_off, int64_t total_boxes,
                                            const int64_t* __restrict__ index, const int64_t* __restrict__ p_oh,
                                            const int64_t* __restrict__ p_ow, const int64_t* __restrict__ p_flip, double max_shrink) {
    DetGeom g;
    int64_t k = index[b];
    k = k < 0 ? 0 : (k >= n_src ? n_src - 1 : k);
    int h = hs[k], w = ws[k];
    const int64_t off = img_off[k];
    int64_t base = off / 3;
    const int64_t b0 = box_off[k], b1 = box_off[k + 1];
    // never read outside the split, whatever the tables say: an entry that does not fit gives an all-zero sample
    const bool valid = h >= 1 && w >= 1 && h <= MAX_SIDE && w <= MAX_SIDE && off >= 0 && base + (int64_t)h * w <= total_pixels &&
                       b0 >= 0 && b1 >= b0 && b1 <= total_boxes;
    if (!valid) { h = 1; w = 1; base = 0; }
    int lo_h = (int)ceil((double)h / max_shrink), lo_w = (int)ceil((double)w / max_shrink);
    lo_h = lo_h < 1 ? 1 : lo_h;
    lo_w = lo_w < 1 ? 1 : lo_w;
    int64_t v = p_oh[b];
    g.oh = (int)(v < lo_h ? lo_h : (v > MAX_SIDE ? MAX_SIDE : v));
    v = p_ow[b];
    g.ow = (int)(v < lo_w ? lo_w : (v > MAX_SIDE ? MAX_SIDE : v));
    g.fl = p_flip[b] != 0;
    g.h = h; g.w = w; g.base = base; g.valid = valid;
    g.box0 = valid ? b0 : 0;
    g.count = valid ? b1 - b0 : 0;
    return g;
}

// the tile's tables (the caller synchronises the workgroup afterwards): threads 0..TW-1 the columns, TW..TW+TH-1 the rows
__device__ __forceinline__ void det_tables(Tables& s, const DetGeom& g, int tid, int i0, int j0, int out_h, int out_w) {
    static_assert(BLOCK >= TW + TH, "thread roles below");
    if (tid < TW) {
        const int j = j0 + tid;
        int xmin = 0, n = -1, coef[KMAX];
#pragma unroll
        for (int u = 0; u < KMAX; ++u) coef[u] = 0;
        if (j < out_w && j < g.ow && g.valid) {
            bilinear_taps(j, g.w, g.ow, xmin, n, coef);           // over the mirrored source where fl ...
            if (g.fl) {                                           // ... whose column x is the source's w - 1 - x (xmin + n <= w)
                int rc[KMAX];
#pragma unroll
                for (int u = 0; u < KMAX; ++u) {
                    int cv = 0;
#pragma unroll
                    for (int q = 0; q < KMAX; ++q) cv = (q == n - 1 - u) ? coef[q] : cv;
                    rc[u] = cv;
                }
#pragma unroll
                for (int u = 0; u < KMAX; ++u) coef[u] = rc[u];
                xmin = g.w - xmin - n;
            }
        }
        s.cmin[tid] = xmin;
        s.cn[tid] = n;
#pragma unroll
        for (int u = 0; u < KMAX; ++u) s.ccoef[u][tid] = coef[u];
    } else if (tid < TW + TH) {
        const int t = tid - TW;
        const int r = i0 + t;
        int xmin = 0, n = -1, coef[KMAX];
#pragma unroll
        for (int u = 0; u < KMAX; ++u) coef[u] = 0;
        if (r < out_h && r < g.oh && g.valid) bilinear_taps(r, g.h, g.oh, xmin, n, coef);
        s.rmin[t] = xmin;
        s.rn[t] = n;
#pragma unroll
        for (int u = 0; u < KMAX; ++u) s.rcoef[u][t] = coef[u];
    }
}

// An item is 4 consecutive columns of one output row (VEC, out_w % 4 == 0: 16-byte stores) or one pixel.  The first workgroup of
// each sample also writes the sample's g_max rows of boxes and labels.
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void det_batch_resize_kernel(
    const uint8_t* __restrict__ images, const int64_t* __restrict__ img_off, const int32_t* __restrict__ hs,
    const int32_t* __restrict__ ws, int64_t n_src, int64_t total_pixels, const float* __restrict__ boxes_src,
    const int64_t* __restrict__ cls_src, const int64_t* __restrict__ box_off, int64_t total_boxes,
    const int64_t* __restrict__ index, const int64_t* __restrict__ p_oh, const int64_t* __restrict__ p_ow,
    const int64_t* __restrict__ p_flip, const float* __restrict__ p_scale, float* __restrict__ out, float* __restrict__ boxes_out,
    int64_t* __restrict__ labels_out, int out_h, int out_w, int g_max, double max_shrink, int tiles_x, int tiles_y) {
    __shared__ Tables s;
    __shared__ float s_quot[256];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x;
    const int ty = (blockIdx.x / tiles_x) % tiles_y;
    const int64_t b = blockIdx.x / (tiles_x * tiles_y);
    const int i0 = ty * TH, j0 = tx * TW;
    const DetGeom g = det_geom(b, img_off, hs, ws, n_src, total_pixels, box_off, total_boxes, index, p_oh, p_ow, p_flip, max_shrink);
    s_quot[tid] = kQuot255.v[tid];
    det_tables(s, g, tid, i0, j0, out_h, out_w);
    __syncthreads();

    const uint8_t* __restrict__ img = images + 3 * g.base;
    const int64_t plane = (int64_t)out_h * out_w;
    float* __restrict__ dst = out + b * 3 * plane;
    constexpr int E = VEC ? 4 : 1;
    constexpr int WQ = TW / E;
    for (int it = tid; it < TH * WQ; it += BLOCK) {
        const int ti = it / WQ;
        const int tq = it - ti * WQ;
        const int i = i0 + ti;
        const int jq = j0 + tq * E;
        if (i >= out_h || jq >= out_w) continue;                  // (VEC: out_w % 4 == 0, so the 4 columns are in or out together)
        float px[3][E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            int c[3];
            sample_rgb(s, img, g.w, ti, tq * E + e, c);           // the padding: 0
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
        } else {
            dst[o] = px[0][0];
            dst[plane + o] = px[1][0];
            dst[2 * plane + o] = px[2][0];
        }
    }

    if (tx == 0 && ty == 0) {                                     // the sample's boxes: a few values, in the same launch
        const float wf = (float)g.w;                              // (image.width: exact in fp32)
        const float sc = p_scale[b];
        for (int j = tid; j < g_max; j += BLOCK) {
            float l = 0.f, t = 0.f, r = 0.f, bt = 0.f;
            int64_t lab = 0;
            if (j < g.count) {
                const float* __restrict__ bp = boxes_src + (g.box0 + j) * 4;
                l = bp[0]; t = bp[1]; r = bp[2]; bt = bp[3];
                if (g.fl) {
                    const float nl = __fsub_rn(wf, r), nr = __fsub_rn(wf, l);
                    l = nl;
                    r = nr;
                }
                l = __fmul_rn(l, sc);
                t = __fmul_rn(t, sc);
                r = __fmul_rn(r, sc);
                bt = __fmul_rn(bt, sc);
                lab = cls_src[g.box0 + j];
            }
            float* __restrict__ bo = boxes_out + (b * g_max + j) * 4;
            bo[0] = l; bo[1] = t; bo[2] = r; bo[3] = bt;
            labels_out[b * g_max + j] = lab;
        }
    }
}
}  // namespace

extern "C" int afan_det_batch_resize_u8(const uint8_t* images, const int64_t* img_off, const int32_t* hs, const int32_t* ws,
                                        int64_t n_src, int64_t total_pixels, const float* boxes_src, const int64_t* cls_src,
                                        const int64_t* box_off, int64_t total_boxes, const int64_t* index, const int64_t* oh,
                                        const int64_t* ow, const int64_t* flip, const float* scale, float* out, float* boxes_out,
                                        int64_t* labels_out, int64_t m, int64_t out_h, int64_t out_w, int64_t g_max,
                                        double max_shrink, afan_stream_t stream) {
    if (m < 0 || out_h < 0 || out_w < 0 || n_src < 0 || total_pixels < 0 || total_boxes < 0 || g_max < 0) return AFAN_ESHAPE;
    if (out_h > (1 << 20) || out_w > (1 << 20) || g_max > (1 << 20)) return AFAN_ESHAPE;
    if (!(max_shrink >= 1.0) || max_shrink > MAX_SHRINK) return AFAN_ESHAPE;   // more than KMAX taps per axis (NaN included)
    const int64_t plane = out_h * out_w;
    if (plane > INT_MAX || (plane > 0 && m > (INT64_MAX / 8) / (3 * plane))) return AFAN_ESHAPE;
    if (g_max > 0 && m > (INT64_MAX / 64) / g_max) return AFAN_ESHAPE;
    if (m == 0 || plane == 0) return AFAN_OK;
    if (!images || !img_off || !hs || !ws || !box_off || !index || !oh || !ow || !flip || !scale || !out) return AFAN_ENULL;
    if ((total_boxes > 0 && (!boxes_src || !cls_src)) || (g_max > 0 && (!boxes_out || !labels_out))) return AFAN_ENULL;
    if (n_src == 0 || total_pixels == 0) return AFAN_ESHAPE;      // a non-empty batch cannot be gathered from an empty split
    if (!aligned(out, 4) || !aligned(boxes_out, 4) || !aligned(labels_out, 8) || !aligned(img_off, 8) || !aligned(hs, 4) ||
        !aligned(ws, 4) || !aligned(boxes_src, 4) || !aligned(cls_src, 8) || !aligned(box_off, 8) || !aligned(index, 8) ||
        !aligned(oh, 8) || !aligned(ow, 8) || !aligned(flip, 8) || !aligned(scale, 4))
        return AFAN_EALIGN;
    const int64_t tiles_x = (out_w + TW - 1) / TW, tiles_y = (out_h + TH - 1) / TH;
    if (tiles_x * tiles_y > INT_MAX / m) return AFAN_ESHAPE;
    const bool vec = (out_w % 4 == 0) && aligned(out, 16);
    hipStream_t st = (hipStream_t)stream;
    // algorithmic bytes per output pixel: 12 written, ~3 source bytes read (the boxes are noise)
    AFAN_PROF("det_batch_resize_kernel", (double)m * (double)plane * 15.0, st);
    const dim3 grid((unsigned)(m * tiles_x * tiles_y));
    if (vec)
        det_batch_resize_kernel<true><<<grid, BLOCK, 0, st>>>(images, img_off, hs, ws, n_src, total_pixels, boxes_src, cls_src, box_off,
                                                             total_boxes, index, oh, ow, flip, scale, out, boxes_out, labels_out,
                                                             (int)out_h, (int)out_w, (int)g_max, max_shrink, (int)tiles_x, (int)tiles_y);
    else
        det_batch_resize_kernel<false><<<grid, BLOCK, 0, st>>>(images, img_off, hs, ws, n_src, total_pixels, boxes_src, cls_src, box_off,
                                                              total_boxes, index, oh, ow, flip, scale, out, boxes_out, labels_out,
                                                              (int)out_h, (int)out_w, (int)g_max, max_shrink, (int)tiles_x, (int)tiles_y);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}
