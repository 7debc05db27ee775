// Segmentation validation's scoring for gfx950: bilinear resize of the classifier's logits, per-pixel arg-max and the confusion
// matrix in ONE launch.
//   Segmentation/network/utils.py:30    F.interpolate(logits, size=input_shape, mode='bilinear', align_corners=False)
//   Segmentation/args.py:187-196        preds = outputs.detach().max(dim=1)[1].cpu().numpy(); metrics.update(targets, preds)
//   Segmentation/metrics/stream_metrics.py:42-49   _fast_hist: mask = (t >= 0) & (t < C); bincount(C * t[mask] + pred[mask])
// The reference materialises the [N, C, H, W] logits (44 MB at 2 x 21 x 513 x 513, see afan_seg.hip above ce2d_up_kernel), reads
// them back for the arg-max, copies the predictions to the host and counts there.  Here a workgroup walks 16 x 16 tiles of OUTPUT
// pixels (a persistent grid: a few workgroups per CU): it stages the tile's source window in LDS, a thread interpolates its
// pixel's C logits one at a time keeping only the running maximum, and counts into a C x C int32 histogram in LDS (LDS atomics).
// At its end the workgroup adds its non-zero bins to the int64 matrix in global memory (64-bit integer atomics: the result does
// not depend on the order).  Nothing but the low-resolution logits and the labels is read; only the matrix is written.
#include "afan_common.h"

using namespace afan;

namespace {

constexpr int BLOCK = 256;
constexpr int CF_MAX_C = 32;     // CE_MAX_C of afan_seg.hip
constexpr int CF_OT = 16;        // output tile side: BLOCK = CF_OT * CF_OT, one thread per pixel

// ATen's area_pixel_compute_source_index in fp32 — the same expressions as src_index of afan_seg.hip (the interpolated logits
// must equal afan_upsample_bilinear_fwd's to the bit); host and device share it: the host sizes the LDS window with it.
struct Src {
    int i0, i1;
    float l0, l1;
};
__host__ __device__ __forceinline__ Src src_index(float scale, int dst, int in_size) {
    float s = fmaf(scale, (float)dst + 0.5f, -0.5f);
    if (s < 0.f) s = 0.f;
    Src r;
    r.i0 = (int)s;
    if (r.i0 > in_size - 1) r.i0 = in_size - 1;
    r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
    r.l1 = s - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

// LDS: [C * C] int32 histogram, then the source window [SH][SW][C] of the current tile (win_cap floats: the host's maximum
// over all tiles, from the same src_index)
__global__ __launch_bounds__(BLOCK) void seg_confusion_up_kernel(const float* __restrict__ lo, const int64_t* __restrict__ target,
                                                                 unsigned long long* __restrict__ hist, int C, int h, int w, int H,
                                                                 int W, float sh, float sw, int tiles_x, int tiles_y,
                                                                 int tiles, int win_cap) {
    extern __shared__ float lds_cf[];
    int* lh = reinterpret_cast<int*>(lds_cf);
    float* st = lds_cf + C * C;
    for (int i = threadIdx.x; i < C * C; i += BLOCK) lh[i] = 0;
    const int per_img = tiles_x * tiles_y;
    const int oyl = threadIdx.x / CF_OT, oxl = threadIdx.x % CF_OT;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int n = tile / per_img, tr = tile - n * per_img;
        const int ty = tr / tiles_x, tx = tr - ty * tiles_x;
        const int y0 = ty * CF_OT, y1 = (y0 + CF_OT < H ? y0 + CF_OT : H) - 1;
        const int x0 = tx * CF_OT, x1 = (x0 + CF_OT < W ? x0 + CF_OT : W) - 1;
        const int s0 = src_index(sh, y0, h).i0, s1 = src_index(sh, y1, h).i1;
        const int t0 = src_index(sw, x0, w).i0, t1 = src_index(sw, x1, w).i1;
        const int SH_ = s1 - s0 + 1, SW_ = t1 - t0 + 1, row = SW_ * C;
        if (SH_ * row > win_cap) continue;        // (never: the host took the maximum over these same windows; block-uniform)
        __syncthreads();                          // the histogram is zeroed / the previous tile's window is no longer read
        const float* base = lo + ((int64_t)n * h * w + (int64_t)s0 * w + t0) * C;
        for (int e = threadIdx.x; e < SH_ * row; e += BLOCK) {      // a window row is one contiguous run of SW * C floats
            const int r = e / row, q = e - r * row;
            st[e] = base[(int64_t)r * w * C + q];
        }
        __syncthreads();
        const int oy = y0 + oyl, ox = x0 + oxl;
        if (oy <= y1 && ox <= x1) {
            const int64_t t = target[((int64_t)n * H + oy) * W + ox];
            if (t >= 0 && t < C) {
                const Src a = src_index(sh, oy, h), b = src_index(sw, ox, w);
                const float* r0 = st + (a.i0 - s0) * row;
                const float* r1 = st + (a.i1 - s0) * row;
                const int q0 = (b.i0 - t0) * C, q1 = (b.i1 - t0) * C;
                float best = 0.f;
                int arg = 0;
                for (int c = 0; c < C; ++c) {     // ATen's association, as upsample_fwd_kernel
                    const float p00 = r0[q0 + c], p01 = r0[q1 + c], p10 = r1[q0 + c], p11 = r1[q1 + c];
                    const float v = a.l0 * (b.l0 * p00 + b.l1 * p01) + a.l1 * (b.l0 * p10 + b.l1 * p11);
                    // torch.max(dim=1): the first maximum; a NaN is the maximum and, once taken, stays
                    if (c == 0 || (best == best && (v > best || v != v))) { best = v; arg = c; }
                }
                atomicAdd(&lh[(int)t * C + arg], 1);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += BLOCK) {
        const int v = lh[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

// the widest source window (rows or columns) a CF_OT-pixel output tile reads along one axis
int max_window(int in_size, int out_size) {
    const float scale = (float)in_size / (float)out_size;
    int worst = 0;
    for (int y0 = 0; y0 < out_size; y0 += CF_OT) {
        const int y1 = (y0 + CF_OT < out_size ? y0 + CF_OT : out_size) - 1;
        const int win = src_index(scale, y1, in_size).i1 - src_index(scale, y0, in_size).i0 + 1;
        if (win > worst) worst = win;
    }
    return worst;
}

}  // namespace

extern "C" {

int afan_seg_confusion_upsampled(const float* logits, const int64_t* target, int64_t n, int64_t c, int64_t h, int64_t w,
                                 int64_t ho, int64_t wo, int64_t* hist, afan_stream_t stream) {
    if (n < 0 || c <= 0 || c > CF_MAX_C || h <= 0 || w <= 0 || ho < h || wo < w || ho > 0x7fffffffLL || wo > 0x7fffffffLL)
        return AFAN_ESHAPE;
    if (n == 0) return AFAN_OK;
    if (!logits || !target || !hist) return AFAN_ENULL;
    if (!aligned(logits, 4) || !aligned(target, 8) || !aligned(hist, 8)) return AFAN_EALIGN;
    const int64_t tx = (wo + CF_OT - 1) / CF_OT, ty = (ho + CF_OT - 1) / CF_OT;
    if (tx * ty > 0x7fffffffLL || n * tx * ty > 0x7fffffffLL) return AFAN_ESHAPE;
    const int64_t tiles = n * tx * ty;
    // up-scaling: 16 output rows read at most 17 source rows; 18 x 18 x 32 floats + the histogram are 45 KB
    const int win_cap = max_window((int)h, (int)ho) * max_window((int)w, (int)wo) * (int)c;
    const size_t lds = ((size_t)c * c + (size_t)win_cap) * 4;
    if (lds > 64 * 1024) return AFAN_ESHAPE;
    static int cus = 0;
    if (!cus) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            return AFAN_ESHAPE;
        cus = v > 0 ? v : 256;
    }
    // persistent: two workgroups per CU (<= 45 KB of LDS each), so a launch flushes at most 2 * CUs * c * c bins
    const int64_t grid = tiles < 2 * (int64_t)cus ? tiles : 2 * (int64_t)cus;
    if ((tiles + grid - 1) / grid * BLOCK > 0x7fffffffLL) return AFAN_ESHAPE;       // a workgroup's counters are int32
    hipStream_t st = (hipStream_t)stream;
    AFAN_PROF("seg_confusion_upsampled_kernel", (double)n * ho * wo * 8.0 + 4.0 * n * h * w * c, st);
    const float sh = (float)h / (float)ho, sw = (float)w / (float)wo;
    seg_confusion_up_kernel<<<(unsigned)grid, BLOCK, lds, st>>>(logits, target, reinterpret_cast<unsigned long long*>(hist), (int)c,
                                                                 (int)h, (int)w, (int)ho, (int)wo, sh, sw, (int)tx, (int)ty,
                                                                 (int)tiles, win_cap);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

}  // extern "C"
