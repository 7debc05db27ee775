// The training batch in one launch (gfx950): gather from a resident uint8 split + random crop + horizontal flip + /255.
// Reference behaviour: Classification/dataset.py:36-39 (RandomCrop(32, padding=4), RandomHorizontalFlip, ToTensor) applied by a
// DataLoader worker per image; here the split lives in HBM and a batch is one kernel.  The random draws are the caller's
// (main_perturb.DeviceLoader draws them on the device generator); the kernel is a pure function of them.
#include "afan_common.h"

#include <limits.h>

using namespace afan;

namespace {
constexpr int BLOCK = 256;

// ToTensor's scaling for every byte value, computed at COMPILE time (IEEE round-to-nearest per operation) as the DEVICE computes
// x.float().div_(255.0): torch's GPU division by a host scalar is a multiplication by the fp32 reciprocal, fl(v * fl(1 / 255)) —
// 126 of the 256 values are one ulp off the correctly rounded quotient fl(v / 255).  The batches the trainers have always seen are
// these products, so the table holds them (tests/test_batch_crop_flip_gpu.py pins all 256 against the device's own div_); a table
// also keeps the value independent of how the device compiler lowers or contracts fp32 arithmetic.
struct Div255 {
    float v[256];
    constexpr Div255() : v() {
        constexpr float inv = 1.0f / 255.0f;
        for (int i = 0; i < 256; ++i) v[i] = (float)i * inv;
    }
};
__constant__ Div255 kDiv255 = Div255();

// One workgroup serves `blocks_per_image` consecutive blockIdx values of ONE image: its four parameters (source index, top, left,
// flip) are read by one thread and handed to the rest through LDS together with the quotient table.  An item is 4 consecutive
// columns of one output row (VEC, w % 4 == 0: one 16-byte store per item) or one pixel (scalar widths); the output offset of item
// `it` inside the image is 4 * it (resp. it), so a wave's 64 stores are 1 KB of consecutive addresses.
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void batch_crop_flip_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ labels_src,
                                                                int64_t n_src, const int64_t* __restrict__ index,
                                                                const int64_t* __restrict__ top, const int64_t* __restrict__ left,
                                                                const uint8_t* __restrict__ flip, float* __restrict__ out,
                                                                int64_t* __restrict__ labels_out, int c, int h, int w, int pad,
                                                                int blocks_per_image) {
    __shared__ float tab[256];
    __shared__ int64_t s_img;
    __shared__ int s_top, s_left, s_flip;
    static_assert(BLOCK == 256, "one table entry per thread");
    const int64_t b = blockIdx.x / blocks_per_image;
    const int chunk = blockIdx.x % blocks_per_image;
    tab[threadIdx.x] = kDiv255.v[threadIdx.x];
    if (threadIdx.x == 0) {
        int64_t k = index[b];
        k = k < 0 ? 0 : (k >= n_src ? n_src - 1 : k);            // never read outside the split, whatever the index says
        s_img = k;
        int64_t t = pad, l = pad;                                 // null augmentation: the centred window = the image itself
        if (top) {
            t = top[b];
            l = left[b];
            t = t < 0 ? 0 : (t > 2 * (int64_t)pad ? 2 * (int64_t)pad : t);
            l = l < 0 ? 0 : (l > 2 * (int64_t)pad ? 2 * (int64_t)pad : l);
        }
        s_top = (int)t - pad;
        s_left = (int)l - pad;
        s_flip = flip ? (flip[b] != 0) : 0;
        if (chunk == 0 && labels_out) labels_out[b] = labels_src[k];
    }
    __syncthreads();
    const int64_t chw = (int64_t)c * h * w;
    const uint8_t* __restrict__ img = src + s_img * chw;
    float* __restrict__ dst = out + b * chw;
    const int dr = s_top, ds = s_left, fl = s_flip;
    const unsigned wq = VEC ? ((unsigned)w >> 2) : (unsigned)w;   // items per row
    const unsigned items = (unsigned)c * (unsigned)h * wq;        // (the host declines images of more than INT_MAX pixels: 32-bit indices)
    const unsigned stride = (unsigned)blocks_per_image * BLOCK;
    for (unsigned it = (unsigned)chunk * BLOCK + threadIdx.x; it < items; it += stride) {
        const unsigned row = it / wq;                             // ch * h + i
        const int jq = (int)(it - row * wq);
        const int i = (int)(row % (unsigned)h);
        const int r = i + dr;
        const bool row_in = r >= 0 && r < h;
        const uint8_t* __restrict__ sp = img + (int64_t)((int)row - i + r) * w; // (dereferenced only when row_in)
        if (VEC) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * jq + e;
                const int s = (fl ? w - 1 - j : j) + ds;
                v[e] = (row_in && s >= 0 && s < w) ? tab[sp[s]] : 0.f;
            }
            Elt<float>::stv(dst + 4 * (int64_t)it, v);
        } else {
            const int s = (fl ? w - 1 - jq : jq) + ds;
            dst[it] = (row_in && s >= 0 && s < w) ? tab[sp[s]] : 0.f;
        }
    }
}
}  // namespace

extern "C" int afan_batch_crop_flip_u8(const uint8_t* src, const int64_t* labels_src, int64_t n_src, const int64_t* index,
                                       const int64_t* top, const int64_t* left, const uint8_t* flip, float* out, int64_t* labels_out,
                                       int64_t m, int64_t c, int64_t h, int64_t w, int pad, afan_stream_t stream) {
    if (m < 0 || c < 0 || h < 0 || w < 0 || pad < 0 || n_src < 0) return AFAN_ESHAPE;
    if (c > INT_MAX || h > INT_MAX || w > INT_MAX || pad > (1 << 20)) return AFAN_ESHAPE;
    const int64_t hw = h * w;                                     // (both <= INT_MAX: no overflow)
    if (hw > 0 && c > 0 && (c > INT_MAX / hw || (m > 0 && m > (INT64_MAX / 4) / (c * hw)))) return AFAN_ESHAPE;   // an image: <= INT_MAX pixels
    if ((labels_src == nullptr) != (labels_out == nullptr)) return AFAN_ENULL;
    const int n_aug = (top != nullptr) + (left != nullptr) + (flip != nullptr);
    if (n_aug != 0 && n_aug != 3) return AFAN_ENULL;
    if (m == 0) return AFAN_OK;
    if (!src || !index || !out) return AFAN_ENULL;
    if (n_src == 0) return AFAN_ESHAPE;                           // a non-empty batch cannot be gathered from an empty split
    if (!aligned(out, 4) || !aligned(index, 8) || (top && (!aligned(top, 8) || !aligned(left, 8))) ||
        (labels_src && (!aligned(labels_src, 8) || !aligned(labels_out, 8))))
        return AFAN_EALIGN;
    const bool vec = (w % 4 == 0) && aligned(out, 16);
    const int64_t items = c * h * (vec ? w / 4 : w);
    int64_t bpi = (items + BLOCK - 1) / BLOCK;
    const int64_t cap = m >= 4096 ? 1 : 4096 / m;                 // ~4096 workgroups at most; a workgroup strides over the rest of its image
    if (bpi > cap) bpi = cap;                                     // (bpi * BLOCK + items < 2^32: the kernel's 32-bit item index cannot wrap)
    if (bpi < 1) bpi = 1;
    if (m > INT_MAX / bpi) return AFAN_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    AFAN_PROF("batch_crop_flip_kernel", (double)m * (double)(c * h * w) * 5.0 + (labels_out ? 16.0 * (double)m : 0.0), st);
    const dim3 grid((unsigned)(m * bpi));
    if (vec)
        batch_crop_flip_kernel<true><<<grid, BLOCK, 0, st>>>(src, labels_src, n_src, index, top, left, flip, out, labels_out, (int)c, (int)h,
                                                            (int)w, pad, (int)bpi);
    else
        batch_crop_flip_kernel<false><<<grid, BLOCK, 0, st>>>(src, labels_src, n_src, index, top, left, flip, out, labels_out, (int)c, (int)h,
                                                             (int)w, pad, (int)bpi);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}
