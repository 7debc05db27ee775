// Detection inference (model.py:369-407 `generate_detections`): per image and foreground class — decode, clip, score filter, sort
// and greedy NMS — as ONE launch for all (image, class) lists, and a second small one that packs the lists into the flat result.
// The per-class loop it replaces costs, per list, a sort, the three launches of afan_nms (built for 12 000 proposals: a 16-wave
// scanner / worker workgroup, a mask in global memory, a workspace) and a host read; the lists of an evaluation hold 300 boxes.
//
// det_class_nms_kernel: one workgroup of 256 threads per (image b, class c >= 1); everything lives in LDS, the waves meet at workgroup
// barriers only, nothing is shared between workgroups.
//   1. decode + clip  box[n] = clip(apply_transformer(proposal[b, n], t[b, n, c] * std + mean)) with box_decode_clip_kernel's arithmetic
//      (afan_det_targets.hip); the multiply and the add round separately (-ffp-contract=off), like the tensor expression they replace.
//   2. filter + key   a box enters the list if prob > min_prob (min_prob < 0: every box).  key = (~ordered(prob)) << 32 | n: ascending
//      keys are descending probabilities, ties by ascending proposal index; rows left out and the padding up to the next power of
//      two hold the all-ones sentinel.
//   3. sort           bitonic, in LDS.
//   4. greedy NMS     the sorted list is walked once; a row that is still alive strikes every later row j with
//      inter / (sa + sb - inter) > threshold (areas and intersections with + 1, fp32, IEEE division: the decision afan_det.hip's
//      iou_over(..., inclusive = 0) is built to equal).  `removed[i]` is settled before the walk reaches i (all writes to it lie
//      before the barrier that ends an earlier kept row), so every thread takes the same branch and only kept rows cost a barrier.
//   5. output         survivors flagged at their proposal index, an exclusive scan of the flags, rows written in ascending
//      proposal index (what `boxes[keep]`, `probs[keep]` give with afan_nms's ascending keep), and the count.
// LDS plan at the cap N = 2048: keys 8 B x 2048 = 16 KB, boxes 16 B x 2048 = 32 KB, areas 4 B x 2048 = 8 KB, removed 2 KB, kept 2 KB,
// scan 1 KB + 4 B: 61 KB + 4 B of the 160 KB a gfx950 workgroup may hold (static, below the 64 KB a kernel gets without asking).
//
// det_pack_kernel: workgroup (b, c) adds the counts of the lists before it and copies its rows behind them: boxes [total, 4] and
// probabilities [total] ordered by image, class, proposal index.  The host reads the counts once and slices.
#include "afan_common.h"

using namespace afan;

namespace {

constexpr int TB = 256;
constexpr int MAX_N = 2048;
constexpr int MAX_C = 64;

// float -> unsigned whose order is the floats' (afan_det_targets.hip)
__device__ __forceinline__ unsigned ordered(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Tensor.clamp(min=0, max=limit) on one coordinate, a NaN handed through (afan_det_targets.hip's clip_coord, the same expression)
__device__ __forceinline__ float clip_coord(float v, float limit) { return v < 0.f ? 0.f : (v > limit ? limit : v); }

__device__ __forceinline__ float area_incl(const float4 a) { return (a.z - a.x + 1.f) * (a.w - a.y + 1.f); }

// nms.cu:36-49 on one pair
__device__ __forceinline__ bool iou_exceeds(const float4 a, float sa, const float4 b, float sb, float thresh) {
    const float left = fmaxf(a.x, b.x), right = fminf(a.z, b.z);
    const float top = fmaxf(a.y, b.y), bottom = fminf(a.w, b.w);
    const float w = fmaxf(right - left + 1.f, 0.f), h = fmaxf(bottom - top + 1.f, 0.f);
    const float inter = w * h;
    const float u = sa + sb - inter;
    return inter / u > thresh;
}

__global__ __launch_bounds__(TB) void det_class_nms_kernel(const float4* __restrict__ proposals, const float4* __restrict__ transformers,
                                                           const float* __restrict__ probs, float4 mean, float4 stdv, int N, int C,
                                                           int P, float right, float bottom, float thresh, float min_prob,
                                                           float4* __restrict__ out_boxes, float* __restrict__ out_probs,
                                                           int64_t* __restrict__ counts) {
    __shared__ unsigned long long key[MAX_N];
    __shared__ float4 box[MAX_N];
    __shared__ float area[MAX_N];
    __shared__ unsigned char removed[MAX_N];
    __shared__ unsigned char kept[MAX_N];
    __shared__ int scan[TB];
    __shared__ int s_valid;

    const int tid = threadIdx.x;
    const int c = 1 + (int)(blockIdx.x % (unsigned)(C - 1));
    const int64_t b = blockIdx.x / (unsigned)(C - 1);
    const int64_t list = b * (C - 1) + (c - 1);

    if (tid == 0) s_valid = 0;
    __syncthreads();

    // 1, 2: decode, clip, filter, key
    int mine = 0;
    for (int n = tid; n < P; n += TB) {
        unsigned long long k = ~0ull;
        if (n < N) {
            const float4 s = proposals[b * N + n];
            const float4 t = transformers[(b * N + n) * C + c];
            float4 d;
            d.x = t.x * stdv.x; d.x = d.x + mean.x;
            d.y = t.y * stdv.y; d.y = d.y + mean.y;
            d.z = t.z * stdv.z; d.z = d.z + mean.z;
            d.w = t.w * stdv.w; d.w = d.w + mean.w;
            const float scx = (s.x + s.z) / 2.f, scy = (s.y + s.w) / 2.f, sw = s.z - s.x, sh = s.w - s.y;
            const float cx = d.x * sw + scx, cy = d.y * sh + scy, w = expf(d.z) * sw, h = expf(d.w) * sh;
            float4 o = make_float4(cx - w / 2.f, cy - h / 2.f, cx + w / 2.f, cy + h / 2.f);
            o.x = clip_coord(o.x, right);
            o.z = clip_coord(o.z, right);
            o.y = clip_coord(o.y, bottom);
            o.w = clip_coord(o.w, bottom);
            box[n] = o;
            area[n] = area_incl(o);
            kept[n] = 0;
            const float p = probs[(b * N + n) * C + c];
            if (min_prob < 0.f || p > min_prob) {
                k = ((unsigned long long)(~ordered(p)) << 32) | (unsigned)n;
                ++mine;
            }
        }
        key[n] = k;
        removed[n] = 0;
    }
    if (mine) atomicAdd(&s_valid, mine);          // (an LDS counter of this workgroup)
    __syncthreads();
    const int M = s_valid;

    // 3: bitonic sort of key[0, P), ascending
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (P >> 1); i += TB) {
                const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1));
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned long long a = key[lo], z = key[hi];
                if ((a > z) == up) { key[lo] = z; key[hi] = a; }
            }
            __syncthreads();
        }
    }

    // 4: greedy NMS over the M rows of the list
    for (int i = 0; i < M; ++i) {
        if (removed[i]) continue;                                    // uniform: settled before an earlier barrier
        const int ni = (int)(unsigned)key[i];
        const float4 bi = box[ni];
        const float sa = area[ni];
        for (int j = i + 1 + tid; j < M; j += TB) {
            if (removed[j]) continue;
            const int nj = (int)(unsigned)key[j];
            if (iou_exceeds(bi, sa, box[nj], area[nj], thresh)) removed[j] = 1;
        }
        __syncthreads();
    }
    __syncthreads();

    // 5: survivors in ascending proposal index
    for (int i = tid; i < M; i += TB)
        if (!removed[i]) kept[(int)(unsigned)key[i]] = 1;
    __syncthreads();
    const int per = (N + TB - 1) / TB;
    const int n0 = tid * per, n1 = n0 + per < N ? n0 + per : N;
    int cnt = 0;
    for (int n = n0; n < n1; ++n) cnt += kept[n];
    scan[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < TB; o <<= 1) {
        const int v = tid >= o ? scan[tid - o] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    int rank = scan[tid] - cnt;
    for (int n = n0; n < n1; ++n) {
        if (kept[n]) {
            out_boxes[list * N + rank] = box[n];
            out_probs[list * N + rank] = probs[(b * N + n) * C + c];
            ++rank;
        }
    }
    if (tid == TB - 1) counts[list] = scan[TB - 1];
}

// lists [L, N] rows -> flat rows behind the lists before them
__global__ __launch_bounds__(TB) void det_pack_kernel(const float4* __restrict__ boxes, const float* __restrict__ probs,
                                                      const int64_t* __restrict__ counts, int64_t N, float4* __restrict__ flat_boxes,
                                                      float* __restrict__ flat_probs) {
    __shared__ long long part[TB];
    const int tid = threadIdx.x;
    const int64_t list = blockIdx.x;
    long long s = 0;
    for (int64_t l = tid; l < list; l += TB) s += counts[l];
    part[tid] = s;
    __syncthreads();
    for (int o = TB >> 1; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
    }
    const int64_t off = part[0];
    int64_t cnt = counts[list];
    cnt = cnt < 0 ? 0 : (cnt > N ? N : cnt);
    for (int64_t r = tid; r < cnt; r += TB) {
        flat_boxes[off + r] = boxes[list * N + r];
        flat_probs[off + r] = probs[list * N + r];
    }
}

}  // namespace

extern "C" {

int afan_det_class_nms_supported(int64_t N, int64_t C) { return (N >= 1 && N <= MAX_N && C >= 2 && C <= MAX_C) ? 1 : 0; }

int afan_det_class_nms(const float* proposals, const float* transformers, const float* probs, const float* norm, int64_t B, int64_t N,
                       int64_t C, float right, float bottom, float nms_threshold, float min_prob, float* out_boxes, float* out_probs,
                       int64_t* counts, afan_stream_t stream) {
    if (B < 0 || !afan_det_class_nms_supported(N, C)) return AFAN_ESHAPE;
    if (B > (1 << 20)) return AFAN_ESHAPE;                            // B * (C - 1) workgroups, B * N * C * 4 elements: far inside int64
    if (B == 0) return AFAN_OK;
    if (!proposals || !transformers || !probs || !norm || !out_boxes || !out_probs || !counts) return AFAN_ENULL;
    if (!aligned(proposals, 16) || !aligned(transformers, 16) || !aligned(probs, 4) || !aligned(norm, 4) || !aligned(out_boxes, 16) ||
        !aligned(out_probs, 4) || !aligned(counts, 8))
        return AFAN_EALIGN;
    int P = 1;
    while (P < N) P <<= 1;
    if (P < 2) P = 2;
    const float4 mean = make_float4(norm[0], norm[1], norm[2], norm[3]);
    const float4 stdv = make_float4(norm[4], norm[5], norm[6], norm[7]);
    hipStream_t st = (hipStream_t)stream;
    AFAN_PROF("det_class_nms_kernel", (double)B * N * (16.0 + (C - 1) * 40.0), st);
    det_class_nms_kernel<<<(unsigned)(B * (C - 1)), TB, 0, st>>>((const float4*)proposals, (const float4*)transformers, probs, mean, stdv,
                                                               (int)N, (int)C, P, right, bottom, nms_threshold, min_prob,
                                                               (float4*)out_boxes, out_probs, counts);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

int afan_det_pack(const float* boxes, const float* probs, const int64_t* counts, int64_t L, int64_t N, float* flat_boxes,
                  float* flat_probs, afan_stream_t stream) {
    if (L < 0 || N < 1 || L > ((int64_t)1 << 26) || N > ((int64_t)1 << 24)) return AFAN_ESHAPE;
    if (L == 0) return AFAN_OK;
    if (!boxes || !probs || !counts || !flat_boxes || !flat_probs) return AFAN_ENULL;
    if (!aligned(boxes, 16) || !aligned(flat_boxes, 16) || !aligned(probs, 4) || !aligned(flat_probs, 4) || !aligned(counts, 8))
        return AFAN_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    AFAN_PROF("det_pack_kernel", (double)L * N * 40.0, st);
    det_pack_kernel<<<(unsigned)L, TB, 0, st>>>((const float4*)boxes, probs, counts, N, (float4*)flat_boxes, flat_probs);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

}  // extern "C"
