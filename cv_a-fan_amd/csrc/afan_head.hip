// Classifier head of the slice protocol: global average pool -> flatten -> linear (resnet_s.py:108-110, run at the end of
// every tail pass: K times inside PGD and for both final passes).  In eager PyTorch this is a mean, a cast, an addmm and,
// backward, two GEMMs, a column sum, an expand/divide and a cast — ten launches of a few microseconds on tensors of a
// few hundred KB.  Here: one forward launch, two backward launches, fp32 arithmetic throughout.
//   forward : pooled[b][c] = mean_hw x[b][hw][c]   (channels-last: lanes along c, coalesced)
//             logits[b][k] = sum_c pooled[b][c] * W[k][c] + bias[k]
//   backward: dx[b][hw][c] = (sum_k dlogits[b][k] * W[k][c]) / HW
//             dW[k][c] (+)= sum_b dlogits[b][k] * pooled[b][c] ;  db[k] (+)= sum_b dlogits[b][k]
#include "afan_common.h"
#include "afan_bn_nhwc.h"

using namespace afan;

namespace {

constexpr int BLOCK = 256;
constexpr int MAXK = 16;      // classes handled with register accumulators; larger heads take the vendor GEMM (caller)

// ---- the arithmetic, each expression once.  head_ce_kernel must give every bit of head_fwd_vec_kernel -> ce_fwd_kernel ->
// head_bwd_dx_kernel, and loss_mean_kernel every bit of ce_fwd_kernel's mean: they call the same functions.  The kernels own
// their data movement (what is loaded when, what stays in registers), these own the order of operations. ----

// Ordered block sum: lanes by wave_sum, waves in index order, one final scale, stored by thread 0.
template <int WAVES>
__device__ __forceinline__ void block_sum_store(float local, float scale, float* dst) {
    __shared__ float red[WAVES];
    const float w = wave_sum(local);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < WAVES; ++i) s += red[i];
        dst[0] = s * scale;
    }
}

// Pooled means and logit partials of a 256-thread image: add() per channel of a thread, finish() once.  w(k) = W[k][c] from wherever
// the caller keeps it.
struct Logits {
    float part[MAXK];
    __device__ __forceinline__ Logits() {
#pragma unroll
        for (int k = 0; k < MAXK; ++k) part[k] = 0.f;
    }
    // t = the channel's sum over the pixels: its mean goes to *pooled_c and into every class's partial
    template <class WF>
    __device__ __forceinline__ void add(float t, float inv, float* pooled_c, int K, WF w) {
        const float m = t * inv;
        *pooled_c = m;
#pragma unroll
        for (int k = 0; k < MAXK; ++k)
            if (k < K) part[k] = fmaf(m, w(k), part[k]);
    }
    // thread k < K: store(bias() + the waves' sums in index order)
    template <class BF, class SF>
    __device__ __forceinline__ void finish(int K, BF bias, SF store) {
        __shared__ float red[BLOCK / AFAN_WAVE][MAXK];
#pragma unroll
        for (int k = 0; k < MAXK; ++k) {
            const float v = wave_sum(part[k]);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
        }
        __syncthreads();
        if (threadIdx.x < K) {
            float t = bias();
            for (int w = 0; w < BLOCK / AFAN_WAVE; ++w) t += red[w][threadIdx.x];
            store(t);
        }
    }
};

// Vector pooling (bf16 channels-last, C % 8 == 0, 256 % (C / 8) == 0): thread (pg, pc) of G = 256 / (C/8) pixel groups adds the
// pixels p0, p0 + G, ... < HW of its 8-channel piece (xb points at it) onto s — zeros, or the sums of the sequence's earlier pixels —
// and leaves the group's sums at grp_row = &grp[pg][pc * 8]; group_sum() adds a channel's groups in index order.
__device__ __forceinline__ void add8(float (&s)[8], const u16x8& v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += bf2f(v[j]);
}
__device__ __forceinline__ void pool_group(float (&s)[8], const uint16_t* xb, int p0, int HW, int G, int C, float* grp_row) {
    for (int p = p0; p < HW; p += G) add8(s, *reinterpret_cast<const u16x8*>(xb + (int64_t)p * C));
#pragma unroll
    for (int j = 0; j < 8; ++j) grp_row[j] = s[j];
}
__device__ __forceinline__ float group_sum(const float* grp, int G, int C, int c) {
    float t = 0.f;
    for (int g = 0; g < G; ++g) t += grp[g * C + c];
    return t;
}

// Cross-entropy of one row of logits (nn.CrossEntropyLoss defaults): lse = max + log sum exp(l - max), loss = lse - l[target],
// dlogit(k) = (exp(l[k] - lse) - [k == target]) / N.  A target outside [0, K) — torch asserts there — poisons the row with NaN
// instead of reading out of range.
struct CeRow {
    float lse;
    bool bad;
    int t;
    __device__ __forceinline__ CeRow(float m, float s, int64_t t64, int K)
        : lse(m + logf(s)), bad(t64 < 0 || t64 >= K), t(bad ? 0 : (int)t64) {}
    // max and sum by one thread walking the row
    __device__ static __forceinline__ CeRow of(const float* l, int K, int64_t t64) {
        float m = l[0];
        for (int k = 1; k < K; ++k) m = fmaxf(m, l[k]);
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += expf(l[k] - m);
        return CeRow(m, s, t64, K);
    }
    __device__ __forceinline__ float loss(const float* l) const { return bad ? NAN : lse - l[t]; }
    __device__ __forceinline__ float dlogit(float lk, int k, float invn) const {
        return bad ? NAN : (expf(lk - lse) - (k == t ? 1.f : 0.f)) * invn;
    }
};

// Head input gradient of one channel, the same at every pixel of the image: (sum_k dl[k] * W[k][c]) / HW, rounded to T.  Two forms of
// the one chain: weights in memory (wc = &W[0][c]) walk k in a loop, weights in registers need the unrolled one.
template <typename T>
__device__ __forceinline__ T head_dx_round(float g, float inv) {
    g *= inv;
    T r;
    Elt<T>::st(&r, g);
    return r;
}
template <typename T>
__device__ __forceinline__ T head_dx_value(const float* dl, int K, float inv, const float* wc, int C) {
    float g = 0.f;
    for (int k = 0; k < K; ++k) g = fmaf(dl[k], wc[(int64_t)k * C], g);
    return head_dx_round<T>(g, inv);
}
template <typename T>
__device__ __forceinline__ T head_dx_value(const float* dl, int K, float inv, const float (&wr)[MAXK]) {
    float g = 0.f;
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
        if (k < K) g = fmaf(dl[k], wr[k], g);
    return head_dx_round<T>(g, inv);
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void head_fwd_kernel(const T* __restrict__ x, const float* __restrict__ W,
                                                         const float* __restrict__ bias, float* __restrict__ pooled,
                                                         float* __restrict__ logits, int C, int HW, int K) {
    const int b = blockIdx.x;
    const T* xb = x + (int64_t)b * HW * C;
    Logits lg;
    const float inv = 1.0f / (float)HW;
    for (int c = threadIdx.x; c < C; c += BLOCK) {
        float s = 0.f;
        for (int p = 0; p < HW; ++p) s += Elt<T>::ld(xb + (int64_t)p * C + c);
        lg.add(s, inv, pooled + (int64_t)b * C + c, K, [&](int k) { return W[(int64_t)k * C + c]; });
    }
    lg.finish(K, [&] { return bias ? bias[threadIdx.x] : 0.f; }, [&](float v) { logits[(int64_t)b * K + threadIdx.x] = v; });
}

// bf16 channels-last with C % 8 == 0 and 256 % (C / 8) == 0 (512 or 64 channels here): 16-byte loads, lanes along
// 8-channel pieces, 256 / (C/8) pixel groups side by side; groups and channels are summed in fixed order.
// (The scalar kernel above took 19.8 us at 512 channels x 16 pixels: 32 dependent 2-byte loads per thread.)
__global__ __launch_bounds__(BLOCK) void head_fwd_vec_kernel(const uint16_t* __restrict__ x, const float* __restrict__ W,
                                                             const float* __restrict__ bias, float* __restrict__ pooled,
                                                             float* __restrict__ logits, int C, int HW, int K) {
    __shared__ float grp[BLOCK * 8];                    // [G][C]
    const int b = blockIdx.x, P = C >> 3, G = BLOCK / P;
    const int pc = threadIdx.x % P, pg = threadIdx.x / P;
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.f;
    pool_group(s, x + (int64_t)b * HW * C + pc * 8, pg, HW, G, C, grp + pg * C + pc * 8);
    __syncthreads();
    Logits lg;
    const float inv = 1.0f / (float)HW;
    for (int c = threadIdx.x; c < C; c += BLOCK)
        lg.add(group_sum(grp, G, C, c), inv, pooled + (int64_t)b * C + c, K, [&](int k) { return W[(int64_t)k * C + c]; });
    lg.finish(K, [&] { return bias ? bias[threadIdx.x] : 0.f; }, [&](float v) { logits[(int64_t)b * K + threadIdx.x] = v; });
}

// dx: block per image, thread per channel
template <typename T>
__global__ __launch_bounds__(BLOCK) void head_bwd_dx_kernel(const float* __restrict__ dlogits, const float* __restrict__ W,
                                                            T* __restrict__ dx, int C, int HW, int K) {
    const int b = blockIdx.x;
    __shared__ float dl[MAXK];
    if (threadIdx.x < K) dl[threadIdx.x] = dlogits[(int64_t)b * K + threadIdx.x];
    __syncthreads();
    const float inv = 1.0f / (float)HW;
    T* xb = dx + (int64_t)b * HW * C;
    for (int c = threadIdx.x; c < C; c += BLOCK) {
        const T g = head_dx_value<T>(dl, K, inv, W + c, C);
        for (int p = 0; p < HW; ++p) xb[(int64_t)p * C + c] = g;
    }
}

// dW / db: 64 (k, c) columns x 16 batch slices per block; a slice walks its images in order, the 16 slice sums are added
// in fixed order (deterministic).  db = the K extra columns whose second factor is 1.  (A thread per column walking the
// whole batch took 148 us at batch 512: a 512-long dependent chain per thread on 20 blocks.)
constexpr int DW_SLICES = 16;
__global__ __launch_bounds__(64 * DW_SLICES) void head_bwd_dw_kernel(const float* __restrict__ dlogits,
                                                                    const float* __restrict__ pooled, float* __restrict__ dW,
                                                                    float* __restrict__ db, int B, int C, int K, int accumulate) {
    __shared__ float red[DW_SLICES][64];
    const int e = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 64 + e;
    const int64_t KC = (int64_t)K * C, total = KC + (db ? K : 0);
    float s = 0.f;
    if (i < KC) {
        const int k = (int)(i / C), c = (int)(i % C);
        for (int b = q; b < B; b += DW_SLICES) s = fmaf(dlogits[(int64_t)b * K + k], pooled[(int64_t)b * C + c], s);
    } else if (i < total) {
        const int k = (int)(i - KC);
        for (int b = q; b < B; b += DW_SLICES) s += dlogits[(int64_t)b * K + k];
    }
    red[q][e] = s;
    __syncthreads();
    if (q == 0 && i < total) {
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < DW_SLICES; ++j) sum += red[j][e];
        float* dst = i < KC ? dW + i : db + (i - KC);
        *dst = accumulate ? *dst + sum : sum;
    }
}

// Mean cross-entropy of the classifier's logits (nn.CrossEntropyLoss defaults: main_perturb.py:71, attack_algo.py:51) and
// its gradient in ONE launch: per row CeRow's loss and dlogits;  loss = (sum_r loss_r) / N, rows summed in fixed order.
// One block (N * K is a few thousand values here); in torch the same is log_softmax, nll_loss, a ones_like fill, two
// backward kernels and a zero fill — at the end of every tail pass, K + 2 times per iteration.
constexpr int CE_BLOCK = 256;
__global__ __launch_bounds__(CE_BLOCK) void ce_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                          float* __restrict__ loss, float* __restrict__ dlogits, int N, int K) {
    const float invn = 1.0f / (float)N;
    float local = 0.f;
    for (int r = threadIdx.x; r < N; r += CE_BLOCK) {
        const float* l = logits + (int64_t)r * K;
        const CeRow row = CeRow::of(l, K, target[r]);
        local += row.loss(l);
        float* d = dlogits + (int64_t)r * K;
        for (int k = 0; k < K; ++k) d[k] = row.dlogit(l[k], k, invn);
    }
    block_sum_store<CE_BLOCK / AFAN_WAVE>(local, invn, loss);
}

// Many classes (ImageNet-shape heads): one WAVE per row, lanes stride over the classes; the 16 waves of the single
// workgroup take rows w, w + 16, ...; row losses are summed per wave in row order (on lane 0, the other lanes add zeros) and
// the waves in index order (deterministic).  64 x 1000 logits: 313 us with the thread-per-row kernel above, ~10 us here.
constexpr int CEW_WAVES = 16;
__global__ __launch_bounds__(64 * CEW_WAVES) void ce_fwd_wide_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                     float* __restrict__ loss, float* __restrict__ dlogits, int N, int K) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float invn = 1.0f / (float)N;
    float local = 0.f;
    for (int r = w; r < N; r += CEW_WAVES) {
        const float* l = logits + (int64_t)r * K;
        float m = -INFINITY;
        for (int k = lane; k < K; k += 64) m = fmaxf(m, l[k]);
        m = wave_max(m);
        float s = 0.f;
        for (int k = lane; k < K; k += 64) s += expf(l[k] - m);
        s = wave_sum(s);
        const CeRow row(m, s, target[r], K);
        if (lane == 0) local += row.loss(l);
        float* d = dlogits + (int64_t)r * K;
        for (int k = lane; k < K; k += 64) d[k] = row.dlogit(l[k], k, invn);
    }
    block_sum_store<CEW_WAVES>(local, invn, loss);
}

// The end of a tail pass in ONE launch, 256 threads per image: everything between the last block's output and its last BatchNorm's
// backward sums is a function of the image's own out[b] and raw[b] —
//   pooled, logits          head_fwd_vec_kernel's: pool_group / group_sum, Logits;
//   loss_row, dlogits       ce_fwd_kernel's: CeRow (dlogits also times `root`, the pass's root gradient: 1 or 1/2, exact);
//   v[b][c]                 head_bwd_dx_kernel's: head_dx_value, once per image and not once per pixel;
//   SUMS (acc given)        the BatchNorm's sums, g = out > 0 ? v : 0:  sum g  and  sum g * (raw - mean), bwd_reduce_kernel's terms,
//                           added to the f64 accumulator block acc[slot][2][C] (slot = image % NS) that bwd_apply_acc_kernel folds.
//                           Without SUMS the BatchNorm's own reduce launch takes them from v, in its slab order, and this launch
//                           neither reads raw / stats nor holds anything for them.
// The first HCE_IT pixel iterations' out (SUMS: and raw) vectors stay in registers between the pooling and the sums (all of them at
// 512 channels x 16 pixels and at 64 channels x 64 pixels); further ones are read again.  The launch is one dependent chain per image,
// so every operand (the maps, the weights a thread uses twice, mean, target, bias) is requested before the first wait.
constexpr int HCE_IT = 4;
constexpr int HCE_WIT = 2;      // channel iterations (c = tid + it * 256) whose K weights stay in registers for the logits and for v
template <bool SUMS>
__global__ __launch_bounds__(BLOCK) void head_ce_kernel(const uint16_t* __restrict__ out, const uint16_t* __restrict__ raw,
                                                        const float* __restrict__ stats, const float* __restrict__ W,
                                                        const float* __restrict__ bias, const int64_t* __restrict__ target,
                                                        float root, float* __restrict__ pooled, float* __restrict__ logits,
                                                        float* __restrict__ loss_row, float* __restrict__ dlogits,
                                                        uint16_t* __restrict__ vrow, double* __restrict__ acc, int N, int C,
                                                        int HW, int K, int NS) {
    __shared__ float grp[(SUMS ? 3 : 1) * BLOCK * 8];   // pooling: [G][C]; SUMS: the sums [2][G][C], then v[b][.] as stored
    __shared__ float lg[MAXK], dl[MAXK];
    float* vs = grp + (SUMS ? 2 : 0) * BLOCK * 8;       // (SUMS only)
    const int b = blockIdx.x, tid = threadIdx.x;
    const int P = C >> 3, G = BLOCK / P;
    const int pc = tid % P, pg = tid / P;
    const int64_t base = (int64_t)b * HW * C + pc * 8;
    const uint16_t* xb = out + base;
    const uint16_t* rb = raw + base;
    // everything the image's chain reads from memory is asked for here, before the first wait
    u16x8 xo[HCE_IT], xr[HCE_IT];
#pragma unroll
    for (int it = 0; it < HCE_IT; ++it) {
        const int p = pg + it * G;
        if (p < HW) {
            xo[it] = *reinterpret_cast<const u16x8*>(xb + (int64_t)p * C);
            if (SUMS) xr[it] = *reinterpret_cast<const u16x8*>(rb + (int64_t)p * C);
        }
    }
    float wr[HCE_WIT][MAXK];
#pragma unroll
    for (int it = 0; it < HCE_WIT; ++it) {
        const int c = tid + it * BLOCK;
#pragma unroll
        for (int k = 0; k < MAXK; ++k) wr[it][k] = (c < C && k < K) ? W[(int64_t)k * C + c] : 0.f;
    }
    float mu[8];
    if (SUMS) {
#pragma unroll
        for (int j = 0; j < 8; ++j) mu[j] = stats[pc * 8 + j];
    }
    const int64_t t64 = target[b];
    const float bias_k = (tid < K && bias) ? bias[tid] : 0.f;
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.f;
#pragma unroll
    for (int it = 0; it < HCE_IT; ++it)
        if (pg + it * G < HW) add8(s, xo[it]);
    pool_group(s, xb, pg + HCE_IT * G, HW, G, C, grp + pg * C + pc * 8);
    __syncthreads();
    Logits part;
    const float inv = 1.0f / (float)HW;
#pragma unroll
    for (int it = 0; it < HCE_WIT; ++it) {
        const int c = tid + it * BLOCK;
        if (c < C) part.add(group_sum(grp, G, C, c), inv, pooled + (int64_t)b * C + c, K, [&](int k) { return wr[it][k]; });
    }
    for (int c = tid + HCE_WIT * BLOCK; c < C; c += BLOCK)
        part.add(group_sum(grp, G, C, c), inv, pooled + (int64_t)b * C + c, K, [&](int k) { return W[(int64_t)k * C + c]; });
    part.finish(K, [&] { return bias_k; }, [&](float v) { lg[tid] = logits[(int64_t)b * K + tid] = v; });
    __syncthreads();
    if (tid < AFAN_WAVE) {                              // the row's loss terms, every lane of the image's first wave for itself
        const CeRow row = CeRow::of(lg, K, t64);
        if (tid == 0) loss_row[b] = row.loss(lg);
        if (tid < K) dl[tid] = dlogits[(int64_t)b * K + tid] = row.dlogit(lg[tid], tid, 1.0f / (float)N) * root;
    }
    __syncthreads();
    auto vput = [&](int c, uint16_t u) {
        vrow[(int64_t)b * C + c] = u;
        if (SUMS) vs[c] = bf2f(u);
    };
#pragma unroll
    for (int it = 0; it < HCE_WIT; ++it) {
        const int c = tid + it * BLOCK;
        if (c < C) vput(c, head_dx_value<uint16_t>(dl, K, inv, wr[it]));
    }
    for (int c = tid + HCE_WIT * BLOCK; c < C; c += BLOCK)
        vput(c, head_dx_value<uint16_t>(dl, K, inv, W + c, C));
    if (!SUMS) return;
    __syncthreads();
    float vv[8], a0[8], a1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        vv[j] = vs[pc * 8 + j];
        a0[j] = a1[j] = 0.f;
    }
    auto add = [&](const u16x8& o, const u16x8& r) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float g = (bf2f(o[j]) > 0.f) ? vv[j] : 0.f;
            a0[j] += g;
            a1[j] += g * (bf2f(r[j]) - mu[j]);
        }
    };
#pragma unroll
    for (int it = 0; it < HCE_IT; ++it)
        if (pg + it * G < HW) add(xo[it], xr[it]);
    for (int p = pg + HCE_IT * G; p < HW; p += G)
        add(*reinterpret_cast<const u16x8*>(xb + (int64_t)p * C), *reinterpret_cast<const u16x8*>(rb + (int64_t)p * C));
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        grp[pg * C + pc * 8 + j] = a0[j];
        grp[BLOCK * 8 + pg * C + pc * 8 + j] = a1[j];
    }
    __syncthreads();
    double* dst = acc + (int64_t)(b & (NS - 1)) * 2 * C;
    for (int item = tid; item < 2 * C; item += BLOCK) {
        const int q = item / C, c = item - q * C;
        const float t = group_sum(grp + q * BLOCK * 8, G, C, c);
        if (t != 0.f) unsafeAtomicAdd(dst + (int64_t)q * C + c, (double)t);     // (an empty mask adds nothing)
    }
}

// The mean of head_ce_kernel's row losses where a pass consumes the loss value: ce_fwd_kernel's order (rows per thread, waves, block).
__global__ __launch_bounds__(CE_BLOCK) void loss_mean_kernel(const float* __restrict__ loss_row, float* __restrict__ loss, int N) {
    float local = 0.f;
    for (int r = threadIdx.x; r < N; r += CE_BLOCK) local += loss_row[r];
    block_sum_store<CE_BLOCK / AFAN_WAVE>(local, 1.0f / (float)N, loss);
}

}  // namespace

extern "C" {

int afan_head_max_classes(void) { return MAXK; }

int afan_head_ce(const void* out, const void* raw, int dtype, int64_t n, int64_t c, int64_t hw, const float* stats,
                 const float* weight, const float* bias, int64_t k, const int64_t* target, float root, float* pooled,
                 float* logits, float* loss_row, float* dlogits, void* v, double* acc, afan_stream_t stream) {
    if (dtype != AFAN_BF16) return AFAN_EDTYPE;
    if (n <= 0 || c <= 0 || hw <= 0 || hw > 64 || k <= 0 || k > MAXK || n * k > (1 << 16)) return AFAN_ESHAPE;
    if (c % 8 != 0 || c / 8 > BLOCK || BLOCK % (c / 8) != 0) return AFAN_ESHAPE;
    if (!out || !raw || !stats || !weight || !target || !pooled || !logits || !loss_row || !dlogits || !v) return AFAN_ENULL;
    if (!aligned(out, 16) || !aligned(raw, 16) || !aligned(v, 16) || !aligned(acc, 8)) return AFAN_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    AFAN_PROF("head_ce_kernel", (acc ? 4.0 : 2.0) * n * hw * c, st);        // out, with the sums also raw
    (acc ? head_ce_kernel<true> : head_ce_kernel<false>)<<<(unsigned)n, BLOCK, 0, st>>>(
        (const uint16_t*)out, (const uint16_t*)raw, stats, weight, bias, target, root, pooled, logits, loss_row, dlogits, (uint16_t*)v, acc,
        (int)n, (int)c, (int)hw, (int)k, afan_nhwc::acc_slot_count(c));
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

int afan_loss_mean(const float* loss_row, int64_t n, float* loss, afan_stream_t stream) {
    if (n <= 0 || n > (1 << 16)) return AFAN_ESHAPE;
    if (!loss_row || !loss) return AFAN_ENULL;
    hipStream_t st = (hipStream_t)stream;
    AFAN_PROF("loss_mean_kernel", 4.0 * n, st);
    loss_mean_kernel<<<1, CE_BLOCK, 0, st>>>(loss_row, loss, (int)n);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

int afan_head_forward(const void* x, int dtype, int64_t n, int64_t c, int64_t hw, const float* weight, const float* bias,
                      int64_t k, float* pooled, float* logits, afan_stream_t stream) {
    if (dtype != AFAN_F32 && dtype != AFAN_BF16) return AFAN_EDTYPE;
    if (n <= 0 || c <= 0 || hw <= 0 || k <= 0 || k > MAXK) return AFAN_ESHAPE;
    if (!x || !weight || !pooled || !logits) return AFAN_ENULL;
    hipStream_t st = (hipStream_t)stream;
    AFAN_PROF("head_fwd_kernel", (double)n * hw * c * (dtype == AFAN_F32 ? 4 : 2), st);
    if (dtype == AFAN_F32)
        head_fwd_kernel<float><<<(unsigned)n, BLOCK, 0, st>>>((const float*)x, weight, bias, pooled, logits, (int)c, (int)hw, (int)k);
    else if (c % 8 == 0 && c / 8 <= BLOCK && BLOCK % (c / 8) == 0 && aligned(x, 16))
        head_fwd_vec_kernel<<<(unsigned)n, BLOCK, 0, st>>>((const uint16_t*)x, weight, bias, pooled, logits, (int)c, (int)hw, (int)k);
    else
        head_fwd_kernel<uint16_t><<<(unsigned)n, BLOCK, 0, st>>>((const uint16_t*)x, weight, bias, pooled, logits, (int)c, (int)hw, (int)k);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

int afan_head_backward(const float* dlogits, const float* weight, const float* pooled, int64_t n, int64_t c, int64_t hw,
                       int64_t k, void* dx, int dx_dtype, float* dweight, float* dbias, int accumulate,
                       afan_stream_t stream) {
    if (dx && dx_dtype != AFAN_F32 && dx_dtype != AFAN_BF16) return AFAN_EDTYPE;
    if (n <= 0 || c <= 0 || hw <= 0 || k <= 0 || k > MAXK) return AFAN_ESHAPE;
    if (!dlogits || !weight || !pooled) return AFAN_ENULL;
    hipStream_t st = (hipStream_t)stream;
    if (dx) {
        AFAN_PROF("head_bwd_dx_kernel", (double)n * hw * c * (dx_dtype == AFAN_F32 ? 4 : 2), st);
        if (dx_dtype == AFAN_F32)
            head_bwd_dx_kernel<float><<<(unsigned)n, BLOCK, 0, st>>>(dlogits, weight, (float*)dx, (int)c, (int)hw, (int)k);
        else
            head_bwd_dx_kernel<uint16_t><<<(unsigned)n, BLOCK, 0, st>>>(dlogits, weight, (uint16_t*)dx, (int)c, (int)hw, (int)k);
        AFAN_LAUNCH_CHECK();
    }
    if (dweight) {
        AFAN_PROF("head_bwd_dw_kernel", 4.0 * n * (c + k), st);
        const unsigned grid = (unsigned)((k * c + (dbias ? k : 0) + 63) / 64);
        head_bwd_dw_kernel<<<grid, 64 * DW_SLICES, 0, st>>>(dlogits, pooled, dweight, dbias, (int)n, (int)c, (int)k, accumulate);
        AFAN_LAUNCH_CHECK();
    }
    return AFAN_OK;
}

int afan_cross_entropy(const float* logits, const int64_t* target, int64_t n, int64_t k, float* loss, float* dlogits,
                       afan_stream_t stream) {
    if (n <= 0 || k <= 0 || n * k > (1 << 16)) return AFAN_ESHAPE;        // one block; larger heads stay with the caller
    if (!logits || !target || !loss || !dlogits) return AFAN_ENULL;
    hipStream_t st = (hipStream_t)stream;
    AFAN_PROF("ce_fwd_kernel", 8.0 * n * k, st);
    if (k >= 64) ce_fwd_wide_kernel<<<1, 64 * CEW_WAVES, 0, st>>>(logits, target, loss, dlogits, (int)n, (int)k);
    else ce_fwd_kernel<<<1, CE_BLOCK, 0, st>>>(logits, target, loss, dlogits, (int)n, (int)k);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

}  // extern "C"
