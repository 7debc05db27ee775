// PGD feature-ascent kernels for gfx950: sign-step (+ L-inf projection) fused with the per-sample
// perturbation norms and the bf16 shadow copy; the image attacks' last step with the clamp to scalar bounds in the
// same launch (Detection/attack_algo.py:171-177); host-noise random start; device-drawn random start (Philox4x32-10);
// the L2 step: per-sample normalised gradient step + projection onto the L2 ball, three launches with deterministic sums.
// Reference behaviour restated (not translated) from Classification/attack_algo.py:9-19,35-36,41-56
// and Classification/main_perturb.py:188-192.  All of these are HBM-bound streaming kernels:
// 16 B per lane per access, grid-stride, >= 2048 workgroups when the tensor allows it.
#include "afan_common.h"

using namespace afan;

namespace {

constexpr int BLOCK = 256;
constexpr int NORM_CHUNK = 4096;  // elements of one sample handled by one workgroup in the norms kernels

__device__ __forceinline__ float sign_of(float g) {
    // torch.sign: 0 -> 0, NaN -> NaN
    return (g != g) ? g : (float)((g > 0.f) - (g < 0.f));
}

// attack_algo.py:9-19 on one element: two compares in its order (NaN compares false and passes through; -0 stays -0 against +0)
__device__ __forceinline__ float clamp_one(float t, float lo, float hi) {
    if (t < lo) t = lo;  // attack_algo.py:14-15
    if (t > hi) t = hi;  // attack_algo.py:16-17
    return t;
}

template <bool CLIP>
__device__ __forceinline__ float project_one(float t, float xc, float eps) {
    // attack_algo.py:36 materialises centre-radius / centre+radius first
    return CLIP ? clamp_one(t, xc - eps, xc + eps) : t;
}

template <bool CLIP>
__device__ __forceinline__ float step_one(float xa, float g, float xc, float gamma, float eps) {
    float d = gamma * sign_of(g);  // exact: +-gamma, 0 or NaN
    float t = xa + d;              // the single rounding of attack_algo.py:53
    return project_one<CLIP>(t, xc, eps);
}

// the last step of an image attack: step_one (STEP; else the iterate as it stands, steps = 0), then the clamp to [lo, hi]
template <bool STEP, bool CLIP>
__device__ __forceinline__ float step_clamp_one(float xa, float g, float xc, float gamma, float eps, float lo, float hi) {
    const float t = STEP ? step_one<CLIP>(xa, g, xc, gamma, eps) : project_one<CLIP>(xa, xc, eps);
    return clamp_one(t, lo, hi);
}

template <typename G> struct GradVec4;
template <> struct GradVec4<float> {
    __device__ static __forceinline__ void ld(const float* p, float (&g)[4]) { Elt<float>::ldv(p, g); }
};
template <> struct GradVec4<uint16_t> {
    __device__ static __forceinline__ void ld(const uint16_t* p, float (&g)[4]) {
        u16x4 t = *reinterpret_cast<const u16x4*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = bf2f(t[i]);
    }
};

// ---- plain step ---------------------------------------------------------------------------------
template <typename G, bool CLIP, bool SHADOW, bool VEC>
__global__ __launch_bounds__(BLOCK) void pgd_step_kernel(float* __restrict__ x_adv,
                                                         const G* __restrict__ grad,
                                                         const float* __restrict__ x_clean,
                                                         uint16_t* __restrict__ shadow, int64_t n,
                                                         float gamma, float eps) {
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * BLOCK;
    if (VEC) {
        const int64_t nvec = n >> 2;
        for (int64_t v = tid; v < nvec; v += nthreads) {
            const int64_t i = v << 2;
            float xa[4], g[4], xc[4] = {0.f, 0.f, 0.f, 0.f};
            Elt<float>::ldv(x_adv + i, xa);
            GradVec4<G>::ld(grad + i, g);
            if (CLIP) Elt<float>::ldv(x_clean + i, xc);
#pragma unroll
            for (int k = 0; k < 4; ++k) xa[k] = step_one<CLIP>(xa[k], g[k], xc[k], gamma, eps);
            Elt<float>::stv(x_adv + i, xa);
            if (SHADOW) {
                u16x4 s;
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = f2bf(xa[k]);
                *reinterpret_cast<u16x4*>(shadow + i) = s;
            }
        }
        // ragged tail (n % 4 elements)
        const int64_t i = (nvec << 2) + tid;
        if (i < n) {
            float t = step_one<CLIP>(x_adv[i], Elt<G>::ld(grad + i), CLIP ? x_clean[i] : 0.f, gamma, eps);
            x_adv[i] = t;
            if (SHADOW) shadow[i] = f2bf(t);
        }
    } else {
        for (int64_t i = tid; i < n; i += nthreads) {
            float t = step_one<CLIP>(x_adv[i], Elt<G>::ld(grad + i), CLIP ? x_clean[i] : 0.f, gamma, eps);
            x_adv[i] = t;
            if (SHADOW) shadow[i] = f2bf(t);
        }
    }
}

// ---- the last step with scalar bounds: pgd_step_kernel's body with two more compares (STEP = false: no gradient is read) --------
template <typename G, bool STEP, bool CLIP, bool SHADOW, bool VEC>
__global__ __launch_bounds__(BLOCK) void pgd_step_clamp_kernel(float* __restrict__ x_adv,
                                                               const G* __restrict__ grad,
                                                               const float* __restrict__ x_clean,
                                                               uint16_t* __restrict__ shadow, int64_t n,
                                                               float gamma, float eps, float lo, float hi) {
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * BLOCK;
    if (VEC) {
        const int64_t nvec = n >> 2;
        for (int64_t v = tid; v < nvec; v += nthreads) {
            const int64_t i = v << 2;
            float xa[4], g[4] = {0.f, 0.f, 0.f, 0.f}, xc[4] = {0.f, 0.f, 0.f, 0.f};
            Elt<float>::ldv(x_adv + i, xa);
            if (STEP) GradVec4<G>::ld(grad + i, g);
            if (CLIP) Elt<float>::ldv(x_clean + i, xc);
#pragma unroll
            for (int k = 0; k < 4; ++k) xa[k] = step_clamp_one<STEP, CLIP>(xa[k], g[k], xc[k], gamma, eps, lo, hi);
            Elt<float>::stv(x_adv + i, xa);
            if (SHADOW) {
                u16x4 s;
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = f2bf(xa[k]);
                *reinterpret_cast<u16x4*>(shadow + i) = s;
            }
        }
        // ragged tail (n % 4 elements)
        const int64_t i = (nvec << 2) + tid;
        if (i < n) {
            float t = step_clamp_one<STEP, CLIP>(x_adv[i], STEP ? Elt<G>::ld(grad + i) : 0.f, CLIP ? x_clean[i] : 0.f, gamma, eps, lo, hi);
            x_adv[i] = t;
            if (SHADOW) shadow[i] = f2bf(t);
        }
    } else {
        for (int64_t i = tid; i < n; i += nthreads) {
            float t = step_clamp_one<STEP, CLIP>(x_adv[i], STEP ? Elt<G>::ld(grad + i) : 0.f, CLIP ? x_clean[i] : 0.f, gamma, eps, lo, hi);
            x_adv[i] = t;
            if (SHADOW) shadow[i] = f2bf(t);
        }
    }
}

// ---- block reduction of (sum of squares, max abs) into one partial per workgroup ----------------
__device__ __forceinline__ void block_reduce_store(float ss, float mx, float* __restrict__ partial,
                                                   int64_t slot) {
    __shared__ float s_ss[BLOCK / AFAN_WAVE];
    __shared__ float s_mx[BLOCK / AFAN_WAVE];
    ss = wave_sum(ss);
    // fmaxf drops NaNs: carry "saw a NaN" separately so the max stays NaN-propagating like torch.norm(p=inf)
    const float nanflag = wave_max((mx != mx) ? 1.f : 0.f);
    mx = wave_max((mx != mx) ? 0.f : mx);
    if (nanflag > 0.f) mx = __builtin_nanf("");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        s_ss[w] = ss;
        s_mx[w] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int k = 0; k < BLOCK / AFAN_WAVE; ++k) {
            a += s_ss[k];
            b = (b != b || s_mx[k] != s_mx[k]) ? __builtin_nanf("") : fmaxf(b, s_mx[k]);
        }
        partial[2 * slot] = a;
        partial[2 * slot + 1] = b;
    }
}

// NaN-propagating |d| max (torch.norm(p=inf) returns NaN if any element is NaN)
__device__ __forceinline__ float absmax_nan(float m, float d) {
    float a = fabsf(d);
    return (a != a || m != m) ? __builtin_nanf("") : fmaxf(m, a);
}

// grid = (slices, batch): workgroup (s, b) owns elements [s*NORM_CHUNK, (s+1)*NORM_CHUNK) of sample b.
template <typename G, bool CLIP, bool SHADOW, bool VEC, bool STEP>
__global__ __launch_bounds__(BLOCK) void pgd_step_norms_kernel(
    float* __restrict__ x_adv, const G* __restrict__ grad, const float* __restrict__ x_clean,
    uint16_t* __restrict__ shadow, int64_t per_sample, float gamma, float eps,
    float* __restrict__ partial) {
    const int64_t b = blockIdx.y;
    const int64_t base = b * per_sample;
    const int64_t lo = (int64_t)blockIdx.x * NORM_CHUNK;
    const int64_t hi = (lo + NORM_CHUNK < per_sample) ? lo + NORM_CHUNK : per_sample;
    float ss = 0.f, mx = 0.f;
    if (VEC) {  // per_sample % 4 == 0 and 16-byte aligned bases
        for (int64_t j = lo + (int64_t)threadIdx.x * 4; j < hi; j += BLOCK * 4) {
            const int64_t i = base + j;
            float xa[4], xc[4], g[4];
            Elt<float>::ldv(x_adv + i, xa);
            Elt<float>::ldv(x_clean + i, xc);
            if (STEP) {
                GradVec4<G>::ld(grad + i, g);
#pragma unroll
                for (int k = 0; k < 4; ++k) xa[k] = step_one<CLIP>(xa[k], g[k], xc[k], gamma, eps);
                Elt<float>::stv(x_adv + i, xa);
                if (SHADOW) {
                    u16x4 s;
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[k] = f2bf(xa[k]);
                    *reinterpret_cast<u16x4*>(shadow + i) = s;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float d = xa[k] - xc[k];  // main_perturb.py:189
                ss += d * d;
                mx = absmax_nan(mx, d);
            }
        }
    } else {
        for (int64_t j = lo + threadIdx.x; j < hi; j += BLOCK) {
            const int64_t i = base + j;
            float xa = x_adv[i], xc = x_clean[i];
            if (STEP) {
                xa = step_one<CLIP>(xa, Elt<G>::ld(grad + i), xc, gamma, eps);
                x_adv[i] = xa;
                if (SHADOW) shadow[i] = f2bf(xa);
            }
            float d = xa - xc;
            ss += d * d;
            mx = absmax_nan(mx, d);
        }
    }
    block_reduce_store(ss, mx, partial, b * gridDim.x + blockIdx.x);
}

// one wave per sample: fold the per-slice partials, L2 = sqrt(sum), Linf = max
__global__ __launch_bounds__(AFAN_WAVE) void norms_finalize_kernel(const float* __restrict__ partial,
                                                                   int slices, float* __restrict__ l2,
                                                                   float* __restrict__ linf) {
    const int64_t b = blockIdx.x;
    float ss = 0.f, mx = 0.f;
    for (int s = threadIdx.x; s < slices; s += AFAN_WAVE) {
        ss += partial[2 * (b * slices + s)];
        float m = partial[2 * (b * slices + s) + 1];
        mx = (m != m || mx != mx) ? __builtin_nanf("") : fmaxf(mx, m);
    }
    ss = wave_sum(ss);
    // NaN-aware wave max
    float isn = (mx != mx) ? 1.f : 0.f;
    isn = wave_max(isn);
    mx = wave_max((mx != mx) ? 0.f : mx);
    if (threadIdx.x == 0) {
        l2[b] = sqrtf(ss);
        linf[b] = (isn > 0.f) ? __builtin_nanf("") : mx;
    }
}

__global__ __launch_bounds__(BLOCK) void axpy_noise_kernel(float* __restrict__ x_adv,
                                                           const float* __restrict__ u, int64_t n,
                                                           float eps, uint16_t* __restrict__ shadow,
                                                           int vec) {
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * BLOCK;
    int64_t done = 0;
    if (vec) {
        const int64_t nvec = n >> 2;
        for (int64_t v = tid; v < nvec; v += nthreads) {
            const int64_t i = v << 2;
            float xa[4], uu[4];
            Elt<float>::ldv(x_adv + i, xa);
            Elt<float>::ldv(u + i, uu);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float t = 2.0f * uu[k];  // attack_algo.py:44, each op rounded on its own
                t = t - 1.0f;
                t = t * eps;
                xa[k] = xa[k] + t;
            }
            Elt<float>::stv(x_adv + i, xa);
            if (shadow) {
                u16x4 s;
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = f2bf(xa[k]);
                *reinterpret_cast<u16x4*>(shadow + i) = s;
            }
        }
        done = nvec << 2;
    }
    for (int64_t i = done + tid; i < n; i += nthreads) {
        float t = 2.0f * u[i];
        t = t - 1.0f;
        t = t * eps;
        t = x_adv[i] + t;
        x_adv[i] = t;
        if (shadow) shadow[i] = f2bf(t);
    }
}

// ---- device-drawn random start ----------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter (q, 0) with q = e >> 2 the
// element's block of four LOGICAL (NCHW) indices, key = the two halves of the seed, output word e & 3.
__device__ __forceinline__ void philox4x32_10(uint64_t q, uint64_t seed, uint32_t (&o)[4]) {
    uint32_t c0 = (uint32_t)q, c1 = (uint32_t)(q >> 32), c2 = 0u, c3 = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

__device__ __forceinline__ float rand_start_one(float x, uint32_t word, float eps) {
    const float u = (float)(word >> 8) * 5.9604644775390625e-08f;  // 24 bits * 2^-24: exact, in [0, 1)
    float t = 2.0f * u;  // afan_axpy_noise's roundings: each operation on its own, one add, no FMA
    t = t - 1.0f;
    t = t * eps;
    return x + t;
}

// One lane per four consecutive elements IN MEMORY (one 16-byte load, one 16-byte store, one 8-byte shadow store).  NHWC = false:
// memory order is logical order, the four share one Philox block.  NHWC = true: each element's logical index is rebuilt from its
// (pixel, channel) position — a block per element, four times the integer work of a kernel that stays bound by its 8 (10) bytes per
// element.  I: the index type of that decomposition (32-bit while the tensor allows it: 64-bit divisions cost tens of instructions).
template <bool NHWC, typename I>
__global__ __launch_bounds__(BLOCK) void pgd_rand_start_kernel(const float* __restrict__ x, float* __restrict__ x_adv,
                                                               uint16_t* __restrict__ shadow, int64_t total, int64_t c,
                                                               int64_t hw, float eps, const uint64_t* __restrict__ state,
                                                               uint64_t* __restrict__ used) {
    const uint64_t seed = state[0];
    if (used && used != state && blockIdx.x == 0 && threadIdx.x == 0) used[0] = seed;
    const int64_t nthreads = (int64_t)gridDim.x * BLOCK;
    for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; (v << 2) < total; v += nthreads) {
        const int64_t i = v << 2;
        uint32_t word[4];
        if (!NHWC) {
            uint32_t o[4];
            philox4x32_10((uint64_t)v, seed, o);
#pragma unroll
            for (int k = 0; k < 4; ++k) word[k] = o[k];
        } else {
            const I C = (I)c, HW = (I)hw;
            I pix = (I)i / C, ch = (I)i - pix * C;   // memory index i = (img * HW + p) * C + ch
            I img = pix / HW, p = pix - img * HW;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t e = ((uint64_t)img * (uint64_t)c + (uint64_t)ch) * (uint64_t)hw + (uint64_t)p;
                uint32_t o[4];
                philox4x32_10(e >> 2, seed, o);
                const uint32_t s = (uint32_t)e & 3u;
                word[k] = s == 0 ? o[0] : s == 1 ? o[1] : s == 2 ? o[2] : o[3];
                if (++ch == C) {
                    ch = 0;
                    if (++p == HW) { p = 0; ++img; }
                }
            }
        }
        if (i + 4 <= total) {
            float xa[4];
            Elt<float>::ldv(x + i, xa);
#pragma unroll
            for (int k = 0; k < 4; ++k) xa[k] = rand_start_one(xa[k], word[k], eps);
            Elt<float>::stv(x_adv + i, xa);
            if (shadow) {
                u16x4 s;
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = f2bf(xa[k]);
                *reinterpret_cast<u16x4*>(shadow + i) = s;
            }
        } else {  // ragged tail: total % 4 elements, by the one lane that owns them
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i + k < total) {
                    const float t = rand_start_one(x[i + k], word[k], eps);
                    x_adv[i + k] = t;
                    if (shadow) shadow[i + k] = f2bf(t);
                }
            }
        }
    }
}

// the generator's step, afan_seg.hip's dropout_advance_kernel: one lane, after the draw on the same stream
__global__ void noise_advance_kernel(uint64_t* state) { state[0] = state[0] * 6364136223846793005ull + 1442695040888963407ull; }

// attack_algo.py:9-19 with arbitrary bound tensors
__global__ __launch_bounds__(BLOCK) void tensor_clamp_kernel(float* __restrict__ t, const float* __restrict__ lo,
                                                             const float* __restrict__ hi, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        float v = t[i];
        const float l = lo[i], h = hi[i];
        if (v < l) v = l;
        if (v > h) v = h;
        t[i] = v;
    }
}

__global__ __launch_bounds__(BLOCK) void cast_bf16_kernel(const float* __restrict__ src,
                                                          uint16_t* __restrict__ dst, int64_t n, int vec) {
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * BLOCK;
    int64_t done = 0;
    if (vec) {
        const int64_t nvec = n >> 3;
        for (int64_t v = tid; v < nvec; v += nthreads) {
            const int64_t i = v << 3;
            float a[4], b[4];
            Elt<float>::ldv(src + i, a);
            Elt<float>::ldv(src + i + 4, b);
            float o[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
            Elt<uint16_t>::stv(dst + i, o);
        }
        done = nvec << 3;
    }
    for (int64_t i = done + tid; i < n; i += nthreads) dst[i] = f2bf(src[i]);
}


// PGD's start (attack_algo.py:41 `x_adv = x.clone()` on the product's bf16 feature map): x in bf16 or fp32 -> the fp32
// reference copy x32 (the centre of the L-inf ball and of the norms; nullable when x is fp32 already), the fp32 iterate
// x_adv, and optionally its bf16 shadow — one pass instead of .float(), .clone() and a cast.
template <typename S>
__global__ __launch_bounds__(BLOCK) void pgd_init_kernel(const S* __restrict__ x, float* __restrict__ x32,
                                                         float* __restrict__ x_adv, uint16_t* __restrict__ shadow, int64_t n, int vec) {
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * BLOCK;
    int64_t done = 0;
    if (vec) {
        const int64_t nvec = n >> 3;
        for (int64_t v = tid; v < nvec; v += nthreads) {
            const int64_t i = v << 3;
            float o[8];
            if constexpr (sizeof(S) == 4) {
                float a[4], b[4];
                Elt<float>::ldv((const float*)x + i, a);
                Elt<float>::ldv((const float*)x + i + 4, b);
#pragma unroll
                for (int e = 0; e < 4; ++e) { o[e] = a[e]; o[4 + e] = b[e]; }
            } else {
                Elt<uint16_t>::ldv((const uint16_t*)x + i, o);
            }
            const float lo[4] = {o[0], o[1], o[2], o[3]}, hi[4] = {o[4], o[5], o[6], o[7]};
            if (x32) { Elt<float>::stv(x32 + i, lo); Elt<float>::stv(x32 + i + 4, hi); }
            Elt<float>::stv(x_adv + i, lo);
            Elt<float>::stv(x_adv + i + 4, hi);
            if (shadow) Elt<uint16_t>::stv(shadow + i, o);
        }
        done = nvec << 3;
    }
    for (int64_t i = done + tid; i < n; i += nthreads) {
        const float v = Elt<S>::ld(x + i);
        if (x32) x32[i] = v;
        x_adv[i] = v;
        if (shadow) shadow[i] = f2bf(v);
    }
}

// ---- L2 step: normalised gradient step + projection onto the L2 ball (afan_hip.h states the arithmetic) ---------------------------
// Workgroup blk = b * chunks + c owns elements [c * L2_CHUNK, (c + 1) * L2_CHUNK) of sample b.  Three launches: the partial sums of
// g^2 (4 B/elt); the step, the shadow and the partial sums of d^2 (18 B/elt); the projection of the samples outside the ball
// (14 B/elt of those).  A sample's partials are added again by every workgroup of the next launch, in one fixed order.
constexpr int L2_CHUNK = 4096;

// the block's sum, the same bits in every thread: butterfly, then the 4 wave sums in order
__device__ __forceinline__ float block_sum_all(float v) {
    __shared__ float s_w[BLOCK / AFAN_WAVE];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < BLOCK / AFAN_WAVE; ++k) a += s_w[k];
    __syncthreads();  // (the next call writes s_w again)
    return a;
}

__device__ __forceinline__ float sample_sum(const float* __restrict__ part, int chunks) {
    float t = 0.f;
    for (int i = threadIdx.x; i < chunks; i += BLOCK) t += part[i];
    return block_sum_all(t);
}

template <typename G, bool VEC>
__global__ __launch_bounds__(BLOCK) void l2_grad_ss_kernel(const G* __restrict__ grad, int64_t per_sample, int chunks,
                                                           float* __restrict__ gpart) {
    constexpr int W = Elt<G>::VEC;
    const int64_t b = blockIdx.x / chunks, c = blockIdx.x - b * chunks;
    const int64_t base = b * per_sample, lo = c * L2_CHUNK;
    const int64_t hi = (lo + L2_CHUNK < per_sample) ? lo + L2_CHUNK : per_sample;
    float ss = 0.f;
    if (VEC) {  // per_sample % W == 0 and a 16-byte aligned base
        for (int64_t j = lo + (int64_t)threadIdx.x * W; j < hi; j += BLOCK * W) {
            float g[W];
            Elt<G>::ldv(grad + base + j, g);
#pragma unroll
            for (int k = 0; k < W; ++k) ss += g[k] * g[k];
        }
    } else {
        for (int64_t j = lo + threadIdx.x; j < hi; j += BLOCK) {
            const float g = Elt<G>::ld(grad + base + j);
            ss += g * g;
        }
    }
    ss = block_sum_all(ss);
    if (threadIdx.x == 0) gpart[blockIdx.x] = ss;
}

// STEP: there is a gradient.  DIST: x_clean is read and the partial sums of d^2 are written.
template <typename G, bool STEP, bool DIST, bool SHADOW, bool VEC>
__global__ __launch_bounds__(BLOCK) void l2_step_kernel(float* __restrict__ x_adv, const G* __restrict__ grad,
                                                        const float* __restrict__ x_clean, uint16_t* __restrict__ shadow,
                                                        int64_t per_sample, int chunks, float gamma,
                                                        const float* __restrict__ gpart, float* __restrict__ dpart,
                                                        float* __restrict__ gnorm_out) {
    constexpr int W = Elt<G>::VEC;
    const int64_t b = blockIdx.x / chunks, c = blockIdx.x - b * chunks;
    const int64_t base = b * per_sample, lo = c * L2_CHUNK;
    const int64_t hi = (lo + L2_CHUNK < per_sample) ? lo + L2_CHUNK : per_sample;
    float a = 0.f, ng = 0.f;
    bool skip = true;
    if (STEP) {
        ng = sqrtf(sample_sum(gpart + b * chunks, chunks));
        skip = ng == 0.f;  // (a NaN norm is not zero: the sample becomes NaN)
        a = gamma / ng;
    }
    if (gnorm_out && c == 0 && threadIdx.x == 0) gnorm_out[b] = ng;
    float ss = 0.f;
    if (VEC) {
        for (int64_t j = lo + (int64_t)threadIdx.x * W; j < hi; j += BLOCK * W) {
            const int64_t i = base + j;
            float g[W];
            if (STEP) Elt<G>::ldv(grad + i, g);
#pragma unroll
            for (int q = 0; q < W; q += 4) {
                float xa[4], xc[4];
                Elt<float>::ldv(x_adv + i + q, xa);
                if (DIST) Elt<float>::ldv(x_clean + i + q, xc);
                if (STEP) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float p = a * g[q + k];
                        xa[k] = skip ? xa[k] : xa[k] + p;
                    }
                    Elt<float>::stv(x_adv + i + q, xa);
                }
                if (SHADOW) {
                    u16x4 s;
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[k] = f2bf(xa[k]);
                    *reinterpret_cast<u16x4*>(shadow + i + q) = s;
                }
                if (DIST) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float d = xa[k] - xc[k];
                        ss += d * d;
                    }
                }
            }
        }
    } else {
        for (int64_t j = lo + threadIdx.x; j < hi; j += BLOCK) {
            const int64_t i = base + j;
            float xa = x_adv[i];
            if (STEP) {
                const float p = a * Elt<G>::ld(grad + i);
                xa = skip ? xa : xa + p;
                x_adv[i] = xa;
            }
            if (SHADOW) shadow[i] = f2bf(xa);
            if (DIST) {
                const float d = xa - x_clean[i];
                ss += d * d;
            }
        }
    }
    if (DIST) {
        ss = block_sum_all(ss);
        if (threadIdx.x == 0) dpart[blockIdx.x] = ss;
    }
}

// The workgroups of a sample inside the ball (nd <= eps, or nd = NaN) return at once: launch 2 wrote its final values and shadow.
template <bool SHADOW, bool VEC>
__global__ __launch_bounds__(BLOCK) void l2_project_kernel(float* __restrict__ x_adv, const float* __restrict__ x_clean,
                                                           uint16_t* __restrict__ shadow, int64_t per_sample, int chunks,
                                                           float eps, const float* __restrict__ dpart,
                                                           float* __restrict__ dnorm_out) {
    const int64_t b = blockIdx.x / chunks, c = blockIdx.x - b * chunks;
    const float nd = sqrtf(sample_sum(dpart + b * chunks, chunks));
    const bool outside = nd > eps;
    if (dnorm_out && c == 0 && threadIdx.x == 0) dnorm_out[b] = outside ? eps : nd;
    if (!outside) return;
    const float s = eps / nd;
    const int64_t base = b * per_sample, lo = c * L2_CHUNK;
    const int64_t hi = (lo + L2_CHUNK < per_sample) ? lo + L2_CHUNK : per_sample;
    if (VEC) {
        for (int64_t j = lo + (int64_t)threadIdx.x * 4; j < hi; j += BLOCK * 4) {
            const int64_t i = base + j;
            float xa[4], xc[4];
            Elt<float>::ldv(x_adv + i, xa);
            Elt<float>::ldv(x_clean + i, xc);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = xa[k] - xc[k];
                const float q = d * s;
                xa[k] = xc[k] + q;
            }
            Elt<float>::stv(x_adv + i, xa);
            if (SHADOW) {
                u16x4 sh;
#pragma unroll
                for (int k = 0; k < 4; ++k) sh[k] = f2bf(xa[k]);
                *reinterpret_cast<u16x4*>(shadow + i) = sh;
            }
        }
    } else {
        for (int64_t j = lo + threadIdx.x; j < hi; j += BLOCK) {
            const int64_t i = base + j;
            const float xc = x_clean[i];
            const float d = x_adv[i] - xc;
            const float q = d * s;
            const float t = xc + q;
            x_adv[i] = t;
            if (SHADOW) shadow[i] = f2bf(t);
        }
    }
}

template <typename G, bool STEP>
int launch_step_l2(float* x_adv, const void* grad, const float* x_clean, uint16_t* shadow, int64_t batch, int64_t per_sample,
                   int chunks, float gamma, float eps, bool dist, float* ws, float* gnorm, float* dnorm, hipStream_t st) {
    constexpr int W = Elt<G>::VEC;
    const unsigned grid = (unsigned)(batch * chunks);
    const double elts = (double)batch * (double)per_sample;
    float* gpart = ws;
    float* dpart = ws + (int64_t)grid;
    const bool xvec = aligned(x_adv, 16) && (!dist || aligned(x_clean, 16)) && (!shadow || aligned(shadow, 8));
    const bool gvec = !STEP || (per_sample % W == 0 && aligned(grad, 16));
    if (STEP) {
        AFAN_PROF("l2_grad_ss_kernel", elts * sizeof(G), st);
        if (gvec) l2_grad_ss_kernel<G, true><<<grid, BLOCK, 0, st>>>((const G*)grad, per_sample, chunks, gpart);
        else l2_grad_ss_kernel<G, false><<<grid, BLOCK, 0, st>>>((const G*)grad, per_sample, chunks, gpart);
        AFAN_LAUNCH_CHECK();
    }
    {
        const bool vec = xvec && gvec && per_sample % W == 0;
        AFAN_PROF("l2_step_kernel", elts * (4.0 + (STEP ? 4.0 + sizeof(G) : 0.0) + (dist ? 4 : 0) + (shadow ? 2 : 0)), st);
#define AFAN_L2(DIST, SHADOW)                                                                                                     \
    if (vec) l2_step_kernel<G, STEP, DIST, SHADOW, true><<<grid, BLOCK, 0, st>>>(x_adv, (const G*)grad, x_clean, shadow, per_sample, \
                                                                                  chunks, gamma, gpart, dpart, gnorm);             \
    else l2_step_kernel<G, STEP, DIST, SHADOW, false><<<grid, BLOCK, 0, st>>>(x_adv, (const G*)grad, x_clean, shadow, per_sample,   \
                                                                               chunks, gamma, gpart, dpart, gnorm);
        if (dist) { if (shadow) { AFAN_L2(true, true) } else { AFAN_L2(true, false) } }
        else { if (shadow) { AFAN_L2(false, true) } else { AFAN_L2(false, false) } }
#undef AFAN_L2
        AFAN_LAUNCH_CHECK();
    }
    if (dist) {
        const bool vec = xvec && per_sample % 4 == 0;
        AFAN_PROF("l2_project_kernel", elts * (8.0 + 4.0 + (shadow ? 2 : 0)), st);  // (upper bound: every sample outside the ball)
        if (shadow) {
            if (vec) l2_project_kernel<true, true><<<grid, BLOCK, 0, st>>>(x_adv, x_clean, shadow, per_sample, chunks, eps, dpart, dnorm);
            else l2_project_kernel<true, false><<<grid, BLOCK, 0, st>>>(x_adv, x_clean, shadow, per_sample, chunks, eps, dpart, dnorm);
        } else {
            if (vec) l2_project_kernel<false, true><<<grid, BLOCK, 0, st>>>(x_adv, x_clean, shadow, per_sample, chunks, eps, dpart, dnorm);
            else l2_project_kernel<false, false><<<grid, BLOCK, 0, st>>>(x_adv, x_clean, shadow, per_sample, chunks, eps, dpart, dnorm);
        }
        AFAN_LAUNCH_CHECK();
    }
    return AFAN_OK;
}

template <typename G, bool CLIP, bool SHADOW>
int launch_step(float* x_adv, const void* grad, const float* x_clean, uint16_t* shadow, int64_t n,
                float gamma, float eps, hipStream_t st) {
    const bool vec = aligned(x_adv, 16) && aligned(grad, 4 * sizeof(G)) &&
                     (!CLIP || aligned(x_clean, 16)) && (!SHADOW || aligned(shadow, 8));
    const int grid = grid_for(vec ? (n + 3) / 4 : n, BLOCK);
    AFAN_PROF("pgd_step_kernel", n * (8.0 + sizeof(G) + (CLIP ? 4 : 0) + (SHADOW ? 2 : 0)), st);
    if (vec)
        pgd_step_kernel<G, CLIP, SHADOW, true><<<grid, BLOCK, 0, st>>>(
            x_adv, (const G*)grad, x_clean, shadow, n, gamma, eps);
    else
        pgd_step_kernel<G, CLIP, SHADOW, false><<<grid, BLOCK, 0, st>>>(
            x_adv, (const G*)grad, x_clean, shadow, n, gamma, eps);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

template <typename G, bool STEP, bool CLIP, bool SHADOW>
int launch_step_clamp(float* x_adv, const void* grad, const float* x_clean, uint16_t* shadow, int64_t n,
                      float gamma, float eps, float lo, float hi, hipStream_t st) {
    const bool vec = aligned(x_adv, 16) && (!STEP || aligned(grad, 4 * sizeof(G))) &&
                     (!CLIP || aligned(x_clean, 16)) && (!SHADOW || aligned(shadow, 8));
    const int64_t lanes = vec ? (n + 3) / 4 : n;  // launch_step's grid: one lane per 4 (1) elements, capped, grid-stride beyond
    const int grid = grid_for(lanes, BLOCK);
    AFAN_PROF("pgd_step_clamp_kernel", n * (8.0 + (STEP ? sizeof(G) : 0) + (CLIP ? 4 : 0) + (SHADOW ? 2 : 0)), st);
    if (vec)
        pgd_step_clamp_kernel<G, STEP, CLIP, SHADOW, true><<<grid, BLOCK, 0, st>>>(
            x_adv, (const G*)grad, x_clean, shadow, n, gamma, eps, lo, hi);
    else
        pgd_step_clamp_kernel<G, STEP, CLIP, SHADOW, false><<<grid, BLOCK, 0, st>>>(
            x_adv, (const G*)grad, x_clean, shadow, n, gamma, eps, lo, hi);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

template <typename G, bool CLIP, bool SHADOW, bool STEP>
int launch_step_norms(float* x_adv, const void* grad, const float* x_clean, uint16_t* shadow,
                      int64_t batch, int64_t per_sample, float gamma, float eps, float* partial,
                      float* l2, float* linf, hipStream_t st) {
    const bool vec = (per_sample % 4 == 0) && aligned(x_adv, 16) && aligned(x_clean, 16) &&
                     (!STEP || aligned(grad, 4 * sizeof(G))) && (!SHADOW || aligned(shadow, 8));
    const int slices = (int)((per_sample + NORM_CHUNK - 1) / NORM_CHUNK);
    dim3 grid(slices, (unsigned)batch);
    {
        const double elts = (double)batch * (double)per_sample;
        AFAN_PROF(STEP ? "pgd_step_norms_kernel" : "perturb_norms_kernel",
                  elts * (STEP ? (12.0 + sizeof(G) + (SHADOW ? 2 : 0)) : 8.0), st);
        if (vec)
            pgd_step_norms_kernel<G, CLIP, SHADOW, true, STEP><<<grid, BLOCK, 0, st>>>(
                x_adv, (const G*)grad, x_clean, shadow, per_sample, gamma, eps, partial);
        else
            pgd_step_norms_kernel<G, CLIP, SHADOW, false, STEP><<<grid, BLOCK, 0, st>>>(
                x_adv, (const G*)grad, x_clean, shadow, per_sample, gamma, eps, partial);
    }
    AFAN_LAUNCH_CHECK();
    AFAN_PROF("norms_finalize_kernel", 8.0 * batch * slices, st);
    norms_finalize_kernel<<<(unsigned)batch, AFAN_WAVE, 0, st>>>(partial, slices, l2, linf);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

}  // namespace

extern "C" {

int afan_version(void) { return 101; }
const char* afan_arch(void) { return "gfx950"; }

int afan_pgd_step(float* x_adv, const void* grad, int grad_dtype, const float* x_clean,
                  uint16_t* shadow_bf16, int64_t n, float gamma, float eps, int clip,
                  afan_stream_t stream) {
    if (n < 0) return AFAN_ESHAPE;
    if (n == 0) return AFAN_OK;
    if (!x_adv || !grad || (clip && !x_clean)) return AFAN_ENULL;
    if (grad_dtype != AFAN_F32 && grad_dtype != AFAN_BF16) return AFAN_EDTYPE;
    if (!aligned(x_adv, 4) || !aligned(grad, grad_dtype == AFAN_F32 ? 4 : 2) ||
        (clip && !aligned(x_clean, 4)) || (shadow_bf16 && !aligned(shadow_bf16, 2)))
        return AFAN_EALIGN;
    hipStream_t st = (hipStream_t)stream;
#define AFAN_DISPATCH(G)                                                                              \
    if (clip) {                                                                                       \
        if (shadow_bf16) return launch_step<G, true, true>(x_adv, grad, x_clean, shadow_bf16, n, gamma, eps, st); \
        return launch_step<G, true, false>(x_adv, grad, x_clean, shadow_bf16, n, gamma, eps, st);     \
    } else {                                                                                          \
        if (shadow_bf16) return launch_step<G, false, true>(x_adv, grad, x_clean, shadow_bf16, n, gamma, eps, st); \
        return launch_step<G, false, false>(x_adv, grad, x_clean, shadow_bf16, n, gamma, eps, st);    \
    }
    if (grad_dtype == AFAN_F32) { AFAN_DISPATCH(float) }
    AFAN_DISPATCH(uint16_t)
#undef AFAN_DISPATCH
}

int afan_pgd_step_clamp(float* x_adv, const void* grad, int grad_dtype, const float* x_clean,
                        uint16_t* shadow_bf16, int64_t n, float gamma, float eps, int clip,
                        float lo, float hi, afan_stream_t stream) {
    if (n < 0) return AFAN_ESHAPE;
    if (n == 0) return AFAN_OK;
    if (!x_adv || (clip && !x_clean)) return AFAN_ENULL;
    if (grad && grad_dtype != AFAN_F32 && grad_dtype != AFAN_BF16) return AFAN_EDTYPE;
    if (!aligned(x_adv, 4) || (grad && !aligned(grad, grad_dtype == AFAN_F32 ? 4 : 2)) ||
        (clip && !aligned(x_clean, 4)) || (shadow_bf16 && !aligned(shadow_bf16, 2)))
        return AFAN_EALIGN;
    hipStream_t st = (hipStream_t)stream;
#define AFAN_DISPATCH(G, STEP)                                                                                            \
    if (clip) {                                                                                                           \
        if (shadow_bf16) return launch_step_clamp<G, STEP, true, true>(x_adv, grad, x_clean, shadow_bf16, n, gamma, eps, lo, hi, st); \
        return launch_step_clamp<G, STEP, true, false>(x_adv, grad, x_clean, shadow_bf16, n, gamma, eps, lo, hi, st);     \
    } else {                                                                                                              \
        if (shadow_bf16) return launch_step_clamp<G, STEP, false, true>(x_adv, grad, x_clean, shadow_bf16, n, gamma, eps, lo, hi, st); \
        return launch_step_clamp<G, STEP, false, false>(x_adv, grad, x_clean, shadow_bf16, n, gamma, eps, lo, hi, st);    \
    }
    if (!grad) { AFAN_DISPATCH(float, false) }
    if (grad_dtype == AFAN_F32) { AFAN_DISPATCH(float, true) }
    AFAN_DISPATCH(uint16_t, true)
#undef AFAN_DISPATCH
}

int64_t afan_norms_workspace_floats(int64_t batch, int64_t per_sample) {
    if (batch <= 0 || per_sample <= 0) return 0;
    return 2 * batch * ((per_sample + NORM_CHUNK - 1) / NORM_CHUNK);
}

int afan_pgd_step_norms(float* x_adv, const void* grad, int grad_dtype, const float* x_clean,
                        uint16_t* shadow_bf16, int64_t batch, int64_t per_sample, float gamma,
                        float eps, int clip, float* partial, float* l2_out, float* linf_out,
                        afan_stream_t stream) {
    if (batch < 0 || per_sample <= 0 || batch > 65535) return AFAN_ESHAPE;
    if (batch == 0) return AFAN_OK;
    if (!x_adv || !grad || !x_clean || !partial || !l2_out || !linf_out) return AFAN_ENULL;
    if (grad_dtype != AFAN_F32 && grad_dtype != AFAN_BF16) return AFAN_EDTYPE;
    if (!aligned(x_adv, 4) || !aligned(grad, grad_dtype == AFAN_F32 ? 4 : 2) || !aligned(x_clean, 4) ||
        !aligned(partial, 4) || (shadow_bf16 && !aligned(shadow_bf16, 2)))
        return AFAN_EALIGN;
    hipStream_t st = (hipStream_t)stream;
#define AFAN_DISPATCH(G)                                                                             \
    if (clip) {                                                                                      \
        if (shadow_bf16)                                                                             \
            return launch_step_norms<G, true, true, true>(x_adv, grad, x_clean, shadow_bf16, batch,  \
                                                          per_sample, gamma, eps, partial, l2_out, linf_out, st); \
        return launch_step_norms<G, true, false, true>(x_adv, grad, x_clean, shadow_bf16, batch,     \
                                                       per_sample, gamma, eps, partial, l2_out, linf_out, st); \
    } else {                                                                                         \
        if (shadow_bf16)                                                                             \
            return launch_step_norms<G, false, true, true>(x_adv, grad, x_clean, shadow_bf16, batch, \
                                                           per_sample, gamma, eps, partial, l2_out, linf_out, st); \
        return launch_step_norms<G, false, false, true>(x_adv, grad, x_clean, shadow_bf16, batch,    \
                                                        per_sample, gamma, eps, partial, l2_out, linf_out, st); \
    }
    if (grad_dtype == AFAN_F32) { AFAN_DISPATCH(float) }
    AFAN_DISPATCH(uint16_t)
#undef AFAN_DISPATCH
}

int afan_perturb_norms(const float* x_adv, const float* x_clean, int64_t batch, int64_t per_sample,
                       float* partial, float* l2_out, float* linf_out, afan_stream_t stream) {
    if (batch < 0 || per_sample <= 0 || batch > 65535) return AFAN_ESHAPE;
    if (batch == 0) return AFAN_OK;
    if (!x_adv || !x_clean || !partial || !l2_out || !linf_out) return AFAN_ENULL;
    if (!aligned(x_adv, 4) || !aligned(x_clean, 4) || !aligned(partial, 4)) return AFAN_EALIGN;
    return launch_step_norms<float, false, false, false>(const_cast<float*>(x_adv), nullptr, x_clean,
                                                         nullptr, batch, per_sample, 0.f, 0.f, partial,
                                                         l2_out, linf_out, (hipStream_t)stream);
}

static int64_t l2_chunks(int64_t per_sample) { return per_sample / L2_CHUNK + (per_sample % L2_CHUNK != 0); }  // (no overflow)

int64_t afan_pgd_step_l2_workspace_floats(int64_t batch, int64_t per_sample) {
    if (batch <= 0 || per_sample <= 0) return 0;
    const int64_t chunks = l2_chunks(per_sample);
    if (chunks > INT32_MAX / batch) return 0;  // (afan_pgd_step_l2 refuses the shape)
    return 2 * batch * chunks;
}

int afan_pgd_step_l2(float* x_adv, const void* grad, int grad_dtype, const float* x_clean,
                     uint16_t* shadow_bf16, int64_t batch, int64_t per_sample,
                     float gamma, float eps, int clip, float* workspace,
                     float* gnorm_out, float* dnorm_out, afan_stream_t stream) {
    if (batch < 0 || per_sample < 0) return AFAN_ESHAPE;
    if (batch == 0 || per_sample == 0) return AFAN_OK;
    const int64_t chunks = l2_chunks(per_sample);
    if (chunks > INT32_MAX / batch || per_sample > INT64_MAX / batch) return AFAN_ESHAPE;
    const bool dist = clip || dnorm_out;
    if (!x_adv || !workspace || (dist && !x_clean)) return AFAN_ENULL;
    if (grad && grad_dtype != AFAN_F32 && grad_dtype != AFAN_BF16) return AFAN_EDTYPE;
    if (!aligned(x_adv, 4) || (grad && !aligned(grad, grad_dtype == AFAN_F32 ? 4 : 2)) || (dist && !aligned(x_clean, 4)) ||
        (shadow_bf16 && !aligned(shadow_bf16, 2)) || !aligned(workspace, 4) || (gnorm_out && !aligned(gnorm_out, 4)) ||
        (dnorm_out && !aligned(dnorm_out, 4)))
        return AFAN_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const float radius = clip ? eps : __builtin_inff();  // (the norm alone: no sample is outside)
    if (!grad)
        return launch_step_l2<float, false>(x_adv, nullptr, x_clean, shadow_bf16, batch, per_sample, (int)chunks, gamma, radius, dist,
                                            workspace, gnorm_out, dnorm_out, st);
    if (grad_dtype == AFAN_F32)
        return launch_step_l2<float, true>(x_adv, grad, x_clean, shadow_bf16, batch, per_sample, (int)chunks, gamma, radius, dist,
                                           workspace, gnorm_out, dnorm_out, st);
    return launch_step_l2<uint16_t, true>(x_adv, grad, x_clean, shadow_bf16, batch, per_sample, (int)chunks, gamma, radius, dist,
                                          workspace, gnorm_out, dnorm_out, st);
}

int afan_axpy_noise(float* x_adv, const float* u, int64_t n, float eps, uint16_t* shadow_bf16,
                    afan_stream_t stream) {
    if (n < 0) return AFAN_ESHAPE;
    if (n == 0) return AFAN_OK;
    if (!x_adv || !u) return AFAN_ENULL;
    if (!aligned(x_adv, 4) || !aligned(u, 4) || (shadow_bf16 && !aligned(shadow_bf16, 2))) return AFAN_EALIGN;
    const int vec = aligned(x_adv, 16) && aligned(u, 16) && (!shadow_bf16 || aligned(shadow_bf16, 8));
    const int grid = grid_for(vec ? (n + 3) / 4 : n, BLOCK);
    AFAN_PROF("axpy_noise_kernel", n * (12.0 + (shadow_bf16 ? 2 : 0)), (hipStream_t)stream);
    axpy_noise_kernel<<<grid, BLOCK, 0, (hipStream_t)stream>>>(x_adv, u, n, eps, shadow_bf16, vec);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

int afan_pgd_rand_start(const float* x, float* x_adv, uint16_t* shadow_bf16, int64_t n, int64_t c, int64_t h, int64_t w,
                        int layout, float eps, uint64_t* state, uint64_t* used, int advance, afan_stream_t stream) {
    if (n < 0 || c < 0 || h < 0 || w < 0 || (layout != AFAN_NCHW && layout != AFAN_NHWC)) return AFAN_ESHAPE;
    if (n == 0 || c == 0 || h == 0 || w == 0) return AFAN_OK;
    const int64_t lim = INT64_MAX >> 2;  // (the kernel shifts element indices left by two)
    if (c > lim / n || h > lim / (n * c) || w > lim / (n * c * h)) return AFAN_ESHAPE;
    if (!x || !x_adv || !state) return AFAN_ENULL;
    if (!aligned(x, 16) || !aligned(x_adv, 16) || (shadow_bf16 && !aligned(shadow_bf16, 16)) || !aligned(state, 8) ||
        (used && !aligned(used, 8)))
        return AFAN_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = n * c * h * w, hw = h * w;
    const bool nhwc = layout == AFAN_NHWC && c > 1 && hw > 1;  // (one channel or one pixel: both layouts are the same memory)
    // one group of four per lane up to 67 M elements: under the usual 2048-workgroup cap a 4 x 3 x 513 x 513 batch is 1.5 rounds of
    // the grid, the second half empty (measured with the generator step behind it: 14.9 -> 13.3 us per start)
    const int grid = grid_for((total + 3) / 4, BLOCK, 1 << 16);
    {
        AFAN_PROF("pgd_rand_start_kernel", total * (8.0 + (shadow_bf16 ? 2 : 0)), st);
        if (!nhwc)
            pgd_rand_start_kernel<false, uint32_t><<<grid, BLOCK, 0, st>>>(x, x_adv, shadow_bf16, total, c, hw, eps, state, used);
        else if (total + 4 < ((int64_t)1 << 32))
            pgd_rand_start_kernel<true, uint32_t><<<grid, BLOCK, 0, st>>>(x, x_adv, shadow_bf16, total, c, hw, eps, state, used);
        else
            pgd_rand_start_kernel<true, uint64_t><<<grid, BLOCK, 0, st>>>(x, x_adv, shadow_bf16, total, c, hw, eps, state, used);
        AFAN_LAUNCH_CHECK();
    }
    if (advance) {
        noise_advance_kernel<<<1, 1, 0, st>>>(state);
        AFAN_LAUNCH_CHECK();
    }
    return AFAN_OK;
}

int afan_tensor_clamp(float* t, const float* lo, const float* hi, int64_t n, afan_stream_t stream) {
    if (n < 0) return AFAN_ESHAPE;
    if (n == 0) return AFAN_OK;
    if (!t || !lo || !hi) return AFAN_ENULL;
    if (!aligned(t, 4) || !aligned(lo, 4) || !aligned(hi, 4)) return AFAN_EALIGN;
    AFAN_PROF("tensor_clamp_kernel", n * 16.0, (hipStream_t)stream);
    tensor_clamp_kernel<<<grid_for(n, BLOCK), BLOCK, 0, (hipStream_t)stream>>>(t, lo, hi, n);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

int afan_cast_bf16(const float* src, uint16_t* dst, int64_t n, afan_stream_t stream) {
    if (n < 0) return AFAN_ESHAPE;
    if (n == 0) return AFAN_OK;
    if (!src || !dst) return AFAN_ENULL;
    if (!aligned(src, 4) || !aligned(dst, 2)) return AFAN_EALIGN;
    const int vec = aligned(src, 16) && aligned(dst, 16);
    const int grid = grid_for(vec ? (n + 7) / 8 : n, BLOCK);
    AFAN_PROF("cast_bf16_kernel", n * 6.0, (hipStream_t)stream);
    cast_bf16_kernel<<<grid, BLOCK, 0, (hipStream_t)stream>>>(src, dst, n, vec);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

int afan_pgd_init(const void* x, int dtype, float* x32, float* x_adv, uint16_t* shadow, int64_t n, afan_stream_t stream) {
    if (dtype != AFAN_F32 && dtype != AFAN_BF16) return AFAN_EDTYPE;
    if (n < 0) return AFAN_ESHAPE;
    if (n == 0) return AFAN_OK;
    if (!x || !x_adv || (dtype == AFAN_BF16 && !x32)) return AFAN_ENULL;
    const size_t a = dtype == AFAN_F32 ? 4 : 2;
    if (!aligned(x, a) || !aligned(x_adv, 4) || (x32 && !aligned(x32, 4)) || (shadow && !aligned(shadow, 2))) return AFAN_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int vec = aligned(x, 16) && aligned(x_adv, 16) && (!x32 || aligned(x32, 16)) && (!shadow || aligned(shadow, 16));
    const int grid = grid_for(vec ? (n + 7) / 8 : n, BLOCK);
    AFAN_PROF("pgd_init_kernel", n * (a + 4.0 + (x32 ? 4 : 0) + (shadow ? 2 : 0)), st);
    if (dtype == AFAN_F32) pgd_init_kernel<float><<<grid, BLOCK, 0, st>>>((const float*)x, x32, x_adv, shadow, n, vec);
    else pgd_init_kernel<uint16_t><<<grid, BLOCK, 0, st>>>((const uint16_t*)x, x32, x_adv, shadow, n, vec);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

}  // extern "C"
