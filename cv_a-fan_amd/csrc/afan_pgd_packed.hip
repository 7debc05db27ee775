// The L-inf PGD loop without an fp32 iterate between its steps (include/afan_hip.h states the arithmetic and the code table).
// The iterate after step t is a pure function of the start x0 (the backbone's bf16 map, exact in fp32), the sign decisions of the
// steps 0..t and the scalars gamma and eps.  A step therefore keeps one byte of 2-bit sign codes per element and the bf16 shadow the
// next tail pass reads; it rebuilds the fp32 iterate in registers by replaying the earlier steps from x0.  Only the last step writes
// the fp32 x_adv (and the fp32 copy of x0 that the trainer returns), with the per-sample norms of afan_pgd_step_norms.
//
// csrc/afan_pgd.hip stays as it is (tests assert on its text).  sign_of, step_one (here split into the sign and step_signed, which
// the replay enters with a decoded sign), GradVec4, block_reduce_store, absmax_nan and the norms' finalize are RESTATED here in the
// same expressions; tests/test_pgd_packed_gpu.py holds the two copies together bit for bit (shadow after every step, x_adv, x32 and
// both norms after the last, against afan_pgd_init -> afan_pgd_step -> afan_pgd_step_norms on the same inputs).
// HBM-bound streams: 7 B/elt (t = 0) or 8 B/elt per plain step with a bf16 gradient, 15 B/elt for the last one.
#include "afan_common.h"

using namespace afan;

namespace {

constexpr int BLOCK = 256;
constexpr int NORM_CHUNK = 4096;                 // afan_pgd.hip's: elements of one sample per workgroup of the norms grid
constexpr int TRIPS = NORM_CHUNK / (BLOCK * 4);  // trips of a thread through its slice on the 4-wide path
constexpr int MAX_CODES = 4;                     // 2-bit codes in one byte

__device__ __forceinline__ float sign_of(float g) {
    // torch.sign: 0 -> 0, NaN -> NaN
    return (g != g) ? g : (float)((g > 0.f) - (g < 0.f));
}

// 0 = zero gradient, 1 = +, 2 = -, 3 = NaN gradient
__device__ __forceinline__ uint32_t code_of(float g) { return (g != g) ? 3u : (g > 0.f) ? 1u : (g < 0.f) ? 2u : 0u; }
// sign_of's value for the gradient that gave the code (a NaN's payload is not kept)
__device__ __forceinline__ float sign_from(uint32_t c) { return c == 0u ? 0.f : c == 1u ? 1.f : c == 2u ? -1.f : __builtin_nanf(""); }

template <bool CLIP>
__device__ __forceinline__ float step_signed(float xa, float s, float xc, float gamma, float eps) {
    float d = gamma * s;  // exact: +-gamma, 0 or NaN (gamma * 0.f is evaluated: x_adv = -0 becomes +0 as in afan_pgd_step)
    float t = xa + d;     // the single rounding of attack_algo.py:53
    if (CLIP) {
        float lo = xc - eps;  // attack_algo.py:36 materialises centre-radius / centre+radius first
        float hi = xc + eps;
        if (t < lo) t = lo;  // attack_algo.py:14-15 (NaN compares false and passes through)
        if (t > hi) t = hi;  // attack_algo.py:16-17
    }
    return t;
}

template <bool CLIP>
__device__ __forceinline__ float step_one(float xa, float g, float xc, float gamma, float eps) {
    return step_signed<CLIP>(xa, sign_of(g), xc, gamma, eps);
}

// the iterate after steps 0..T-1, from the start xc and the byte that holds their codes (step s in bits 2s..2s+1)
template <bool CLIP, int T>
__device__ __forceinline__ float replay(float xc, uint32_t byte, float gamma, float eps) {
    float xa = xc;
#pragma unroll
    for (int s = 0; s < T; ++s) xa = step_signed<CLIP>(xa, sign_from((byte >> (2 * s)) & 3u), xc, gamma, eps);
    return xa;
}

// the byte after step T: the T earlier codes kept, step T's code above them, the rest zero
template <int T>
__device__ __forceinline__ uint32_t with_code(uint32_t byte, float g) {
    return (byte & ((1u << (2 * T)) - 1u)) | (code_of(g) << (2 * T));
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

// ---- plain step: 8 elements per lane (16 B of x0, 16 / 32 B of gradient, 8 B of codes, 16 B of shadow) ----------------------------
template <typename G, bool CLIP, bool VEC, int T>
__global__ __launch_bounds__(BLOCK) void pgd_packed_step_kernel(const uint16_t* __restrict__ x0, const G* __restrict__ grad,
                                                                uint8_t* __restrict__ codes, uint16_t* __restrict__ shadow,
                                                                int64_t n, float gamma, float eps) {
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * BLOCK;
    int64_t done = 0;
    if (VEC) {
        const int64_t nvec = n >> 3;
        for (int64_t v = tid; v < nvec; v += nthreads) {
            const int64_t i = v << 3;
            float xc[8], g[8], xa[8];
            Elt<uint16_t>::ldv(x0 + i, xc);
            if constexpr (sizeof(G) == 4) {
                float a[4], b[4];
                Elt<float>::ldv((const float*)grad + i, a);
                Elt<float>::ldv((const float*)grad + i + 4, b);
#pragma unroll
                for (int k = 0; k < 4; ++k) { g[k] = a[k]; g[4 + k] = b[k]; }
            } else {
                Elt<uint16_t>::ldv((const uint16_t*)grad + i, g);
            }
            uint32_t c[2] = {0u, 0u}, o[2] = {0u, 0u};
            if (T > 0) {
                const uint2 cc = *reinterpret_cast<const uint2*>(codes + i);
                c[0] = cc.x;
                c[1] = cc.y;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t byte = (c[k >> 2] >> (8 * (k & 3))) & 0xffu;
                xa[k] = step_one<CLIP>(replay<CLIP, T>(xc[k], byte, gamma, eps), g[k], xc[k], gamma, eps);
                o[k >> 2] |= with_code<T>(byte, g[k]) << (8 * (k & 3));
            }
            *reinterpret_cast<uint2*>(codes + i) = make_uint2(o[0], o[1]);
            Elt<uint16_t>::stv(shadow + i, xa);
        }
        done = nvec << 3;  // the ragged tail (n % 8 elements) follows
    }
    for (int64_t i = done + tid; i < n; i += nthreads) {
        const float xc = bf2f(x0[i]), g = Elt<G>::ld(grad + i);
        const uint32_t byte = T > 0 ? (uint32_t)codes[i] : 0u;
        const float t = step_one<CLIP>(replay<CLIP, T>(xc, byte, gamma, eps), g, xc, gamma, eps);
        codes[i] = (uint8_t)with_code<T>(byte, g);
        shadow[i] = f2bf(t);
    }
}

// ---- block reduction of (sum of squares, max abs) into one partial per workgroup ----------------
__device__ __forceinline__ void block_reduce_store(float ss, float mx, float* __restrict__ partial, int64_t slot) {
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

// ---- last step with the norms ------------------------------------------------------------------------------------------------------
// pgd_step_norms_kernel's grid and walk: workgroup (s, b) owns elements [s*NORM_CHUNK, (s+1)*NORM_CHUNK) of sample b; a thread takes 4
// consecutive elements per trip, BLOCK * 4 apart, and adds d*d in element order, trip after trip.  The loads of all TRIPS trips are
// issued before the arithmetic.  x32, shadow and partial may be NULL (partial == NULL: no norms).
template <typename G, bool CLIP, bool VEC, int T>
__global__ __launch_bounds__(BLOCK) void pgd_packed_last_kernel(const uint16_t* __restrict__ x0, const G* __restrict__ grad,
                                                                const uint8_t* __restrict__ codes, float* __restrict__ x32,
                                                                float* __restrict__ x_adv, uint16_t* __restrict__ shadow,
                                                                int64_t per_sample, float gamma, float eps,
                                                                float* __restrict__ partial) {
    const int64_t b = blockIdx.y;
    const int64_t base = b * per_sample;
    const int64_t lo = (int64_t)blockIdx.x * NORM_CHUNK;
    const int64_t hi = (lo + NORM_CHUNK < per_sample) ? lo + NORM_CHUNK : per_sample;
    float ss = 0.f, mx = 0.f;
    if (VEC) {  // per_sample % 4 == 0 and bases aligned to four elements
        float xc[TRIPS][4], g[TRIPS][4];
        uint32_t c[TRIPS];
#pragma unroll
        for (int r = 0; r < TRIPS; ++r) {
            const int64_t j = lo + (int64_t)threadIdx.x * 4 + (int64_t)r * (BLOCK * 4);
            c[r] = 0u;
            if (j < hi) {
                const int64_t i = base + j;
                GradVec4<uint16_t>::ld(x0 + i, xc[r]);
                GradVec4<G>::ld(grad + i, g[r]);
                if (T > 0) c[r] = *reinterpret_cast<const uint32_t*>(codes + i);
            }
        }
#pragma unroll
        for (int r = 0; r < TRIPS; ++r) {
            const int64_t j = lo + (int64_t)threadIdx.x * 4 + (int64_t)r * (BLOCK * 4);
            if (j < hi) {
                const int64_t i = base + j;
                float xa[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    xa[k] = step_one<CLIP>(replay<CLIP, T>(xc[r][k], (c[r] >> (8 * k)) & 0xffu, gamma, eps), g[r][k], xc[r][k], gamma, eps);
                Elt<float>::stv(x_adv + i, xa);
                if (x32) Elt<float>::stv(x32 + i, xc[r]);
                if (shadow) {
                    u16x4 s;
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[k] = f2bf(xa[k]);
                    *reinterpret_cast<u16x4*>(shadow + i) = s;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float d = xa[k] - xc[r][k];  // main_perturb.py:189
                    ss += d * d;
                    mx = absmax_nan(mx, d);
                }
            }
        }
    } else {
        for (int64_t j = lo + threadIdx.x; j < hi; j += BLOCK) {
            const int64_t i = base + j;
            const float xc = bf2f(x0[i]);
            const uint32_t byte = T > 0 ? (uint32_t)codes[i] : 0u;
            const float xa = step_one<CLIP>(replay<CLIP, T>(xc, byte, gamma, eps), Elt<G>::ld(grad + i), xc, gamma, eps);
            x_adv[i] = xa;
            if (x32) x32[i] = xc;
            if (shadow) shadow[i] = f2bf(xa);
            float d = xa - xc;
            ss += d * d;
            mx = absmax_nan(mx, d);
        }
    }
    if (partial) block_reduce_store(ss, mx, partial, b * gridDim.x + blockIdx.x);
}

// one wave per sample: fold the per-slice partials, L2 = sqrt(sum), Linf = max
__global__ __launch_bounds__(AFAN_WAVE) void pgd_packed_finalize_kernel(const float* __restrict__ partial, int slices,
                                                                        float* __restrict__ l2, float* __restrict__ linf) {
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

#define AFAN_EACH_T(X, TMAX)      \
    switch (t) {                  \
        case 0: X(0) break;       \
        case 1: X(1) break;       \
        case 2: X(2) break;       \
        case 3: X(3) break;       \
        default:                  \
            if (TMAX > 3) { X(TMAX) } \
            break;                \
    }

template <typename G, bool CLIP>
int launch_step(const uint16_t* x0, const void* grad, uint8_t* codes, int t, int64_t n, float gamma, float eps, uint16_t* shadow,
                hipStream_t st) {
    const bool vec = aligned(x0, 16) && aligned(grad, 16) && aligned(codes, 8) && aligned(shadow, 16);
    const int grid = grid_for(vec ? (n + 7) / 8 : n, BLOCK);
    AFAN_PROF("pgd_step_kernel", n * (2.0 + sizeof(G) + (t > 0 ? 1 : 0) + 1 + 2), st);
#define AFAN_STEP(T_)                                                                                                            \
    if (vec) pgd_packed_step_kernel<G, CLIP, true, T_><<<grid, BLOCK, 0, st>>>(x0, (const G*)grad, codes, shadow, n, gamma, eps); \
    else pgd_packed_step_kernel<G, CLIP, false, T_><<<grid, BLOCK, 0, st>>>(x0, (const G*)grad, codes, shadow, n, gamma, eps);
    AFAN_EACH_T(AFAN_STEP, 3)
#undef AFAN_STEP
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

template <typename G, bool CLIP>
int launch_last(const uint16_t* x0, const void* grad, const uint8_t* codes, int t, int64_t batch, int64_t per_sample, float gamma,
                float eps, float* x32, float* x_adv, uint16_t* shadow, float* partial, float* l2, float* linf, hipStream_t st) {
    const bool vec = (per_sample % 4 == 0) && aligned(x0, 8) && aligned(grad, 4 * sizeof(G)) && (t == 0 || aligned(codes, 4)) &&
                     aligned(x_adv, 16) && (!x32 || aligned(x32, 16)) && (!shadow || aligned(shadow, 8));
    const int slices = (int)((per_sample + NORM_CHUNK - 1) / NORM_CHUNK);
    dim3 grid(slices, (unsigned)batch);
    {
        const double elts = (double)batch * (double)per_sample;
        AFAN_PROF("pgd_step_norms_kernel", elts * (2.0 + sizeof(G) + (t > 0 ? 1 : 0) + 4 + (x32 ? 4 : 0) + (shadow ? 2 : 0)), st);
#define AFAN_LAST(T_)                                                                                                         \
    if (vec) pgd_packed_last_kernel<G, CLIP, true, T_><<<grid, BLOCK, 0, st>>>(x0, (const G*)grad, codes, x32, x_adv, shadow, \
                                                                               per_sample, gamma, eps, partial);              \
    else pgd_packed_last_kernel<G, CLIP, false, T_><<<grid, BLOCK, 0, st>>>(x0, (const G*)grad, codes, x32, x_adv, shadow,    \
                                                                            per_sample, gamma, eps, partial);
        AFAN_EACH_T(AFAN_LAST, 4)
#undef AFAN_LAST
        AFAN_LAUNCH_CHECK();
    }
    if (partial) {
        AFAN_PROF("norms_finalize_kernel", 8.0 * batch * slices, st);
        pgd_packed_finalize_kernel<<<(unsigned)batch, AFAN_WAVE, 0, st>>>(partial, slices, l2, linf);
        AFAN_LAUNCH_CHECK();
    }
    return AFAN_OK;
}

}  // namespace

extern "C" {

int afan_pgd_packed_step(const uint16_t* x0, const void* grad, int grad_dtype, uint8_t* codes, int t, int64_t n, float gamma,
                         float eps, int clip, uint16_t* shadow, afan_stream_t stream) {
    if (n < 0 || t < 0 || t >= MAX_CODES) return AFAN_ESHAPE;
    if (n == 0) return AFAN_OK;
    if (!x0 || !grad || !codes || !shadow) return AFAN_ENULL;
    if (grad_dtype != AFAN_F32 && grad_dtype != AFAN_BF16) return AFAN_EDTYPE;
    hipStream_t st = (hipStream_t)stream;
    if (grad_dtype == AFAN_F32)
        return clip ? launch_step<float, true>(x0, grad, codes, t, n, gamma, eps, shadow, st)
                    : launch_step<float, false>(x0, grad, codes, t, n, gamma, eps, shadow, st);
    return clip ? launch_step<uint16_t, true>(x0, grad, codes, t, n, gamma, eps, shadow, st)
                : launch_step<uint16_t, false>(x0, grad, codes, t, n, gamma, eps, shadow, st);
}

int afan_pgd_packed_last(const uint16_t* x0, const void* grad, int grad_dtype, const uint8_t* codes, int t, int64_t batch,
                         int64_t per_sample, float gamma, float eps, int clip, float* x32, float* x_adv, uint16_t* shadow,
                         float* workspace, float* l2, float* linf, afan_stream_t stream) {
    if (batch < 0 || per_sample <= 0 || batch > 65535 || t < 0 || t > MAX_CODES) return AFAN_ESHAPE;
    if (batch == 0) return AFAN_OK;
    if (!x0 || !grad || !x_adv || (t > 0 && !codes) || (l2 && (!linf || !workspace))) return AFAN_ENULL;
    if (grad_dtype != AFAN_F32 && grad_dtype != AFAN_BF16) return AFAN_EDTYPE;
    hipStream_t st = (hipStream_t)stream;
    float* partial = l2 ? workspace : nullptr;
    if (grad_dtype == AFAN_F32)
        return clip ? launch_last<float, true>(x0, grad, codes, t, batch, per_sample, gamma, eps, x32, x_adv, shadow, partial, l2, linf, st)
                    : launch_last<float, false>(x0, grad, codes, t, batch, per_sample, gamma, eps, x32, x_adv, shadow, partial, l2, linf, st);
    return clip ? launch_last<uint16_t, true>(x0, grad, codes, t, batch, per_sample, gamma, eps, x32, x_adv, shadow, partial, l2, linf, st)
                : launch_last<uint16_t, false>(x0, grad, codes, t, batch, per_sample, gamma, eps, x32, x_adv, shadow, partial, l2, linf, st);
}

}  // extern "C"
