// Training-mode BatchNorm for NCHW activations on gfx950 — the "feature-norm stats" kernels.
// The A-FAN step runs every tail BN K+2 times and every head BN twice per iteration
// (reference: Classification/main_perturb.py:173,195-196 + attack_algo.py:50 through nn.BatchNorm2d,
// resnet_s.py:52-55,88), so BN is the bandwidth-bound part of the step.
//
// Mapping: grid = (S slices, C channels).  Workgroup (s, c) streams every S-th 256-vector chunk of
// channel c's N*HW elements with 16-byte accesses (lanes run along W, so NCHW planes are read
// coalesced), keeps shifted sums in registers, folds them with wave64 shuffles, then across the 4
// waves through LDS, and writes ONE partial per workgroup.  The second launch uses the SAME
// (s, c) -> data mapping: its prologue folds the <= 64 partials of its channel (L2-resident) with
// one wave, so no separate finalize launch and no float atomics (bitwise reproducible).
//   forward : stats partials -> [fold] normalise + affine (+ residual) (+ ReLU), running stats by s==0
//   backward: (sum g, sum g*xhat) partials -> [fold] dx (+ d_residual), dweight/dbias by s==0
#include "afan_bn_nhwc.h"

using namespace afan;
using namespace afan_nhwc;   // the request records and helpers of afan_bn_nhwc.h

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_SLICES = 64;
constexpr int WS_STRIDE = 4;  // floats per partial

struct Geo {
    uint32_t hwv;      // vectors per (n,c) plane
    uint32_t V;        // vectors per channel = N*hwv
    int64_t plane;     // HW elements
    int64_t nstride;   // C*HW elements
    int shift;         // log2(hwv) if power of two else -1
};

__device__ __forceinline__ int64_t vec_offset(const Geo& g, uint32_t v, int c, int vec) {
    uint32_t n, j;
    if (g.shift >= 0) {
        n = v >> g.shift;
        j = v & (g.hwv - 1);
    } else {
        n = v / g.hwv;
        j = v - n * g.hwv;
    }
    return (int64_t)n * g.nstride + (int64_t)c * g.plane + (int64_t)j * vec;
}

template <typename T, int VEC> struct Ld {
    __device__ static __forceinline__ void ld(const T* p, float (&v)[VEC]) {
        if constexpr (VEC == 1) v[0] = Elt<T>::ld(p);
        else Elt<T>::ldv(p, v);
    }
    __device__ static __forceinline__ void st(T* p, const float (&v)[VEC]) {
        if constexpr (VEC == 1) Elt<T>::st(p, v[0]);
        else Elt<T>::stv(p, v);
    }
};

// alpha/beta of y = x*alpha + beta; ONE definition so forward and the backward mask recompute agree bitwise
__device__ __forceinline__ void affine_coeffs(float mu, float is, const float* weight, const float* bias,
                                              int c, float& alpha, float& beta) {
    alpha = is * (weight ? weight[c] : 1.f);
    beta = fmaf(-mu, alpha, bias ? bias[c] : 0.f);
}

// ---- fold helpers (one wave folds the channel's partials, result broadcast through LDS) ---------
__device__ __forceinline__ Moments fold_moments(const float* __restrict__ ws, int c, int S) {
    __shared__ float sh[3];
    if (threadIdx.x < AFAN_WAVE) {
        Moments m{0.f, 0.f, 0.f};
        if ((int)threadIdx.x < S) {
            const float* p = ws + ((int64_t)c * MAX_SLICES + threadIdx.x) * WS_STRIDE;
            m.n = p[0]; m.mean = p[1]; m.m2 = p[2];
        }
        m = wave_merge(m);
        if (threadIdx.x == 0) { sh[0] = m.n; sh[1] = m.mean; sh[2] = m.m2; }
    }
    __syncthreads();
    return Moments{sh[0], sh[1], sh[2]};
}

__device__ __forceinline__ void fold_sums(const float* __restrict__ ws, int c, int S, float& a, float& b) {
    __shared__ float sh[2];
    if (threadIdx.x < AFAN_WAVE) {
        float x = 0.f, y = 0.f;
        if ((int)threadIdx.x < S) {
            const float* p = ws + ((int64_t)c * MAX_SLICES + threadIdx.x) * WS_STRIDE;
            x = p[0]; y = p[1];
        }
        x = wave_sum(x);
        y = wave_sum(y);
        if (threadIdx.x == 0) { sh[0] = x; sh[1] = y; }
    }
    __syncthreads();
    a = sh[0];
    b = sh[1];
}

// ---- forward launch 1: per-(channel, slice) moments ----------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(BLOCK) void bn_stats_kernel(const T* __restrict__ x, Geo g,
                                                         float* __restrict__ ws) {
    const int c = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    float shift = 0.f, sum = 0.f, ssq = 0.f, cnt = 0.f;
    bool first = true;
#pragma unroll 2
    for (uint32_t v = s * BLOCK + threadIdx.x; v < g.V; v += S * BLOCK) {
        float e[VEC];
        Ld<T, VEC>::ld(x + vec_offset(g, v, c, VEC), e);
        if (first) { shift = e[0]; first = false; }  // shifted sums: no cancellation when |mean| >> std
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float d = e[k] - shift;
            sum += d;
            ssq += d * d;
        }
        cnt += (float)VEC;
    }
    Moments m{cnt, 0.f, 0.f};
    if (cnt > 0.f) {
        float dm = sum / cnt;
        m.mean = shift + dm;
        m.m2 = fmaxf(ssq - sum * dm, 0.f);
    }
    m = wave_merge(m);
    __shared__ float sh[BLOCK / AFAN_WAVE][3];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { sh[w][0] = m.n; sh[w][1] = m.mean; sh[w][2] = m.m2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        Moments t{sh[0][0], sh[0][1], sh[0][2]};
#pragma unroll
        for (int k = 1; k < BLOCK / AFAN_WAVE; ++k) t = merge(t, Moments{sh[k][0], sh[k][1], sh[k][2]});
        float* p = ws + ((int64_t)c * MAX_SLICES + s) * WS_STRIDE;
        p[0] = t.n; p[1] = t.mean; p[2] = t.m2;
    }
}

// ---- stand-alone finalize (afan_bn_stats) --------------------------------------------------------
__device__ __forceinline__ void write_stats(const Moments& m, int c, float eps, float momentum,
                                            float* mean, float* invstd, float* rmean, float* rvar) {
    const float var_b = m.m2 / m.n;
    mean[c] = m.mean;
    invstd[c] = 1.0f / sqrtf(var_b + eps);
    if (rmean) {
        // torch uses the unbiased estimate for running_var; one element per channel: 0 / 0 otherwise, guarded as the
        // accumulator path guards its M / (M - 1)
        const float var_u = m.m2 / (m.n > 1.0f ? m.n - 1.0f : 1.0f);
        rmean[c] = (1.0f - momentum) * rmean[c] + momentum * m.mean;
        rvar[c] = (1.0f - momentum) * rvar[c] + momentum * var_u;
    }
}

__global__ __launch_bounds__(AFAN_WAVE) void bn_finalize_kernel(const float* __restrict__ ws, int S,
                                                                float eps, float momentum,
                                                                float* mean, float* invstd, float* rmean,
                                                                float* rvar, int64_t* nbt) {
    const int c = blockIdx.x;
    Moments m = fold_moments(ws, c, S);
    if (threadIdx.x == 0) {
        write_stats(m, c, eps, momentum, mean, invstd, rmean, rvar);
        if (c == 0 && nbt) *nbt += 1;
    }
}

// ---- forward launch 2: fold + apply ---------------------------------------------------------------
template <typename T, int VEC, bool RES, bool RELU, bool TRAIN>
__global__ __launch_bounds__(BLOCK) void bn_apply_kernel(const T* __restrict__ x,
                                                         const T* __restrict__ res, T* __restrict__ y,
                                                         Geo g, const float* __restrict__ ws, float eps,
                                                         float momentum, const float* __restrict__ weight,
                                                         const float* __restrict__ bias, float* mean,
                                                         float* invstd, float* rmean, float* rvar,
                                                         int64_t* nbt) {
    const int c = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    float mu, is;
    if (TRAIN) {
        Moments m = fold_moments(ws, c, S);
        mu = m.mean;
        is = 1.0f / sqrtf(m.m2 / m.n + eps);
        if (s == 0 && threadIdx.x == 0) {
            write_stats(m, c, eps, momentum, mean, invstd, rmean, rvar);
            if (c == 0 && nbt) *nbt += 1;
        }
    } else {
        mu = mean[c];
        is = invstd[c];
    }
    float alpha, beta;
    affine_coeffs(mu, is, weight, bias, c, alpha, beta);
#pragma unroll 2
    for (uint32_t v = s * BLOCK + threadIdx.x; v < g.V; v += S * BLOCK) {
        const int64_t off = vec_offset(g, v, c, VEC);
        float e[VEC], r[VEC];
        Ld<T, VEC>::ld(x + off, e);
        if (RES) Ld<T, VEC>::ld(res + off, r);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float t = fmaf(e[k], alpha, beta);
            if (RES) t += r[k];
            if (RELU) t = (t > 0.f) ? t : ((t != t) ? t : 0.f);  // NaN propagates like torch.relu
            e[k] = t;
        }
        Ld<T, VEC>::st(y + off, e);
    }
}

// ---- backward launch 1: per-(channel, slice) sums of g and g*xhat ---------------------------------
// mask source: y (when given) else recomputed fmaf(x,alpha,beta) exactly as the forward did.
template <typename T, int VEC, bool RELU, bool HAVE_Y>
__global__ __launch_bounds__(BLOCK) void bn_bwd_reduce_kernel(const T* __restrict__ dy,
                                                              const T* __restrict__ x,
                                                              const T* __restrict__ y, Geo g,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ invstd,
                                                              const float* __restrict__ weight,
                                                              const float* __restrict__ bias,
                                                              float* __restrict__ ws) {
    const int c = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const float mu = mean[c], is = invstd[c];
    float alpha, beta;
    affine_coeffs(mu, is, weight, bias, c, alpha, beta);
    float sg = 0.f, sgx = 0.f;
#pragma unroll 2
    for (uint32_t v = s * BLOCK + threadIdx.x; v < g.V; v += S * BLOCK) {
        const int64_t off = vec_offset(g, v, c, VEC);
        float d[VEC], e[VEC], o[VEC];
        Ld<T, VEC>::ld(dy + off, d);
        Ld<T, VEC>::ld(x + off, e);
        if (RELU && HAVE_Y) Ld<T, VEC>::ld(y + off, o);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float gk = d[k];
            if (RELU) {
                const float act = HAVE_Y ? o[k] : fmaf(e[k], alpha, beta);
                gk = (act > 0.f) ? gk : 0.f;
            }
            sg += gk;
            sgx += gk * ((e[k] - mu) * is);
        }
    }
    sg = wave_sum(sg);
    sgx = wave_sum(sgx);
    __shared__ float sh[BLOCK / AFAN_WAVE][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { sh[w][0] = sg; sh[w][1] = sgx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int k = 0; k < BLOCK / AFAN_WAVE; ++k) { a += sh[k][0]; b += sh[k][1]; }
        float* p = ws + ((int64_t)c * MAX_SLICES + s) * WS_STRIDE;
        p[0] = a; p[1] = b;
    }
}

// ---- backward launch 2: fold + dx (+ d_residual) ---------------------------------------------------
template <typename T, int VEC, bool RELU, bool HAVE_Y, bool DRES>
__global__ __launch_bounds__(BLOCK) void bn_bwd_apply_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ y, T* __restrict__ dx,
    T* __restrict__ dres, Geo g, const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ weight, const float* __restrict__ bias, const float* __restrict__ ws,
    float inv_m, float* dweight, float* dbias, int accumulate) {
    const int c = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    float sum_g, sum_gx;
    fold_sums(ws, c, S, sum_g, sum_gx);
    if (s == 0 && threadIdx.x == 0) {
        if (dweight) dweight[c] = accumulate ? dweight[c] + sum_gx : sum_gx;
        if (dbias) dbias[c] = accumulate ? dbias[c] + sum_g : sum_g;
    }
    const float mu = mean[c], is = invstd[c];
    float alpha, beta;
    affine_coeffs(mu, is, weight, bias, c, alpha, beta);
    const float k1 = sum_g * inv_m, k2 = sum_gx * inv_m;
#pragma unroll 2
    for (uint32_t v = s * BLOCK + threadIdx.x; v < g.V; v += S * BLOCK) {
        const int64_t off = vec_offset(g, v, c, VEC);
        float d[VEC], e[VEC], o[VEC];
        Ld<T, VEC>::ld(dy + off, d);
        Ld<T, VEC>::ld(x + off, e);
        if (RELU && HAVE_Y) Ld<T, VEC>::ld(y + off, o);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float gk = d[k];
            if (RELU) {
                const float act = HAVE_Y ? o[k] : fmaf(e[k], alpha, beta);
                gk = (act > 0.f) ? gk : 0.f;
            }
            d[k] = gk;
            const float xh = (e[k] - mu) * is;
            e[k] = (gk - k1 - xh * k2) * alpha;
        }
        Ld<T, VEC>::st(dx + off, e);
        if (DRES) Ld<T, VEC>::st(dres + off, d);
    }
}

// ---- per-channel input normalisation (resnet_s.py:87) ----------------------------------------------
// i indexes the OUTPUT; NHWC output gathers from the NCHW input image
template <typename TO, bool NHWC_OUT>
__global__ __launch_bounds__(BLOCK) void normalize_kernel(const float* __restrict__ x, TO* __restrict__ y,
                                                          int64_t total, int64_t c, int64_t hw,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ std) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * BLOCK) {
        int64_t ch, src;
        if (NHWC_OUT) {
            ch = i % c;
            const int64_t pix = i / c;            // n*hw + p
            src = (pix / hw) * c * hw + ch * hw + (pix % hw);
        } else {
            ch = (i / hw) % c;
            src = i;
        }
        Elt<TO>::st(y + i, (x[src] - mean[ch]) / std[ch]);
    }
}

// ---- host side ------------------------------------------------------------------------------------
// The NCHW launch code reads the request records of afan_bn_nhwc.h: sources Slab (train) and Given (eval) forward, Slab backward;
// bn.stats is [2][C] = mean | invstd here.
struct Plan {
    Geo g;
    int vec;  // elements per access
    dim3 grid;
    double tensor_bytes;  // bytes of one full activation tensor (algorithmic-traffic unit for the profiler)
};

template <typename T>
bool make_plan(int64_t n, int64_t c, int64_t hw, std::initializer_list<const void*> ptrs, Plan& p) {
    constexpr int NV = Elt<T>::VEC;
    bool vec_ok = (hw % NV == 0);
    for (const void* q : ptrs)
        if (q && !aligned(q, 16)) vec_ok = false;
    p.vec = vec_ok ? NV : 1;
    const int64_t hwv = hw / p.vec;
    const int64_t V = n * hwv;
    if (V <= 0 || V > 0x7fffffffLL || c > 65535) return false;
    p.g.hwv = (uint32_t)hwv;
    p.g.V = (uint32_t)V;
    p.g.plane = hw;
    p.g.nstride = c * hw;
    p.g.shift = ((hwv & (hwv - 1)) == 0) ? __builtin_ctzll((unsigned long long)hwv) : -1;
    // enough workgroups to fill 256 CUs x 8, at most MAX_SLICES per channel, >= 1 chunk each
    int64_t S = (2048 + c - 1) / c;
    const int64_t chunks = (V + BLOCK - 1) / BLOCK;
    if (S > chunks) S = chunks;
    if (S > MAX_SLICES) S = MAX_SLICES;
    if (S < 1) S = 1;
    p.grid = dim3((unsigned)S, (unsigned)c);
    p.tensor_bytes = (double)n * (double)c * (double)hw * sizeof(T);
    return true;
}

template <typename T>
void launch_stats(const Plan& p, const BnFwd& r) {
    AFAN_PROF("bn_stats_kernel", p.tensor_bytes, r.st);
    if (p.vec == 1) bn_stats_kernel<T, 1><<<p.grid, BLOCK, 0, r.st>>>((const T*)r.x, p.g, r.ws);
    else bn_stats_kernel<T, Elt<T>::VEC><<<p.grid, BLOCK, 0, r.st>>>((const T*)r.x, p.g, r.ws);
}

template <typename T>
int bn_stats_impl(const BnFwd& r) {
    const BnOperands& b = r.bn;
    Plan p;
    if (!make_plan<T>(r.n, r.c, r.hw, {r.x}, p)) return AFAN_ESHAPE;
    launch_stats<T>(p, r);
    AFAN_LAUNCH_CHECK();
    AFAN_PROF("bn_finalize_kernel", 16.0 * r.c * p.grid.x, r.st);
    bn_finalize_kernel<<<(unsigned)r.c, AFAN_WAVE, 0, r.st>>>(r.ws, (int)p.grid.x, b.eps, b.momentum, b.stats, b.stats + r.c,
                                                              b.rmean, b.rvar, b.nbt);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

template <typename T, int VEC, bool TRAIN>
void launch_apply(const Plan& p, const BnFwd& r) {
    const BnOperands& b = r.bn;
    float* mean = TRAIN ? b.stats : const_cast<float*>(r.mean_in);
    float* invstd = TRAIN ? b.stats + r.c : const_cast<float*>(r.invstd_in);
    AFAN_PROF("bn_apply_kernel", p.tensor_bytes * (r.res ? 3 : 2), r.st);
    with_flag(r.res, [&](auto RES) { with_flag(r.relu, [&](auto RELU) {
        bn_apply_kernel<T, VEC, RES(), RELU(), TRAIN><<<p.grid, BLOCK, 0, r.st>>>(
            (const T*)r.x, (const T*)r.res, (T*)r.y, p.g, r.ws, b.eps, b.momentum, b.weight, b.bias, mean, invstd, b.rmean,
            b.rvar, b.nbt);
    }); });
    ++afan::prof::g_launches;       // (the caller checks the launch; the profiling scope above counts it here)
}

template <typename T>
int bn_forward_impl(const BnFwd& r) {
    Plan p;
    if (!make_plan<T>(r.n, r.c, r.hw, {r.x, r.res, r.y}, p)) return AFAN_ESHAPE;
    constexpr int NV = Elt<T>::VEC;
    if (r.src == BnSource::Slab) {
        launch_stats<T>(p, r);
        AFAN_LAUNCH_CHECK();
        if (p.vec == 1) launch_apply<T, 1, true>(p, r);
        else launch_apply<T, NV, true>(p, r);
    } else {
        if (p.vec == 1) launch_apply<T, 1, false>(p, r);
        else launch_apply<T, NV, false>(p, r);
    }
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

template <typename T, int VEC>
int bn_backward_vec(const Plan& p, const BnBwd& r) {
    const T* dy_ = (const T*)r.dy; const T* x_ = (const T*)r.x; const T* y_ = (const T*)r.y;
    const float *mean = r.stats, *invstd = r.stats + r.c;
    const float inv_m = 1.0f / (float)((double)r.n * (double)r.hw);
    const int mask_read = (r.relu && r.y) ? 1 : 0;   // the forward's output is read as the ReLU mask
    hipStream_t st = r.st;
    {
        AFAN_PROF("bn_bwd_reduce_kernel", p.tensor_bytes * (2 + mask_read), st);
        with_mask(r.relu, r.y, [&](auto RELU, auto HY) {
            bn_bwd_reduce_kernel<T, VEC, RELU(), HY()><<<p.grid, BLOCK, 0, st>>>(dy_, x_, y_, p.g, mean, invstd, r.weight, r.bias, r.ws);
        });
    }
    AFAN_LAUNCH_CHECK();
    AFAN_PROF("bn_bwd_apply_kernel", p.tensor_bytes * (3 + mask_read + (r.dres ? 1 : 0)), st);
    with_mask(r.relu, r.y, [&](auto RELU, auto HY) { with_flag(r.dres, [&](auto DR) {
        bn_bwd_apply_kernel<T, VEC, RELU(), HY(), DR()><<<p.grid, BLOCK, 0, st>>>(dy_, x_, y_, (T*)r.dx, (T*)r.dres, p.g, mean, invstd,
            r.weight, r.bias, r.ws, inv_m, r.dweight, r.dbias, r.accumulate);
    }); });
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

template <typename T>
int bn_backward_impl(const BnBwd& r) {
    Plan p;
    if (!make_plan<T>(r.n, r.c, r.hw, {r.dy, r.x, r.y, r.dx, r.dres}, p)) return AFAN_ESHAPE;
    if (p.vec == 1) return bn_backward_vec<T, 1>(p, r);
    return bn_backward_vec<T, Elt<T>::VEC>(p, r);
}

// the statistics alone, in either layout (defined in front of run_fwd: the code object's kernels follow the order of instantiation)
int run_stats(const BnFwd& r, int layout) {
    if (layout == AFAN_NHWC) return afan_nhwc::stats(r);
    return with_dtype(r.dtype, [&](auto t) { return bn_stats_impl<decltype(t)>(r); });
}
// a forward in either layout (the NCHW kernels apply one running-statistics update per pass: a pending repeat count is refused loudly)
int run_fwd(const BnFwd& r, int layout) {
    if (layout == AFAN_NHWC) return afan_nhwc::fwd(r);
    if (r.src == BnSource::Slab && r.updates != 1) return AFAN_ESHAPE;
    return with_dtype(r.dtype, [&](auto t) { return bn_forward_impl<decltype(t)>(r); });
}

// ---- the exports' argument checks, in the order every export applies them ----------------------------------------
// dtype, shape, layout (exports without a layout argument pass AFAN_NHWC), then the operands that must be there
int check_request(int dtype, int layout, int64_t n, int64_t c, int64_t hw, std::initializer_list<const void*> required) {
    if (dtype != AFAN_F32 && dtype != AFAN_BF16) return AFAN_EDTYPE;
    if (n <= 0 || c <= 0 || hw <= 0) return AFAN_ESHAPE;
    if (layout != AFAN_NCHW && layout != AFAN_NHWC) return AFAN_ELAYOUT;
    for (const void* q : required)
        if (!q) return AFAN_ENULL;
    return AFAN_OK;
}
bool paired(const BnOperands& b) { return (b.rmean == nullptr) == (b.rvar == nullptr); }   // running mean and variance: both or neither
// a filled request: check_request; the convolution's partials (channels-last only, a positive count); the running statistics;
// with accumulator blocks (`accs`) the channel mapping; every tensor that is there on an element boundary and every block on
// 16 bytes; the image groups
int check(const afan_nhwc::BnReq& r, int layout, std::initializer_list<const void*> required,
          std::initializer_list<const void*> tensors, bool running_ok = true, std::initializer_list<const void*> accs = {}) {
    if (const int e = check_request(r.dtype, layout, r.n, r.c, r.hw, required)) return e;
    if (r.src == BnSource::ConvPartials && (layout != AFAN_NHWC || r.partials_g <= 0)) return AFAN_ESHAPE;
    if (!running_ok) return AFAN_ENULL;
    if (accs.size() && !afan_nhwc::acc_supported(r.dtype, r.c)) return AFAN_ESHAPE;
    for (const void* q : tensors)
        if (q && !aligned(q, r.dtype == AFAN_F32 ? 4 : 2)) return AFAN_EALIGN;
    for (const void* q : accs)
        if (!aligned(q, 16)) return AFAN_EALIGN;
    return (r.groups < 1 || r.n % r.groups != 0) ? AFAN_ESHAPE : AFAN_OK;
}

// what every request starts from
template <typename R>
R request(int dtype, int64_t n, int64_t c, int64_t hw, int relu, afan_stream_t stream) {
    R r;
    r.dtype = dtype; r.n = n; r.c = c; r.hw = hw; r.relu = relu;
    r.st = (hipStream_t)stream;
    return r;
}

// One more running-statistics update of a train-mode BatchNorm from the moments of an EARLIER forward pass (its saved
// statistics: mean | invstd): the step runs the clean tail pass once where main_perturb.py runs it twice (first PGD pass and
// the final clean forward, attack_algo.py:50 / main_perturb.py:196) — the second pass's only other effect is this update,
// which comes last in the reference's order.  The biased variance is recovered as 1/invstd^2 - eps (relative error ~1e-6).
// the same for up to RU_MAX layers in one launch (block = layer): a network's tail has 15-50 BatchNorms
struct RUEntry { const float* stats; float* rm; float* rv; int64_t* nbt; int c; float unbias, eps, momentum; };
constexpr int RU_MAX = 64;
struct RUBatch { RUEntry e[RU_MAX]; int n; };
__global__ __launch_bounds__(256) void running_update_batched_kernel(const RUBatch b) {
    const RUEntry& e = b.e[blockIdx.x];
    for (int c = threadIdx.x; c < e.c; c += blockDim.x) {
        const float mean = e.stats[c], is = e.stats[e.c + c];
        // biased variance back from the saved 1/sqrt(var + eps), in f64 (no second rounding on top of invstd's own: what is
        // left is invstd's fp32 ulp, ~1.2e-7 * (var + eps) absolute — relevant only for channels with var << eps)
        const float varb = (float)fmax(1.0 / ((double)is * (double)is) - (double)e.eps, 0.0);
        e.rm[c] = (1.0f - e.momentum) * e.rm[c] + e.momentum * mean;
        e.rv[c] = (1.0f - e.momentum) * e.rv[c] + e.momentum * (varb * e.unbias);
    }
    if (threadIdx.x == 0 && e.nbt) *e.nbt += 1;
}

__global__ void running_update_kernel(const float* __restrict__ stats, int C, float eps, float momentum, float unbias,
                                      float* __restrict__ rmean, float* __restrict__ rvar, int64_t* nbt) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) {
        const float mean = stats[c], is = stats[C + c];
        const float varb = (float)fmax(1.0 / ((double)is * (double)is) - (double)eps, 0.0);
        rmean[c] = (1.0f - momentum) * rmean[c] + momentum * mean;
        rvar[c] = (1.0f - momentum) * rvar[c] + momentum * (varb * unbias);
    }
    if (c == 0 && nbt) *nbt += 1;
}

}  // namespace

extern "C" {

int64_t afan_bn_workspace_floats(int64_t c) {
    if (c <= 0) return 0;
    const int64_t a = c * MAX_SLICES * WS_STRIDE, b = afan_nhwc::workspace_floats(c);
    return a > b ? a : b;
}

int afan_bn_stats(const void* x, int dtype, int layout, int64_t n, int64_t c, int64_t hw, float eps, float momentum,
                  float* workspace, float* stats, float* running_mean, float* running_var, int64_t* num_batches,
                  afan_stream_t stream) {
    BnFwd r = request<BnFwd>(dtype, n, c, hw, /*relu*/ 0, stream);
    r.x = x; r.ws = workspace; r.updates = running_updates();
    r.bn.eps = eps; r.bn.momentum = momentum;
    r.bn.stats = stats; r.bn.rmean = running_mean; r.bn.rvar = running_var; r.bn.nbt = num_batches;
    const int e = check(r, layout, {x, workspace, stats}, {x}, paired(r.bn));
    return e ? e : run_stats(r, layout);
}

int afan_bn_train_forward(const void* x, const void* residual, void* y, int dtype, int layout, int64_t n, int64_t c,
                          int64_t hw, float eps, float momentum, const float* weight, const float* bias, int relu,
                          float* workspace, float* save_stats, float* running_mean, float* running_var,
                          int64_t* num_batches, afan_stream_t stream) {
    BnFwd r = request<BnFwd>(dtype, n, c, hw, relu, stream);
    r.x = x; r.res = residual; r.y = y; r.ws = workspace; r.updates = running_updates();
    r.bn.weight = weight; r.bn.bias = bias; r.bn.eps = eps; r.bn.momentum = momentum;
    r.bn.stats = save_stats; r.bn.rmean = running_mean; r.bn.rvar = running_var; r.bn.nbt = num_batches;
    const int e = check(r, layout, {x, y, workspace, save_stats}, {x, y, residual}, paired(r.bn));
    return e ? e : run_fwd(r, layout);
}

int afan_bn_train_forward_partials(const void* x, const void* residual, void* y, int dtype, int64_t n, int64_t c,
                                   int64_t hw, float eps, float momentum, const float* weight, const float* bias,
                                   int relu, const float* partials, int64_t partials_g, const float* partials_shift,
                                   float* save_stats, float* running_mean, float* running_var, int64_t* num_batches,
                                   afan_stream_t stream) {
    BnFwd r = request<BnFwd>(dtype, n, c, hw, relu, stream);
    r.x = x; r.res = residual; r.y = y; r.updates = running_updates();
    r.src = BnSource::ConvPartials;
    r.partials = partials; r.partials_g = partials_g; r.partials_shift = partials_shift;
    r.bn.weight = weight; r.bn.bias = bias; r.bn.eps = eps; r.bn.momentum = momentum;
    r.bn.stats = save_stats; r.bn.rmean = running_mean; r.bn.rvar = running_var; r.bn.nbt = num_batches;
    const int e = check(r, AFAN_NHWC, {x, y, partials, save_stats}, {x, y, residual}, paired(r.bn));
    return e ? e : afan_nhwc::fwd(r);
}

int afan_bn_apply(const void* x, const void* residual, void* y, int dtype, int layout, int64_t n, int64_t c, int64_t hw,
                  const float* mean, const float* invstd, const float* weight, const float* bias, int relu,
                  float* workspace, afan_stream_t stream) {
    BnFwd r = request<BnFwd>(dtype, n, c, hw, relu, stream);
    r.x = x; r.res = residual; r.y = y;
    r.src = BnSource::Given;
    r.mean_in = mean; r.invstd_in = invstd;
    r.bn.weight = weight; r.bn.bias = bias;
    if (const int e = check(r, layout, {x, y, mean, invstd}, {x, y, residual})) return e;
    if (layout == AFAN_NHWC) {   // the coefficient block is built in the tail of the workspace
        if (!workspace) return AFAN_ENULL;
        r.ws = workspace;
        r.bn.stats = workspace + afan_nhwc::workspace_floats(c) - 4 * c;
    }
    return run_fwd(r, layout);
}

int afan_affine_coefs(const float* mean, const float* invstd, const float* weight, const float* bias, int64_t c,
                      float* coefs, afan_stream_t stream) {
    if (c <= 0) return AFAN_ESHAPE;
    if (!mean || !invstd || !coefs) return AFAN_ENULL;
    if (!aligned(coefs, 16)) return AFAN_EALIGN;
    return afan_nhwc::coefs(c, mean, invstd, weight, bias, coefs, (hipStream_t)stream);
}

int afan_affine_apply(const void* x, const void* residual, void* y, int dtype, int64_t n, int64_t c, int64_t hw,
                      const float* coefs, int relu, afan_stream_t stream) {
    BnFwd r = request<BnFwd>(dtype, n, c, hw, relu, stream);
    r.x = x; r.res = residual; r.y = y;
    r.src = BnSource::Coefs;
    r.bn.stats = const_cast<float*>(coefs);
    const int e = check(r, AFAN_NHWC, {x, y, coefs}, {x, y, residual});
    return e ? e : afan_nhwc::fwd(r);
}

int afan_bn_backward(const void* dy, const void* x, const void* y, void* dx, void* d_residual, int dtype, int layout,
                     int64_t n, int64_t c, int64_t hw, const float* save_stats, const float* weight, const float* bias,
                     int relu, float* workspace, float* dweight, float* dbias, int accumulate, const float* partials,
                     int64_t partials_g, afan_stream_t stream) {
    BnBwd r = request<BnBwd>(dtype, n, c, hw, relu, stream);
    r.dy = dy; r.x = x; r.y = y; r.dx = dx; r.dres = d_residual;
    r.stats = save_stats; r.weight = weight; r.bias = bias; r.ws = workspace;
    r.dweight = dweight; r.dbias = dbias; r.accumulate = accumulate;
    if (partials) r.src = BnSource::ConvPartials;
    r.partials = partials; r.partials_g = partials_g;
    if (const int e = check(r, layout, {dy, x, dx, save_stats, workspace}, {dy, x, dx, y, d_residual})) return e;
    if (layout == AFAN_NHWC) return afan_nhwc::bwd(r);
    return with_dtype(dtype, [&](auto t) { return bn_backward_impl<decltype(t)>(r); });
}

int64_t afan_bn_acc_doubles(int64_t c) { return afan_nhwc::acc_doubles(c); }

int afan_bn_running_update_batched(const float* const* stats, float* const* running_mean, float* const* running_var,
                                   int64_t* const* num_batches, const int64_t* c, const double* m_count, const float* eps,
                                   const float* momentum, int n, afan_stream_t stream) {
    if (n < 0) return AFAN_ESHAPE;
    if (n == 0) return AFAN_OK;
    if (!stats || !running_mean || !running_var || !num_batches || !c || !m_count || !eps || !momentum) return AFAN_ENULL;
    for (int i0 = 0; i0 < n; i0 += RU_MAX) {
        RUBatch b{};
        b.n = n - i0 < RU_MAX ? n - i0 : RU_MAX;
        for (int i = 0; i < b.n; ++i) {
            const int j = i0 + i;
            if (c[j] <= 0 || m_count[j] < 1.0) return AFAN_ESHAPE;
            if (!stats[j] || !running_mean[j] || !running_var[j]) return AFAN_ENULL;
            b.e[i] = RUEntry{stats[j], running_mean[j], running_var[j], num_batches[j], (int)c[j],
                             m_count[j] > 1.0 ? (float)(m_count[j] / (m_count[j] - 1.0)) : 1.0f, eps[j], momentum[j]};
        }
        running_update_batched_kernel<<<(unsigned)b.n, 256, 0, (hipStream_t)stream>>>(b);
        AFAN_LAUNCH_CHECK();
    }
    return AFAN_OK;
}

int afan_bn_set_running_updates(int n) { return afan_nhwc::set_running_updates(n); }

int afan_bn_running_update(const float* stats, int64_t c, double m_count, float eps, float momentum, float* running_mean,
                           float* running_var, int64_t* num_batches, afan_stream_t stream) {
    if (c <= 0 || m_count < 1.0) return AFAN_ESHAPE;
    if (!stats || !running_mean || !running_var) return AFAN_ENULL;
    const float unbias = m_count > 1.0 ? (float)(m_count / (m_count - 1.0)) : 1.0f;
    running_update_kernel<<<(unsigned)((c + 255) / 256), 256, 0, (hipStream_t)stream>>>(stats, (int)c, eps, momentum, unbias,
                                                                                       running_mean, running_var, num_batches);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

int afan_bn_acc_supported(int dtype, int64_t c) {
    if (dtype != AFAN_F32 && dtype != AFAN_BF16) return 0;
    return afan_nhwc::acc_supported(dtype, c);
}

int afan_bn_train_forward_acc(const void* x, const void* residual, void* y, int dtype, int64_t n, int64_t c,
                              int64_t hw, float eps, float momentum, const float* weight, const float* bias, int relu,
                              double* acc, int acc_ready, float* save_stats, float* running_mean, float* running_var,
                              int64_t* num_batches, int groups, afan_stream_t stream) {
    BnFwd r = request<BnFwd>(dtype, n, c, hw, relu, stream);
    r.x = x; r.res = residual; r.y = y; r.updates = running_updates();
    r.src = acc_ready ? BnSource::AccReady : BnSource::AccFill;
    r.groups = groups;
    r.bn.weight = weight; r.bn.bias = bias; r.bn.eps = eps; r.bn.momentum = momentum; r.bn.acc = acc;
    r.bn.stats = save_stats; r.bn.rmean = running_mean; r.bn.rvar = running_var; r.bn.nbt = num_batches;
    const int e = check(r, AFAN_NHWC, {x, y, acc, save_stats}, {x, y, residual}, paired(r.bn), {acc});
    return e ? e : afan_nhwc::fwd_acc(r);
}

int afan_bn_train_forward_acc_dual(const void* x_a, const void* x_b, void* y, int dtype, int64_t n, int64_t c, int64_t hw,
                                   float eps_a, float momentum_a, const float* weight_a, const float* bias_a, double* acc_a,
                                   float* save_stats_a, float* running_mean_a, float* running_var_a, int64_t* num_batches_a,
                                   float eps_b, float momentum_b, const float* weight_b, const float* bias_b, double* acc_b,
                                   float* save_stats_b, float* running_mean_b, float* running_var_b, int64_t* num_batches_b,
                                   afan_stream_t stream) {
    BnFwd r = request<BnFwd>(dtype, n, c, hw, /*relu*/ 1, stream);
    r.x = x_a; r.res = x_b; r.y = y; r.updates = running_updates();
    r.src = BnSource::AccReady;
    BnOperands &a = r.bn, &b = r.bn_b;
    a.weight = weight_a; a.bias = bias_a; a.eps = eps_a; a.momentum = momentum_a; a.acc = acc_a;
    a.stats = save_stats_a; a.rmean = running_mean_a; a.rvar = running_var_a; a.nbt = num_batches_a;
    b.weight = weight_b; b.bias = bias_b; b.eps = eps_b; b.momentum = momentum_b; b.acc = acc_b;
    b.stats = save_stats_b; b.rmean = running_mean_b; b.rvar = running_var_b; b.nbt = num_batches_b;
    const int e = check(r, AFAN_NHWC, {x_a, x_b, y, acc_a, acc_b, save_stats_a, save_stats_b}, {x_a, x_b, y}, paired(a) && paired(b),
                        {acc_a, acc_b});
    return e ? e : afan_nhwc::fwd_dual(r);
}

int afan_bn_backward_acc(const void* dy, const void* x, const void* y, void* dx, void* d_residual, int dtype,
                         int64_t n, int64_t c, int64_t hw, const float* save_stats, int relu, double* acc,
                         int acc_ready, float* dweight, float* dbias, int accumulate, int groups,
                         afan_stream_t stream) {
    BnBwd r = request<BnBwd>(dtype, n, c, hw, relu, stream);
    r.dy = dy; r.x = x; r.y = y; r.dx = dx; r.dres = d_residual;
    r.stats = save_stats; r.acc = acc;
    r.src = acc_ready ? BnSource::AccReady : BnSource::AccFill;
    r.groups = groups;
    r.dweight = dweight; r.dbias = dbias; r.accumulate = accumulate;
    const int e = check(r, AFAN_NHWC, {dy, x, dx, save_stats, acc}, {dy, x, dx, y, d_residual}, true, {acc});
    return e ? e : afan_nhwc::bwd_acc(r);
}

int afan_bn_backward_rows(const void* dy_rows, const void* x, const void* y, void* dx, void* d_residual, int dtype, int64_t n,
                          int64_t c, int64_t hw, const float* save_stats, float* workspace, float* dweight, float* dbias,
                          int accumulate, afan_stream_t stream) {
    BnBwd r = request<BnBwd>(dtype, n, c, hw, /*relu*/ 1, stream);
    r.dy = dy_rows; r.x = x; r.y = y; r.dx = dx; r.dres = d_residual;
    r.stats = save_stats; r.ws = workspace;
    r.dy_rows = 1;
    r.dweight = dweight; r.dbias = dbias; r.accumulate = accumulate;
    const int e = check(r, AFAN_NHWC, {dy_rows, x, y, dx, d_residual, save_stats, workspace}, {dy_rows, x, dx, y, d_residual});
    return e ? e : afan_nhwc::bwd(r);
}

int afan_bn_backward_acc_rows(const void* dy_rows, const void* x, const void* y, void* dx, void* d_residual, int dtype,
                              int64_t n, int64_t c, int64_t hw, const float* save_stats, double* acc, float* dweight,
                              float* dbias, int accumulate, afan_stream_t stream) {
    BnBwd r = request<BnBwd>(dtype, n, c, hw, /*relu*/ 1, stream);
    r.dy = dy_rows; r.x = x; r.y = y; r.dx = dx; r.dres = d_residual;
    r.stats = save_stats; r.acc = acc;
    r.src = BnSource::AccReady;
    r.dy_rows = 1;
    r.dweight = dweight; r.dbias = dbias; r.accumulate = accumulate;
    const int e = check(r, AFAN_NHWC, {dy_rows, x, y, dx, d_residual, save_stats, acc}, {dy_rows, x, dx, y, d_residual}, true, {acc});
    return e ? e : afan_nhwc::bwd_acc(r);
}


int afan_normalize_nchw(const float* x, void* y, int out_dtype, int out_layout, int64_t n, int64_t c, int64_t hw,
                        const float* mean, const float* std, afan_stream_t stream) {
    const int e = check_request(out_dtype, out_layout, n, c, hw, {x, y, mean, std});
    if (e) return e;
    const int64_t total = n * c * hw;
    const int grid = grid_for(total, BLOCK);
    hipStream_t st = (hipStream_t)stream;
    AFAN_PROF("normalize_kernel", total * (4.0 + (out_dtype == AFAN_F32 ? 4 : 2)), st);
    if (out_dtype == AFAN_F32) {
        if (out_layout == AFAN_NHWC) normalize_kernel<float, true><<<grid, BLOCK, 0, st>>>(x, (float*)y, total, c, hw, mean, std);
        else normalize_kernel<float, false><<<grid, BLOCK, 0, st>>>(x, (float*)y, total, c, hw, mean, std);
    } else {
        if (out_layout == AFAN_NHWC) normalize_kernel<uint16_t, true><<<grid, BLOCK, 0, st>>>(x, (uint16_t*)y, total, c, hw, mean, std);
        else normalize_kernel<uint16_t, false><<<grid, BLOCK, 0, st>>>(x, (uint16_t*)y, total, c, hw, mean, std);
    }
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

}  // extern "C"
