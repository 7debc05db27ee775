// Layer-wise SAT evaluation points (Detection/eval_sat_layers.py -> evaluator.py:131-180) for gfx950, channels-last.
// Reference behaviour: attack_algo.get_sample_points(feature_map, feature_adv, 5)[sat_layer] (Detection/attack_algo.py:236-245),
// then with --mix `mix_feature(point, feature_map)` (:254-265 called with its arguments REVERSED against every training script,
// evaluator.py:159): the POINT is normalised and the CLEAN map's per-pixel channel statistics are the target.
// One launch writes up to 10 (weight, mix) outputs from one read of the two maps — the table of five points, each without and with
// the mix — in fp32 or bf16 (the cast the tail's entry would make).  Arithmetic, lane-to-channel map and merge order are those of
// afan_mix.hip's mix_feature_nhwc_kernel / lerp_points_kernel, so every output equals the separate launches bit for bit.
#include "afan_common.h"

using namespace afan;

namespace {

constexpr int BLOCK = 256;
constexpr int SAT_MAX = 10;

struct SatW {
    float w[SAT_MAX];
};

// w == 0: clean's bits, w == 1: adv's bits, else ATen's two lerp forms around 0.5 (lerp_points_kernel's expression)
__device__ __forceinline__ float sat_point(float a, float b, float w) {
    if (w == 0.0f) return a;
    if (w == 1.0f) return b;
    const bool small = fabsf(w) < 0.5f;
    return fmaf(small ? w : w - 1.0f, b - a, small ? a : b);
}

// shifted one-pass moments of one lane's channels, as mix_feature_nhwc_kernel's `take` keeps them
struct LaneSums {
    float sh = 0.f, s = 0.f, q = 0.f, cnt = 0.f;
    bool first = true;
    __device__ __forceinline__ void take(float v) {
        if (first) { sh = v; first = false; }
        const float d = v - sh;
        s += d; q += d * d;
        cnt += 1.f;
    }
    __device__ __forceinline__ Moments moments() const {
        Moments m{cnt, 0.f, 0.f};
        if (cnt > 0.f) {
            const float dm = s / cnt;
            m.mean = sh + dm; m.m2 = fmaxf(q - s * dm, 0.f);
        }
        return m;
    }
};

// Chan butterfly in the lane-symmetric merge order: every lane ends with the same bits
__device__ __forceinline__ Moments wave_merge_sym(Moments m, int lane) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Moments t{__shfl_xor(m.n, o, 64), __shfl_xor(m.mean, o, 64), __shfl_xor(m.m2, o, 64)};
        m = (lane & o) == 0 ? merge(m, t) : merge(t, m);
    }
    return m;
}

// ONE WAVE owns one pixel and loops with the wave stride (the grid's size changes no bit).  A lane's channels lane + k*64, k < KEEP, of
// clean and adv stay in registers for all points; channels beyond 64*KEEP are re-read.  The clean map's moments are computed once.
template <typename TO, int KEEP>
__global__ __launch_bounds__(BLOCK) void sat_points_nhwc_kernel(const float* __restrict__ clean, const float* __restrict__ adv,
                                                                TO* __restrict__ out, int C, int64_t pixels, int64_t total, SatW sw,
                                                                int npts, unsigned mask, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (BLOCK / AFAN_WAVE) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (BLOCK / AFAN_WAVE);
    const float denom = (float)C - 1.0f;  // unbiased: torch.var default (C == 1 -> NaN, like the reference)
    for (int64_t p = wave0; p < pixels; p += nwaves) {
        const float* pc = clean + p * C;
        const float* pa = adv + p * C;
        // keep[] is indexed by unrolled loop counters only (a run-time index becomes relative register addressing: afan_mix.hip)
        float kc[KEEP], ka[KEEP];
#pragma unroll
        for (int k = 0; k < KEEP; ++k) {
            const int c = lane + k * AFAN_WAVE;
            kc[k] = 0.f; ka[k] = 0.f;
            if (c < C) { kc[k] = pc[c]; ka[k] = pa[c]; }
        }
        float mean_x = 0.f, std_x = 1.f;
        if (mask) {
            LaneSums sx;
#pragma unroll
            for (int k = 0; k < KEEP; ++k)
                if (lane + k * AFAN_WAVE < C) sx.take(kc[k]);
            for (int c = lane + KEEP * AFAN_WAVE; c < C; c += AFAN_WAVE) sx.take(pc[c]);
            const Moments mx = wave_merge_sym(sx.moments(), lane);
            mean_x = mx.mean; std_x = sqrtf(mx.m2 / denom + eps);
        }
        for (int j = 0; j < npts; ++j) {
            const float w = sw.w[j];
            TO* po = out + (int64_t)j * total + p * C;
            if (!((mask >> j) & 1u)) {
#pragma unroll
                for (int k = 0; k < KEEP; ++k) {
                    const int c = lane + k * AFAN_WAVE;
                    if (c < C) Elt<TO>::st(po + c, sat_point(kc[k], ka[k], w));
                }
                for (int c = lane + KEEP * AFAN_WAVE; c < C; c += AFAN_WAVE) Elt<TO>::st(po + c, sat_point(pc[c], pa[c], w));
                continue;
            }
            LaneSums sp;
#pragma unroll
            for (int k = 0; k < KEEP; ++k)
                if (lane + k * AFAN_WAVE < C) sp.take(sat_point(kc[k], ka[k], w));
            for (int c = lane + KEEP * AFAN_WAVE; c < C; c += AFAN_WAVE) sp.take(sat_point(pc[c], pa[c], w));
            const Moments mp = wave_merge_sym(sp.moments(), lane);
            const float mean_p = mp.mean, std_p = sqrtf(mp.m2 / denom + eps);
            // (point - mean_p) / std_p * std_x + mean_x, op by op as attack_algo.py:263-264 with the reversed roles
            auto put = [&](int c, float v) {
                float t = (v - mean_p) / std_p;
                t = t * std_x;
                t = t + mean_x;
                Elt<TO>::st(po + c, t);
            };
#pragma unroll
            for (int k = 0; k < KEEP; ++k) {
                const int c = lane + k * AFAN_WAVE;
                if (c < C) put(c, sat_point(kc[k], ka[k], w));
            }
            for (int c = lane + KEEP * AFAN_WAVE; c < C; c += AFAN_WAVE) put(c, sat_point(pc[c], pa[c], w));
        }
    }
}

template <typename TO>
int sat_points_impl(const float* clean, const float* adv, void* out, int64_t pixels, int64_t c, SatW sw, int npts, unsigned mask,
                    float eps, hipStream_t st) {
    const int grid = grid_for(pixels * AFAN_WAVE, BLOCK, 8192);
    AFAN_PROF("sat_points_nhwc_kernel", (8.0 + sizeof(TO) * npts) * pixels * c, st);
    if (c <= 64 * 8) sat_points_nhwc_kernel<TO, 8><<<grid, BLOCK, 0, st>>>(clean, adv, (TO*)out, (int)c, pixels, pixels * c, sw, npts, mask, eps);
    else sat_points_nhwc_kernel<TO, 20><<<grid, BLOCK, 0, st>>>(clean, adv, (TO*)out, (int)c, pixels, pixels * c, sw, npts, mask, eps);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

}  // namespace

extern "C" {

int afan_sat_points_nhwc(const float* clean, const float* adv, void* out, int out_dtype, int64_t pixels, int64_t c,
                         const float* weights, int n_points, unsigned mix_mask, float eps, afan_stream_t stream) {
    if (out_dtype != AFAN_F32 && out_dtype != AFAN_BF16) return AFAN_EDTYPE;
    if (pixels < 0 || c <= 0 || c > 0x7fffffffLL || n_points < 1 || n_points > SAT_MAX || (mix_mask >> n_points)) return AFAN_ESHAPE;
    if (!weights) return AFAN_ENULL;
    SatW sw;
    for (int k = 0; k < SAT_MAX; ++k) {
        sw.w[k] = k < n_points ? weights[k] : 0.f;
        if (!(sw.w[k] >= 0.f && sw.w[k] <= 1.f)) return AFAN_ESHAPE;
    }
    if (pixels == 0) return AFAN_OK;
    if (!clean || !adv || !out) return AFAN_ENULL;
    if (!aligned(clean, 4) || !aligned(adv, 4) || !aligned(out, out_dtype == AFAN_F32 ? 4 : 2)) return AFAN_EALIGN;
    if (out_dtype == AFAN_F32) return sat_points_impl<float>(clean, adv, out, pixels, c, sw, n_points, mix_mask, eps, (hipStream_t)stream);
    return sat_points_impl<uint16_t>(clean, adv, out, pixels, c, sw, n_points, mix_mask, eps, (hipStream_t)stream);
}

}  // extern "C"
