// The frozen stem's image gradient in ONE launch: from the gradient at the max-pool output back to the fp32 NCHW image, through
// max pool 3x3/2/1 -> ReLU -> frozen-BatchNorm scale -> 7x7/2/3 convolution (3 -> 64) -> the normaliser's division by std.
// What a robust evaluation of Detection runs per attack step and image (det_eval.RobustEvaluator): layer by layer it is
// afan_maxpool3x3s2_bwd, afan_affine_relu_bwd, a 1x1 MFMA problem 64 -> 152 into a bf16 column tensor (41 MB at 600 x 904),
// afan_conv_stem7_col2im, the normaliser's backward and a cast — two 17 MB maps and the column tensor written and read back.
// Here: 17.4 MB (y1) + 4.3 MB (gy) read, 6.5 MB (dx) written, nothing else.
//
//   g1[n,p,q,k]  = alpha[k] * [y1 > 0] * sum of gy over the pool windows whose winner is (p, q)      (winner: afan_hip.h, max pool)
//   dx[n,c,i,j]  = inv_std[c] * sum over k, r, s of g1[n,(i+3-r)/2,(j+3-s)/2,k] * w[k,r,s,c]          (exact divisions, in range)
//
// VARIANT: g1 is rounded to bf16 ONCE — fp32 sum of the windows' bf16 gradients in window order, times alpha in fp32, then RNE to
// bf16 (the affine backward's output format; the chain rounds twice, after the pool's sum and after the scale).  The products
// g1 * w are exact in fp32 and accumulate in fp32 by fmaf; the two k halves are added once and inv_std multiplies last.
//
// Gather form, VALU: a workgroup (512 threads) owns a TILE x TILE block of image pixels.  It stages
//   * the weights as bf16 [tap][k][c pad 4] (25 088 B: one 8-byte broadcast read and three shifts / masks feed 12 FMAs), and
//   * g1 for the tile's (TILE/2 + 3)^2 = 19 x 19 stem positions x 64 channels as bf16, PSTR = 68 per position (49 096 B),
//     from the pool's winners recomputed from y1 once per window (11 x 11 windows x 64 channels, one byte each: 7 744 B; no index
//     map in memory, no workspace).  The winners are dead once g1 stands, so the weights are staged over them behind a barrier, and
//     the tile's results later over the weights: 25 088 + 49 096 = 74 184 B of LDS and at most 128 VGPRs, two workgroups (16 waves)
//     per CU — one stages while the other multiplies.  Both staging passes issue a task's global loads together (9 window elements;
//     4 window gradients) with clamped addresses — one memory latency per task, not one per element.
// The tile's pixels fall into the four stride-2 parity classes (i & 1, j & 1) with 3 or 4 taps per axis: 9 / 12 / 12 / 16 taps.  A wave
// takes one class (16 x 16 pixels, 4 adjacent same-class pixels per lane: 7 g1 positions serve their 16 (pixel, tap) pairs) and one
// half of the 64 channels; waves w and w + 4 take classes w and 3 - w (9 + 16 and 12 + 12 taps) so that waves sharing a SIMD under
// the cyclic placement carry equal work.  The halves meet in LDS (the tile's 3 x 32 x 32 fp32 results, over the weights' space),
// and the tile is stored in rows.  No atomics, no workspace, nothing shared between workgroups; every global access is bounds-checked.
#include "afan_common.h"

using namespace afan;

namespace {

constexpr int TILE = 32;                     // image pixels per tile side
constexpr int HALO = TILE / 2 + 3;           // 19 stem positions per side: p in [i0/2 - 1, i0/2 + 17]
constexpr int THREADS = 512;
constexpr int CO = 64, KK = 7, TAPS = KK * KK;
constexpr int PSTR = 68;                     // bf16 per staged position (64 + 4: 8-byte aligned rows, 34 dwords)
constexpr int W_ELEMS = TAPS * CO * 4;       // 12 544 bf16: [tap][k][c pad 4]
constexpr int G1_ELEMS = HALO * HALO * PSTR; // 24 548
constexpr int WIN = TILE / 4 + 3;             // 11 pool windows per side touch the staged positions: hp in [i0/4 - 1, i0/4 + 9]
constexpr int ARG_BYTES = WIN * WIN * CO;    // 7 744: each window's winner, one byte per channel
constexpr size_t LDS_BYTES = (size_t)W_ELEMS * 2 + (size_t)G1_ELEMS * 2;
static_assert(ARG_BYTES <= W_ELEMS * 2 && 3 * TILE * TILE * 4 <= W_ELEMS * 2, "the winners, then the weights, then the tile's results share one space");
static_assert(2 * LDS_BYTES <= 160 * 1024, "LDS budget: two workgroups per CU");

// One parity class: 4 same-class pixels (columns b = 4 bg + t) of class row a, channels [k0, k0 + 32).
template <int PI, int PJ>
__device__ __forceinline__ void accumulate(const uint16_t* __restrict__ g1l, const uint16_t* __restrict__ wl, int a, int bg, int k0,
                                           float (&acc)[4][3]) {
    constexpr int R0 = (PI + 1) & 1, NR = PI ? 4 : 3, ROFF = (PI + 3 - R0) / 2;   // r = R0 + 2u, staged row a + 1 + ROFF - u
    constexpr int S0 = (PJ + 1) & 1, NS = PJ ? 4 : 3, SOFF = (PJ + 3 - S0) / 2;   // s = S0 + 2v, staged column b + 1 + SOFF - v
    constexpr int NP = NS + 3;                                                      // positions the 4 pixels' taps touch
    const int lq0 = bg * 4 + 1 + SOFF - (NS - 1);                                   // (= 4 bg; m = t - v + NS - 1 indexes from it)
#pragma unroll
    for (int u = 0; u < NR; ++u) {
        const int r = R0 + 2 * u, lp = a + 1 + ROFF - u;
        const uint16_t* row = g1l + (lp * HALO + lq0) * PSTR + k0;
        const uint16_t* wr = wl + (r * KK * CO + k0) * 4;
#pragma unroll 1
        for (int k = 0; k < CO / 2; k += 4) {
            float g[NP][4];
#pragma unroll
            for (int m = 0; m < NP; ++m) {
                const uint2 v = *reinterpret_cast<const uint2*>(row + m * PSTR + k);
                g[m][0] = __builtin_bit_cast(float, v.x << 16);
                g[m][1] = __builtin_bit_cast(float, v.x & 0xffff0000u);
                g[m][2] = __builtin_bit_cast(float, v.y << 16);
                g[m][3] = __builtin_bit_cast(float, v.y & 0xffff0000u);
            }
#pragma unroll
            for (int v = 0; v < NS; ++v) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const uint2 wv = *reinterpret_cast<const uint2*>(wr + ((S0 + 2 * v) * CO + k + kk) * 4);
                    const float w0 = __builtin_bit_cast(float, wv.x << 16), w1 = __builtin_bit_cast(float, wv.x & 0xffff0000u);
                    const float w2 = __builtin_bit_cast(float, wv.y << 16);
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float gv = g[t - v + NS - 1][kk];
                        acc[t][0] = fmaf(gv, w0, acc[t][0]);
                        acc[t][1] = fmaf(gv, w1, acc[t][1]);
                        acc[t][2] = fmaf(gv, w2, acc[t][2]);
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(THREADS, 4) void stem_image_grad_kernel(const uint16_t* __restrict__ gy, const uint16_t* __restrict__ y1,
                                                                  const uint16_t* __restrict__ w, const float* __restrict__ alpha,
                                                                  const float* __restrict__ inv_std, float* __restrict__ dx, int Hi,
                                                                  int Wi, int Ho, int Wo, int Hp, int Wp) {
    extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
    uint8_t* argl = reinterpret_cast<uint8_t*>(lds);                   // [WIN][WIN][CO] winners; then ...
    uint16_t* wl = lds;                                                // ... the weights [tap][k][4]; then the tile's results [3][TILE][TILE] fp32
    uint16_t* g1l = lds + W_ELEMS;                                     // [HALO][HALO][PSTR]
    const int n = blockIdx.z, i0 = blockIdx.y * TILE, j0 = blockIdx.x * TILE;
    const int p_lo = i0 / 2 - 1, q_lo = j0 / 2 - 1;

    // the pool's winners, once per window: one task = one window x 8 channels, its 9 elements loaded together (clamped addresses)
    const int hp_lo = i0 / 4 - 1, wq_lo = j0 / 4 - 1;
    for (int task = threadIdx.x; task < WIN * WIN * (CO / 8); task += THREADS) {
        const int cg = task & 7, wdx = task >> 3;
        const int lh = wdx / WIN, lw = wdx - lh * WIN;
        const int hp = hp_lo + lh, wq = wq_lo + lw;
        uint32_t packed[2] = {0xffffffffu, 0xffffffffu};                // (no position inside a window: matches nobody)
        if (hp >= 0 && hp < Hp && wq >= 0 && wq < Wp) {
            const int h0 = 2 * hp - 1, w0 = 2 * wq - 1;
            u16x8 v[9];
#pragma unroll
            for (int d = 0; d < 9; ++d) {
                int h = h0 + d / 3, x = w0 + d % 3;
                h = h < 0 ? 0 : (h >= Ho ? Ho - 1 : h);
                x = x < 0 ? 0 : (x >= Wo ? Wo - 1 : x);
                v[d] = *reinterpret_cast<const u16x8*>(y1 + (((int64_t)n * Ho + h) * Wo + x) * CO + cg * 8);
            }
            // first maximum in (h, w) scan order over the elements inside the map, NaN winning (pool_window's rule)
            float best[8];
            int arg[8];
            const int first = (h0 < 0 ? 3 : 0) + (w0 < 0 ? 1 : 0);
#pragma unroll
            for (int e = 0; e < 8; ++e) { best[e] = -INFINITY; arg[e] = first; }
#pragma unroll
            for (int d = 0; d < 9; ++d) {
                const int h = h0 + d / 3, x = w0 + d % 3;
                if (h < 0 || h >= Ho || x < 0 || x >= Wo) continue;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float f = bf2f(v[d][e]);
                    if (f > best[e] || f != f) { best[e] = f; arg[e] = d; }
                }
            }
            packed[0] = packed[1] = 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) packed[e >> 2] |= (uint32_t)arg[e] << ((e & 3) * 8);
        }
        *reinterpret_cast<uint2*>(argl + wdx * CO + cg * 8) = make_uint2(packed[0], packed[1]);
    }
    __syncthreads();

    // g1 of the staged positions: one task = one position x 8 channels; its (up to) four windows' gradients loaded together
    for (int task = threadIdx.x; task < HALO * HALO * (CO / 8); task += THREADS) {
        const int cg = task & 7, pos = task >> 3;
        const int lp = pos / HALO, lq = pos - lp * HALO;
        const int p = p_lo + lp, q = q_lo + lq;
        uint32_t out[4] = {0u, 0u, 0u, 0u};
        if (p >= 0 && p < Ho && q >= 0 && q < Wo) {
            const u16x8 mine = *reinterpret_cast<const u16x8*>(y1 + (((int64_t)n * Ho + p) * Wo + q) * CO + cg * 8);
            // windows hp in {p / 2, (p + 1) / 2} x wq in {q / 2, (q + 1) / 2}, ascending; the second of a pair only where it differs and exists
            const int hpA = p / 2, wqA = q / 2;
            const int hpB = (p + 1) / 2 < Hp ? (p + 1) / 2 : hpA, wqB = (q + 1) / 2 < Wp ? (q + 1) / 2 : wqA;
            const int hps[4] = {hpA, hpA, hpB, hpB}, wqs[4] = {wqA, wqB, wqA, wqB};
            const bool use[4] = {true, wqB != wqA, hpB != hpA, hpB != hpA && wqB != wqA};
            u16x8 gv[4];
            uint2 ab[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                gv[i] = *reinterpret_cast<const u16x8*>(gy + (((int64_t)n * Hp + hps[i]) * Wp + wqs[i]) * CO + cg * 8);
                ab[i] = *reinterpret_cast<const uint2*>(argl + ((hps[i] - hp_lo) * WIN + (wqs[i] - wq_lo)) * CO + cg * 8);
            }
            float sum[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) sum[e] = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!use[i]) continue;
                const uint32_t me = (uint32_t)((p - (2 * hps[i] - 1)) * 3 + (q - (2 * wqs[i] - 1)));
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint32_t a8 = ((e < 4 ? ab[i].x : ab[i].y) >> ((e & 3) * 8)) & 0xffu;
                    if (a8 == me) sum[e] += bf2f(gv[i][e]);
                }
            }
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(alpha + cg * 8), a1 = *reinterpret_cast<const f32x4*>(alpha + cg * 8 + 4);
            const float al[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t b = bf2f(mine[e]) > 0.f ? (uint32_t)f2bf(al[e] * sum[e]) : 0u;
                out[e >> 1] |= b << ((e & 1) * 16);
            }
        }
        uint2* dst = reinterpret_cast<uint2*>(g1l + pos * PSTR + cg * 8);
        dst[0] = make_uint2(out[0], out[1]);
        dst[1] = make_uint2(out[2], out[3]);
    }
    __syncthreads();                                                    // the winners are consumed: their space takes the weights
    for (int i = threadIdx.x; i < CO * TAPS * 3; i += THREADS) {       // w[k][tap][c] -> wl[tap][k][c]
        const int k = i / (TAPS * 3), rem = i - k * (TAPS * 3);
        const int tap = rem / 3, c = rem - tap * 3;
        wl[(tap * CO + k) * 4 + c] = w[i];
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int cls = wave < 4 ? wave : 7 - wave, k0 = wave < 4 ? 0 : CO / 2;
    const int pi = cls >> 1, pj = cls & 1, a = lane & 15, bg = lane >> 4;
    float acc[4][3];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t][0] = acc[t][1] = acc[t][2] = 0.f;
    switch (cls) {                                                      // (wave-uniform)
        case 0: accumulate<0, 0>(g1l, wl, a, bg, k0, acc); break;
        case 1: accumulate<0, 1>(g1l, wl, a, bg, k0, acc); break;
        case 2: accumulate<1, 0>(g1l, wl, a, bg, k0, acc); break;
        default: accumulate<1, 1>(g1l, wl, a, bg, k0, acc); break;
    }
    __syncthreads();                                                    // every wave is done with the weights
    float* res = reinterpret_cast<float*>(lds);                         // [3][TILE][TILE]
    const int il = 2 * a + pi;
    if (k0 != 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int c = 0; c < 3; ++c) res[(c * TILE + il) * TILE + 2 * (bg * 4 + t) + pj] = acc[t][c];
    }
    __syncthreads();
    if (k0 == 0) {
        const float is[3] = {inv_std[0], inv_std[1], inv_std[2]};
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float* o = res + (c * TILE + il) * TILE + 2 * (bg * 4 + t) + pj;
                *o = is[c] * (acc[t][c] + *o);
            }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 3 * TILE * TILE; e += THREADS) {
        const int jl = e & (TILE - 1), r = (e >> 5) & (TILE - 1), c = e >> 10;
        const int i = i0 + r, j = j0 + jl;
        if (i < Hi && j < Wi) dx[(((int64_t)n * 3 + c) * Hi + i) * Wi + j] = res[e];
    }
}

}  // namespace

extern "C" {

int afan_frozen_stem_image_grad_tile(void) { return TILE; }

// dx[N,3,Hi,Wi] (fp32 NCHW) from gy[N,Hp,Wp,64], y1[N,Ho,Wo,64] (bf16 channels-last), w[64,7,7,3] (bf16 KRSC), alpha[64], inv_std[3]
int afan_frozen_stem_image_grad(const void* gy, const void* y1, const void* w, const float* alpha, const float* inv_std, float* dx,
                                int64_t n, int64_t hi, int64_t wi, afan_stream_t stream) {
    if (n <= 0 || hi <= 0 || wi <= 0 || n > 65535 || hi > 0x3fffffff || wi > 0x3fffffff) return AFAN_ESHAPE;
    if (!gy || !y1 || !w || !alpha || !inv_std || !dx) return AFAN_ENULL;
    if (!aligned(gy, 16) || !aligned(y1, 16) || !aligned(w, 2) || !aligned(alpha, 16) || !aligned(inv_std, 4) || !aligned(dx, 4))
        return AFAN_EALIGN;
    const int64_t ho = (hi - 1) / 2 + 1, wo = (wi - 1) / 2 + 1, hp = (ho - 1) / 2 + 1, wp = (wo - 1) / 2 + 1;
    const int64_t ty = (hi + TILE - 1) / TILE, tx = (wi + TILE - 1) / TILE;
    if (ty > 65535) return AFAN_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)stem_image_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
        if (e != hipSuccess) return (int)e;
        attr_done = true;
    }
    const double M = (double)n * ho * wo;
    AFAN_PROF_FLOPS("stem_image_grad_kernel", 2.0 * CO * (M + (double)n * hp * wp) + 12.0 * n * hi * wi, 2.0 * M * CO * TAPS * 3, st);
    dim3 grid((unsigned)tx, (unsigned)ty, (unsigned)n);
    stem_image_grad_kernel<<<grid, THREADS, LDS_BYTES, st>>>((const uint16_t*)gy, (const uint16_t*)y1, (const uint16_t*)w, alpha, inv_std,
                                                             dx, (int)hi, (int)wi, (int)ho, (int)wo, (int)hp, (int)wp);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

}  // extern "C"
