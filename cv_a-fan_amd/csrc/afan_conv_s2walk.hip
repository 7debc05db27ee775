// The stride-2 pair-form input gradient (a block's first 3x3 / 2 convolution and its 1x1 / 2 projection) with ONE workgroup walking
// all four output-parity classes of its tile: the plain form of afan_conv_dgrad_sc_nhwc_bf16 (no BatchNorm operands, no addend), the
// launch PGD's d loss / d feature_map leaves the tail through.
//
//   dx[n, 2h'+ph, 2w'+pw, :] = sum over the class's taps (a,b) of dy[n, h'+(ph+1-a)/2, w'+(pw+1-b)/2, :] * wt10[:, a*3+b, :]
//                              (+ dy_sc[n, h', w', :] * wt10[:, 9, :] in class (0,0); dy pixels outside the image count as zero)
//
// dgrad_impl runs this as four sets of workgroups (one per class: 1+1 / 2 / 2 / 4 taps), each with its own prologue, each fetching its
// own copy of the dy pixels.  With hi and wi even the four classes share ONE lattice of half-resolution positions (n, h', w'), so
// here a workgroup owns BM lattice positions x 64 dx channels and produces all four classes:
//   - the dy neighbourhood of the tile is staged in LDS once per 64-channel chunk of the reduction: the tile's positions plus one halo
//     row below and one halo column to the right, as a contiguous range of the raster padded to (Hg+1) x (Wg+1) per image (the pad
//     row / column are zeros from the buffer range check).  A tap is a shifted view: position P reads P + dh * (Wg+1) + dw, dh, dw
//     in {0, 1}.  dy_sc's tile (shift 0 only) sits in a compact buffer of its own.
//   - the ten weight tiles of a chunk (64 dx channels x 64 reduction channels each) stream through a four-deep LDS ring, three tiles
//     ahead of the MFMAs, by LDS-DMA with counted s_waitcnt vmcnt + bare s_barrier (afan_conv.hip's deep pipeline).
//   - each tap belongs to exactly one class, so a K-step is one 64 x BM x 64 product into that class's accumulators; the step count
//     (10 per chunk) is the old launch's total, the prologue and the dy traffic are paid once instead of four times.
// Summation order per dx element = the tiled kernel's: chunk-outer, tap-inner in ConvClass order (tap slot ascending, the projection
// last in class (0,0)), four 32x32x16 bf16 MFMA steps per chunk ascending, the same operand roles and lane -> k assignment as
// conv_igemm_body, one fp32 accumulator, rounded to bf16 once.  Padding pixels are multiplied as zeros like there.
// No workgroup waits for another; no atomics.
#include "afan_common.h"
#include "afan_conv_s2walk.h"
#include <stdlib.h>

using namespace afan;

namespace afan_s2walk {

static int env_on() {
    const char* v = getenv("AFAN_S2_WALK");
    return (v && atoi(v) == 0) ? 0 : 1;
}
int g_on = env_on();

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 512;      // 8 MFMA waves, 4 (positions) x 2 (dx channels); every wave also issues its share of the DMAs
constexpr int BN = 64;            // dx channels per workgroup
constexpr int NS = 4;             // weight ring: three tiles in flight
constexpr int WBYTES = BN * 128;  // one weight tile: 64 rows of 64 reduction channels
constexpr int LDC = BN + 8;       // epilogue tile row (elements)
constexpr uint32_t OOB = 0x80000000u;

// halo capacity in pixels (a multiple of the 64 pixels one workgroup-wide DMA instruction lands)
template <int BM> struct Cap { static constexpr int HPM = BM == 128 ? 192 : 320; };

struct WalkP {
    const uint16_t* dy; const uint16_t* sc; const uint16_t* w; uint16_t* dx;
    int N, Hg, Wg;        // the lattice: hi / 2 x wi / 2 positions per image (= dy's size)
    int Ci, Co;           // dx channels, reduction channels (dy's)
    uint32_t M;           // N * Hg * Wg
};

constexpr int vmcnt_imm(int n) { return (n & 15) | (7 << 4) | (15 << 8) | ((n >> 4) << 14); }
// wait until at most n of this wave's DMAs are outstanding (n is wave-uniform, 0..6 here; anything else waits for all)
__device__ __forceinline__ void wait_vm(int n) {
    switch (n) {
        case 1: __builtin_amdgcn_s_waitcnt(vmcnt_imm(1)); break;
        case 2: __builtin_amdgcn_s_waitcnt(vmcnt_imm(2)); break;
        case 3: __builtin_amdgcn_s_waitcnt(vmcnt_imm(3)); break;
        case 4: __builtin_amdgcn_s_waitcnt(vmcnt_imm(4)); break;
        case 5: __builtin_amdgcn_s_waitcnt(vmcnt_imm(5)); break;
        case 6: __builtin_amdgcn_s_waitcnt(vmcnt_imm(6)); break;
        default: __builtin_amdgcn_s_waitcnt(vmcnt_imm(0)); break;
    }
}

// tap slot s of wt10 (0..8: tap (a, b) = (s / 3, s % 3) of the 3x3; 9: the projection): its output-parity class and its shift
constexpr int par_of(int a) { return (a + 1) & 1; }                 // ph + 1 - a even
constexpr int shift_of(int a) { return (par_of(a) + 1 - a) / 2; }   // a = 0: 1, a = 1: 0, a = 2: 0
constexpr int cls_of(int s) { return s == 9 ? 0 : par_of(s / 3) * 2 + par_of(s % 3); }
constexpr int dh_of(int s) { return s == 9 ? 0 : shift_of(s / 3); }
constexpr int dw_of(int s) { return s == 9 ? 0 : shift_of(s % 3); }

template <int BM>
constexpr size_t lds_bytes() {
    const size_t loop = (size_t)NS * WBYTES + 2 * (size_t)Cap<BM>::HPM * 128 + (size_t)BM * 128;
    const size_t epi = 4 * (size_t)BM * LDC * 2;
    return loop > epi ? loop : epi;
}

template <int BM>
__global__ __launch_bounds__(THREADS) void conv_s2walk_dgrad_kernel(const WalkP p) {
    constexpr int HPM = Cap<BM>::HPM;
    constexpr int HI = HPM / 64;          // halo DMAs per thread and chunk
    constexpr int SI = BM / 64;           // dy_sc DMAs per thread and chunk
    constexpr int TM = BM / 4, MI = TM / 32;
    constexpr int HBYTES = HPM * 128, W_OFF = 0, H_OFF = NS * WBYTES, S_OFF = H_OFF + 2 * HBYTES;
    static_assert(HI <= 7 && SI <= 4, "a chunk's halo / dy_sc DMAs ride with its first taps and must be older than the last two slots");
    extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
    __shared__ int out_off[BM];
    char* const L = reinterpret_cast<char*>(lds);
    typedef __attribute__((address_space(3))) void* lptr;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const uint32_t Hg = (uint32_t)p.Hg, Wg = (uint32_t)p.Wg, H1 = Hg + 1, W1 = Wg + 1, M = p.M;
    const uint32_t m0 = blockIdx.y * BM;
    const int ci0 = blockIdx.x * BN;
    const int Co = p.Co, chunks = Co / 64;

    auto padded = [&](uint32_t m) -> uint32_t {           // position m in the raster padded to H1 x W1 per image
        const uint32_t t1 = m / Wg, x = m - t1 * Wg;
        const uint32_t n = t1 / Hg, y = t1 - n * Hg;
        return (n * H1 + y) * W1 + x;
    };
    const uint32_t Pb = padded(m0);
    const uint32_t m_last = (m0 + BM < M ? m0 + BM : M) - 1;
    const int HPn = (int)(padded(m_last) - Pb + W1 + 2);  // halo pixels of this tile (launcher: <= HPM)

    const int dy_bytes = (int)((int64_t)M * Co * 2);
    const __amdgpu_buffer_rsrc_t dyr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.dy), 0, dy_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t scr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.sc), 0, dy_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.w), 0, (int)((int64_t)p.Ci * 10 * Co * 2), 0x00020000);

    // ---- DMA bookkeeping.  A workgroup-wide instruction lands 64 rows of 128 bytes; wave w's 1 KiB is rows 8 w .. 8 w + 7.  Row r keeps
    // its 16-byte piece q at slot q ^ ((r >> 1) & 7) (conflict-free ds_read_b128 of 16 consecutive rows, as in afan_conv.hip); seen
    // from the source side this thread (row tid / 8 + 64 i, slot tid & 7) fetches the same logical piece for every i.
    const int piece = (tid & 7) ^ ((tid >> 4) & 7);
    const int row0 = tid >> 3;
    uint32_t hv[HI], sv[SI];
#pragma unroll
    for (int i = 0; i < HI; ++i) {
        const int j = i * 64 + row0;
        const uint32_t P = Pb + (uint32_t)j, t1 = P / W1, x = P - t1 * W1;
        const uint32_t n = t1 / H1, y = t1 - n * H1;
        const bool ok = (j < HPn) & (n < (uint32_t)p.N) & (y < Hg) & (x < Wg);
        hv[i] = ok ? ((((n * Hg + y) * Wg + x) * (uint32_t)Co + piece * 8) * 2u) : OOB;
    }
#pragma unroll
    for (int i = 0; i < SI; ++i) {
        const uint32_t m = m0 + i * 64 + row0;
        sv[i] = m < M ? ((m * (uint32_t)Co + piece * 8) * 2u) : OOB;
    }
    const uint32_t wv = (((uint32_t)(ci0 + row0) * 10u * (uint32_t)Co) + piece * 8) * 2u;

    auto dma_h = [&](int hb, int i, int q) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(dyr, (lptr)(L + H_OFF + hb * HBYTES + i * 8192 + wave * 1024), 16, (int)hv[i], q * 128, 0, 0);
    };
    auto dma_s = [&](int i, int q) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(scr, (lptr)(L + S_OFF + i * 8192 + wave * 1024), 16, (int)sv[i], q * 128, 0, 0);
    };
    auto dma_w = [&](int wb, int s, int q) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (lptr)(L + W_OFF + wb * WBYTES + wave * 1024), 16, (int)wv, (s * Co + q * 64) * 2, 0, 0);
    };

    // ---- prologue: chunk 0's halo and dy_sc tile, then the first three weight tiles (the youngest: what step 0 may leave in flight)
#pragma unroll
    for (int i = 0; i < HI; ++i) dma_h(0, i, 0);
#pragma unroll
    for (int i = 0; i < SI; ++i) dma_s(i, 0);
#pragma unroll
    for (int s = 0; s < NS - 1; ++s) dma_w(s, s, 0);

    // fragment rows of this lane: weights (MFMA operand A: a lane ends up with 4 consecutive dx channels of one position per register
    // quad) and positions (operand B), exactly conv_igemm_body's compute()
    const int frow = lane & 31, fhalf = lane >> 5;
    const int wrow = wc * 32 + frow, wsw = (wrow >> 1) & 7;
    int jrow[MI], srow[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const uint32_t r = wr * TM + i * 32 + frow, m = m0 + r;
        jrow[i] = m < M ? (int)(padded(m) - Pb) : 0;       // (rows beyond M: any staged pixel; their outputs are not stored)
        srow[i] = (int)r;
    }
    for (int r = tid; r < BM; r += THREADS) {
        const uint32_t m = m0 + r;
        int off = -1;
        if (m < M) {
            const uint32_t t1 = m / Wg, x = m - t1 * Wg;
            const uint32_t n = t1 / Hg, y = t1 - n * Hg;
            off = (int)(((n * 2u * Hg + 2u * y) * (2u * Wg) + 2u * x) * (uint32_t)p.Ci);
        }
        out_off[r] = off;
    }

    f32x16 acc[4][MI];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][i][r] = 0.f;

    // ---- K loop: chunk-outer, tap slot inner.  Slot (q, s) waits for weight tile g = 10 q + s (issued three slots ago, the LAST
    // instruction of its slot), meets the workgroup, issues what the slot carries — halo group s of chunk q + 1 into the other halo
    // buffer (free since this chunk's first barrier), dy_sc group s of THIS chunk (q > 0; its buffer is free since the same barrier and
    // read only by slot 9), weight tile g + 3 into the ring buffer slot g - 1 read — and multiplies.  c1 / c2: instructions issued by
    // the last / the last but one slot = what may stay in flight at the wait.
    int c1 = 1, c2 = 1;
    for (int q = 0; q < chunks; ++q) {
        const bool more = q + 1 < chunks;
        const int hb = q & 1;
#pragma unroll
        for (int s = 0; s < 10; ++s) {
            wait_vm(c1 + c2);
            __builtin_amdgcn_s_barrier();
            int cnt = 0;
            if (s < HI && more) { dma_h(hb ^ 1, s, q + 1); ++cnt; }
            if (s < SI && q > 0) { dma_s(s, q); ++cnt; }
            if (s + NS - 1 < 10) { dma_w((q * 10 + s + NS - 1) & (NS - 1), s + NS - 1, q); ++cnt; }
            else if (more) { dma_w((q * 10 + s + NS - 1) & (NS - 1), s + NS - 1 - 10, q + 1); ++cnt; }
            c2 = c1; c1 = cnt;

            constexpr int FB = MI == 1 ? 4 : 2;      // k16 slices of fragments in flight before their MFMAs (registers: 128 accumulators at MI = 2)
            const char* Wt = L + W_OFF + ((q * 10 + s) & (NS - 1)) * WBYTES;
#pragma unroll
            for (int k0 = 0; k0 < 4; k0 += FB) {
            bf16x8 fw[FB], fx[FB][MI];
#pragma unroll
            for (int b = 0; b < FB; ++b) {
                const int kk = k0 + b;
                fw[b] = *reinterpret_cast<const bf16x8*>(Wt + wrow * 128 + (((kk * 2 + fhalf) ^ wsw) * 16));
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    if (s < 9) {
                        const int j = jrow[i] + dh_of(s) * (int)W1 + dw_of(s);
                        fx[b][i] = *reinterpret_cast<const bf16x8*>(L + H_OFF + hb * HBYTES + j * 128 + (((kk * 2 + fhalf) ^ ((j >> 1) & 7)) * 16));
                    } else {
                        const int r = srow[i];
                        fx[b][i] = *reinterpret_cast<const bf16x8*>(L + S_OFF + r * 128 + (((kk * 2 + fhalf) ^ ((r >> 1) & 7)) * 16));
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int b = 0; b < FB; ++b)
#pragma unroll
                for (int i = 0; i < MI; ++i)
                    acc[cls_of(s)][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[b], fx[b][i], acc[cls_of(s)][i], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    __syncthreads();      // every DMA has landed (the last two slots issue nothing) and every fragment read is done: LDS is free

    // ---- epilogue: the four classes' accumulators -> bf16 tiles [class][position][channel] in LDS -> 16-byte stores.  A thread's
    // piece index runs channel piece, then pw, then position: the two pw classes of one dx row interleave into contiguous runs.
    uint16_t* const C = lds;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int pix = wr * TM + i * 32 + frow;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = wc * 32 + 8 * g + 4 * fhalf;
                u16x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = f2bf(acc[c][i][4 * g + e]);
                *reinterpret_cast<u16x4*>(C + ((size_t)c * BM + pix) * LDC + ch) = v;
            }
        }
    __syncthreads();
    const int Wo = 2 * (int)Wg;
    constexpr int PASSES = BM * 4 * 8 / THREADS;
#pragma unroll 4
    for (int ps = 0; ps < PASSES; ++ps) {
        const int e = ps * THREADS + tid;
        const int pc = e & 7, pw = (e >> 3) & 1, rr = e >> 4;
        const int r = rr & (BM - 1), ph = rr / BM;
        const int off = out_off[r];
        if (off >= 0) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(C + ((size_t)(ph * 2 + pw) * BM + r) * LDC + pc * 8);
            *reinterpret_cast<u32x4*>(p.dx + (size_t)off + (size_t)(ph * Wo + pw) * p.Ci + ci0 + pc * 8) = v;
        }
    }
}

// every tile's halo range fits the kernel's capacity?
static bool halo_fits(int64_t M, int64_t Hg, int64_t Wg, int bm, int cap) {
    const int64_t H1 = Hg + 1, W1 = Wg + 1;
    auto padded = [&](int64_t m) { const int64_t t1 = m / Wg, x = m % Wg, n = t1 / Hg, y = t1 % Hg; return (n * H1 + y) * W1 + x; };
    for (int64_t m0 = 0; m0 < M; m0 += bm) {
        const int64_t ml = (m0 + bm < M ? m0 + bm : M) - 1;
        if (padded(ml) - padded(m0) + W1 + 2 > cap) return false;
    }
    return true;
}

template <int BM>
static int launch(const WalkP& p, hipStream_t st) {
    constexpr size_t lds = lds_bytes<BM>();
    static bool attr_done = false;
    if (!attr_done && lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)conv_s2walk_dgrad_kernel<BM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        attr_done = true;
    }
    const dim3 grid((unsigned)(p.Ci / BN), (unsigned)((p.M + BM - 1) / BM), 1);
    conv_s2walk_dgrad_kernel<BM><<<grid, THREADS, lds, st>>>(p);
    AFAN_LAUNCH_CHECK();
    return AFAN_OK;
}

}  // namespace

bool try_launch(const void* dy, const void* dy_sc, const void* wt10, void* dx, int64_t n, int64_t hi, int64_t wi, int64_t ci, int64_t co,
                hipStream_t st, int* rc) {
    if (!g_on) return false;
    if (!dy || !dy_sc || !wt10 || !dx) return false;
    if (!aligned(dy, 16) || !aligned(dy_sc, 16) || !aligned(wt10, 16) || !aligned(dx, 16)) return false;
    if (n <= 0 || hi < 2 || wi < 2 || ((hi | wi) & 1) || ci <= 0 || co <= 0 || ci % 64 || co % 64) return false;
    const int64_t Hg = hi / 2, Wg = wi / 2, M = n * Hg * Wg, tensor = M * co;
    // what dgrad_impl asks of the pair: dy_sc behind dy, everything inside 32-bit byte offsets (its error codes stay its own)
    const int64_t sc_off = (const uint16_t*)dy_sc - (const uint16_t*)dy;
    if (sc_off < tensor || (sc_off + tensor) * 2 > 0x7fffffffLL) return false;
    if (n * hi * wi * ci * 2 > 0x7fffffffLL || ci * 10 * co * 2 > 0x7fffffffLL) return false;
    static const int bm_env = [] { const char* v = getenv("AFAN_S2_WALK_BM"); return v ? atoi(v) : 0; }();   // 128 / 256: the tile (A/B)
    int bm = bm_env == 128 || bm_env == 256 ? bm_env : 256;
    if (bm == 256 && (M <= 128 || !halo_fits(M, Hg, Wg, 256, Cap<256>::HPM))) bm = 128;
    if (bm == 128 && !halo_fits(M, Hg, Wg, 128, Cap<128>::HPM)) return false;
    if ((M + bm - 1) / bm > 65535) return false;
    WalkP p{};
    p.dy = (const uint16_t*)dy; p.sc = (const uint16_t*)dy_sc; p.w = (const uint16_t*)wt10; p.dx = (uint16_t*)dx;
    p.N = (int)n; p.Hg = (int)Hg; p.Wg = (int)Wg; p.Ci = (int)ci; p.Co = (int)co; p.M = (uint32_t)M;
    // the figures dgrad_impl records for the pair form
    const double bytes = 2.0 * ((double)tensor + (double)n * hi * wi * ci + (double)co * 9 * ci) + 2.0 * ((double)tensor + (double)co * ci);
    AFAN_PROF_FLOPS("conv_s2walk_dgrad_kernel", bytes, 2.0 * (double)tensor * 10 * ci, st);
    *rc = bm == 256 ? launch<256>(p, st) : launch<128>(p, st);
    return true;
}

}  // namespace afan_s2walk

extern "C" int afan_conv_s2walk(int on) {
    const int old = afan_s2walk::g_on;
    afan_s2walk::g_on = on ? 1 : 0;
    return old;
}
