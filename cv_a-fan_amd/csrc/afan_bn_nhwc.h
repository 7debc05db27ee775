// What afan_bn.hip (the extern "C" layer) and afan_conv.hip use from afan_bn_nhwc.hip: the BatchNorm request records, filled by
// the exports and read by the launch code of both layouts, and the channels-last entry points.
#pragma once
#include "afan_common.h"
#include <type_traits>

namespace afan_nhwc {

// where a request's moments (forward), sums (backward) or coefficients come from
enum class BnSource {
    Slab,           // the call's own reduce pass, into the workspace slab `ws`
    ConvPartials,   // `partials`: partials_g per channel, summed by the producing convolution's epilogue (forward: about partials_shift)
    AccFill,        // the call's own reduce pass, into the (zeroed) accumulator block
    AccReady,       // the accumulator block, already filled by the producing convolution's epilogue
    Given,          // forward, eval mode: mean_in | invstd_in; the coefficient block is built into bn.stats first
    Coefs,          // forward, eval mode: bn.stats already holds the coefficient block
};

// one BatchNorm's own operands (the dual forward has two)
struct BnOperands {
    const float *weight = nullptr, *bias = nullptr;
    float eps = 0.f, momentum = 0.f;
    float* stats = nullptr;                     // saved statistics: NHWC [4][C] mean | invstd | alpha | beta, NCHW [2][C] mean | invstd
    float *rmean = nullptr, *rvar = nullptr;    // running statistics: both or neither
    int64_t* nbt = nullptr;                     // batch counter
    double* acc = nullptr;                      // accumulator block, double[acc_doubles(C)]
};

// what a forward and a backward request share
struct BnReq {
    int dtype = AFAN_BF16;
    int64_t n = 0, c = 0, hw = 0;
    int relu = 0, groups = 1;                   // groups: image groups with statistics of their own (accumulator sources only)
    BnSource src = BnSource::Slab;
    float* ws = nullptr;
    const float* partials = nullptr;
    int64_t partials_g = 0;
    hipStream_t st = nullptr;
    int64_t rows() const { return n / groups * hw; }   // positions per channel and group
};

struct BnFwd : BnReq {
    const void *x = nullptr, *res = nullptr;    // res: the residual added before the ReLU; the dual form's second input
    void* y = nullptr;
    BnOperands bn, bn_b;                        // bn_b: the dual form's second BatchNorm, applied to `res`
    const float* partials_shift = nullptr;
    const float *mean_in = nullptr, *invstd_in = nullptr;
    int updates = 1;                            // running-statistics updates this forward stands for (afan_bn_set_running_updates)
};

struct BnBwd : BnReq {
    const void *dy = nullptr, *x = nullptr, *y = nullptr;   // y: the forward's output (ReLU mask); NULL: recomputed from x
    void *dx = nullptr, *dres = nullptr;        // dres: the masked gradient for the residual branch, optional
    const float* stats = nullptr;               // the forward's saved statistics
    const float *weight = nullptr, *bias = nullptr;   // NCHW only (the NHWC statistics block carries alpha | beta)
    double* acc = nullptr;
    float *dweight = nullptr, *dbias = nullptr;
    int accumulate = 0;
    int dy_rows = 0;                            // 1 (Slab or AccReady, one group): dy is one [C] row per image, the same at each of its hw positions
};

// f(T{}) with T the storage type of `dtype` (AFAN_F32: float, else bf16 bits)
template <typename F> inline int with_dtype(int dtype, F&& f) { return dtype == AFAN_F32 ? f(float{}) : f(uint16_t{}); }

// f(std::true_type / std::false_type) for a run-time flag that is a kernel template argument
template <typename F> inline void with_flag(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
// f(RELU, HAVE_Y) for the three ReLU-mask forms the backward kernels have: none, the stored output y, recomputed from x.
// (RELU = false never comes with HAVE_Y = true: two nested with_flag would instantiate kernels that nothing launches.)
template <typename F> inline void with_mask(bool relu, bool have_y, F&& f) {
    if (!relu) f(std::false_type{}, std::false_type{});
    else if (have_y) f(std::true_type{}, std::true_type{});
    else f(std::true_type{}, std::false_type{});
}

int fwd(const BnFwd& r);        // sources Slab, ConvPartials, Given, Coefs
int fwd_acc(const BnFwd& r);    // sources AccFill, AccReady
int fwd_dual(const BnFwd& r);   // y = relu(bn(x) + bn_b(res)), both from ready accumulator blocks
int stats(const BnFwd& r);      // the Slab source's statistics alone
int bwd(const BnBwd& r);        // sources Slab, ConvPartials
int bwd_acc(const BnBwd& r);    // sources AccFill, AccReady
int coefs(int64_t C, const float* mean, const float* invstd, const float* w, const float* b, float* out, hipStream_t st);

int64_t workspace_floats(int64_t c);
int64_t acc_doubles(int64_t C);     // doubles per accumulator block
int acc_slot_count(int64_t C);      // accumulator copies per channel
int acc_supported(int dtype, int64_t C);
int running_updates();              // what the next forward's `updates` will be
int set_running_updates(int n);     // returns the previous value

}  // namespace afan_nhwc
