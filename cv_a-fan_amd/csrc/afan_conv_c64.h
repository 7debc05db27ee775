// 3x3 / stride 1 / 64 -> 64 channel convolution (ResNet-18's layer1 inside the PGD tail): see afan_conv_c64.hip.
#pragma once
#include "afan_common.h"

namespace afan_c64 {

struct Params {
    const uint16_t* x;       // [N, H, W, 64] bf16 channels-last
    const uint16_t* w;       // [64 out][9 taps][64 in] bf16 (KRSC for the forward, CRSK for the input gradient)
    uint16_t* y;             // [N, H, W, 64]
    int N, H, W;
    int flip;                // 0: tap (r, s) reads x[h + r - 1][w + s - 1]; 1: x[h + 1 - r][w + 1 - s] (input gradient)
    // epilogue fusions, same meaning as ConvP in afan_conv.hip
    double* acc;             // f64 accumulator block (BN moments, or BN-backward sums when bnx != NULL)
    int acc_ns;
    const float* shift;
    const uint16_t* bnx;
    const float* bn_stats;
    int bn_relu;
    const uint16_t* bny;
    const uint16_t* addend;
    // forward only, a separate instantiation: the frozen BatchNorm behind the convolution (afan_conv_fwd_affine_nhwc_bf16 with any_family = 1),
    // y = [relu](bf16(conv) * alpha + beta [+ aff_res]) with aff an afan_affine_coefs block [4][64]; no addend, no sums
    // input gradient (flip = 1) with aff set, a third instantiation (afan_conv_dgrad_affine_nhwc_bf16 with any_family = 1): aff = the alpha row [64] of
    // the frozen BatchNorm in front of the convolution, aff_res = its stored output (NULL: no ReLU mask),
    // y = bf16((aff_res > 0 ? bf16(dgrad) : 0) * alpha)
    const float* aff;
    const uint16_t* aff_res;
    int aff_relu;
};

// shapes this kernel takes: ci == co == 64, k == 3, stride == 1, W a power of two in [4, 32], H a multiple of 128 / W
bool eligible(int64_t n, int64_t h, int64_t w, int64_t ci, int64_t co, int k, int stride);
int launch(const Params& p, hipStream_t st);

}  // namespace afan_c64
