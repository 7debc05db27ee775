// The stride-2 pair-form input gradient as ONE walk over the four output-parity classes (afan_conv_s2walk.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace afan_s2walk {

extern int g_on;          // afan_conv_s2walk(): 1 = eligible calls of afan_conv_dgrad_sc_nhwc_bf16 take the walk kernel (AFAN_S2_WALK=0: off at load)

// The plain pair form (no BatchNorm operands, no addend): dx = conv_transpose(dy, 3x3 / 2) + conv_transpose(dy_sc, 1x1 / 2), bit for bit
// what dgrad_impl's four-class launch writes.  true: the call was taken, *rc is its return code.  false: not this call (switch off, or
// not eligible) — nothing has run, the caller goes on to dgrad_impl, which also owns every error code.
bool try_launch(const void* dy, const void* dy_sc, const void* wt10, void* dx, int64_t n, int64_t hi, int64_t wi, int64_t ci, int64_t co,
                hipStream_t st, int* rc);

}  // namespace afan_s2walk
