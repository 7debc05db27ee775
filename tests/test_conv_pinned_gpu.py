"""The bf16 convolution kernels (tiled implicit GEMM in every instantiation dispatch() picks, the 64-channel kernel, the small-
channel kernel, the stems, the weight-gradient tiles) pinned ELEMENTWISE to float64, at every convolution problem of the five
benchmarked workloads and at the edges where tiled kernels go wrong.

Two checks per problem and direction:
  * exact: sparse ternary operands, so that every partial sum is a small integer (asserted: |result| <= 256 for the bf16 outputs,
    sum |a*b| < 2^24 for everything).  fp32 accumulation is then exact in any order and the kernel must equal float64 BIT FOR BIT:
    any indexing, masking, padding, tail or tap error shows.
  * rounding-aware: Gaussian bf16 operands.  bf16 outputs must be the round-to-nearest-even bf16 of the float64 result; the other
    neighbour is accepted only where the float64 value lies within C * 2^-24 * S of the rounding midpoint, S = conv(|x|, |w|) (the
    scale the fp32 accumulation noise is relative to, as in test_conv_f32_gpu.py).  fp32 weight gradients: |g - g64| <= C * 2^-24 * S.

The float64 references run on the GPU (aten's own im2col + GEMM: the vendor library takes no float64); one test checks them against
the CPU.  Every numerical failure names the instantiation that ran (ops.conv_trace).  Two coverage tests keep the pins from eroding:
the table must reach exactly EXPECTED_VARIANTS, and every launch of one iteration of each workload must be a pinned problem on a
pinned instantiation.
"""
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
C_BF16 = 32.0                # fwd / dgrad: the midpoint window, in units of 2^-24 * S
C_WGRAD = 8.0                # wgrad: |g - g64| <= C_WGRAD * 2^-24 * S, about 3x the measured worst ratio below
C_MOMENTS = 16.0             # epilogue moments against float64 sums of the stored tile: 2^-20 = C_MOMENTS * 2^-24 of the sum of |terms|
WGRAD_MEASURED = 2.53        # worst |g - g64| / (2^-24 * S) over the table on an MI355X (DeepLab's 2048 -> 256 atrous 3x3, rate 12)

# ---------------------------------------------------------------------------------------------------------------- the table
# (tag, n, hi, wi, ci, co, k, stride, dilation): one LAYER problem (input hi x wi, ci -> co channels, padding dilation * (k // 2)).
# Workload rows: every distinct convolution problem one training iteration of a benchmarked workload launches, at bench size
# (test_workload_launches_are_pinned checks that list against a traced iteration).
WORKLOAD_ROWS = [
    # resnet18
    ('resnet18_32x32_3to64_k3s1_n256', 256, 32, 32, 3, 64, 3, 1, 1),
    ('resnet18_32x32_64to64_k3s1_n256', 256, 32, 32, 64, 64, 3, 1, 1),
    ('resnet18_32x32_64to128_k1s2_n256', 256, 32, 32, 64, 128, 1, 2, 1),
    ('resnet18_32x32_64to128_k1s2_n512', 512, 32, 32, 64, 128, 1, 2, 1),
    ('resnet18_32x32_64to128_k3s2_n256', 256, 32, 32, 64, 128, 3, 2, 1),
    ('resnet18_32x32_64to128_k3s2_n512', 512, 32, 32, 64, 128, 3, 2, 1),
    ('resnet18_16x16_128to128_k3s1_n256', 256, 16, 16, 128, 128, 3, 1, 1),
    ('resnet18_16x16_128to128_k3s1_n512', 512, 16, 16, 128, 128, 3, 1, 1),
    ('resnet18_16x16_128to256_k1s2_n256', 256, 16, 16, 128, 256, 1, 2, 1),
    ('resnet18_16x16_128to256_k1s2_n512', 512, 16, 16, 128, 256, 1, 2, 1),
    ('resnet18_16x16_128to256_k3s2_n256', 256, 16, 16, 128, 256, 3, 2, 1),
    ('resnet18_16x16_128to256_k3s2_n512', 512, 16, 16, 128, 256, 3, 2, 1),
    ('resnet18_8x8_256to256_k3s1_n256', 256, 8, 8, 256, 256, 3, 1, 1),
    ('resnet18_8x8_256to256_k3s1_n512', 512, 8, 8, 256, 256, 3, 1, 1),
    ('resnet18_8x8_256to512_k1s2_n256', 256, 8, 8, 256, 512, 1, 2, 1),
    ('resnet18_8x8_256to512_k1s2_n512', 512, 8, 8, 256, 512, 1, 2, 1),
    ('resnet18_8x8_256to512_k3s2_n256', 256, 8, 8, 256, 512, 3, 2, 1),
    ('resnet18_8x8_256to512_k3s2_n512', 512, 8, 8, 256, 512, 3, 2, 1),
    ('resnet18_4x4_512to512_k3s1_n256', 256, 4, 4, 512, 512, 3, 1, 1),
    ('resnet18_4x4_512to512_k3s1_n512', 512, 4, 4, 512, 512, 3, 1, 1),
    # resnet20s
    ('resnet20s_32x32_3to16_k3s1_n128', 128, 32, 32, 3, 16, 3, 1, 1),
    ('resnet20s_32x32_16to16_k3s1_n128', 128, 32, 32, 16, 16, 3, 1, 1),
    ('resnet20s_32x32_16to32_k3s2_n128', 128, 32, 32, 16, 32, 3, 2, 1),
    ('resnet20s_32x32_16to32_k3s2_n256', 256, 32, 32, 16, 32, 3, 2, 1),
    ('resnet20s_16x16_32to32_k3s1_n128', 128, 16, 16, 32, 32, 3, 1, 1),
    ('resnet20s_16x16_32to32_k3s1_n256', 256, 16, 16, 32, 32, 3, 1, 1),
    ('resnet20s_16x16_32to64_k3s2_n128', 128, 16, 16, 32, 64, 3, 2, 1),
    ('resnet20s_16x16_32to64_k3s2_n256', 256, 16, 16, 32, 64, 3, 2, 1),
    ('resnet20s_8x8_64to64_k3s1_n128', 128, 8, 8, 64, 64, 3, 1, 1),
    ('resnet20s_8x8_64to64_k3s1_n256', 256, 8, 8, 64, 64, 3, 1, 1),
    # resnet56s
    # resnet50
    ('resnet50_112x112_152to64_k1s1_n64', 64, 112, 112, 152, 64, 1, 1, 1),
    ('resnet50_56x56_64to64_k1s1_n64', 64, 56, 56, 64, 64, 1, 1, 1),
    ('resnet50_56x56_64to64_k3s1_n64', 64, 56, 56, 64, 64, 3, 1, 1),
    ('resnet50_56x56_64to256_k1s1_n64', 64, 56, 56, 64, 256, 1, 1, 1),
    ('resnet50_56x56_128to128_k3s2_n64', 64, 56, 56, 128, 128, 3, 2, 1),
    ('resnet50_56x56_128to128_k3s2_n128', 128, 56, 56, 128, 128, 3, 2, 1),
    ('resnet50_56x56_256to64_k1s1_n64', 64, 56, 56, 256, 64, 1, 1, 1),
    ('resnet50_56x56_256to128_k1s1_n64', 64, 56, 56, 256, 128, 1, 1, 1),
    ('resnet50_56x56_256to128_k1s1_n128', 128, 56, 56, 256, 128, 1, 1, 1),
    ('resnet50_56x56_256to512_k1s2_n64', 64, 56, 56, 256, 512, 1, 2, 1),
    ('resnet50_56x56_256to512_k1s2_n128', 128, 56, 56, 256, 512, 1, 2, 1),
    ('resnet50_28x28_128to128_k3s1_n64', 64, 28, 28, 128, 128, 3, 1, 1),
    ('resnet50_28x28_128to128_k3s1_n128', 128, 28, 28, 128, 128, 3, 1, 1),
    ('resnet50_28x28_128to512_k1s1_n64', 64, 28, 28, 128, 512, 1, 1, 1),
    ('resnet50_28x28_128to512_k1s1_n128', 128, 28, 28, 128, 512, 1, 1, 1),
    ('resnet50_28x28_256to256_k3s2_n64', 64, 28, 28, 256, 256, 3, 2, 1),
    ('resnet50_28x28_256to256_k3s2_n128', 128, 28, 28, 256, 256, 3, 2, 1),
    ('resnet50_28x28_512to128_k1s1_n64', 64, 28, 28, 512, 128, 1, 1, 1),
    ('resnet50_28x28_512to128_k1s1_n128', 128, 28, 28, 512, 128, 1, 1, 1),
    ('resnet50_28x28_512to256_k1s1_n64', 64, 28, 28, 512, 256, 1, 1, 1),
    ('resnet50_28x28_512to256_k1s1_n128', 128, 28, 28, 512, 256, 1, 1, 1),
    ('resnet50_28x28_512to1024_k1s2_n64', 64, 28, 28, 512, 1024, 1, 2, 1),
    ('resnet50_28x28_512to1024_k1s2_n128', 128, 28, 28, 512, 1024, 1, 2, 1),
    ('resnet50_14x14_256to256_k3s1_n64', 64, 14, 14, 256, 256, 3, 1, 1),
    ('resnet50_14x14_256to256_k3s1_n128', 128, 14, 14, 256, 256, 3, 1, 1),
    ('resnet50_14x14_256to1024_k1s1_n64', 64, 14, 14, 256, 1024, 1, 1, 1),
    ('resnet50_14x14_256to1024_k1s1_n128', 128, 14, 14, 256, 1024, 1, 1, 1),
    ('resnet50_14x14_512to512_k3s2_n64', 64, 14, 14, 512, 512, 3, 2, 1),
    ('resnet50_14x14_512to512_k3s2_n128', 128, 14, 14, 512, 512, 3, 2, 1),
    ('resnet50_14x14_1024to256_k1s1_n64', 64, 14, 14, 1024, 256, 1, 1, 1),
    ('resnet50_14x14_1024to256_k1s1_n128', 128, 14, 14, 1024, 256, 1, 1, 1),
    ('resnet50_14x14_1024to512_k1s1_n64', 64, 14, 14, 1024, 512, 1, 1, 1),
    ('resnet50_14x14_1024to512_k1s1_n128', 128, 14, 14, 1024, 512, 1, 1, 1),
    ('resnet50_14x14_1024to2048_k1s2_n64', 64, 14, 14, 1024, 2048, 1, 2, 1),
    ('resnet50_14x14_1024to2048_k1s2_n128', 128, 14, 14, 1024, 2048, 1, 2, 1),
    ('resnet50_7x7_512to512_k3s1_n64', 64, 7, 7, 512, 512, 3, 1, 1),
    ('resnet50_7x7_512to512_k3s1_n128', 128, 7, 7, 512, 512, 3, 1, 1),
    ('resnet50_7x7_512to2048_k1s1_n64', 64, 7, 7, 512, 2048, 1, 1, 1),
    ('resnet50_7x7_512to2048_k1s1_n128', 128, 7, 7, 512, 2048, 1, 1, 1),
    ('resnet50_7x7_2048to512_k1s1_n64', 64, 7, 7, 2048, 512, 1, 1, 1),
    ('resnet50_7x7_2048to512_k1s1_n128', 128, 7, 7, 2048, 512, 1, 1, 1),
    # deeplab
    ('deeplab_257x257_152to64_k1s1_n2', 2, 257, 257, 152, 64, 1, 1, 1),
    ('deeplab_129x129_64to64_k1s1_n2', 2, 129, 129, 64, 64, 1, 1, 1),
    ('deeplab_129x129_64to64_k3s1_n2', 2, 129, 129, 64, 64, 3, 1, 1),
    ('deeplab_129x129_64to256_k1s1_n2', 2, 129, 129, 64, 256, 1, 1, 1),
    ('deeplab_129x129_128to128_k3s2_n2', 2, 129, 129, 128, 128, 3, 2, 1),
    ('deeplab_129x129_256to48_k1s1_n2', 2, 129, 129, 256, 48, 1, 1, 1),
    ('deeplab_129x129_256to48_k1s1_n4', 4, 129, 129, 256, 48, 1, 1, 1),
    ('deeplab_129x129_256to64_k1s1_n2', 2, 129, 129, 256, 64, 1, 1, 1),
    ('deeplab_129x129_256to128_k1s1_n2', 2, 129, 129, 256, 128, 1, 1, 1),
    ('deeplab_129x129_256to512_k1s2_n2', 2, 129, 129, 256, 512, 1, 2, 1),
    ('deeplab_129x129_304to256_k3s1_n2', 2, 129, 129, 304, 256, 3, 1, 1),
    ('deeplab_129x129_304to256_k3s1_n4', 4, 129, 129, 304, 256, 3, 1, 1),
    ('deeplab_65x65_128to128_k3s1_n2', 2, 65, 65, 128, 128, 3, 1, 1),
    ('deeplab_65x65_128to512_k1s1_n2', 2, 65, 65, 128, 512, 1, 1, 1),
    ('deeplab_65x65_256to256_k3s2_n2', 2, 65, 65, 256, 256, 3, 2, 1),
    ('deeplab_65x65_512to128_k1s1_n2', 2, 65, 65, 512, 128, 1, 1, 1),
    ('deeplab_65x65_512to256_k1s1_n2', 2, 65, 65, 512, 256, 1, 1, 1),
    ('deeplab_65x65_512to1024_k1s2_n2', 2, 65, 65, 512, 1024, 1, 2, 1),
    ('deeplab_33x33_256to256_k3s1_n2', 2, 33, 33, 256, 256, 3, 1, 1),
    ('deeplab_33x33_256to1024_k1s1_n2', 2, 33, 33, 256, 1024, 1, 1, 1),
    ('deeplab_33x33_512to512_k3s1_n2', 2, 33, 33, 512, 512, 3, 1, 1),
    ('deeplab_33x33_512to512_k3s1d2_n2', 2, 33, 33, 512, 512, 3, 1, 2),
    ('deeplab_33x33_512to512_k3s1_n4', 4, 33, 33, 512, 512, 3, 1, 1),
    ('deeplab_33x33_512to512_k3s1d2_n4', 4, 33, 33, 512, 512, 3, 1, 2),
    ('deeplab_33x33_512to2048_k1s1_n2', 2, 33, 33, 512, 2048, 1, 1, 1),
    ('deeplab_33x33_512to2048_k1s1_n4', 4, 33, 33, 512, 2048, 1, 1, 1),
    ('deeplab_33x33_1024to256_k1s1_n2', 2, 33, 33, 1024, 256, 1, 1, 1),
    ('deeplab_33x33_1024to512_k1s1_n2', 2, 33, 33, 1024, 512, 1, 1, 1),
    ('deeplab_33x33_1024to512_k1s1_n4', 4, 33, 33, 1024, 512, 1, 1, 1),
    ('deeplab_33x33_1024to2048_k1s1_n2', 2, 33, 33, 1024, 2048, 1, 1, 1),
    ('deeplab_33x33_1024to2048_k1s1_n4', 4, 33, 33, 1024, 2048, 1, 1, 1),
    ('deeplab_33x33_1280to256_k1s1_n2', 2, 33, 33, 1280, 256, 1, 1, 1),
    ('deeplab_33x33_1280to256_k1s1_n4', 4, 33, 33, 1280, 256, 1, 1, 1),
    ('deeplab_33x33_2048to256_k1s1_n2', 2, 33, 33, 2048, 256, 1, 1, 1),
    ('deeplab_33x33_2048to256_k1s1_n4', 4, 33, 33, 2048, 256, 1, 1, 1),
    ('deeplab_33x33_2048to256_k3s1d12_n2', 2, 33, 33, 2048, 256, 3, 1, 12),
    ('deeplab_33x33_2048to256_k3s1d18_n2', 2, 33, 33, 2048, 256, 3, 1, 18),
    ('deeplab_33x33_2048to256_k3s1d6_n2', 2, 33, 33, 2048, 256, 3, 1, 6),
    ('deeplab_33x33_2048to256_k3s1d12_n4', 4, 33, 33, 2048, 256, 3, 1, 12),
    ('deeplab_33x33_2048to256_k3s1d18_n4', 4, 33, 33, 2048, 256, 3, 1, 18),
    ('deeplab_33x33_2048to256_k3s1d6_n4', 4, 33, 33, 2048, 256, 3, 1, 6),
    ('deeplab_33x33_2048to512_k1s1_n2', 2, 33, 33, 2048, 512, 1, 1, 1),
    ('deeplab_33x33_2048to512_k1s1_n4', 4, 33, 33, 2048, 512, 1, 1, 1),
    # faster_rcnn
    ('faster_rcnn_300x452_64to152_k1s1_n1', 1, 300, 452, 64, 152, 1, 1, 1),
    ('faster_rcnn_300x452_152to64_k1s1_n1', 1, 300, 452, 152, 64, 1, 1, 1),
    ('faster_rcnn_150x226_64to64_k1s1_n1', 1, 150, 226, 64, 64, 1, 1, 1),
    ('faster_rcnn_150x226_64to64_k3s1_n1', 1, 150, 226, 64, 64, 3, 1, 1),
    ('faster_rcnn_150x226_64to256_k1s1_n1', 1, 150, 226, 64, 256, 1, 1, 1),
    ('faster_rcnn_150x226_128to128_k3s2_n1', 1, 150, 226, 128, 128, 3, 2, 1),
    ('faster_rcnn_150x226_256to64_k1s1_n1', 1, 150, 226, 256, 64, 1, 1, 1),
    ('faster_rcnn_150x226_256to128_k1s1_n1', 1, 150, 226, 256, 128, 1, 1, 1),
    ('faster_rcnn_150x226_256to512_k1s2_n1', 1, 150, 226, 256, 512, 1, 2, 1),
    ('faster_rcnn_75x113_128to128_k3s1_n1', 1, 75, 113, 128, 128, 3, 1, 1),
    ('faster_rcnn_75x113_128to512_k1s1_n1', 1, 75, 113, 128, 512, 1, 1, 1),
    ('faster_rcnn_75x113_256to256_k3s2_n1', 1, 75, 113, 256, 256, 3, 2, 1),
    ('faster_rcnn_75x113_256to256_k3s2_n3', 3, 75, 113, 256, 256, 3, 2, 1),
    ('faster_rcnn_75x113_512to128_k1s1_n1', 1, 75, 113, 512, 128, 1, 1, 1),
    ('faster_rcnn_75x113_512to256_k1s1_n1', 1, 75, 113, 512, 256, 1, 1, 1),
    ('faster_rcnn_75x113_512to256_k1s1_n3', 3, 75, 113, 512, 256, 1, 1, 1),
    ('faster_rcnn_75x113_512to1024_k1s2_n1', 1, 75, 113, 512, 1024, 1, 2, 1),
    ('faster_rcnn_75x113_512to1024_k1s2_n3', 3, 75, 113, 512, 1024, 1, 2, 1),
    ('faster_rcnn_38x57_256to256_k3s1_n1', 1, 38, 57, 256, 256, 3, 1, 1),
    ('faster_rcnn_38x57_256to256_k3s1_n3', 3, 38, 57, 256, 256, 3, 1, 1),
    ('faster_rcnn_38x57_256to1024_k1s1_n1', 1, 38, 57, 256, 1024, 1, 1, 1),
    ('faster_rcnn_38x57_256to1024_k1s1_n3', 3, 38, 57, 256, 1024, 1, 1, 1),
    ('faster_rcnn_38x57_1024to256_k1s1_n1', 1, 38, 57, 1024, 256, 1, 1, 1),
    ('faster_rcnn_38x57_1024to256_k1s1_n3', 3, 38, 57, 1024, 256, 1, 1, 1),
    ('faster_rcnn_38x57_1024to512_k3s1_n1', 1, 38, 57, 1024, 512, 3, 1, 1),
    ('faster_rcnn_38x57_1024to512_k3s1_n3', 3, 38, 57, 1024, 512, 3, 1, 1),
    ('faster_rcnn_38x57_1024to512_k3s1_n7', 7, 38, 57, 1024, 512, 3, 1, 1),
    ('faster_rcnn_7x7_512to512_k3s2_n128', 128, 7, 7, 512, 512, 3, 2, 1),
    ('faster_rcnn_7x7_512to512_k3s2_n384', 384, 7, 7, 512, 512, 3, 2, 1),
    ('faster_rcnn_7x7_512to512_k3s2_n896', 896, 7, 7, 512, 512, 3, 2, 1),
    ('faster_rcnn_7x7_1024to512_k1s1_n128', 128, 7, 7, 1024, 512, 1, 1, 1),
    ('faster_rcnn_7x7_1024to512_k1s1_n384', 384, 7, 7, 1024, 512, 1, 1, 1),
    ('faster_rcnn_7x7_1024to512_k1s1_n896', 896, 7, 7, 1024, 512, 1, 1, 1),
    ('faster_rcnn_7x7_1024to2048_k1s2_n128', 128, 7, 7, 1024, 2048, 1, 2, 1),
    ('faster_rcnn_7x7_1024to2048_k1s2_n384', 384, 7, 7, 1024, 2048, 1, 2, 1),
    ('faster_rcnn_7x7_1024to2048_k1s2_n896', 896, 7, 7, 1024, 2048, 1, 2, 1),
    ('faster_rcnn_4x4_512to512_k3s1_n128', 128, 4, 4, 512, 512, 3, 1, 1),
    ('faster_rcnn_4x4_512to512_k3s1_n384', 384, 4, 4, 512, 512, 3, 1, 1),
    ('faster_rcnn_4x4_512to512_k3s1_n896', 896, 4, 4, 512, 512, 3, 1, 1),
    ('faster_rcnn_4x4_512to2048_k1s1_n128', 128, 4, 4, 512, 2048, 1, 1, 1),
    ('faster_rcnn_4x4_512to2048_k1s1_n384', 384, 4, 4, 512, 2048, 1, 1, 1),
    ('faster_rcnn_4x4_512to2048_k1s1_n896', 896, 4, 4, 512, 2048, 1, 1, 1),
    ('faster_rcnn_4x4_2048to512_k1s1_n128', 128, 4, 4, 2048, 512, 1, 1, 1),
    ('faster_rcnn_4x4_2048to512_k1s1_n384', 384, 4, 4, 2048, 512, 1, 1, 1),
    ('faster_rcnn_4x4_2048to512_k1s1_n896', 896, 4, 4, 2048, 512, 1, 1, 1),
]

# Edge rows: shapes where a tiled kernel goes wrong, and the variants no workload reaches
EDGE_ROWS = [
    ("edge_ragged_rows_n1", 1, 9, 9, 64, 128, 3, 1, 1),          # M = 81: the last 64 / 128-row tile ragged; n = 1
    ("edge_ragged_rows_odd", 3, 7, 11, 128, 128, 3, 1, 1),       # M = 231, odd width
    ("edge_halo_straddle6", 8, 6, 6, 64, 128, 3, 1, 1),          # halo tiles straddling image borders
    ("edge_halo_straddle10", 6, 10, 10, 128, 256, 3, 1, 1),
    ("edge_s2_odd", 2, 13, 11, 64, 128, 3, 2, 1),                # stride-2 input gradient: unequal parity classes
    ("edge_s2_odd_1x1", 2, 9, 7, 128, 256, 1, 2, 1),             # 1x1 / 2 input gradient at odd sizes: empty classes
    ("edge_1x1_s2", 2, 16, 16, 128, 256, 1, 2, 1),               # 1x1 / 2 input gradient: three classes exactly zero
    ("edge_ch40_48", 2, 10, 10, 40, 48, 3, 1, 1),                # ragged channel chunks / tiles
    ("edge_ch48_40_s2", 2, 11, 9, 48, 40, 1, 2, 1),
    ("edge_ch152", 2, 12, 12, 152, 64, 1, 1, 1),
    ("edge_ch304", 1, 10, 10, 304, 304, 3, 1, 1),
    ("edge_ch1280", 2, 7, 7, 1280, 256, 1, 1, 1),
    ("edge_atrous_out", 2, 9, 9, 128, 128, 3, 1, 12),            # every tap but the centre outside the map
    ("edge_atrous_part", 1, 10, 10, 64, 64, 3, 1, 6),            # some taps outside, some in
    ("edge_stem_n1", 1, 5, 64, 3, 16, 3, 1, 1),                  # the 3-channel stem
    ("edge_stem7_odd", 1, 21, 19, 3, 64, 7, 2, 1),               # the 7x7 / 2 stem at odd sizes
]

ROWS = WORKLOAD_ROWS + EDGE_ROWS
IDS = [r[0] for r in ROWS]

# The instantiations the table launches with default settings (test_every_default_variant_is_pinned): every tiled form dispatch()
# picks, as forward and input gradient, with the group-straddling epilogue (gs1) where a forward takes per-half moments; the
# 64-channel, small-channel and stem kernels; the weight-gradient tiles with and without the incremental pixel walk.
# Not reachable with default settings: igemm_fwd<64,128,3,2,4,...> — a forward launch has one class, so choose_bm() gives 64-row
# tiles only below 257 workgroups of 64 rows, where the four-stage forms take it (the input gradient's four classes reach it);
# the dgrad gs1 forms need grouped BatchNorm-backward sums (allowlisted below).
EXPECTED_VARIANTS = {
    'c64_dgrad',
    'c64_fwd',
    'igemm_dgrad<128,128,3,2,4,0,4,0,gs0,bf0>',
    'igemm_dgrad<128,128,5,2,2,4,4,0,gs0,bf0>',
    'igemm_dgrad<128,128,5,2,2,4,4,320,gs0,bf0>',
    'igemm_dgrad<128,64,3,4,2,0,4,0,gs0,bf0>',
    'igemm_dgrad<128,64,7,2,2,4,4,320,gs0,bf0>',
    'igemm_dgrad<256,128,5,4,2,4,2,328,gs0,bf0>',
    'igemm_dgrad<256,64,7,4,1,4,2,400,gs0,bf0>',
    'igemm_dgrad<64,128,3,2,4,0,4,0,gs0,bf0>',
    'igemm_dgrad<64,128,5,2,2,4,4,0,gs0,bf0>',
    'igemm_dgrad<64,128,5,2,2,4,4,320,gs0,bf0>',
    'igemm_dgrad<64,64,3,2,2,0,4,0,gs0,bf0>',
    'igemm_dgrad<64,64,5,2,2,4,4,0,gs0,bf0>',
    'igemm_dgrad<64,64,7,2,2,4,4,320,gs0,bf0>',
    'igemm_fwd<128,128,3,2,4,0,4,0,gs0,bf0>',
    'igemm_fwd<128,128,3,2,4,0,4,0,gs1,bf0>',
    'igemm_fwd<128,128,5,2,2,4,4,0,gs0,bf0>',
    'igemm_fwd<128,128,5,2,2,4,4,0,gs1,bf0>',
    'igemm_fwd<128,128,5,2,2,4,4,320,gs0,bf0>',
    'igemm_fwd<128,128,5,2,2,4,4,320,gs1,bf0>',
    'igemm_fwd<128,64,3,4,2,0,4,0,gs0,bf0>',
    'igemm_fwd<128,64,3,4,2,0,4,0,gs1,bf0>',
    'igemm_fwd<128,64,7,2,2,4,4,320,gs0,bf0>',
    'igemm_fwd<128,64,7,2,2,4,4,320,gs1,bf0>',
    'igemm_fwd<256,128,5,4,2,4,2,328,gs0,bf0>',
    'igemm_fwd<256,64,7,4,1,4,2,400,gs0,bf0>',
    'igemm_fwd<64,128,5,2,2,4,4,0,gs0,bf0>',
    'igemm_fwd<64,128,5,2,2,4,4,0,gs1,bf0>',
    'igemm_fwd<64,128,5,2,2,4,4,320,gs0,bf0>',
    'igemm_fwd<64,128,5,2,2,4,4,320,gs1,bf0>',
    'igemm_fwd<64,64,3,2,2,0,4,0,gs0,bf0>',
    'igemm_fwd<64,64,3,2,2,0,4,0,gs1,bf0>',
    'igemm_fwd<64,64,5,2,2,4,4,0,gs0,bf0>',
    'igemm_fwd<64,64,5,2,2,4,4,0,gs1,bf0>',
    'igemm_fwd<64,64,7,2,2,4,4,320,gs0,bf0>',
    'igemm_fwd<64,64,7,2,2,4,4,320,gs1,bf0>',
    'small_dgrad<1>',
    'small_dgrad<2>',
    'small_dgrad<4>',
    'small_fwd<1>',
    'small_fwd<2>',
    'stem7_fwd',
    'stem7_wgrad',
    'stem_fwd<1>',
    'stem_fwd<2>',
    'stem_wgrad<1>',
    'stem_wgrad<2>',
    'wgrad<128,128,inc0>',
    'wgrad<128,128,inc1>',
    'wgrad<128,64,inc0>',
    'wgrad<128,64,inc1>',
    'wgrad<64,128,inc0>',
    'wgrad<64,64,inc0>',
    'wgrad<64,64,inc1>',
    'wgrad_small',
}

# Instantiations a workload launches that no table row of THIS module reaches: the fused forms, each pinned elementwise to float64 by the
# named test of tests/test_conv_fused_pinned_gpu.py (whose own coverage test holds its tables to exactly these keys):
#   *bf1: the in-launch BatchNorm (afan_conv_fwd_bn / afan_conv_dgrad_bn);
#   dgrad *gs1: the input gradient with grouped BatchNorm-backward sums, a half-batch that is not a whole number of row tiles;
#   wgrad_multi<...>: several layers' weight gradients in one launch.
_BNF_FWD = "tests/test_conv_fused_pinned_gpu.py::test_conv_fwd_bn_pinned"
_BNF_DGRAD = "tests/test_conv_fused_pinned_gpu.py::test_conv_dgrad_bn_pinned"
_GROUPED = "tests/test_conv_fused_pinned_gpu.py::test_grouped_dgrad_sums_pinned"
_WMULTI = "tests/test_conv_fused_pinned_gpu.py::test_conv_wgrad_multi_pinned"
FUSED_ALLOWLIST = {
    "igemm_fwd<128,128,3,2,4,0,4,0,gs0,bf1>": _BNF_FWD,
    "igemm_fwd<128,128,5,2,2,4,4,0,gs0,bf1>": _BNF_FWD,
    "igemm_fwd<128,64,7,2,2,4,4,320,gs0,bf1>": _BNF_FWD,
    "igemm_fwd<256,128,5,4,2,4,2,328,gs0,bf1>": _BNF_FWD,
    "igemm_fwd<256,64,7,4,1,4,2,400,gs0,bf1>": _BNF_FWD,
    "igemm_fwd<64,128,5,2,2,4,4,0,gs0,bf1>": _BNF_FWD,
    "igemm_fwd<64,64,5,2,2,4,4,0,gs0,bf1>": _BNF_FWD,
    "igemm_fwd<64,64,7,2,2,4,4,320,gs0,bf1>": _BNF_FWD,
    "igemm_dgrad<128,128,3,2,4,0,4,0,gs0,bf1>": _BNF_DGRAD,
    "igemm_dgrad<128,128,5,2,2,4,4,0,gs0,bf1>": _BNF_DGRAD,
    "igemm_dgrad<128,64,7,2,2,4,4,320,gs0,bf1>": _BNF_DGRAD,
    "igemm_dgrad<256,128,5,4,2,4,2,328,gs0,bf1>": _BNF_DGRAD,
    "igemm_dgrad<256,64,7,4,1,4,2,400,gs0,bf1>": _BNF_DGRAD,
    "igemm_dgrad<64,128,5,2,2,4,4,0,gs0,bf1>": _BNF_DGRAD,
    "igemm_dgrad<64,64,5,2,2,4,4,0,gs0,bf1>": _BNF_DGRAD,
    "igemm_dgrad<64,64,7,2,2,4,4,320,gs0,bf1>": _BNF_DGRAD,
    "igemm_dgrad<128,128,3,2,4,0,4,0,gs1,bf0>": _GROUPED,
    "igemm_dgrad<128,128,5,2,2,4,4,0,gs1,bf0>": _GROUPED,
    "igemm_dgrad<128,128,5,2,2,4,4,320,gs1,bf0>": _GROUPED,
    "wgrad_multi<128,128,inc0>": _WMULTI,
    "wgrad_multi<128,128,inc1>": _WMULTI,
    "wgrad_multi<128,64,inc0>": _WMULTI,
    "wgrad_multi<64,64,inc0>": _WMULTI,
    "wgrad_multi<64,64,inc1>": _WMULTI,
}


def _base_form(name):
    """The plain instantiation an allowlisted fused form is held equal to."""
    return name.replace(",bf1>", ",bf0>").replace(",gs1,", ",gs0,").replace("wgrad_multi<", "wgrad<")

TUNING_PREFIXES = ("AFAN_CONV_", "AFAN_WGRAD_", "AFAN_C64", "AFAN_STEM")


def _tuned():
    return sorted(k for k in os.environ if k.startswith(TUNING_PREFIXES))


# -------------------------------------------------------------------------------------------------------------- helpers
def _pad(k, d):
    return d * (k // 2)


def _out_hw(hi, wi, k, s, d):
    p = _pad(k, d)
    return (hi + 2 * p - d * (k - 1) - 1) // s + 1, (wi + 2 * p - d * (k - 1) - 1) // s + 1


def _is_stem7(row):
    return row[4] == 3 and row[6] == 7


def _ternary(shape, density, g, dev):
    v = torch.randint(-1, 2, shape, generator=g, device=dev, dtype=torch.int8)
    keep = torch.rand(shape, generator=g, device=dev) < density
    return (v * keep).to(torch.bfloat16)


def _gauss(shape, scale, g, dev):
    return (torch.randn(shape, generator=g, device=dev) * scale).to(torch.bfloat16)


def _cl(t):
    return t.contiguous(memory_format=CL)


def _key(b):
    """bf16 tensor -> integer key monotone in the value (adjacent bf16 values differ by 1)."""
    i = b.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i >= 0, i, -32768 - i)


def _ref_fwd(x, w, s, d):
    k = w.shape[-1]
    return F.conv2d(x.double(), w.double(), None, s, _pad(k, d), d)


def _ref_dgrad(dy, w, in_shape, s, d):
    k = w.shape[-1]
    return torch.nn.grad.conv2d_input(in_shape, w.double(), dy.double(), s, _pad(k, d), d)


def _ref_wgrad(x, dy, w_shape, s, d):
    k = w_shape[-1]
    return torch.nn.grad.conv2d_weight(x.double(), w_shape, dy.double(), s, _pad(k, d), d)


def _kernels(t):
    return sorted({r["kernel"] for r in t.records})


def _check_bf16(got, ref, bound, what):
    """got: bf16 kernel output; ref: float64; bound: float64 S.  The kernel rounds an fp32 sum within C_BF16 * 2^-24 * S of ref, so
    got must lie between the RNE bf16 of ref - tol and of ref + tol: the RNE bf16 of ref itself unless a rounding midpoint lies within
    tol of ref, then also the neighbour across it (and, where cancellation leaves |ref| << S, every bf16 value of that window)."""
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    tol = C_BF16 * 2.0 ** -24 * bound
    gk = _key(got)
    lo, hi = _key((ref - tol).float().to(torch.bfloat16)), _key((ref + tol).float().to(torch.bfloat16))
    bad = (gk < lo) | (gk > hi)
    nbad = int(bad.sum())
    if nbad:
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {nbad} of {got.numel()} elements are not the RNE bf16 of a value within {C_BF16} * 2^-24 * S of "
                             f"the float64 result; first at {idx}: got {float(got[tuple(idx)])}, float64 {float(ref[tuple(idx)])}, "
                             f"S {float(bound[tuple(idx)])}")
    # how many elements took the other neighbour: the window must stay the exception, not the rule
    off = int((gk != _key(ref.float().to(torch.bfloat16))).sum())
    assert off <= max(8, got.numel() // 1000), f"{what}: {off} of {got.numel()} elements off the RNE bf16 of the float64 result"


def _check_exact(got, ref, what):
    g = got.double()
    ok = g == ref
    if not bool(ok.all()):
        nbad = int((~ok).sum())
        idx = (~ok).nonzero()[0].tolist()
        raise AssertionError(f"{what}: {nbad} of {got.numel()} elements differ from the exact float64 result; first at {idx}: "
                             f"got {float(g[tuple(idx)])}, exact {float(ref[tuple(idx)])}")


def _density(reduction, target=48.0):
    """per-operand density for ~target nonzero products per output, so that |result| stays far below 256."""
    return min(1.0, (target / max(reduction, 1)) ** 0.5)


def _assert_exact_range(ref, bound, limit, what):
    assert float(ref.abs().max()) <= limit, f"{what}: exact operands give |result| > {limit}: not exact in the output type"
    assert float(bound.max()) < 2.0 ** 24, f"{what}: sum |a*b| >= 2^24: fp32 partial sums may round"


def _seed(row, salt):
    return (zlib.crc32(repr(row).encode()) * 31 + salt) % (1 << 31)


# --------------------------------------------------------------------------------------------------------------- callers
def _fwd(pkg, x, w, row):
    _, n, hi, wi, ci, co, k, s, d = row
    if _is_stem7(row):
        return pkg.ops.conv_stem7_fwd(x, w)
    return pkg.ops.conv_fwd(x, w, s, dilation=d)


def _wt(w):
    return _cl(w.permute(1, 0, 2, 3))


def _dgrad(pkg, dy, w, row, addend=None):
    _, n, hi, wi, ci, co, k, s, d = row
    return pkg.ops.conv_dgrad(dy, _wt(w), (hi, wi), s, addend=addend, dilation=d)


def _wgrad(pkg, x, dy, row, grad=None, accumulate=False):
    _, n, hi, wi, ci, co, k, s, d = row
    if _is_stem7(row):
        return pkg.ops.conv_stem7_wgrad(x, dy, grad=grad, accumulate=accumulate)
    return pkg.ops.conv_wgrad(x, dy, k, s, grad=grad, accumulate=accumulate, dilation=d)


def _fwd_grouped(pkg, x, w, s, shift, d):
    """conv_fwd with per-half moments (groups = 2), or None where the library declines the shape (AFAN_ESHAPE: nothing ran)."""
    try:
        return pkg.ops.conv_fwd(x, w, s, stats_shift=shift, want_stats=True, groups=2, dilation=d)
    except pkg._lib.AfanLibraryError as e:
        if "AFAN_ESHAPE" not in str(e):
            raise
        return None


def _has_dgrad(row):
    return row[4] != 3


# ------------------------------------------------------------------------------------------------------- numerical pins
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_fwd_pinned(pkg, gpu, row):
    tag, n, hi, wi, ci, co, k, s, d = row
    ho, wo = _out_hw(hi, wi, k, s, d)
    g = torch.Generator(device=gpu).manual_seed(_seed(row, 1))
    # exact
    p = _density(k * k * ci)
    x, w = _cl(_ternary((n, ci, hi, wi), p, g, gpu)), _cl(_ternary((co, ci, k, k), p, g, gpu))
    with pkg.ops.conv_trace() as t:
        y = _fwd(pkg, x, w, row)
    ref = _ref_fwd(x, w, s, d)
    S = _ref_fwd(x.abs(), w.abs(), s, d)
    what = f"fwd {tag} exact on {_kernels(t)}"
    _assert_exact_range(ref, S, 256, what)
    assert y.shape == (n, co, ho, wo)
    _check_exact(y, ref, what)
    # Gaussian
    x, w = _cl(_gauss((n, ci, hi, wi), 1.0, g, gpu)), _cl(_gauss((co, ci, k, k), (k * k * ci) ** -0.5, g, gpu))
    with pkg.ops.conv_trace() as t:
        y = _fwd(pkg, x, w, row)
    _check_bf16(y, _ref_fwd(x, w, s, d), _ref_fwd(x.abs(), w.abs(), s, d), f"fwd {tag} Gaussian on {_kernels(t)}")
    # the moments taken in the epilogue: same raw output, float64 moments of the stored bf16 output
    if _is_stem7(row):
        return
    shift = (torch.randn(co, generator=g, device=gpu) * 0.1).float()
    with pkg.ops.conv_trace() as t:
        y2, st = pkg.ops.conv_fwd(x, w, s, stats_shift=shift, want_stats=True, dilation=d)
    what = f"fwd {tag} want_stats on {_kernels(t)}"
    assert torch.equal(y2.view(torch.int16), y.view(torch.int16)), f"{what}: raw output differs from the plain call's"
    if st is None:
        return
    c = (y.double() - shift.double().view(1, co, 1, 1))
    m1, m2 = c.sum(dim=(0, 2, 3)), (c * c).sum(dim=(0, 2, 3))
    if st.acc is not None:
        ns = st.acc.numel() // (2 * co)
        a = st.acc[:ns * 2 * co].view(ns, 2, co).sum(0)
    else:
        a = st.partials[:2 * co * st.g].view(2, co, st.g).double().sum(-1)
    tol1 = C_MOMENTS * 2.0 ** -24 * c.abs().sum(dim=(0, 2, 3)) + 1e-30
    tol2 = C_MOMENTS * 2.0 ** -24 * m2 + 1e-30
    assert bool(((a[0] - m1).abs() <= tol1).all()), f"{what}: first moment off: max {float((a[0] - m1).abs().max())}"
    assert bool(((a[1] - m2).abs() <= tol2).all()), f"{what}: second moment off: max {float((a[1] - m2).abs().max())}"
    # grouped moments (two concatenated half-batches, the final passes' form): per-half sums, the same raw output
    if n % 2 or st.acc is None:
        return
    with pkg.ops.conv_trace() as t:
        r3 = _fwd_grouped(pkg, x, w, s, shift, d)
    if r3 is None:
        return
    y3, st3 = r3
    what = f"fwd {tag} want_stats groups=2 on {_kernels(t)}"
    assert torch.equal(y3.view(torch.int16), y.view(torch.int16)), f"{what}: raw output differs from the plain call's"
    for h in range(2):
        ch = c[h * (n // 2):(h + 1) * (n // 2)]
        acc = st3.group(h, co).acc
        a = acc[:ns * 2 * co].view(ns, 2, co).sum(0)
        m1, m2 = ch.sum(dim=(0, 2, 3)), (ch * ch).sum(dim=(0, 2, 3))
        assert bool(((a[0] - m1).abs() <= C_MOMENTS * 2.0 ** -24 * ch.abs().sum(dim=(0, 2, 3)) + 1e-30).all()), f"{what}: half {h} first moment off"
        assert bool(((a[1] - m2).abs() <= C_MOMENTS * 2.0 ** -24 * m2 + 1e-30).all()), f"{what}: half {h} second moment off"


@pytest.mark.parametrize("row", [r for r in ROWS if _has_dgrad(r)], ids=[r[0] for r in ROWS if _has_dgrad(r)])
def test_dgrad_pinned(pkg, gpu, row):
    tag, n, hi, wi, ci, co, k, s, d = row
    ho, wo = _out_hw(hi, wi, k, s, d)
    g = torch.Generator(device=gpu).manual_seed(_seed(row, 2))
    # exact, without and with the addend
    p = _density(k * k * co)
    dy, w = _cl(_ternary((n, co, ho, wo), p, g, gpu)), _cl(_ternary((co, ci, k, k), p, g, gpu))
    add = _cl(_ternary((n, ci, hi, wi), 0.5, g, gpu))
    ref = _ref_dgrad(dy, w, (n, ci, hi, wi), s, d)
    S = _ref_dgrad(dy.abs(), w.abs(), (n, ci, hi, wi), s, d)
    with pkg.ops.conv_trace() as t:
        dx = _dgrad(pkg, dy, w, row)
    what = f"dgrad {tag} exact on {_kernels(t)}"
    _assert_exact_range(ref + add.double(), S, 256, what)
    _check_exact(dx, ref, what)
    with pkg.ops.conv_trace() as t:
        dxa = _dgrad(pkg, dy, w, row, addend=add)
    _check_exact(dxa, ref + add.double(), f"dgrad+addend {tag} exact on {_kernels(t)}")
    # Gaussian; the addend is a second rounding: bf16(bf16(dgrad) + addend), the separate add's arithmetic
    dy, w = _cl(_gauss((n, co, ho, wo), 1.0, g, gpu)), _cl(_gauss((co, ci, k, k), (k * k * co) ** -0.5, g, gpu))
    add = _cl(_gauss((n, ci, hi, wi), 1.0, g, gpu))
    with pkg.ops.conv_trace() as t:
        dx = _dgrad(pkg, dy, w, row)
    _check_bf16(dx, _ref_dgrad(dy, w, (n, ci, hi, wi), s, d), _ref_dgrad(dy.abs(), w.abs(), (n, ci, hi, wi), s, d),
                f"dgrad {tag} Gaussian on {_kernels(t)}")
    with pkg.ops.conv_trace() as t:
        dxa = _dgrad(pkg, dy, w, row, addend=add)
    want = (dx.float() + add.float()).to(torch.bfloat16)
    assert torch.equal(dxa.view(torch.int16), want.view(torch.int16)), \
        f"dgrad+addend {tag} Gaussian on {_kernels(t)}: not bf16(bf16(dgrad) + addend)"


_wgrad_worst = {}


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_wgrad_pinned(pkg, gpu, row):
    tag, n, hi, wi, ci, co, k, s, d = row
    ho, wo = _out_hw(hi, wi, k, s, d)
    g = torch.Generator(device=gpu).manual_seed(_seed(row, 3))
    wshape = (co, ci, k, k)
    # exact, plain and accumulating into an integer start
    p = _density(n * ho * wo, target=4096.0)
    x, dy = _cl(_ternary((n, ci, hi, wi), p, g, gpu)), _cl(_ternary((n, co, ho, wo), p, g, gpu))
    ref = _ref_wgrad(x, dy, wshape, s, d)
    S = _ref_wgrad(x.abs(), dy.abs(), wshape, s, d)
    start = _cl(torch.randint(-64, 65, wshape, generator=g, device=gpu).float())
    with pkg.ops.conv_trace() as t:
        gw = _wgrad(pkg, x, dy, row)
    what = f"wgrad {tag} exact on {_kernels(t)}"
    _assert_exact_range(ref.abs() + 64, S + 64, 2.0 ** 24, what)
    _check_exact(gw, ref, what)
    acc = start.clone()
    with pkg.ops.conv_trace() as t:
        _wgrad(pkg, x, dy, row, grad=acc, accumulate=True)
    _check_exact(acc, ref + start.double(), f"wgrad accumulate {tag} exact on {_kernels(t)}")
    # Gaussian
    x, dy = _cl(_gauss((n, ci, hi, wi), 1.0, g, gpu)), _cl(_gauss((n, co, ho, wo), 1.0, g, gpu))
    ref = _ref_wgrad(x, dy, wshape, s, d)
    S = _ref_wgrad(x.abs(), dy.abs(), wshape, s, d)
    with pkg.ops.conv_trace() as t:
        gw = _wgrad(pkg, x, dy, row)
    ratio = float(((gw.double() - ref).abs() / (2.0 ** -24 * S + 1e-300)).max())
    _wgrad_worst[tag] = ratio
    assert ratio <= C_WGRAD, f"wgrad {tag} Gaussian on {_kernels(t)}: |g - g64| = {ratio:.1f} * 2^-24 * S > {C_WGRAD}"
    start = _cl(torch.randn(wshape, generator=g, device=gpu))
    acc = start.clone()
    with pkg.ops.conv_trace() as t:
        _wgrad(pkg, x, dy, row, grad=acc, accumulate=True)
    # accumulate: one more fp32 addition onto the reduced gradient
    err = (acc.double() - (ref + start.double())).abs()
    lim = C_WGRAD * 2.0 ** -24 * S + 2.0 ** -23 * (ref.abs() + start.double().abs())
    assert bool((err <= lim).all()), f"wgrad accumulate {tag} Gaussian on {_kernels(t)}: max excess {float((err - lim).max())}"


def test_float64_reference_matches_cpu(gpu):
    """The GPU float64 references (aten's im2col + GEMM) against the CPU's on a few small problems of every direction."""
    g = torch.Generator().manual_seed(11)
    for (n, hi, wi, ci, co, k, s, d) in ((2, 9, 7, 40, 48, 3, 2, 1), (1, 10, 10, 64, 64, 3, 1, 6), (2, 9, 7, 128, 256, 1, 2, 1),
                                         (1, 21, 19, 3, 64, 7, 2, 1)):
        x = torch.randn(n, ci, hi, wi, generator=g, dtype=torch.float64)
        w = torch.randn(co, ci, k, k, generator=g, dtype=torch.float64)
        y = _ref_fwd(x, w, s, d)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        for a, b in ((_ref_fwd(x.to(gpu), w.to(gpu), s, d), y),
                     (_ref_dgrad(dy.to(gpu), w.to(gpu), x.shape, s, d), _ref_dgrad(dy, w, x.shape, s, d)),
                     (_ref_wgrad(x.to(gpu), dy.to(gpu), w.shape, s, d), _ref_wgrad(x, dy, w.shape, s, d))):
            np.testing.assert_allclose(a.cpu().numpy(), b.numpy(), rtol=1e-12, atol=1e-12)


# ----------------------------------------------------------------------------------------------------------- coverage
def _launch_row(pkg, row, dev):
    """Every direction and epilogue form the numerical pins run for one row, on zero operands (the trace is what matters)."""
    tag, n, hi, wi, ci, co, k, s, d = row
    ho, wo = _out_hw(hi, wi, k, s, d)
    x = _cl(torch.zeros(n, ci, hi, wi, dtype=torch.bfloat16, device=dev))
    w = _cl(torch.zeros(co, ci, k, k, dtype=torch.bfloat16, device=dev))
    dy = _cl(torch.zeros(n, co, ho, wo, dtype=torch.bfloat16, device=dev))
    _fwd(pkg, x, w, row)
    if not _is_stem7(row):
        _, st = pkg.ops.conv_fwd(x, w, s, stats_shift=torch.zeros(co, device=dev), want_stats=True, dilation=d)
        if n % 2 == 0 and st is not None and st.acc is not None:
            _fwd_grouped(pkg, x, w, s, torch.zeros(co, device=dev), d)
    if _has_dgrad(row):
        _dgrad(pkg, dy, w, row)
        _dgrad(pkg, dy, w, row, addend=x)
    gw = _wgrad(pkg, x, dy, row)
    _wgrad(pkg, x, dy, row, grad=gw, accumulate=True)


def _variants(records):
    return {r["kernel"] for r in records}


def test_every_default_variant_is_pinned(pkg, gpu):
    if _tuned():
        pytest.skip(f"kernel tuning variables set ({_tuned()}): dispatch is not the default one")
    per_row = {}
    for row in ROWS:
        with pkg.ops.conv_trace() as t:
            _launch_row(pkg, row, gpu)
        for r in t.records:
            per_row.setdefault(r["kernel"], row[0])
        assert all(r["op"] is not None for r in t.records), f"{row[0]}: a launch without a named problem"
    torch.cuda.synchronize()
    got = set(per_row)
    assert got == EXPECTED_VARIANTS, (f"table reaches {sorted(got - EXPECTED_VARIANTS)} beyond EXPECTED_VARIANTS "
                                      f"(first rows: {[per_row[v] for v in sorted(got - EXPECTED_VARIANTS)]}), "
                                      f"misses {sorted(EXPECTED_VARIANTS - got)}")


# ------------------------------------------------------------------------------------------------------ the workloads
def _classifier_iteration(pkg, dev, arch, batch, side, ncls, K):
    torch.manual_seed(3)
    ctor, idx = pkg.resnet_s.ARCHS[arch]
    m = ctor()
    m.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).train()
    tr = pkg.train_step.AfanTrainer(m, nn.CrossEntropyLoss(), steps=K, gamma=0.5, eps=2.0, perturb_idx=idx, lr=0.1)
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand(batch, 3, side, side, generator=g).to(dev), torch.randint(0, ncls, (batch,), generator=g).to(dev)
    with pkg.ops.conv_trace() as t:
        for _ in range(3):                 # eager, then the hipGraph capture
            tr.step(x, y)
        torch.cuda.synchronize()
    return t.records


def _deeplab_iteration(pkg, dev):
    torch.manual_seed(3)
    model = pkg.deeplab.deeplabv3plus_resnet101(num_classes=21, output_stride=16)
    model.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).train()
    tr = pkg.seg_trainer.SegTrainer(model, nn.CrossEntropyLoss(ignore_index=255, reduction="mean"), steps=3, eps=2.0, gamma_se=0.5,
                                    gamma_sd=0.5, pertub_idx_se=3, pertub_idx_sd="aspp", mix_layer="11", mix_sd=True, lr=0.01)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 513, 513, generator=g)
    y = torch.randint(0, 21, (2, 513, 513), generator=g)
    y[torch.rand(2, 513, 513, generator=g) < 0.05] = 255
    with pkg.ops.conv_trace() as t:
        for _ in range(3):
            tr.step(x.to(dev), y.to(dev))
            tr.scheduler.step()
        torch.cuda.synchronize()
    return t.records


def _faster_rcnn_iteration(pkg, dev):
    torch.manual_seed(3)
    model = pkg.det_model.fasterrcnn_resnet101(21, pooler_mode="align")
    for b in model.modules():
        if isinstance(b, pkg.det_model.Bottleneck):
            b.bn3.weight.data.mul_(0.2)
    model.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).train()
    tr = pkg.det_trainer.DetTrainer(model, lr=0.001, momentum=0.9, weight_decay=0.0005, loss_settings=1, noise_ahead=True)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(1, 3, 600, 904, generator=g).to(dev)
    x0, y0 = torch.rand(1, 6, 1, generator=g) * (904 - 260), torch.rand(1, 6, 1, generator=g) * (600 - 260)
    wh = 60 + torch.rand(1, 6, 2, generator=g) * 200
    boxes = torch.cat([x0, y0, x0 + wh[..., :1], y0 + wh[..., 1:]], dim=-1).to(dev)
    labels = torch.randint(1, 21, (1, 6), generator=g).to(dev)
    with pkg.ops.conv_trace() as t:
        torch.manual_seed(1)
        tr.step(x, boxes, labels)
        torch.cuda.synchronize()
    return t.records


WORKLOADS = {
    "resnet18": lambda pkg, dev: _classifier_iteration(pkg, dev, "resnet18", 256, 32, 10, 5),
    "resnet20s": lambda pkg, dev: _classifier_iteration(pkg, dev, "resnet20s", 128, 32, 10, 5),
    "resnet56s": lambda pkg, dev: _classifier_iteration(pkg, dev, "resnet56s", 128, 32, 10, 5),
    "resnet50": lambda pkg, dev: _classifier_iteration(pkg, dev, "resnet50", 64, 224, 1000, 3),
    "deeplab": _deeplab_iteration,
    "faster_rcnn": _faster_rcnn_iteration,
}


def _problem_of(row):
    return tuple(row[1:])


@pytest.mark.parametrize("workload", sorted(WORKLOADS))
def test_workload_launches_are_pinned(pkg, gpu, workload):
    if _tuned():
        pytest.skip(f"kernel tuning variables set ({_tuned()}): dispatch is not the default one")
    records = WORKLOADS[workload](pkg, gpu)
    assert records, "no convolution launch traced"
    table = {_problem_of(r) for r in ROWS}
    unnamed = [r for r in records if r["op"] is None]
    assert not unnamed, f"{workload}: launches without a named problem: {sorted({r['kernel'] for r in unnamed})}"
    missing = sorted({(r["op"],) + r["problem"] for r in records if r["problem"] not in table})
    assert not missing, f"{workload}: problems not in the table (op, n, hi, wi, ci, co, k, stride, dilation): {missing}"
    unpinned = sorted({r["kernel"] for r in records} - EXPECTED_VARIANTS - set(FUSED_ALLOWLIST))
    assert not unpinned, f"{workload}: instantiations neither pinned nor allowlisted: {unpinned}"


def test_allowlisted_forms_stand_for_pinned_ones():
    """Every allowlisted fused form's plain instantiation is pinned, and none is pinned itself (then it needs no allowlist)."""
    assert not set(FUSED_ALLOWLIST) & EXPECTED_VARIANTS, sorted(set(FUSED_ALLOWLIST) & EXPECTED_VARIANTS)
    assert all(_base_form(k) in EXPECTED_VARIANTS for k in FUSED_ALLOWLIST), \
        sorted(k for k in FUSED_ALLOWLIST if _base_form(k) not in EXPECTED_VARIANTS)
