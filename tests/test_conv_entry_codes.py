"""The return code of every bf16 convolution entry for calls that are refused before anything is launched: a literal table of
(entry, arguments) -> code, recorded from library version 100 (through the entry names it had: the affine and bottleneck entries of
that version map onto today's as include/afan_hip.h states) and never regenerated from a later build.  It pins which of AFAN_ENULL /
AFAN_EALIGN / AFAN_ESHAPE wins where several apply, so that the host code in front of the launches can be reshaped without a caller
seeing a different answer.

Every row is one entry's BASE call (a problem the tiled kernel would take) with a few arguments replaced.  All pointers are host
addresses that the library never dereferences (the pointer arrays of the multi-problem entries are real arrays), so no GPU is
needed.

Rows left out, because the call would go on to a launch (or to a query of the device):
  * every base call itself, and a misaligned coefficient / alpha row on a shape of the tiled kernel (only the small-channel and the
    64 -> 64 kernels read those rows as 16-byte vectors);
  * what only dispatch_bnf or launch_gs refuse for the in-launch BatchNorm forms (co % 128, residency, class sizes);
  * a 64 -> 64 problem at dilation > 1 in the input-gradient affine entry with any_family = 1 (it goes to the tiled kernel);
  * the bottleneck backward with g given beyond its own argument checks (its first step is a launch);
  * "unequal output sizes" in the multi-problem forward: with k in {1, 3} and padding dilation * (k / 2) every problem has the output
    size (h - 1) / stride + 1, so that refusal cannot be reached through arguments that pass the checks in front of it."""
import ctypes

ESHAPE, ENULL, EALIGN = -3, -4, -2

# pointer tokens
P = "P"            # aligned to 64 bytes
ODD = "ODD"        # P + 2: aligned to 2 bytes only
ODD1 = "ODD1"      # P + 1
P16 = "P16"        # P + 16: aligned to 16 bytes, not to 64 (the grid barrier's alignment)
FAR = "FAR"        # P + 1 MiB: "behind dy in one allocation", further than one tensor
NEAR = "NEAR"      # P + 64: closer than one tensor

_PTR_ARRAYS = {"w", "y", "stats_shift", "stats_acc"}          # of the multi-problem entries
_INT_ARRAYS = {"ksize", "dilation"}
_FLOATS = {"eps", "momentum", "sc_eps", "sc_momentum"}

# entry -> (C symbol, argument names, base call)
ENTRIES = {
    "fwd": ("afan_conv_fwd_nhwc_bf16",
            "x w y n hi wi ci co k stride dilation stats_partials stats_shift stats_acc groups stream",
            (P, P, P, 2, 8, 8, 128, 128, 3, 1, 1, None, None, None, 1, None)),
    "dgrad": ("afan_conv_dgrad_nhwc_bf16",
              "dy wt dx n hi wi ci co k stride dilation addend bn_x bn_stats bn_relu bn_y bn_partials bn_acc groups stream",
              (P, P, P, 2, 8, 8, 128, 128, 3, 1, 1, None, None, None, 0, None, None, None, 1, None)),
    "fwd_affine": ("afan_conv_fwd_affine_nhwc_bf16",
                   "x w y n hi wi ci co k stride dilation coefs residual relu any_family stream",
                   (P, P, P, 2, 8, 8, 128, 128, 3, 1, 1, P, None, 1, 0, None)),
    "dgrad_affine": ("afan_conv_dgrad_affine_nhwc_bf16",
                     "dy wt dx n hi wi ci co k stride dilation alpha act any_family stream",
                     (P, P, P, 2, 8, 8, 128, 128, 3, 1, 1, P, P, 0, None)),
    "dgrad_dual": ("afan_conv_dgrad_dual_nhwc_bf16",
                   "dy wt d3 dres n hi wi ci co k stride addend alpha act stream",
                   (P, P, P, P, 2, 8, 8, 128, 128, 1, 1, None, P, P, None)),
    "dgrad_sc": ("afan_conv_dgrad_sc_nhwc_bf16",
                 "dy dy_sc wt10 dx n hi wi ci co bn_x bn_stats bn_relu bn_y bn_partials bn_acc stream",
                 (P, FAR, P, P, 2, 8, 8, 128, 128, None, None, 0, None, None, None, None)),
    "fwd_multi": ("afan_conv_fwd_multi_nhwc_bf16",
                  "x w y nb n hi wi ci co ksize stride dilation stats_shift stats_acc groups stream",
                  (P, [P, P], [P, P], 2, 2, 8, 8, 128, 128, [3, 1], 2, [1, 1], None, None, 1, None)),
    "fwd_multi_bn": ("afan_conv_fwd_multi_bn_nhwc_bf16",
                     "x w y nb n hi wi ci co ksize stride dilation stats_shift stats_acc y_act0 bn_weight bn_bias eps momentum stats0 "
                     "running_mean running_var num_batches relu barrier stream",
                     (P, [P, P], [P, P], 2, 2, 8, 8, 128, 128, [3, 1], 2, [1, 1], [P, P], [P, P], P, P, P, 1e-5, 0.1, P, P, P, P, 1, P, None)),
    "fwd_bn": ("afan_conv_fwd_bn_nhwc_bf16",
               "x w y_raw y_act n hi wi ci co ksize dilation acc shift bn_weight bn_bias eps momentum stats running_mean running_var "
               "num_batches residual relu sc_raw sc_acc sc_weight sc_bias sc_eps sc_momentum sc_stats sc_running_mean sc_running_var "
               "sc_num_batches barrier stream",
               (P, P, P, P, 2, 8, 8, 128, 128, 3, 1, P, P, P, P, 1e-5, 0.1, P, P, P, P, None, 1, None, None, None, None, 0.0, 0.0, None,
                None, None, None, P, None)),
    "dgrad_bn": ("afan_conv_dgrad_bn_nhwc_bf16",
                 "dy wt dx dres n hi wi ci co ksize dilation addend bn_x bn_stats bn_relu bn_y bn_acc dweight dbias accumulate sc_x sc_stats "
                 "sc_acc d_sc sc_dweight sc_dbias barrier stream",
                 (P, P, P, P, 2, 8, 8, 128, 128, 3, 1, None, P, P, 1, P, P, P, P, 0, None, None, None, None, None, None, P, None)),
    "dgrad_sc_bn": ("afan_conv_dgrad_sc_bn_nhwc_bf16",
                    "dy dy_sc wt10 dx dres n hi wi ci co bn_x bn_stats bn_relu bn_y bn_acc dweight dbias accumulate barrier stream",
                    (P, FAR, P, P, P, 2, 8, 8, 128, 128, P, P, 1, P, P, P, P, 0, P, None)),
    "block_fwd": ("afan_frozen_bottleneck_fwd",
                  "x n h w cin planes stride dilation w1 w2 w3 wd k1 k2 k3 kd scratch a1 a2 out stream",
                  (P, 1, 9, 9, 256, 64, 1, 1, P, P, P, None, P, P, P, None, P, P, P, P, None)),
    "block_bwd": ("afan_frozen_bottleneck_bwd",
                  "g pre_d3 pre_dres x a1 a2 out n h w cin planes stride dilation wt1 wt2 wt3 wtd al1 al2 al3 ald gw1 gw2 gw3 gwd wgrad_ws "
                  "scratch dx prev_al3 prev_d3 prev_dres stream",
                  (P, None, None, P, P, P, P, 1, 9, 9, 256, 64, 1, 1, P, P, P, None, P, P, P, None, None, None, None, None, None, P, P, None,
                   None, None, None)),
}

SMALL = dict(ci=32, co=64)                         # a shape of the small-channel kernel, forward and input gradient
C64 = dict(ci=64, co=64, hi=16, wi=8)              # ... of the 64 -> 64 weights-in-registers kernel (3x3, stride 1, dilation 1)
STEM = dict(ci=3, co=16, wi=32)                    # ... of the 3-channel image stem
PLAIN, ANY, DIL = dict(dilation=1, any_family=0), dict(dilation=1, any_family=1), dict(dilation=2, any_family=1)
BN_SUMS = dict(bn_x=P, bn_stats=P)
PROJ = dict(wd=P, kd=P)
PROJ_T = dict(wtd=P, ald=P)
CHAINED = dict(g=None, pre_d3=P, pre_dres=P)


def _r(entry, code, *overrides, **more):
    args = {}
    for o in overrides:
        args.update(o)
    args.update(more)
    return entry, args, code


ROWS = [
    # ---- afan_conv_fwd_nhwc_bf16 ----
    _r("fwd", ENULL, x=None), _r("fwd", ENULL, w=None), _r("fwd", ENULL, y=None),
    _r("fwd", EALIGN, x=ODD), _r("fwd", EALIGN, w=ODD), _r("fwd", EALIGN, y=ODD),
    _r("fwd", ESHAPE, n=0), _r("fwd", ESHAPE, stride=3), _r("fwd", ESHAPE, k=5), _r("fwd", ESHAPE, k=2),
    _r("fwd", ESHAPE, dilation=0), _r("fwd", ESHAPE, dilation=65), _r("fwd", ESHAPE, dilation=2, stride=2), _r("fwd", ESHAPE, dilation=2, k=1),
    _r("fwd", ESHAPE, ci=20), _r("fwd", ESHAPE, ci=36), _r("fwd", ESHAPE, ci=44), _r("fwd", ESHAPE, co=36), _r("fwd", ESHAPE, co=44),
    _r("fwd", ESHAPE, stats_partials=P, stats_acc=P),
    _r("fwd", EALIGN, stats_acc=ODD),
    _r("fwd", ESHAPE, groups=2), _r("fwd", ESHAPE, groups=2, stats_partials=P), _r("fwd", ESHAPE, groups=3, stats_acc=P),
    _r("fwd", ESHAPE, groups=2, stats_acc=P, n=3),
    _r("fwd", ESHAPE, SMALL, stats_partials=P),                       # the small-channel kernel has no partial-slab form
    _r("fwd", ESHAPE, SMALL, groups=2, stats_acc=P),                  # ... and walks whole 128-row tiles per image group
    _r("fwd", ENULL, x=None, w=ODD), _r("fwd", ESHAPE, x=None, stride=3), _r("fwd", ESHAPE, x=ODD, ci=20),
    _r("fwd", EALIGN, x=ODD, stats_partials=P, stats_acc=P), _r("fwd", ESHAPE, stats_partials=P, stats_acc=ODD),
    _r("fwd", EALIGN, stats_acc=ODD, groups=3), _r("fwd", ENULL, y=None, groups=2),
    _r("fwd", ENULL, STEM, x=None), _r("fwd", ENULL, STEM, y=None), _r("fwd", EALIGN, STEM, x=ODD1), _r("fwd", EALIGN, STEM, w=ODD1),
    _r("fwd", EALIGN, STEM, y=ODD), _r("fwd", EALIGN, STEM, stats_acc=ODD),
    _r("fwd", ESHAPE, STEM, wi=30), _r("fwd", ESHAPE, STEM, co=128), _r("fwd", ESHAPE, STEM, k=1), _r("fwd", ESHAPE, STEM, stride=2),
    _r("fwd", ESHAPE, STEM, stats_partials=P), _r("fwd", ESHAPE, STEM, groups=2, stats_acc=P), _r("fwd", ESHAPE, STEM, dilation=2),
    _r("fwd", ESHAPE, STEM, x=None, dilation=2), _r("fwd", ENULL, STEM, x=None, y=ODD),
    # ---- afan_conv_dgrad_nhwc_bf16 ----
    _r("dgrad", ENULL, dy=None), _r("dgrad", ENULL, wt=None), _r("dgrad", ENULL, dx=None),
    _r("dgrad", EALIGN, dy=ODD), _r("dgrad", EALIGN, wt=ODD), _r("dgrad", EALIGN, dx=ODD),
    _r("dgrad", ESHAPE, n=0), _r("dgrad", ESHAPE, stride=3), _r("dgrad", ESHAPE, k=5), _r("dgrad", ESHAPE, dilation=0),
    _r("dgrad", ESHAPE, dilation=2, stride=2), _r("dgrad", ESHAPE, dilation=2, k=1),
    _r("dgrad", ESHAPE, ci=20), _r("dgrad", ESHAPE, co=44), _r("dgrad", ESHAPE, ci=3, co=16),
    _r("dgrad", ESHAPE, BN_SUMS, bn_partials=P, bn_acc=P),
    _r("dgrad", ENULL, bn_acc=P, bn_stats=P), _r("dgrad", ENULL, bn_acc=P, bn_x=P), _r("dgrad", ENULL, bn_partials=P),
    _r("dgrad", EALIGN, BN_SUMS, bn_acc=ODD),
    _r("dgrad", ESHAPE, BN_SUMS, bn_partials=P, groups=2), _r("dgrad", ESHAPE, BN_SUMS, bn_acc=P, groups=2, n=3),
    _r("dgrad", ESHAPE, BN_SUMS, bn_acc=P, groups=3), _r("dgrad", ESHAPE, BN_SUMS, bn_acc=P, groups=2, stride=2, hi=7),
    _r("dgrad", ESHAPE, SMALL, BN_SUMS, bn_partials=P), _r("dgrad", ESHAPE, SMALL, BN_SUMS, bn_acc=P, groups=2),
    _r("dgrad", ESHAPE, SMALL, BN_SUMS, bn_partials=P, stride=2),
    _r("dgrad", ENULL, dy=None, wt=ODD), _r("dgrad", ESHAPE, dy=None, stride=3), _r("dgrad", EALIGN, BN_SUMS, dy=ODD, bn_partials=P, bn_acc=P),
    _r("dgrad", ESHAPE, bn_partials=P, bn_acc=P), _r("dgrad", ENULL, bn_acc=ODD), _r("dgrad", EALIGN, BN_SUMS, bn_acc=ODD, groups=3),
    # ---- afan_conv_fwd_affine_nhwc_bf16 ----
    *[_r("fwd_affine", ENULL, form, **{a: None}) for form in (PLAIN, ANY, DIL) for a in ("x", "w", "y", "coefs")],
    *[_r("fwd_affine", EALIGN, form, **{a: ODD}) for form in (PLAIN, ANY, DIL) for a in ("x", "w", "y", "residual")],
    *[_r("fwd_affine", ESHAPE, form, **o) for form in (PLAIN, ANY, DIL)
      for o in (dict(n=0), dict(stride=3), dict(k=5), dict(ci=20), dict(co=44))],
    *[_r("fwd_affine", ESHAPE, DIL, **o) for o in (dict(stride=2), dict(k=1), dict(dilation=0), dict(dilation=65))],
    _r("fwd_affine", ESHAPE, PLAIN, SMALL), _r("fwd_affine", ESHAPE, PLAIN, C64), _r("fwd_affine", ESHAPE, PLAIN, STEM),
    _r("fwd_affine", ESHAPE, DIL, SMALL), _r("fwd_affine", ESHAPE, DIL, STEM),
    _r("fwd_affine", EALIGN, ANY, SMALL, coefs=ODD), _r("fwd_affine", EALIGN, ANY, C64, coefs=ODD),
    _r("fwd_affine", ESHAPE, PLAIN, SMALL, coefs=ODD), _r("fwd_affine", ESHAPE, DIL, SMALL, coefs=ODD),
    _r("fwd_affine", EALIGN, PLAIN, SMALL, x=ODD), _r("fwd_affine", ENULL, PLAIN, C64, coefs=None),
    _r("fwd_affine", ENULL, ANY, x=None, residual=ODD), _r("fwd_affine", ESHAPE, ANY, coefs=None, stride=3),
    _r("fwd_affine", ENULL, ANY, STEM, x=None), _r("fwd_affine", ENULL, ANY, STEM, coefs=None), _r("fwd_affine", ESHAPE, ANY, STEM, residual=P),
    _r("fwd_affine", EALIGN, ANY, STEM, x=ODD1), _r("fwd_affine", EALIGN, ANY, STEM, y=ODD), _r("fwd_affine", EALIGN, ANY, STEM, coefs=ODD),
    _r("fwd_affine", ESHAPE, ANY, STEM, wi=30), _r("fwd_affine", ESHAPE, ANY, STEM, x=None, residual=P),
    _r("fwd_affine", ENULL, ANY, STEM, x=None, coefs=ODD),
    # ---- afan_conv_dgrad_affine_nhwc_bf16 ----
    *[_r("dgrad_affine", ENULL, form, **{a: None}) for form in (PLAIN, ANY, DIL) for a in ("dy", "wt", "dx", "alpha")],
    *[_r("dgrad_affine", EALIGN, form, **{a: ODD}) for form in (PLAIN, ANY, DIL) for a in ("dy", "wt", "dx")],
    *[_r("dgrad_affine", ESHAPE, form, act=ODD) for form in (PLAIN, ANY, DIL)],                 # a misaligned mask is a shape error
    *[_r("dgrad_affine", ESHAPE, form, **o) for form in (PLAIN, ANY, DIL)
      for o in (dict(n=0), dict(stride=3), dict(k=5), dict(ci=20), dict(co=44))],
    *[_r("dgrad_affine", ESHAPE, DIL, **o) for o in (dict(stride=2), dict(k=1), dict(dilation=0), dict(dilation=65))],
    _r("dgrad_affine", ENULL, PLAIN, act=None), _r("dgrad_affine", ESHAPE, ANY, act=None), _r("dgrad_affine", ESHAPE, DIL, act=None),
    _r("dgrad_affine", ENULL, PLAIN, act=None, stride=3), _r("dgrad_affine", ESHAPE, ANY, act=None, stride=3),
    _r("dgrad_affine", ENULL, ANY, alpha=None, stride=3), _r("dgrad_affine", ENULL, DIL, alpha=None, dy=ODD),
    _r("dgrad_affine", ESHAPE, PLAIN, C64), _r("dgrad_affine", ESHAPE, PLAIN, SMALL), _r("dgrad_affine", ESHAPE, DIL, SMALL),
    _r("dgrad_affine", ESHAPE, PLAIN, SMALL, stride=2),
    _r("dgrad_affine", EALIGN, ANY, C64, alpha=ODD), _r("dgrad_affine", EALIGN, ANY, SMALL, alpha=ODD),
    _r("dgrad_affine", EALIGN, ANY, SMALL, alpha=ODD, stride=2), _r("dgrad_affine", EALIGN, ANY, C64, alpha=ODD, act=None),
    _r("dgrad_affine", ESHAPE, PLAIN, C64, alpha=ODD), _r("dgrad_affine", ESHAPE, DIL, SMALL, alpha=ODD),
    _r("dgrad_affine", EALIGN, PLAIN, C64, dy=ODD), _r("dgrad_affine", EALIGN, ANY, dy=ODD, act=ODD),
    _r("dgrad_affine", ENULL, ANY, dy=None, act=ODD),
    # ---- afan_conv_dgrad_dual_nhwc_bf16 ----
    *[_r("dgrad_dual", ENULL, **{a: None}) for a in ("dy", "wt", "d3", "dres", "alpha", "act")],
    *[_r("dgrad_dual", EALIGN, **{a: ODD}) for a in ("dy", "wt", "d3", "dres", "addend")],
    _r("dgrad_dual", ESHAPE, act=ODD), _r("dgrad_dual", ESHAPE, act=ODD, dres=ODD),
    _r("dgrad_dual", ESHAPE, stride=3), _r("dgrad_dual", ESHAPE, k=5), _r("dgrad_dual", ESHAPE, ci=20),
    _r("dgrad_dual", ESHAPE, C64, k=3), _r("dgrad_dual", ESHAPE, SMALL), _r("dgrad_dual", ESHAPE, SMALL, k=3, stride=2),
    _r("dgrad_dual", ENULL, dres=None, stride=3), _r("dgrad_dual", ESHAPE, dy=None, stride=3), _r("dgrad_dual", EALIGN, dy=ODD, act=ODD),
    _r("dgrad_dual", EALIGN, C64, k=3, dres=ODD),
    # ---- afan_conv_dgrad_sc_nhwc_bf16 ----
    *[_r("dgrad_sc", ENULL, **{a: None}) for a in ("dy", "dy_sc", "wt10", "dx")],
    *[_r("dgrad_sc", EALIGN, **{a: ODD}) for a in ("dy", "dy_sc", "wt10", "dx")],
    _r("dgrad_sc", ESHAPE, dy_sc=NEAR), _r("dgrad_sc", ESHAPE, SMALL), _r("dgrad_sc", ESHAPE, ci=20), _r("dgrad_sc", ESHAPE, co=44),
    _r("dgrad_sc", ESHAPE, n=0),
    _r("dgrad_sc", ESHAPE, BN_SUMS, bn_partials=P, bn_acc=P), _r("dgrad_sc", ENULL, bn_acc=P), _r("dgrad_sc", EALIGN, BN_SUMS, bn_acc=ODD),
    _r("dgrad_sc", ENULL, dy_sc=None, ci=20), _r("dgrad_sc", ESHAPE, dy=None, ci=20), _r("dgrad_sc", ESHAPE, dy_sc=ODD, ci=32, co=64),
    _r("dgrad_sc", EALIGN, dy=ODD, dy_sc=NEAR),
    # ---- afan_conv_fwd_multi_nhwc_bf16 ----
    _r("fwd_multi", ESHAPE, nb=0), _r("fwd_multi", ESHAPE, nb=5),
    *[_r("fwd_multi", ENULL, **{a: None}) for a in ("x", "w", "y", "ksize", "dilation")],
    _r("fwd_multi", ENULL, w=[P, None]), _r("fwd_multi", ENULL, y=[None, P]), _r("fwd_multi", EALIGN, w=[ODD, P]), _r("fwd_multi", EALIGN, y=[P, ODD]),
    _r("fwd_multi", EALIGN, x=ODD),
    _r("fwd_multi", ESHAPE, stats_acc=[P, P]), _r("fwd_multi", ESHAPE, stats_shift=[P, P]),
    _r("fwd_multi", ENULL, stats_shift=[P, P], stats_acc=[P, None]), _r("fwd_multi", EALIGN, stats_shift=[P, P], stats_acc=[P, ODD]),
    _r("fwd_multi", ESHAPE, stats_shift=[P, None], stats_acc=[P, P]), _r("fwd_multi", ESHAPE, stats_shift=[None, P], stats_acc=[P, P]),
    _r("fwd_multi", ESHAPE, groups=2), _r("fwd_multi", ESHAPE, groups=3, stats_shift=[P, P], stats_acc=[P, P]),
    _r("fwd_multi", ESHAPE, groups=2, n=3, stats_shift=[P, P], stats_acc=[P, P]),
    _r("fwd_multi", ESHAPE, SMALL), _r("fwd_multi", ESHAPE, ci=20), _r("fwd_multi", ESHAPE, ci=44), _r("fwd_multi", ESHAPE, STEM),
    _r("fwd_multi", ESHAPE, ksize=[5, 1]), _r("fwd_multi", ESHAPE, ksize=[3, 2]), _r("fwd_multi", ESHAPE, dilation=[2, 1]),
    _r("fwd_multi", ESHAPE, dilation=[1, 2], stride=1), _r("fwd_multi", ESHAPE, stride=3), _r("fwd_multi", ESHAPE, n=0),
    _r("fwd_multi", ESHAPE, x=None, nb=5), _r("fwd_multi", ENULL, x=ODD, w=[P, None]), _r("fwd_multi", EALIGN, SMALL, x=ODD),
    _r("fwd_multi", EALIGN, x=None, y=[ODD, P]), _r("fwd_multi", ESHAPE, w=None, groups=2),
    _r("fwd_multi", ESHAPE, w=[None, P], stride=3), _r("fwd_multi", EALIGN, w=[ODD, None]),
    # ---- afan_conv_fwd_multi_bn_nhwc_bf16 ----
    *[_r("fwd_multi_bn", ENULL, **{a: None}) for a in ("y_act0", "stats0", "barrier", "stats_acc", "stats_shift", "x", "w")],
    _r("fwd_multi_bn", EALIGN, y_act0=ODD), _r("fwd_multi_bn", EALIGN, barrier=P16), _r("fwd_multi_bn", EALIGN, x=ODD),
    _r("fwd_multi_bn", ESHAPE, nb=1, w=[P], y=[P], ksize=[3], dilation=[1], stats_shift=[P], stats_acc=[P]),
    _r("fwd_multi_bn", ESHAPE, ci=72), _r("fwd_multi_bn", ESHAPE, co=72), _r("fwd_multi_bn", ESHAPE, SMALL), _r("fwd_multi_bn", ESHAPE, nb=5),
    _r("fwd_multi_bn", ENULL, barrier=None, nb=5), _r("fwd_multi_bn", EALIGN, barrier=P16, nb=5), _r("fwd_multi_bn", ENULL, y_act0=ODD, stats0=None),
    _r("fwd_multi_bn", ENULL, stats_acc=[P, None]), _r("fwd_multi_bn", ESHAPE, stats_shift=[P, None]),
    # ---- afan_conv_fwd_bn_nhwc_bf16 ----
    _r("fwd_bn", ESHAPE, ksize=5), _r("fwd_bn", ESHAPE, ksize=2), _r("fwd_bn", ESHAPE, dilation=0), _r("fwd_bn", ESHAPE, ksize=1, dilation=2),
    _r("fwd_bn", ESHAPE, dilation=65), _r("fwd_bn", ESHAPE, n=0),
    *[_r("fwd_bn", ENULL, **{a: None}) for a in ("x", "w", "y_raw", "y_act", "acc", "stats", "barrier")],
    *[_r("fwd_bn", EALIGN, **{a: ODD}) for a in ("x", "w", "y_raw", "y_act", "acc", "residual")],
    _r("fwd_bn", EALIGN, barrier=P16), _r("fwd_bn", EALIGN, sc_raw=ODD, sc_acc=P, sc_stats=P),
    _r("fwd_bn", ESHAPE, sc_raw=P, sc_acc=P, sc_stats=P, residual=P), _r("fwd_bn", ESHAPE, sc_raw=P, sc_stats=P),
    _r("fwd_bn", ESHAPE, sc_raw=P, sc_acc=P), _r("fwd_bn", ESHAPE, sc_raw=P, sc_acc=P, sc_stats=P, relu=0),
    _r("fwd_bn", ESHAPE, ci=72), _r("fwd_bn", ESHAPE, co=72), _r("fwd_bn", ESHAPE, SMALL), _r("fwd_bn", ESHAPE, ci=20), _r("fwd_bn", ESHAPE, C64),
    _r("fwd_bn", ESHAPE, x=None, ksize=5), _r("fwd_bn", ENULL, x=None, ci=72), _r("fwd_bn", EALIGN, x=ODD, sc_raw=P, residual=P),
    _r("fwd_bn", ESHAPE, x=None, ci=20), _r("fwd_bn", ENULL, barrier=None, x=ODD), _r("fwd_bn", EALIGN, C64, barrier=P16),
    # ---- afan_conv_dgrad_bn_nhwc_bf16 ----
    _r("dgrad_bn", ENULL, barrier=None), _r("dgrad_bn", ENULL, bn_acc=None), _r("dgrad_bn", EALIGN, barrier=P16), _r("dgrad_bn", EALIGN, dres=ODD),
    _r("dgrad_bn", ESHAPE, ci=72), _r("dgrad_bn", ESHAPE, co=72), _r("dgrad_bn", ESHAPE, ksize=5), _r("dgrad_bn", ESHAPE, dilation=0),
    _r("dgrad_bn", ESHAPE, ksize=1, dilation=2), _r("dgrad_bn", ESHAPE, SMALL), _r("dgrad_bn", ESHAPE, C64),
    _r("dgrad_bn", ENULL, sc_x=P, sc_acc=P, d_sc=P), _r("dgrad_bn", ENULL, sc_x=P, sc_stats=P, d_sc=P), _r("dgrad_bn", ENULL, sc_x=P, sc_stats=P, sc_acc=P),
    _r("dgrad_bn", EALIGN, sc_x=ODD, sc_stats=P, sc_acc=P, d_sc=P), _r("dgrad_bn", EALIGN, sc_x=P, sc_stats=P, sc_acc=ODD, d_sc=P),
    _r("dgrad_bn", EALIGN, sc_x=P, sc_stats=P, sc_acc=P, d_sc=ODD), _r("dgrad_bn", ESHAPE, sc_x=P, sc_stats=P, sc_acc=P, d_sc=P, bn_y=None),
    _r("dgrad_bn", ENULL, dy=None), _r("dgrad_bn", ENULL, wt=None), _r("dgrad_bn", ENULL, dx=None), _r("dgrad_bn", EALIGN, dy=ODD),
    _r("dgrad_bn", ENULL, bn_x=None), _r("dgrad_bn", ENULL, bn_stats=None), _r("dgrad_bn", EALIGN, bn_acc=ODD), _r("dgrad_bn", ESHAPE, n=0),
    _r("dgrad_bn", ENULL, barrier=None, ci=72), _r("dgrad_bn", EALIGN, barrier=P16, ksize=5), _r("dgrad_bn", ESHAPE, dy=None, ci=72),
    _r("dgrad_bn", ENULL, C64, dy=None), _r("dgrad_bn", ESHAPE, sc_x=P, ci=72),
    # ---- afan_conv_dgrad_sc_bn_nhwc_bf16 ----
    _r("dgrad_sc_bn", ENULL, dy_sc=None), _r("dgrad_sc_bn", ENULL, barrier=None), _r("dgrad_sc_bn", ENULL, bn_acc=None),
    _r("dgrad_sc_bn", EALIGN, barrier=P16), _r("dgrad_sc_bn", EALIGN, dres=ODD), _r("dgrad_sc_bn", ESHAPE, ci=72), _r("dgrad_sc_bn", ESHAPE, co=72),
    _r("dgrad_sc_bn", ESHAPE, hi=7), _r("dgrad_sc_bn", ESHAPE, wi=7), _r("dgrad_sc_bn", ESHAPE, dy_sc=NEAR),
    _r("dgrad_sc_bn", ENULL, dy=None), _r("dgrad_sc_bn", EALIGN, dy_sc=ODD), _r("dgrad_sc_bn", EALIGN, wt10=ODD),
    _r("dgrad_sc_bn", ENULL, bn_x=None), _r("dgrad_sc_bn", EALIGN, bn_acc=ODD),
    _r("dgrad_sc_bn", ENULL, barrier=None, ci=72), _r("dgrad_sc_bn", EALIGN, dres=ODD, hi=7), _r("dgrad_sc_bn", ENULL, dy=None, hi=7),
    # ---- afan_frozen_bottleneck_fwd ----
    *[_r("block_fwd", ENULL, **{a: None}) for a in ("x", "w1", "w2", "w3", "k1", "k2", "k3", "scratch", "a1", "a2", "out")],
    _r("block_fwd", ENULL, wd=P), _r("block_fwd", ESHAPE, n=0), _r("block_fwd", ESHAPE, stride=3), _r("block_fwd", ESHAPE, cin=128),
    _r("block_fwd", ESHAPE, stride=2), _r("block_fwd", ESHAPE, dilation=0), _r("block_fwd", ESHAPE, PROJ, stride=2, dilation=2),
    _r("block_fwd", ESHAPE, PROJ, dilation=0),
    _r("block_fwd", EALIGN, x=ODD), _r("block_fwd", EALIGN, w1=ODD), _r("block_fwd", EALIGN, a1=ODD), _r("block_fwd", EALIGN, x=ODD, dilation=2),
    _r("block_fwd", ESHAPE, PROJ, cin=80, planes=20), _r("block_fwd", ENULL, x=None, n=0), _r("block_fwd", ESHAPE, x=ODD, stride=3),
    # ---- afan_frozen_bottleneck_bwd ----
    *[_r("block_bwd", ENULL, **{a: None}) for a in ("x", "a1", "a2", "out", "wt1", "wt2", "wt3", "al1", "al2", "al3", "scratch")],
    _r("block_bwd", ENULL, g=None), _r("block_bwd", ENULL, g=None, pre_d3=P), _r("block_bwd", ENULL, g=None, pre_dres=P),
    _r("block_bwd", ENULL, prev_al3=P, prev_d3=P, prev_dres=P), _r("block_bwd", ENULL, dx=None, prev_al3=P, prev_dres=P),
    _r("block_bwd", ENULL, dx=None, prev_al3=P, prev_d3=P), _r("block_bwd", ENULL, wtd=P), _r("block_bwd", ENULL, gw1=P), _r("block_bwd", ENULL, PROJ_T, gwd=P),
    _r("block_bwd", ESHAPE, n=0), _r("block_bwd", ESHAPE, stride=3), _r("block_bwd", ESHAPE, cin=128), _r("block_bwd", ESHAPE, stride=2),
    _r("block_bwd", ESHAPE, dilation=0), _r("block_bwd", ESHAPE, PROJ_T, stride=2, dilation=2),
    _r("block_bwd", ENULL, x=None, stride=3), _r("block_bwd", ENULL, g=None, dilation=0),
    _r("block_bwd", EALIGN, CHAINED, pre_d3=ODD), _r("block_bwd", EALIGN, CHAINED, wt3=ODD), _r("block_bwd", EALIGN, CHAINED, pre_d3=ODD, dilation=2),
    _r("block_bwd", ESHAPE, CHAINED, PROJ_T, cin=80, planes=20),
]


def _pointers():
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 63) & ~63
    return buf, {P: base, ODD: base + 2, ODD1: base + 1, P16: base + 16, FAR: base + (1 << 20), NEAR: base + 64}


def build_call(entry, overrides, ptrs, keep):
    """The ctypes argument list of one row (keep: the arrays that must outlive the call)."""
    _, names, base = ENTRIES[entry]
    names = names.split()
    assert len(names) == len(base) and set(overrides) <= set(names), (entry, overrides)
    args = []
    for name, v in zip(names, base):
        v = overrides.get(name, v)
        if isinstance(v, list) and name in _PTR_ARRAYS:
            arr = (ctypes.c_void_p * len(v))(*[None if t is None else ptrs[t] for t in v])
            keep.append(arr)
            v = ctypes.cast(arr, ctypes.c_void_p)
        elif isinstance(v, list) and name in _INT_ARRAYS:
            arr = (ctypes.c_int * len(v))(*v)
            keep.append(arr)
            v = ctypes.cast(arr, ctypes.c_void_p)
        elif isinstance(v, str):
            v = ctypes.c_void_p(ptrs[v])
        elif name in _FLOATS:
            v = float(v)
        args.append(v)
    return args


def test_every_entry_has_rows():
    assert {r[0] for r in ROWS} == set(ENTRIES) and len(ROWS) > 300
    assert all(code in (ESHAPE, ENULL, EALIGN) for _, _, code in ROWS)


def test_return_codes_of_refused_calls(pkg):
    lib = pkg._lib.load()
    buf, ptrs = _pointers()
    wrong = []
    for entry, overrides, code in ROWS:
        keep = []
        got = getattr(lib, ENTRIES[entry][0])(*build_call(entry, overrides, ptrs, keep))
        if got != code:
            wrong.append((entry, overrides, code, got))
    assert not wrong, "\n".join(f"{e} {o}: {g}, recorded {c}" for e, o, c, g in wrong)
