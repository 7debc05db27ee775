"""The return code of every BatchNorm entry for calls that end before anything is launched: a literal table of
(entry, arguments) -> code, recorded from library version 101 as of commit ceaa8af, the last one before the BatchNorm host code was
reshaped into request records, and never regenerated from a later build.  It pins which of AFAN_EDTYPE / AFAN_ESHAPE / AFAN_ELAYOUT / AFAN_ENULL / AFAN_EALIGN wins where
several apply, so that the host code in front of the launches can be reshaped without a caller seeing a different answer.  The three
queries (afan_bn_workspace_floats, afan_bn_acc_doubles, afan_bn_acc_supported) have a table of values at the channel counts of
test_bn_pinned_gpu.py's predicate test.

Every row is one entry's BASE call (bf16, channels-last, n = 2, c = 64, hw = 16: a problem the vector mapping takes) with a few
arguments replaced.  All pointers are host addresses that the library never dereferences (the arrays of the batched running update
are real arrays), so no GPU is needed.

Rows left out, because the call would go on to a launch:
  * every base call itself, with and without its optional operands;
  * pointers that are element-aligned but not 16-byte aligned, and channel counts outside the vector mapping, in the slab, partials
    and eval forms (they take the generic kernels; only the accumulator forms refuse them);
  * afan_bn_apply in NCHW without a workspace (it needs none), afan_affine_apply with misaligned coefficients (generic kernel);
  * afan_affine_coefs with coefficients at + 16 bytes (aligned enough);
  * a pending update count other than 1 in the channels-last forms and in afan_bn_stats (they apply it);
  * afan_bn_running_update_batched with a bad item behind the first 64 (the first batch is launched before it is looked at);
  * afan_bn_set_running_updates itself (no code; its effect is the NCHW row run under a count of 2)."""
import ctypes
import os

OK, EDTYPE, EALIGN, ESHAPE, ENULL, ELAYOUT = 0, -1, -2, -3, -4, -5
F32, BF16, NCHW, NHWC = 0, 1, 0, 1

# pointer tokens
P = "P"            # aligned to 64 bytes
ODD = "ODD"        # P + 2: a bf16 element boundary, no fp32 one, not 16 bytes
ODD1 = "ODD1"      # P + 1
P16 = "P16"        # P + 16

_FLOATS = {"eps", "momentum", "eps_a", "momentum_a", "eps_b", "momentum_b"}
_DOUBLES = {"m_count"}

# entry -> (argument names, base call); the C symbol is afan_<entry>
ENTRIES = {
    "bn_stats": ("x dtype layout n c hw eps momentum workspace stats running_mean running_var num_batches stream",
                 (P, BF16, NHWC, 2, 64, 16, 1e-5, 0.1, P, P, P, P, P, None)),
    "bn_train_forward": ("x residual y dtype layout n c hw eps momentum weight bias relu workspace save_stats running_mean running_var "
                         "num_batches stream",
                         (P, None, P, BF16, NHWC, 2, 64, 16, 1e-5, 0.1, P, P, 1, P, P, P, P, P, None)),
    "bn_train_forward_partials": ("x residual y dtype n c hw eps momentum weight bias relu partials partials_g partials_shift save_stats "
                                  "running_mean running_var num_batches stream",
                                  (P, None, P, BF16, 2, 64, 16, 1e-5, 0.1, P, P, 1, P, 4, P, P, P, P, P, None)),
    "bn_train_forward_acc": ("x residual y dtype n c hw eps momentum weight bias relu acc acc_ready save_stats running_mean running_var "
                             "num_batches groups stream",
                             (P, None, P, BF16, 2, 64, 16, 1e-5, 0.1, P, P, 1, P, 1, P, P, P, P, 1, None)),
    "bn_train_forward_acc_dual": ("x_a x_b y dtype n c hw eps_a momentum_a weight_a bias_a acc_a save_stats_a running_mean_a running_var_a "
                                  "num_batches_a eps_b momentum_b weight_b bias_b acc_b save_stats_b running_mean_b running_var_b "
                                  "num_batches_b stream",
                                  (P, P, P, BF16, 2, 64, 16, 1e-5, 0.1, P, P, P, P, P, P, P, 1e-5, 0.1, P, P, P, P, P, P, P, None)),
    "bn_apply": ("x residual y dtype layout n c hw mean invstd weight bias relu workspace stream",
                 (P, None, P, BF16, NHWC, 2, 64, 16, P, P, P, P, 1, P, None)),
    "affine_coefs": ("mean invstd weight bias c coefs stream", (P, P, P, P, 64, P, None)),
    "affine_apply": ("x residual y dtype n c hw coefs relu stream", (P, None, P, BF16, 2, 64, 16, P, 1, None)),
    "bn_backward": ("dy x y dx d_residual dtype layout n c hw save_stats weight bias relu workspace dweight dbias accumulate partials "
                    "partials_g stream",
                    (P, P, None, P, None, BF16, NHWC, 2, 64, 16, P, P, P, 1, P, P, P, 0, None, 0, None)),
    "bn_backward_acc": ("dy x y dx d_residual dtype n c hw save_stats relu acc acc_ready dweight dbias accumulate groups stream",
                        (P, P, None, P, None, BF16, 2, 64, 16, P, 1, P, 1, P, P, 0, 1, None)),
    "bn_running_update": ("stats c m_count eps momentum running_mean running_var num_batches stream",
                          (P, 64, 32.0, 1e-5, 0.1, P, P, P, None)),
    # lists become real arrays (of pointers, int64, double, float); a token in their place is passed as the array's address
    "bn_running_update_batched": ("stats running_mean running_var num_batches c m_count eps momentum n stream",
                                  ([P, P], [P, P], [P, P], [P, P], [64, 16], [32.0, 8.0], [1e-5, 1e-5], [0.1, 0.1], 2, None)),
    "normalize_nchw": ("x y out_dtype out_layout n c hw mean std stream", (P, P, BF16, NHWC, 2, 3, 16, P, P, None)),
}
_ARRAYS = {"stats": ctypes.c_void_p, "running_mean": ctypes.c_void_p, "running_var": ctypes.c_void_p, "num_batches": ctypes.c_void_p,
           "c": ctypes.c_int64, "m_count": ctypes.c_double, "eps": ctypes.c_float, "momentum": ctypes.c_float}

FP32 = dict(dtype=F32)
PLANES = dict(layout=NCHW)
BIG_C = dict(c=(1 << 20) + 1)                      # more channels than the channels-last plan takes
NCHW_BIG_C = dict(layout=NCHW, c=65536)            # ... than the NCHW grid's y dimension
NCHW_BIG_V = dict(layout=NCHW, n=1 << 31, hw=1)    # more than 2^31 - 1 accesses per channel
NO_VEC = dict(c=12)                                # bf16: 12 % 8 != 0, outside the vector mapping (and the accumulator forms)
PART = dict(partials=P, partials_g=4)              # the backward's optional partial sums
UPDATES2 = {"@updates": 2}                         # the row runs under afan_bn_set_running_updates(2)


def _r(entry, code, *overrides, **more):
    args = {}
    for o in overrides:
        args.update(o)
    args.update(more)
    return entry, args, code


ROWS = [
    # ---- afan_bn_stats ----
    _r("bn_stats", EDTYPE, dtype=7), _r("bn_stats", EDTYPE, dtype=-1), _r("bn_stats", ESHAPE, n=0), _r("bn_stats", ESHAPE, c=0),
    _r("bn_stats", ESHAPE, hw=-1), _r("bn_stats", ELAYOUT, layout=2), _r("bn_stats", ELAYOUT, layout=-1),
    *[_r("bn_stats", ENULL, lay, **{a: None}) for lay in ({}, PLANES) for a in ("x", "workspace", "stats")],
    _r("bn_stats", ENULL, running_mean=None), _r("bn_stats", ENULL, running_var=None), _r("bn_stats", ENULL, PLANES, running_var=None),
    _r("bn_stats", EALIGN, x=ODD1), _r("bn_stats", EALIGN, FP32, x=ODD), _r("bn_stats", EALIGN, PLANES, x=ODD1),
    _r("bn_stats", ESHAPE, BIG_C), _r("bn_stats", ESHAPE, NCHW_BIG_C), _r("bn_stats", ESHAPE, NCHW_BIG_V),
    _r("bn_stats", ESHAPE, FP32, NCHW_BIG_V),
    _r("bn_stats", EDTYPE, dtype=7, layout=2), _r("bn_stats", EDTYPE, dtype=7, n=0), _r("bn_stats", ESHAPE, n=0, layout=2),
    _r("bn_stats", ELAYOUT, layout=2, x=None), _r("bn_stats", ENULL, workspace=None, x=ODD1), _r("bn_stats", ENULL, running_mean=None, x=ODD1),
    _r("bn_stats", ESHAPE, BIG_C, x=None, c=0), _r("bn_stats", ENULL, BIG_C, x=None), _r("bn_stats", EALIGN, BIG_C, x=ODD1),
    _r("bn_stats", EALIGN, NCHW_BIG_C, x=ODD1),
    # ---- afan_bn_train_forward ----
    _r("bn_train_forward", EDTYPE, dtype=2), _r("bn_train_forward", ESHAPE, n=0), _r("bn_train_forward", ESHAPE, c=-3),
    _r("bn_train_forward", ESHAPE, hw=0), _r("bn_train_forward", ELAYOUT, layout=2),
    *[_r("bn_train_forward", ENULL, lay, **{a: None}) for lay in ({}, PLANES) for a in ("x", "y", "workspace", "save_stats")],
    _r("bn_train_forward", ENULL, running_mean=None), _r("bn_train_forward", ENULL, running_var=None),
    _r("bn_train_forward", ENULL, PLANES, running_mean=None),
    *[_r("bn_train_forward", EALIGN, lay, **{a: ODD1}) for lay in ({}, PLANES) for a in ("x", "y", "residual")],
    *[_r("bn_train_forward", EALIGN, FP32, **{a: ODD}) for a in ("x", "y", "residual")],
    _r("bn_train_forward", ESHAPE, BIG_C), _r("bn_train_forward", ESHAPE, NCHW_BIG_C), _r("bn_train_forward", ESHAPE, NCHW_BIG_V),
    _r("bn_train_forward", ESHAPE, UPDATES2, PLANES), _r("bn_train_forward", ESHAPE, UPDATES2, PLANES, FP32),
    _r("bn_train_forward", ESHAPE, {"@updates": 0}, PLANES),
    _r("bn_train_forward", ENULL, UPDATES2, PLANES, x=None), _r("bn_train_forward", EALIGN, UPDATES2, PLANES, y=ODD1),
    _r("bn_train_forward", ENULL, UPDATES2, PLANES, running_var=None), _r("bn_train_forward", ELAYOUT, UPDATES2, layout=2),
    _r("bn_train_forward", EDTYPE, dtype=2, layout=2), _r("bn_train_forward", ESHAPE, hw=0, layout=2, x=None),
    _r("bn_train_forward", ELAYOUT, layout=2, y=None), _r("bn_train_forward", ENULL, y=None, x=ODD1),
    _r("bn_train_forward", ENULL, running_mean=None, residual=ODD1), _r("bn_train_forward", ENULL, BIG_C, save_stats=None),
    _r("bn_train_forward", EALIGN, BIG_C, residual=ODD1), _r("bn_train_forward", EALIGN, NCHW_BIG_V, x=ODD1),
    # ---- afan_bn_train_forward_partials ----
    _r("bn_train_forward_partials", EDTYPE, dtype=7), _r("bn_train_forward_partials", ESHAPE, n=0), _r("bn_train_forward_partials", ESHAPE, c=0),
    _r("bn_train_forward_partials", ESHAPE, hw=0),
    *[_r("bn_train_forward_partials", ENULL, **{a: None}) for a in ("x", "y", "partials", "save_stats")],
    _r("bn_train_forward_partials", ESHAPE, partials_g=0), _r("bn_train_forward_partials", ESHAPE, partials_g=-1),
    _r("bn_train_forward_partials", ENULL, running_mean=None), _r("bn_train_forward_partials", ENULL, running_var=None),
    *[_r("bn_train_forward_partials", EALIGN, **{a: ODD1}) for a in ("x", "y", "residual")],
    _r("bn_train_forward_partials", EALIGN, FP32, x=ODD), _r("bn_train_forward_partials", ESHAPE, BIG_C),
    _r("bn_train_forward_partials", EDTYPE, dtype=7, x=None), _r("bn_train_forward_partials", ENULL, partials=None, partials_g=0),
    _r("bn_train_forward_partials", ESHAPE, partials_g=0, running_mean=None), _r("bn_train_forward_partials", ESHAPE, partials_g=0, x=ODD1),
    _r("bn_train_forward_partials", ENULL, running_var=None, y=ODD1), _r("bn_train_forward_partials", EALIGN, BIG_C, x=ODD1),
    # ---- afan_bn_train_forward_acc ----
    _r("bn_train_forward_acc", EDTYPE, dtype=7), _r("bn_train_forward_acc", ESHAPE, n=0), _r("bn_train_forward_acc", ESHAPE, c=0),
    _r("bn_train_forward_acc", ESHAPE, hw=0),
    *[_r("bn_train_forward_acc", ENULL, **{a: None}) for a in ("x", "y", "acc", "save_stats")],
    _r("bn_train_forward_acc", ENULL, running_mean=None), _r("bn_train_forward_acc", ENULL, running_var=None),
    _r("bn_train_forward_acc", ESHAPE, NO_VEC), _r("bn_train_forward_acc", ESHAPE, c=4), _r("bn_train_forward_acc", ESHAPE, c=4096),
    _r("bn_train_forward_acc", ESHAPE, FP32, c=2048), _r("bn_train_forward_acc", ESHAPE, BIG_C),
    *[_r("bn_train_forward_acc", EALIGN, **{a: ODD1}) for a in ("x", "y", "residual", "acc")],
    _r("bn_train_forward_acc", EALIGN, acc=ODD), _r("bn_train_forward_acc", EALIGN, FP32, x=ODD),
    _r("bn_train_forward_acc", ESHAPE, groups=0), _r("bn_train_forward_acc", ESHAPE, groups=-1), _r("bn_train_forward_acc", ESHAPE, groups=3),
    _r("bn_train_forward_acc", ESHAPE, groups=2, n=3),
    _r("bn_train_forward_acc", ESHAPE, groups=2, acc_ready=0),                           # groups need sums that are ready
    _r("bn_train_forward_acc", ESHAPE, x=ODD), _r("bn_train_forward_acc", ESHAPE, y=ODD), _r("bn_train_forward_acc", ESHAPE, residual=ODD),
    _r("bn_train_forward_acc", ESHAPE, acc_ready=0, x=ODD),                              # outside the vector mapping: !p.vec
    _r("bn_train_forward_acc", ESHAPE, save_stats=ODD), _r("bn_train_forward_acc", ESHAPE, save_stats=ODD1),
    _r("bn_train_forward_acc", ESHAPE, groups=2, save_stats=ODD),
    _r("bn_train_forward_acc", ENULL, acc=None, c=12), _r("bn_train_forward_acc", ENULL, running_mean=None, c=12),
    _r("bn_train_forward_acc", ESHAPE, NO_VEC, acc=ODD), _r("bn_train_forward_acc", ESHAPE, NO_VEC, groups=3),
    _r("bn_train_forward_acc", EALIGN, acc=ODD, groups=3), _r("bn_train_forward_acc", EALIGN, x=ODD1, save_stats=ODD),
    _r("bn_train_forward_acc", EALIGN, acc=ODD, groups=2, acc_ready=0), _r("bn_train_forward_acc", ENULL, x=None, acc=ODD),
    _r("bn_train_forward_acc", ESHAPE, acc=P16, save_stats=ODD),                         # + 16 is aligned enough for the block
    # ---- afan_bn_train_forward_acc_dual ----
    _r("bn_train_forward_acc_dual", EDTYPE, dtype=7), _r("bn_train_forward_acc_dual", ESHAPE, n=0), _r("bn_train_forward_acc_dual", ESHAPE, c=0),
    _r("bn_train_forward_acc_dual", ESHAPE, hw=0),
    *[_r("bn_train_forward_acc_dual", ENULL, **{a: None}) for a in ("x_a", "x_b", "y", "acc_a", "acc_b", "save_stats_a", "save_stats_b")],
    *[_r("bn_train_forward_acc_dual", ENULL, **{a: None}) for a in ("running_mean_a", "running_var_a", "running_mean_b", "running_var_b")],
    _r("bn_train_forward_acc_dual", ESHAPE, NO_VEC), _r("bn_train_forward_acc_dual", ESHAPE, FP32, c=2048),
    *[_r("bn_train_forward_acc_dual", EALIGN, **{a: ODD1}) for a in ("x_a", "x_b", "y", "acc_a", "acc_b")],
    _r("bn_train_forward_acc_dual", EALIGN, acc_b=ODD),
    *[_r("bn_train_forward_acc_dual", ESHAPE, **{a: ODD}) for a in ("x_a", "x_b", "y", "save_stats_a", "save_stats_b")],
    _r("bn_train_forward_acc_dual", ENULL, running_var_b=None, c=12), _r("bn_train_forward_acc_dual", ESHAPE, NO_VEC, acc_a=ODD),
    _r("bn_train_forward_acc_dual", EALIGN, acc_a=ODD, save_stats_b=ODD), _r("bn_train_forward_acc_dual", ENULL, x_b=None, x_a=ODD1),
    _r("bn_train_forward_acc_dual", ESHAPE, acc_a=P16, x_a=ODD),
    # ---- afan_bn_apply ----
    _r("bn_apply", EDTYPE, dtype=7), _r("bn_apply", ESHAPE, n=0), _r("bn_apply", ESHAPE, c=0), _r("bn_apply", ESHAPE, hw=0),
    _r("bn_apply", ELAYOUT, layout=2),
    *[_r("bn_apply", ENULL, lay, **{a: None}) for lay in ({}, PLANES) for a in ("x", "y", "mean", "invstd")],
    *[_r("bn_apply", EALIGN, lay, **{a: ODD1}) for lay in ({}, PLANES) for a in ("x", "y", "residual")],
    _r("bn_apply", EALIGN, FP32, y=ODD), _r("bn_apply", ENULL, workspace=None),
    _r("bn_apply", ESHAPE, BIG_C), _r("bn_apply", ESHAPE, NCHW_BIG_C), _r("bn_apply", ESHAPE, NCHW_BIG_V),
    _r("bn_apply", ESHAPE, NCHW_BIG_C, workspace=None),
    _r("bn_apply", EDTYPE, dtype=7, layout=2), _r("bn_apply", ELAYOUT, layout=2, mean=None), _r("bn_apply", ENULL, mean=None, x=ODD1),
    _r("bn_apply", EALIGN, workspace=None, x=ODD1), _r("bn_apply", ENULL, workspace=None, mean=None),
    _r("bn_apply", ENULL, BIG_C, workspace=None), _r("bn_apply", ELAYOUT, layout=2, workspace=None),
    # ---- afan_affine_coefs ----
    _r("affine_coefs", ESHAPE, c=0), _r("affine_coefs", ESHAPE, c=-1),
    *[_r("affine_coefs", ENULL, **{a: None}) for a in ("mean", "invstd", "coefs")],
    _r("affine_coefs", EALIGN, coefs=ODD), _r("affine_coefs", EALIGN, coefs=ODD1),
    _r("affine_coefs", ESHAPE, c=0, mean=None), _r("affine_coefs", ENULL, invstd=None, coefs=ODD), _r("affine_coefs", ESHAPE, c=0, coefs=ODD),
    # ---- afan_affine_apply ----
    _r("affine_apply", EDTYPE, dtype=7), _r("affine_apply", ESHAPE, n=0), _r("affine_apply", ESHAPE, c=0), _r("affine_apply", ESHAPE, hw=0),
    *[_r("affine_apply", ENULL, **{a: None}) for a in ("x", "y", "coefs")],
    *[_r("affine_apply", EALIGN, **{a: ODD1}) for a in ("x", "y", "residual")], _r("affine_apply", EALIGN, FP32, residual=ODD),
    _r("affine_apply", ESHAPE, BIG_C),
    _r("affine_apply", EDTYPE, dtype=7, n=0), _r("affine_apply", ESHAPE, n=0, x=None), _r("affine_apply", ENULL, coefs=None, x=ODD1),
    _r("affine_apply", EALIGN, BIG_C, y=ODD1), _r("affine_apply", ENULL, BIG_C, coefs=None),
    # ---- afan_bn_backward ----
    _r("bn_backward", EDTYPE, dtype=7), _r("bn_backward", ESHAPE, n=0), _r("bn_backward", ESHAPE, c=0), _r("bn_backward", ESHAPE, hw=0),
    _r("bn_backward", ELAYOUT, layout=2),
    *[_r("bn_backward", ENULL, lay, **{a: None}) for lay in ({}, PLANES) for a in ("dy", "x", "dx", "save_stats", "workspace")],
    _r("bn_backward", ESHAPE, PLANES, PART), _r("bn_backward", ESHAPE, partials=P, partials_g=0), _r("bn_backward", ESHAPE, partials=P, partials_g=-2),
    *[_r("bn_backward", EALIGN, lay, **{a: ODD1}) for lay in ({}, PLANES) for a in ("dy", "x", "dx", "y", "d_residual")],
    _r("bn_backward", EALIGN, FP32, dy=ODD), _r("bn_backward", EALIGN, PART, d_residual=ODD1),
    _r("bn_backward", ESHAPE, BIG_C), _r("bn_backward", ESHAPE, BIG_C, PART), _r("bn_backward", ESHAPE, NCHW_BIG_C),
    _r("bn_backward", ESHAPE, NCHW_BIG_V),
    _r("bn_backward", EDTYPE, dtype=7, layout=2), _r("bn_backward", ELAYOUT, layout=2, dy=None), _r("bn_backward", ELAYOUT, PART, layout=2),
    _r("bn_backward", ENULL, PLANES, PART, dy=None), _r("bn_backward", ESHAPE, PLANES, PART, dy=ODD1),
    _r("bn_backward", ESHAPE, partials=P, partials_g=0, y=ODD1), _r("bn_backward", ENULL, workspace=None, x=ODD1),
    _r("bn_backward", EALIGN, BIG_C, dx=ODD1),
    # ---- afan_bn_backward_acc ----
    _r("bn_backward_acc", EDTYPE, dtype=7), _r("bn_backward_acc", ESHAPE, n=0), _r("bn_backward_acc", ESHAPE, c=0), _r("bn_backward_acc", ESHAPE, hw=0),
    *[_r("bn_backward_acc", ENULL, **{a: None}) for a in ("dy", "x", "dx", "save_stats", "acc")],
    _r("bn_backward_acc", ESHAPE, NO_VEC), _r("bn_backward_acc", ESHAPE, FP32, c=2048), _r("bn_backward_acc", ESHAPE, BIG_C),
    *[_r("bn_backward_acc", EALIGN, **{a: ODD1}) for a in ("dy", "x", "dx", "y", "d_residual", "acc")],
    _r("bn_backward_acc", EALIGN, acc=ODD), _r("bn_backward_acc", EALIGN, FP32, dx=ODD),
    _r("bn_backward_acc", ESHAPE, groups=0), _r("bn_backward_acc", ESHAPE, groups=3), _r("bn_backward_acc", ESHAPE, groups=2, n=3),
    _r("bn_backward_acc", ESHAPE, groups=2, acc_ready=0),
    *[_r("bn_backward_acc", ESHAPE, **{a: ODD}) for a in ("dy", "x", "dx", "y", "d_residual", "save_stats")],
    _r("bn_backward_acc", ESHAPE, acc_ready=0, dy=ODD), _r("bn_backward_acc", ESHAPE, groups=2, save_stats=ODD),
    _r("bn_backward_acc", ENULL, acc=None, c=12), _r("bn_backward_acc", ESHAPE, NO_VEC, acc=ODD), _r("bn_backward_acc", ESHAPE, NO_VEC, groups=3),
    _r("bn_backward_acc", EALIGN, acc=ODD, groups=3), _r("bn_backward_acc", EALIGN, y=ODD1, save_stats=ODD),
    _r("bn_backward_acc", ENULL, dy=None, acc=ODD), _r("bn_backward_acc", ESHAPE, acc=P16, save_stats=ODD),
    # ---- afan_bn_running_update ----
    _r("bn_running_update", ESHAPE, c=0), _r("bn_running_update", ESHAPE, c=-1), _r("bn_running_update", ESHAPE, m_count=0.5),
    _r("bn_running_update", ESHAPE, m_count=0.0),
    *[_r("bn_running_update", ENULL, **{a: None}) for a in ("stats", "running_mean", "running_var")],
    _r("bn_running_update", ESHAPE, c=0, stats=None), _r("bn_running_update", ESHAPE, m_count=0.5, running_var=None),
    # ---- afan_bn_running_update_batched ----
    _r("bn_running_update_batched", ESHAPE, n=-1), _r("bn_running_update_batched", OK, n=0),
    _r("bn_running_update_batched", ESHAPE, n=-1, stats=None), _r("bn_running_update_batched", OK, n=0, stats=None),
    *[_r("bn_running_update_batched", ENULL, **{a: None})
      for a in ("stats", "running_mean", "running_var", "num_batches", "c", "m_count", "eps", "momentum")],
    _r("bn_running_update_batched", ESHAPE, c=[0, 16]), _r("bn_running_update_batched", ESHAPE, c=[64, -1]),
    _r("bn_running_update_batched", ESHAPE, m_count=[32.0, 0.5]),
    _r("bn_running_update_batched", ENULL, stats=[None, P]), _r("bn_running_update_batched", ENULL, running_mean=[P, None]),
    _r("bn_running_update_batched", ENULL, running_var=[P, None]),
    _r("bn_running_update_batched", ESHAPE, c=[0, 16], stats=[None, P]),              # within an item: the size first
    _r("bn_running_update_batched", ENULL, c=[64, 0], stats=[None, P]),               # across items: the first bad item
    _r("bn_running_update_batched", ESHAPE, m_count=[0.0, 8.0], running_var=[P, None]),
    # ---- afan_normalize_nchw ----
    _r("normalize_nchw", EDTYPE, out_dtype=7), _r("normalize_nchw", ESHAPE, n=0), _r("normalize_nchw", ESHAPE, c=0),
    _r("normalize_nchw", ESHAPE, hw=0), _r("normalize_nchw", ELAYOUT, out_layout=2),
    *[_r("normalize_nchw", ENULL, **{a: None}) for a in ("x", "y", "mean", "std")],
    _r("normalize_nchw", EDTYPE, out_dtype=7, out_layout=2), _r("normalize_nchw", ESHAPE, hw=0, out_layout=2),
    _r("normalize_nchw", ELAYOUT, out_layout=2, x=None), _r("normalize_nchw", ENULL, out_layout=NCHW, std=None),
]

# (c, afan_bn_workspace_floats(c), afan_bn_acc_doubles(c), afan_bn_acc_supported(F32 | BF16 | 7, c)): the channel counts of
# test_bn_pinned_gpu.py::test_predicates_agree_with_library, and two that are no channel count
QUERIES = [
    (-1, 0, 0, 0, 0, 0),
    (0, 0, 0, 0, 0, 0),
    (1, 1030, 33, 0, 0, 0),
    (2, 2060, 65, 0, 0, 0),
    (3, 3090, 98, 0, 0, 0),
    (4, 4120, 130, 1, 0, 0),
    (5, 5150, 163, 0, 0, 0),
    (6, 6180, 195, 0, 0, 0),
    (8, 8240, 260, 1, 1, 0),
    (12, 12360, 390, 0, 0, 0),
    (16, 16480, 520, 1, 1, 0),
    (24, 24720, 780, 0, 0, 0),
    (40, 41200, 1300, 0, 0, 0),
    (48, 49440, 1560, 0, 0, 0),
    (64, 65920, 2080, 1, 1, 0),
    (96, 98880, 1584, 0, 0, 0),
    (128, 131840, 2112, 1, 1, 0),
    (200, 206000, 1700, 0, 0, 0),
    (256, 263680, 2176, 1, 1, 0),
    (304, 313120, 1368, 0, 0, 0),
    (512, 527360, 2304, 1, 1, 0),
    (1024, 1054720, 2560, 1, 1, 0),
    (2048, 2109440, 5120, 0, 1, 0),
    (4096, 4218880, 10240, 0, 0, 0),
    (8192, 8437760, 20480, 0, 0, 0),
]


def _pointers():
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 63) & ~63
    return buf, {P: base, ODD: base + 2, ODD1: base + 1, P16: base + 16}


def build_call(entry, overrides, ptrs, keep):
    """The ctypes argument list of one row (keep: the arrays that must outlive the call)."""
    names, base = ENTRIES[entry]
    names = names.split()
    assert len(names) == len(base) and {k for k in overrides if k[0] != "@"} <= set(names), (entry, overrides)
    args = []
    for name, v in zip(names, base):
        v = overrides.get(name, v)
        if isinstance(v, list):
            ctype = _ARRAYS[name]
            arr = (ctype * len(v))(*[ptrs.get(t, t) if isinstance(t, str) else t for t in v])
            keep.append(arr)
            v = ctypes.cast(arr, ctypes.c_void_p)
        elif isinstance(v, str):
            v = ctypes.c_void_p(ptrs[v])
        elif v is not None and (name in _FLOATS or name in _DOUBLES):
            v = float(v)
        args.append(v)
    return args


def test_every_entry_has_rows():
    assert {r[0] for r in ROWS} == set(ENTRIES) and len(ROWS) > 350
    codes = {code for _, _, code in ROWS}
    assert codes == {OK, EDTYPE, EALIGN, ESHAPE, ENULL, ELAYOUT}
    assert all(entry == "bn_running_update_batched" for entry, _, code in ROWS if code == OK)     # n == 0: nothing to do
    assert len({(e, tuple(sorted((k, str(v)) for k, v in o.items()))) for e, o, _ in ROWS}) == len(ROWS), "a row is there twice"


def test_return_codes_of_refused_calls(pkg):
    lib = pkg._lib.load()
    buf, ptrs = _pointers()
    wrong = []
    for entry, overrides, code in ROWS:
        keep = []
        args = build_call(entry, overrides, ptrs, keep)
        updates = overrides.get("@updates", 1)
        before = lib.afan_bn_set_running_updates(updates)
        try:
            got = getattr(lib, "afan_" + entry)(*args)
        finally:
            during = lib.afan_bn_set_running_updates(before)
        assert during == updates, (entry, overrides)              # the call itself leaves the count alone
        if got != code:
            wrong.append((entry, overrides, code, got))
    assert lib.afan_bn_set_running_updates(1) == 1, "the update count was left changed"
    assert not wrong, "\n".join(f"{e} {o}: {g}, recorded {c}" for e, o, c, g in wrong)


def test_update_count_semantics(pkg):
    """afan_bn_set_running_updates returns the previous value; n < 0 stands for 1, 0 is kept (a deferred update)."""
    lib = pkg._lib.load()
    assert lib.afan_bn_set_running_updates(3) == 1
    assert lib.afan_bn_set_running_updates(0) == 3
    assert lib.afan_bn_set_running_updates(-5) == 0
    assert lib.afan_bn_set_running_updates(1) == 1


def test_query_values(pkg):
    lib = pkg._lib.load()
    got = [(c, lib.afan_bn_workspace_floats(c), lib.afan_bn_acc_doubles(c), lib.afan_bn_acc_supported(F32, c),
            lib.afan_bn_acc_supported(BF16, c), lib.afan_bn_acc_supported(7, c)) for c, *_ in QUERIES]
    if "AFAN_BN_SLOTS" in os.environ:        # the one tuning variable these queries read: it sizes the accumulator block
        drop = lambda rows: [r[:2] + r[3:] for r in rows]
        assert drop(got) == drop(QUERIES)
    else:
        assert got == QUERIES
