"""References of afan_pgd_step_l2 (csrc/afan_pgd.hip): the normalised-gradient L2 step and the projection onto the L2 ball.
tests/test_pgd_l2_gpu.py holds the kernel to them through the C ABI; tests/test_pgd_l2_ref.py checks them on the CPU against
float64 and against the recorded outputs of the reference's own l2ball_proj (tests/golden/l2ball_proj.npz).

Two references, over [batch, per_sample] arrays (sample b is row b):

  step_l2      the fp32 RESTATEMENT: one numpy float32 operation per rounding of include/afan_hip.h's lines.  The two norms are its
               INPUTS (ng [batch], nd [batch]): given the norms a run computed, every other line is one correctly rounded operation,
               so x_adv and the shadow are met in every bit.
  step_l2_f64  the same formula in float64: the norms and the whole result; its own error (2^-53 per operation) is ignored beside
               the fp32 windows below.

The counted window of the norms.  u = 2^-24 is fp32's unit roundoff.  A sum S of non-negative terms computed with at most c
roundings on the path of any term lies within gamma(c) * S of the exact sum, gamma(c) = c u / (1 - c u); the root of it, rounded
once more, within (gamma(c) / 2 + u + gamma(c) u) of the exact norm (sqrt(1 + e) <= 1 + e / 2).  The kernel's summation
(L2_CHUNK = 4096 elements per workgroup of BLOCK = 256 threads):

    the product g * g                                                                          1
    a thread's chain over its share of the chunk, L2_CHUNK / BLOCK products in index order    16
        (16 scalar trips; 4 float4 trips; 2 eight-wide trips with a bf16 gradient)
    the 64-lane butterfly                                                                      6
    the block's 4 wave sums, added in order                                                    4
    in the next launch: a thread's chain over the sample's partials                            ceil(chunks / 256)
    its butterfly and 4 wave sums                                                              6 + 4
                                                                          C_G(per_sample)  =  37 + ceil(chunks / 256)

and for Sd two more, the rounding of d = x_new - x_clean, which the square doubles: C_D = C_G + 2.  A product that underflows loses
at most 2^-126 (flushed or rounded), which adds per_sample * 2^-126 to the sum's bound.

dnorm against the float64 FORMULA needs the step's own error on top.  With e_g the relative window of ng: a = fl(gamma / ng) is
within e_a = (1 + u) / (1 - e_g) - 1 of gamma / ng64, p = fl(a g) within e_p = (1 + e_a)(1 + u) - 1 of its float64 value, and
x_new = fl(x_adv + p) within u |x_new| of the sum; the vector of the p's has norm gamma exactly, so the stored iterate is within
    delta = e_p (1 + u) gamma + u ||x_new64||_2
of the float64 one in the 2-norm, and nd within  delta + (nd64 + delta) e_d  of nd64 (the triangle inequality, then the window of
the sum over the stored values).  Without a step delta = 0.

The elementwise bound of the projection (used on the CPU, where the reference's recorded outputs and the restatement are both
held to the float64 formula): q = d * eps / nd carries three roundings (d, the quotient, the product) and the norm's window,
e_q = (1 + u)^3 / (1 - e_d) - 1, and the last sum one more: |out - out64| <= e_q |q64| + u (|out64| + e_q |q64|).  The reference
rounds in another order (d / dist, then * dist) with the same count of roundings, so the same bound holds for it wherever its norm is
inside the same window — which a sample of at most 32 elements guarantees whatever the order of torch's sum (at most 31 + 3
roundings per term, below C_D = 40).
"""
import numpy as np

from update_pinned_refs import bf16_bits, bf16_widen, same_bf16, same_f32  # noqa: F401  (shared, not restated)

F = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -126
BLOCK = 256
L2_CHUNK = 4096                     # csrc/afan_pgd.hip


def chunks_of(per_sample):
    return -(-per_sample // L2_CHUNK)


def workspace_floats(batch, per_sample):
    return 0 if batch <= 0 or per_sample <= 0 else 2 * batch * chunks_of(per_sample)


def c_g(per_sample):
    return 1 + L2_CHUNK // BLOCK + 6 + 4 + -(-chunks_of(per_sample) // BLOCK) + 6 + 4


def c_d(per_sample):
    return c_g(per_sample) + 2


def gamma_c(c):
    return c * U / (1.0 - c * U)


def norm_rel(c):
    """Relative window of sqrt(sum) for a sum with c roundings per term."""
    g = gamma_c(c)
    return g / 2 + U + g * U


def norm_window(norm64, c, per_sample):
    """Absolute window of a computed norm around the float64 one (array over the batch).  The underflow term: a sum off by t moves
    its root by at most sqrt(t)."""
    norm64 = np.asarray(norm64, np.float64)
    return norm_rel(c) * norm64 + np.sqrt(per_sample * TINY)


def dnorm_window(nd64, xnew_norm64, gamma, per_sample, stepped):
    """Window of dnorm (before the min with eps) around nd64 of the float64 formula; `stepped` [batch] bool: the sample took a step."""
    e_g = norm_rel(c_g(per_sample))
    e_a = (1 + U) / (1 - e_g) - 1
    e_p = (1 + e_a) * (1 + U) - 1
    delta = np.where(stepped, e_p * (1 + U) * abs(float(gamma)) + U * np.asarray(xnew_norm64, np.float64), 0.0)
    return delta + norm_window(np.asarray(nd64, np.float64) + delta, c_d(per_sample), per_sample)


def proj_elem_bound(out64, q64, per_sample):
    e_d = norm_rel(c_d(per_sample))
    e_q = (1 + U) ** 3 / (1 - e_d) - 1
    return e_q * np.abs(q64) + U * (np.abs(out64) + e_q * np.abs(q64))


# ================================================================================================================== the restatement
def step_l2(xa, g, xc, gamma, eps, clip, ng, nd):
    """(x_adv, shadow bits) after afan_pgd_step_l2, fp32 operation by operation.  xa, g (or None: the projection alone), xc (or None
    without clip): [batch, per_sample] float32; ng, nd: [batch] float32, the norms as the run computed them (nd is the norm of the
    STEPPED iterate minus xc, before the min with eps; unused without clip)."""
    xa = np.array(xa, F, copy=True)
    gamma, eps = F(gamma), F(eps)
    out = np.empty_like(xa)
    with np.errstate(all="ignore"):
        for b in range(xa.shape[0]):
            xn = xa[b]
            if g is not None and not (F(ng[b]) == F(0)):          # (a NaN norm is not zero)
                a = F(gamma / F(ng[b]))
                p = (a * np.asarray(g[b], F)).astype(F)
                xn = (xa[b] + p).astype(F)
            if clip and F(nd[b]) > eps:
                s = F(eps / F(nd[b]))
                d = (xn - xc[b]).astype(F)
                q = (d * s).astype(F)
                xn = (xc[b] + q).astype(F)
            out[b] = xn
    return out, bf16_bits(out)


def stepped_iterate(xa, g, gamma, ng):
    """The iterate after the step alone (what the ball test reads): step_l2 without clip."""
    return step_l2(xa, g, None, gamma, 0.0, False, ng, None)[0]


# ======================================================================================================================= float64
def step_l2_f64(xa, g, xc, gamma, eps, clip):
    """The whole formula in float64 on the fp32 inputs: dict of ng, x_new, nd (None without xc), q (the rescaled perturbation where
    projected, else d), out."""
    xa64 = np.asarray(xa, np.float64)
    gam, ep = float(F(gamma)), float(F(eps))
    with np.errstate(all="ignore"):
        if g is None:
            ng = np.zeros(xa64.shape[0])
            xn = xa64.copy()
        else:
            g64 = np.asarray(g, np.float64)
            ng = np.sqrt((g64 * g64).sum(axis=1))
            a = np.where(ng == 0, 0.0, gam / np.where(ng == 0, 1.0, ng))
            xn = xa64 + a[:, None] * g64
        r = {"ng": ng, "x_new": xn, "nd": None, "q": None, "out": xn}
        if xc is not None:
            d = xn - np.asarray(xc, np.float64)
            nd = np.sqrt((d * d).sum(axis=1))
            r["nd"], r["q"] = nd, d
            if clip:
                s = np.where(nd > ep, ep / np.where(nd > ep, nd, 1.0), 1.0)
                r["q"] = d * s[:, None]
                r["out"] = np.where((nd > ep)[:, None], np.asarray(xc, np.float64) + r["q"], xn)
    return r


def nearest_norm(v):
    """[batch] float32: the float64 norm of each row, rounded once (inside every window above)."""
    v = np.asarray(v, np.float64)
    return np.sqrt((v * v).sum(axis=1)).astype(F)
