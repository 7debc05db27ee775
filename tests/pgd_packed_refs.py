"""numpy restatement of csrc/afan_pgd_packed.hip: the byte of 2-bit sign codes, the replay of the earlier steps from the bf16 start, and
one packed step, all built on update_pinned_refs.pgd_step / sign / clamp (one numpy operation per fp32 rounding), and the plain
chain of pgd_step they must equal.  bf16 values are uint16 bit patterns.  Shared by tests/test_pgd_packed_ref.py (CPU) and
tests/test_pgd_packed_gpu.py."""
import numpy as np

import update_pinned_refs as R

F = R.F
GAMMA, EPS = F(0.5 / 255), F(2 / 255)           # the issue's scalars: at K = 5 the clamp of clip=True is active (5 gamma > eps)
MAX_CODES = 4
X0_SPECIAL = (-0.0, 0.0, 1e-30, 3e4, -3e4, 1e6, 1.0, -0.5)         # 3e4: an ulp of 2^-9 next to gamma; 1e6: +-gamma is absorbed
G_SPECIAL = (0.0, -0.0, np.nan, np.inf, -np.inf, 1e-30, -1e-30, 2.5, -2.5)


def code_of(g):
    """0 = zero gradient, 1 = positive, 2 = negative, 3 = NaN."""
    g = np.asarray(g, F)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(g), 3, np.where(g > 0, 1, np.where(g < 0, 2, 0))).astype(np.uint8)


def sign_from(c):
    """sign()'s value for the gradient that gave the code."""
    return np.array([0.0, 1.0, -1.0, np.nan], F)[np.asarray(c, np.uint8) & 3]


def replay(x0_bits, codes, t, gamma, eps, clip):
    """The fp32 iterate after steps 0..t-1 from the bf16 start and the code bytes (step s in bits 2s..2s+1)."""
    xc = R.bf16_widen(x0_bits)
    xa = xc.copy()
    for s in range(t):
        xa = R.pgd_step(xa, sign_from((np.asarray(codes, np.uint8) >> (2 * s)) & 3), xc, gamma, eps, clip)
    return xa


def packed_step(x0_bits, grad, codes, t, gamma, eps, clip):
    """Step t: (the new code bytes, the bf16 shadow of the new iterate, the new fp32 iterate).  codes is ignored at t == 0."""
    codes = np.zeros(np.shape(x0_bits), np.uint8) if t == 0 else np.asarray(codes, np.uint8)
    xa = R.pgd_step(replay(x0_bits, codes, t, gamma, eps, clip), np.asarray(grad, F), R.bf16_widen(x0_bits), gamma, eps, clip)
    new = (codes & np.uint8((1 << (2 * t)) - 1)) | (code_of(grad) << np.uint8(2 * t)).astype(np.uint8) if t < MAX_CODES else codes
    return new.astype(np.uint8), R.bf16_bits(xa), xa


def chain(x0_bits, grads, gamma, eps, clip):
    """The plain chain: the fp32 iterates after each step of pgd_step from the widened start."""
    xc = R.bf16_widen(x0_bits)
    xa, out = xc.copy(), []
    for g in grads:
        xa = R.pgd_step(xa, np.asarray(g, F), xc, gamma, eps, clip)
        out.append(xa)
    return out


def inputs(n, steps, seed):
    """(x0 as bf16 bits, [grad_t as fp32 values that are exact in bf16]) of n elements: every pair of (special start, special gradient)
    first where n allows, the gradients rolled from step to step so that an element meets different specials in turn; the rest random,
    a quarter of the gradients exactly zero."""
    rng = np.random.default_rng(seed)
    x0 = (rng.standard_normal(n) * 2).astype(F)
    xs, gs = np.array(X0_SPECIAL, F), np.array(G_SPECIAL, F)
    m = min(n, xs.size * gs.size)
    x0[:m] = np.repeat(xs, gs.size)[:m]
    x0_bits = R.bf16_bits(x0)
    grads = []
    for t in range(steps):
        g = rng.standard_normal(n).astype(F)
        g[rng.random(n) < 0.25] = 0.0
        g[:m] = np.roll(np.tile(gs, xs.size), t)[:m]
        with np.errstate(over="ignore"):
            grads.append(R.bf16_widen(R.bf16_bits(g)))
    return x0_bits, grads
