"""float64 references of the frozen stem's image gradient (csrc/afan_stem_grad.hip, include/afan_hip.h), written from the definition:

    g1[n,p,q,k] = alpha[k] * [y1 > 0] * sum of gy over the 3x3 / 2 / 1 pool windows whose winner is (p, q)
    dx[n,c,i,j] = inv_std[c] * sum over k, r, s of g1[n,(i+3-r)/2,(j+3-s)/2,k] * w[k,r,s,c]     (divisions exact, position in range)

The winner of a window is the first maximum in (h, w) scan order, NaN winning (`v > best or v != v`, best starting at -inf: the last
NaN of a window wins it).  Arrays are numpy, channels-last: gy [N,Hp,Wp,64], y1 [N,Ho,Wo,64], w [64,7,7,3] (KRSC), dx [N,3,Hi,Wi].

The kernel rounds g1 to bf16 ONCE: the fp32 sum of the windows' gradients in window order (hp, then wq, ascending), times alpha in
fp32, then RNE to bf16.  `g1_of(..., bf16=True)` rounds at that point with those fp32 operations; bf16=False keeps float64.
tests/test_stem_image_grad_gpu.py::test_reference_matches_autograd checks bf16=False against torch autograd on the CPU."""
import numpy as np
import torch


def geometry(hi, wi):
    ho, wo = (hi - 1) // 2 + 1, (wi - 1) // 2 + 1
    return ho, wo, (ho - 1) // 2 + 1, (wo - 1) // 2 + 1


def window_stack(y1):
    """[9, N, Hp, Wp, K]: the pool windows' elements in scan order, -inf outside the map."""
    n, ho, wo, k = y1.shape
    hp, wp = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
    pad = np.full((n, ho + 3, wo + 3, k), -np.inf)
    pad[:, 1:ho + 1, 1:wo + 1] = y1
    return np.stack([pad[:, dh:dh + 2 * hp:2, dw:dw + 2 * wp:2] for dh in range(3) for dw in range(3)])


def pool_winners(y1):
    """arg [N,Hp,Wp,K]: the winner's position inside its window, dh * 3 + dw."""
    n, ho, wo, k = y1.shape
    hp, wp = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
    best = np.full((n, hp, wp, k), -np.inf)
    arg = np.zeros((n, hp, wp, k), dtype=np.int64)
    hh, ww = np.arange(hp) * 2 - 1, np.arange(wp) * 2 - 1
    # the start value: the first in-range element (what a window of -inf alone keeps)
    arg[:] = (np.where(hh < 0, 1, 0)[:, None] * 3 + np.where(ww < 0, 1, 0)[None, :])[None, :, :, None]
    pad = np.full((n, ho + 3, wo + 3, k), -np.inf)
    inr = np.zeros((ho + 3, wo + 3), dtype=bool)
    pad[:, 1:ho + 1, 1:wo + 1] = y1
    inr[1:ho + 1, 1:wo + 1] = True
    for dh in range(3):
        for dw in range(3):
            v = pad[:, dh:dh + 2 * hp:2, dw:dw + 2 * wp:2]
            ok = inr[dh:dh + 2 * hp:2, dw:dw + 2 * wp:2][None, :, :, None]
            with np.errstate(invalid="ignore"):
                upd = ok & ((v > best) | np.isnan(v))
            best = np.where(upd, v, best)
            arg = np.where(upd, dh * 3 + dw, arg)
    return arg


def pooled_grad(gy, y1, dtype=np.float64):
    """g0 [N,Ho,Wo,K]: per position the sum of gy over the windows it won, added in window order (hp, then wq, ascending) in `dtype`."""
    n, ho, wo, k = y1.shape
    hp, wp = gy.shape[1], gy.shape[2]
    arg = pool_winners(np.asarray(y1, dtype=np.float64))
    full = np.zeros((n, 2 * hp + 2, 2 * wp + 2, k), dtype=dtype)       # position (p, q) at [p + 1, q + 1]
    g = np.asarray(gy, dtype=dtype)
    for dh in (2, 1, 0):            # a position's windows in ascending hp are its descending dh
        for dw in (2, 1, 0):
            view = full[:, dh:dh + 2 * hp:2, dw:dw + 2 * wp:2]
            view[...] = np.where(arg == dh * 3 + dw, (view + g).astype(dtype), view)
    return full[:, 1:ho + 1, 1:wo + 1]


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def g1_of(gy, y1, alpha, bf16):
    y1 = np.asarray(y1, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        mask = y1 > 0
    if bf16:
        g0 = pooled_grad(gy, y1, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            g1 = bf16_round(np.asarray(alpha, dtype=np.float32)[None, None, None, :] * g0)
    else:
        g1 = np.asarray(alpha, dtype=np.float64)[None, None, None, :] * pooled_grad(gy, y1, np.float64)
    return np.where(mask, g1, 0.0)


def conv_adjoint(g1, w, inv_std, hi, wi):
    """dx [N,3,Hi,Wi] float64 from g1 [N,Ho,Wo,K] and w [K,7,7,3]."""
    n, ho, wo, _ = g1.shape
    w = np.asarray(w, dtype=np.float64)
    full = np.zeros((n, 2 * ho + 6, 2 * wo + 6, 3))                      # pixel (i, j) at [i + 3, j + 3]: i + 3 = 2p + r
    for r in range(7):
        for s in range(7):
            full[:, r:r + 2 * ho:2, s:s + 2 * wo:2] += np.einsum("npqk,kc->npqc", g1, w[:, r, s, :])
    dx = full[:, 3:3 + hi, 3:3 + wi] * np.asarray(inv_std, dtype=np.float64)[None, None, None, :]
    return np.ascontiguousarray(dx.transpose(0, 3, 1, 2))


def image_grad(gy, y1, w, alpha, inv_std, hi, wi, bf16):
    """(dx, S): the definition in float64 and the same expression on absolute values (the conv's sum over |g1| * |w| * |inv_std|)."""
    g1 = g1_of(gy, y1, alpha, bf16)
    return conv_adjoint(g1, w, inv_std, hi, wi), conv_adjoint(np.abs(g1), np.abs(np.asarray(w, dtype=np.float64)), np.abs(inv_std), hi, wi)
