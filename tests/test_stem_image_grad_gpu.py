"""afan_frozen_stem_image_grad (csrc/afan_stem_grad.hip) pinned ELEMENTWISE to float64, called through the C ABI with ctypes.
The references are tests/stem_grad_refs.py, written from the definition in include/afan_hip.h; test_reference_matches_autograd
(CPU, not marked gpu) checks them against torch autograd in float64 over normalise -> conv2d -> affine -> relu -> max_pool2d.

VARIANT under test: g1 rounded to bf16 ONCE (fp32 window sum x alpha, RNE) — the reference rounds at the same point
(stem_grad_refs.g1_of(bf16=True)); products accumulate in fp32.

Shapes, each with N = 2 (the batch stride): smaller than one tile (9 x 11), odd sides (37 x 51), even sides (38 x 50) and three tiles
in each direction with ragged last tiles, from the kernel's own constant TILE = afan_frozen_stem_image_grad_tile() = 32:
(2 TILE + 6) x (3 TILE + 5) = 70 x 101.

  * exact: ternary weights, integer gy in [-4, 4], power-of-two alpha (both signs) and inv_std, y1 on the levels {0, .5, 1, 1.5}, five in eight zero (pool
    windows tie at positive values and hold all-zero windows): every fp32 operation is exact in any order — equal to float64 bit for bit.
  * rounding-aware: Gaussian operands; |got - float64| <= C * 2^-24 * S elementwise, S the same expression on absolute values,
    C = 32 * 16 + 2 = 514: a wave adds at most 32 channels x 16 taps products by fmaf (one rounding each), the two channel halves
    are added once (1) and inv_std multiplies last (1).  Prints "STEMGRAD <case> <worst ratio>" (run with -s).
  * NaN: one NaN in y1 wins its windows (their gradients go to its position, which the ReLU mask then zeroes).

Worst ratios on an MI355X (every exact and NaN case bit for bit):
    9x11 0.0014   37x51 0.0028   38x50 0.0026   70x101 0.0025
"""
import ctypes

import numpy as np
import pytest
import torch

import stem_grad_refs as R

TILE = 32                                     # csrc/afan_stem_grad.hip TILE (checked against the library below)
SHAPES = [(9, 11), (37, 51), (38, 50), (2 * TILE + 6, 3 * TILE + 5)]
N = 2
C_ROUNDINGS = 32 * 16 + 2
BF16 = torch.bfloat16


def _bf(a):
    """numpy -> the bf16 tensor and the float64 array of the values it holds."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(BF16)
    return t, t.to(torch.float64).numpy()


def _operands(hi, wi, exact, seed):
    rng = np.random.default_rng(seed)
    ho, wo, hp, wp = R.geometry(hi, wi)
    if exact:
        gy = rng.integers(-4, 5, (N, hp, wp, 64)).astype(np.float64)
        y1 = rng.choice([0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 1.0, 1.5], (N, ho, wo, 64))
        w = rng.integers(-1, 2, (64, 7, 7, 3)).astype(np.float64)
        alpha = (2.0 ** rng.integers(-2, 2, 64)) * rng.choice([-1.0, 1.0], 64)
        inv_std = np.array([4.0, 2.0, 8.0])
    else:
        gy = rng.standard_normal((N, hp, wp, 64))
        y1 = np.maximum(rng.standard_normal((N, ho, wo, 64)), 0.0)
        w = 0.1 * rng.standard_normal((64, 7, 7, 3))
        alpha = 1.0 + 0.3 * rng.standard_normal(64)
        inv_std = 1.0 / np.array([0.229, 0.224, 0.225])
    return gy, y1, w, alpha.astype(np.float32), inv_std.astype(np.float32)


def _run(pkg, gpu, gy, y1, w, alpha, inv_std, hi, wi):
    """The kernel through the C ABI on bf16 copies of the operands; returns (dx fp32 on the host, the operands' float64 values)."""
    lib = pkg._lib.load()
    assert lib.afan_frozen_stem_image_grad_tile() == TILE
    tg, vg = _bf(gy)
    ty, vy = _bf(y1)
    tw, vw = _bf(w)
    dg, dy, dw = tg.to(gpu), ty.to(gpu), tw.to(gpu)
    da, ds = torch.from_numpy(alpha).to(gpu), torch.from_numpy(inv_std).to(gpu)
    dx = torch.full((N, 3, hi, wi), float("nan"), dtype=torch.float32, device=gpu)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.afan_frozen_stem_image_grad(P(dg), P(dy), P(dw), P(da), P(ds), P(dx), N, hi, wi,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, f"afan_frozen_stem_image_grad returned {rc}"
    torch.cuda.synchronize()
    return dx.cpu().numpy(), (vg, vy, vw)


@pytest.mark.gpu
@pytest.mark.parametrize("hi,wi", SHAPES)
def test_exact(pkg, gpu, hi, wi):
    gy, y1, w, alpha, inv_std = _operands(hi, wi, True, 11 + hi)
    got, (vg, vy, vw) = _run(pkg, gpu, gy, y1, w, alpha, inv_std, hi, wi)
    assert np.array_equal(vg, gy) and np.array_equal(vy, y1) and np.array_equal(vw, w)          # bf16 holds the operands exactly
    st = R.window_stack(vy)
    top = st.max(axis=0)
    assert (top == 0).any() and (((st == top) & (st > 0)).sum(axis=0) >= 2).any()                # all-zero windows, ties at positive values
    ref, _ = R.image_grad(vg, vy, vw, alpha, inv_std, hi, wi, bf16=True)
    ref64, _ = R.image_grad(vg, vy, vw, alpha, inv_std, hi, wi, bf16=False)
    assert np.array_equal(ref, ref64)                                                            # (the bf16 rounding of g1 is exact here)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    bad = got.astype(np.float64) != ref
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} elements differ from float64; first at {tuple(np.argwhere(bad)[0])}"


@pytest.mark.gpu
@pytest.mark.parametrize("hi,wi", SHAPES)
def test_rounding_aware(pkg, gpu, hi, wi):
    gy, y1, w, alpha, inv_std = _operands(hi, wi, False, 23 + wi)
    got, (vg, vy, vw) = _run(pkg, gpu, gy, y1, w, alpha, inv_std, hi, wi)
    ref, S = R.image_grad(vg, vy, vw, alpha, inv_std, hi, wi, bf16=True)
    assert np.isfinite(got).all()
    noise = C_ROUNDINGS * 2.0 ** -24 * S
    err = np.abs(got.astype(np.float64) - ref)
    pos = noise > 0
    ratio = float((err[pos] / noise[pos]).max())
    print(f"STEMGRAD {hi}x{wi} {ratio:.4f}")
    assert not (err[~pos] > 0).any()
    assert ratio <= 1.0, f"worst |got - float64| / (C 2^-24 S) = {ratio}"


@pytest.mark.gpu
def test_nan_wins_its_window(pkg, gpu):
    hi, wi = 37, 51
    gy, y1, w, alpha, inv_std = _operands(hi, wi, True, 5)
    y1[1, 5, 7, 9] = np.nan                     # odd row, odd column: inside four windows
    y1[1, 4:7, 6:9, 9] = np.where(np.isnan(y1[1, 4:7, 6:9, 9]), np.nan, 1.5)      # the largest level all round it
    gy[1, 2:4, 3:5, 9] = 3.0
    arg = R.pool_winners(y1)
    assert [int(arg[1, a, b, 9]) for a in (2, 3) for b in (3, 4)] == [8, 6, 2, 0]      # the NaN's place in each of the four windows
    got, (vg, vy, vw) = _run(pkg, gpu, gy, y1, w, alpha, inv_std, hi, wi)
    ref, _ = R.image_grad(vg, vy, vw, alpha, inv_std, hi, wi, bf16=True)
    y_no = np.where(np.isnan(vy), 1.5, vy)
    other, _ = R.image_grad(vg, y_no, vw, alpha, inv_std, hi, wi, bf16=True)
    assert not np.array_equal(ref, other)        # (without the NaN the 12 units of gradient would arrive somewhere)
    assert np.isfinite(got).all()
    assert np.array_equal(got.astype(np.float64), ref)


@pytest.mark.parametrize("hi,wi", [(9, 11), (22, 19)])
def test_reference_matches_autograd(hi, wi):
    """stem_grad_refs against torch autograd in float64 over normalise -> conv2d -> affine -> relu -> max_pool2d on tie-free inputs
    (Gaussian: positive values do not tie; tied zeros carry no gradient past the ReLU)."""
    rng = np.random.default_rng(3)
    ho, wo, hp, wp = R.geometry(hi, wi)
    x = torch.from_numpy(rng.standard_normal((N, 3, hi, wi))).requires_grad_(True)
    w = torch.from_numpy(0.2 * rng.standard_normal((64, 3, 7, 7)))
    mean, std = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64), torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64)
    alpha, beta = torch.from_numpy(1.0 + 0.3 * rng.standard_normal(64)), torch.from_numpy(0.1 * rng.standard_normal(64))
    gy = torch.from_numpy(rng.standard_normal((N, 64, hp, wp)))
    xn = (x - mean[None, :, None, None]) / std[None, :, None, None]
    y1 = torch.relu(torch.nn.functional.conv2d(xn, w, stride=2, padding=3) * alpha[None, :, None, None] + beta[None, :, None, None])
    yp = torch.nn.functional.max_pool2d(y1, 3, 2, 1)
    assert tuple(yp.shape) == (N, 64, hp, wp)
    (yp * gy).sum().backward()
    pos = y1.detach()[y1.detach() > 0].numpy()
    assert len(np.unique(pos)) == len(pos)
    ref, S = R.image_grad(gy.permute(0, 2, 3, 1).numpy(), y1.detach().permute(0, 2, 3, 1).numpy(), w.permute(0, 2, 3, 1).numpy(),
                          alpha.numpy(), (1.0 / std).numpy(), hi, wi, bf16=False)
    assert np.abs(ref - x.grad.numpy()).max() <= 2048 * 2.0 ** -53 * S.max()
    assert np.abs(x.grad.numpy()).max() > 0
