"""The references of the L2 step (tests/pgd_l2_refs.py) on the CPU: the fp32 restatement against the float64 formula inside the counted
bounds, and both against the recorded outputs of the reference's own l2ball_proj (tests/golden/l2ball_proj.npz, written by
tools/gen_l2_golden.py from Classification/attack_algo.py:21-33; every sample has at most 32 elements).

What the golden cases show.  On every sample with a non-zero perturbation the reference's output and the restatement's both lie
within pgd_l2_refs.proj_elem_bound of the float64 formula, element by element.  The restatement differs from the reference in
behaviour in exactly the two documented ways: a sample inside the ball keeps its bits (the reference rounds it through
`/ dist * dist`: still inside the bound, but not the input's bits in every case), and a zero perturbation stays zero (the reference
returns NaN for the whole sample).  Outside the ball the two are different roundings of one formula (d / dist * radius against
d * (radius / dist)), both inside the bound."""
import numpy as np
import pytest

import pgd_l2_refs as L
from conftest import golden

F = np.float32


def _cases():
    g = golden("l2ball_proj")
    for k in range(int(g["cases"])):
        c, t, out = g[f"c{k}_center"], g[f"c{k}_t"], g[f"c{k}_out"]
        b = c.shape[0]
        yield k, c.reshape(b, -1), t.reshape(b, -1), F(g[f"c{k}_radius"]), g[f"c{k}_kind"], out.reshape(b, -1)


def test_golden_has_every_kind():
    kinds = np.concatenate([kd for _, _, _, _, kd, _ in _cases()])
    assert len(list(_cases())) >= 24 and all((kinds == v).sum() >= 3 for v in (0, 1, 2))
    assert all(c.shape[1] <= 32 for _, c, _, _, _, _ in _cases())


def test_reference_and_restatement_lie_in_the_counted_bound_of_float64():
    worst_ref = worst_res = 0.0
    for k, c, t, radius, kind, ref_out in _cases():
        per = c.shape[1]
        r64 = L.step_l2_f64(t, None, c, 0.0, radius, True)
        nd = L.nearest_norm(t.astype(np.float64) - c.astype(np.float64))
        res, _ = L.step_l2(t, None, c, 0.0, radius, True, None, nd)
        q64 = np.where((r64["nd"] > float(radius))[:, None], r64["q"], t.astype(np.float64) - c.astype(np.float64))
        bound = L.proj_elem_bound(r64["out"], q64, per)
        live = kind != 2
        assert live.any() or (kind == 2).all()
        for name, got in (("reference", ref_out), ("restatement", res)):
            err = np.abs(got.astype(np.float64) - r64["out"])[live]
            assert np.isfinite(err).all() and (err <= bound[live]).all(), (name, k, float((err / bound[live]).max()))
        worst_ref = max(worst_ref, float((np.abs(ref_out.astype(np.float64) - r64["out"])[live] / bound[live]).max(initial=0)))
        worst_res = max(worst_res, float((np.abs(res.astype(np.float64) - r64["out"])[live] / bound[live]).max(initial=0)))
    print(f"L2REF worst error / bound: reference {worst_ref:.3f}, restatement {worst_res:.3f}")


def test_the_two_documented_differences():
    inside_moved = 0
    for k, c, t, radius, kind, ref_out in _cases():
        nd = L.nearest_norm(t.astype(np.float64) - c.astype(np.float64))
        res, sh = L.step_l2(t, None, c, 0.0, radius, True, None, nd)
        for b, kd in enumerate(kind):
            if kd == 1:          # inside: the input's bits; the reference may move it
                assert L.same_f32(res[b], t[b]) is None, (k, b)
                inside_moved += L.same_f32(ref_out[b], t[b]) is not None
            elif kd == 2:        # a zero perturbation: stays the centre; the reference is NaN throughout
                assert L.same_f32(res[b], c[b]) is None and L.same_f32(res[b], t[b]) is None, (k, b)
                assert np.isnan(ref_out[b]).all(), (k, b)
            else:                # outside: on the sphere, and not the input
                assert L.same_f32(res[b], t[b]) is not None, (k, b)
                d = np.sqrt(((res[b].astype(np.float64) - c[b]) ** 2).sum())
                assert abs(d - float(radius)) <= 8 * L.U * (float(radius) + np.abs(c[b]).max() * np.sqrt(c.shape[1])), (k, b, d)
        assert L.same_bf16(sh, L.bf16_bits(res)) is None
    assert inside_moved > 0, "no inside sample of the golden set shows the reference's / dist * dist rounding"


def test_restatement_special_samples():
    eps = F(0.5)
    # one non-zero element with |d| == eps exactly stays (sqrt(fl(d * d)) == |d| in binary floating point); nextafter(eps) is projected
    up = np.nextafter(eps, F(np.inf))
    xa = np.zeros((2, 5), F)
    xa[0, 2], xa[1, 3] = eps, -up
    xc = np.zeros_like(xa)
    nd = np.sqrt((xa * xa).astype(F).sum(axis=1, dtype=F)).astype(F)
    assert nd[0] == eps and nd[1] == up
    out, _ = L.step_l2(xa, None, xc, 0.0, eps, True, None, nd)
    assert L.same_f32(out[0], xa[0]) is None
    assert out[1, 3] == -eps and L.same_f32(out[1], xa[1]) is not None
    # a zero gradient adds nothing (and -0.0 stays -0.0); a NaN gradient takes its own sample and no other
    xa = np.array([[1, -0.0, 3], [4, 5, 6], [7, 8, 9]], F)
    g = np.array([[0, 0, 0], [1, np.nan, 2], [3, 4, 0]], F)
    ng = np.array([0, np.nan, 5], F)
    out, _ = L.step_l2(xa, g, None, F(0.25), 0.0, False, ng, None)
    assert L.same_f32(out[0], xa[0]) is None and np.isnan(out[1]).all()
    assert L.same_f32(out[2], np.array([F(7) + F(F(0.25) / F(5)) * F(3), F(8) + F(F(0.25) / F(5)) * F(4), 9], F)) is None


@pytest.mark.parametrize("per", [1, 5, 64, 3072, 4100])
def test_restatement_lies_in_the_windows_of_float64(per):
    rng = np.random.default_rng(per)
    b, gamma, eps = 4, F(0.125), F(0.5)
    xc = rng.standard_normal((b, per)).astype(F)
    dl = rng.standard_normal((b, per))
    dl *= (np.array([0.3, 3.0, 0.3, 3.0]) * float(eps) / np.sqrt((dl * dl).sum(axis=1)))[:, None]
    xa, g = (xc + dl).astype(F), rng.standard_normal((b, per)).astype(F)
    r64 = L.step_l2_f64(xa, g, xc, gamma, eps, True)
    ng = L.nearest_norm(g)
    xn = L.stepped_iterate(xa, g, gamma, ng)
    nd = L.nearest_norm(xn.astype(np.float64) - xc)
    assert (np.abs(nd - r64["nd"]) <= L.dnorm_window(r64["nd"], np.sqrt((r64["x_new"] ** 2).sum(axis=1)), gamma, per, ng != 0)).all()
    assert ((r64["nd"] < 0.9 * float(eps)) | (r64["nd"] > 1.1 * float(eps))).all()
    out, _ = L.step_l2(xa, g, xc, gamma, eps, True, ng, nd)
    # as one 2-norm per sample: the stepped iterate's own error (within the dnorm window), the rescaling's share of the norm's error
    # (eps * |nd - nd64| / nd64 <= the window again), and the projection's elementwise bound
    err = np.sqrt(((out.astype(np.float64) - r64["out"]) ** 2).sum(axis=1))
    win = 2 * L.dnorm_window(r64["nd"], np.sqrt((r64["x_new"] ** 2).sum(axis=1)), gamma, per, ng != 0) \
        + np.sqrt((L.proj_elem_bound(r64["out"], r64["q"], per) ** 2).sum(axis=1))
    assert (err <= win).all(), (err / win)


def test_counts():
    assert L.c_g(1) == L.c_g(4096) == L.c_g(256 * 4096) == 38 and L.c_g(256 * 4096 + 1) == 39 and L.c_d(3072) == 40
    assert L.workspace_floats(5, 4097) == 20 and L.workspace_floats(0, 7) == 0
