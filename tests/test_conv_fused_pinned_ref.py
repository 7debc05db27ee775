"""The composed float64 references of tests/conv_fused_pinned_refs.py (what tests/test_conv_fused_pinned_gpu.py holds the fused
convolution epilogues and the in-launch BatchNorm to) against torch autograd in float64 on the CPU — the chain conv -> BatchNorm(train)
-> (+ residual | + BatchNorm(projection)) -> ReLU, forwards and backwards, the bf16 rounding of the intermediate entering as a
straight-through constant — and the restated dispatch_bnf / choose_bm / halo_ok / launch_gs predicates at hand-computed points."""
import pytest
import torch
import torch.nn.functional as F

import conv_fused_pinned_refs as R

TOL = 1e-12


def _rel(got, ref):
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def _ste(v):
    return v + (R.rne_bf16(v.detach()) - v.detach())


def _bn(t, w, b, eps):
    return F.batch_norm(t, None, None, w, b, True, 0.0, eps)


def _operands(seed, n=3, ci=8, co=16, h=6, k=3):
    g = torch.Generator().manual_seed(seed)
    q = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).double()
    f = lambda *s: torch.randn(*s, generator=g).float().double()
    return dict(x=q(n, ci, h, h), w=q(co, ci, k, k) * 0.25, res=q(n, co, h, h), raw_sc=q(n, co, h, h), dy=q(n, co, h, h),
                bw=f(co) + 1.5, bb=f(co), sw=f(co) - 1.5, sb=f(co))


@pytest.mark.parametrize("form", ["plain", "residual", "projection"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("k,d", [(3, 1), (1, 1), (3, 2)])
def test_forward_and_backward_chain_match_autograd(form, relu, k, d):
    o = _operands(k * 10 + d, k=k)
    eps, eps2 = 1e-5, 1e-3
    bw, bb, sw, sb = (o[n].clone().requires_grad_(True) for n in ("bw", "bb", "sw", "sb"))
    res, raw_sc = o["res"].clone().requires_grad_(True), o["raw_sc"].clone().requires_grad_(True)
    x = o["x"].clone().requires_grad_(True)
    raw64 = F.conv2d(x, o["w"], None, 1, d * (k // 2), d)
    assert _rel(R._ref_fwd(o["x"], o["w"], 1, d), raw64.detach()) <= TOL
    raw = _ste(raw64)
    raw.retain_grad()
    t = _bn(raw, bw, bb, eps)
    if form == "projection":
        t = t + _bn(raw_sc, sw, sb, eps2)
    elif form == "residual":
        t = t + res
    y = torch.relu(t) if relu else t
    y.backward(o["dy"])
    # forwards: the BatchNorm definition on the ROUNDED tile
    rr = R.rne_bf16(raw64.detach())
    assert bool((rr == raw.detach()).all()) and bool((rr.to(torch.bfloat16).double() == rr).all())
    sc = (o["raw_sc"], o["sw"], o["sb"], eps2) if form == "projection" else None
    f = R.ref_fwd_bn(rr, o["bw"], o["bb"], eps, o["res"] if form == "residual" else None, sc, relu)
    assert _rel(f["y"], y.detach()) <= TOL
    assert _rel(f["mean"], rr.mean((0, 2, 3))) <= TOL and _rel(f["var"], rr.var((0, 2, 3), unbiased=False)) <= TOL
    # backwards, from the reference's own statistics; the mask is the stored output's
    mask = (y.detach() > 0) if relu else None
    scb = (o["raw_sc"], f["mean2"], f["invstd2"], f["alpha2"]) if form == "projection" else None
    b = R.ref_dgrad_bn(o["dy"], rr, f["mean"], f["invstd"], f["alpha"], mask, scb)
    assert _rel(b["dx"], raw.grad) <= TOL and _rel(b["dw"], bw.grad) <= TOL and _rel(b["db"], bb.grad) <= TOL
    # (the rounding is a straight-through constant: the gradient entering the convolution is the one leaving the BatchNorm)
    assert _rel(R._ref_dgrad(b["dx"], o["w"], tuple(x.shape), 1, d), x.grad) <= TOL
    if form == "residual":
        assert _rel(b["g"], res.grad) <= TOL
    if form == "projection":
        assert _rel(b["sc_dx"], raw_sc.grad) <= TOL and _rel(b["sc_dw"], sw.grad) <= TOL and _rel(b["sc_db"], sb.grad) <= TOL
    # the scales bound their results
    assert bool((b["s_dx"] >= b["dx"].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("with_addend", [False, True])
def test_input_gradient_then_batchnorm_backward_matches_autograd(with_addend):
    """The backward launch's own order: g = RNE(RNE(dgrad(dy, w)) + addend) enters the backward of the BatchNorm (+ residual, ReLU)
    in FRONT of the convolution as a constant."""
    o = _operands(77, ci=16, co=8)
    eps = 1e-5
    xin = o["x"].clone().requires_grad_(True)                       # [n, 16, h, h]: the BatchNorm's input
    g = torch.Generator().manual_seed(5)
    bw, bb = (torch.randn(16, generator=g).double() + 1.0).requires_grad_(True), torch.randn(16, generator=g).double().requires_grad_(True)
    res = torch.randn(xin.shape, generator=g).to(torch.bfloat16).double()
    addend = torch.randn(xin.shape, generator=g).to(torch.bfloat16).double()
    a = torch.relu(_bn(xin, bw, bb, eps) + res)
    seen = {}
    g_ref = R.rne_bf16(R._ref_dgrad(o["dy"], o["w"], tuple(xin.shape), 1, 1))
    if with_addend:
        g_ref = R.rne_bf16(g_ref + addend)

    def hook(gr):
        seen["g"] = gr
        return g_ref

    a.register_hook(hook)
    loss = (F.conv2d(a, o["w"], None, 1, 1) * o["dy"]).sum() + ((a * addend).sum() if with_addend else 0.0)
    loss.backward()
    exact = R._ref_dgrad(o["dy"], o["w"], tuple(xin.shape), 1, 1) + (addend if with_addend else 0.0)
    assert _rel(exact, seen["g"]) <= TOL
    mean, var = R.ref_moments(xin.detach())
    invstd = 1.0 / torch.sqrt(var + eps)
    b = R.ref_dgrad_bn(g_ref, xin.detach(), mean, invstd, invstd * bw.detach(), a.detach() > 0)
    assert _rel(b["dx"], xin.grad) <= TOL and _rel(b["dw"], bw.grad) <= TOL and _rel(b["db"], bb.grad) <= TOL


def test_fma32_and_rne_helpers():
    a, b, c = (torch.tensor(v, dtype=torch.float64) for v in ([1.0 + 2.0 ** -23, 3.0], [1.0 + 2.0 ** -23, 0.5], [2.0 ** -30, 2.0 ** -24]))
    r, tie = R.fma32(a, b, c)
    assert float(r[0]) == 1.0 + 2.0 ** -22 and not bool(tie[0])      # 1 + 2^-22 + 2^-46 + 2^-30: rounds down to 1 + 2^-22
    assert bool(tie[1]) and float(r[1]) in (1.5, 1.5 + 2.0 ** -23)   # 1.5 + 2^-24: an fp32 midpoint
    v = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 257.0, -0.0], dtype=torch.float64)
    assert R.rne_bf16(v).tolist() == [1.0, 1.0 + 2.0 ** -6, 256.0, -0.0]


# ------------------------------------------------------------------------------------------------------------------ predicates
def test_predicates_at_hand_computed_points():
    assert [R.acc_slots(c) for c in (64, 128, 256, 512, 1024, 2048)] == [16, 8, 4, 2, 1, 1]
    assert R.acc_ok(128) and R.acc_ok(2048) and not R.acc_ok(384) and not R.acc_ok(4096)
    # choose_bm: 128 rows from 256 workgroups of 128 rows on, or for 257..768 workgroups of 64 rows of one class; else 64
    assert R.choose_bm(512, 128) == 64 and R.choose_bm(16384, 128) == 64           # 256 workgroups of 64 rows: not beyond 256
    assert R.choose_bm(16640, 128) == 128                                          # 260 of 64 rows: the tall rule
    assert R.choose_bm(16640, 256) == 128 and R.choose_bm(49216, 128) == 128       # 260 / 385 of 128 rows
    assert R.choose_bm(16640, 128, 4) == 128 and R.choose_bm(4160, 128, 4) == 64   # four classes: only the first rule (520 / 132)
    assert R.choose_bm(4160, 128, 4, True) == 128                                  # equal classes: 260 of 64 rows
    # halo_ok: one 8 x 8 image per 64-row tile spans its 10 x 10 padded raster exactly: 100 pixels
    assert R.halo_ok(8, 8, 8, 128, 128, 3, 1, 64) and not R.halo_ok(8, 8, 8, 128, 128, 1, 1, 64)
    assert not R.halo_ok(8, 8, 8, 128, 128, 3, 2, 64) and not R.halo_ok(8, 8, 8, 128, 64, 3, 1, 64)
    assert R.halo_ok(8, 8, 8, 128, 128, 3, 1, 64, cap=100) and not R.halo_ok(8, 8, 8, 128, 128, 3, 1, 64, cap=99)
    # one 16 x 16 image per 256-row tile: 18 x 18 = 324 pixels; four 8 x 8 images: 400
    assert R.halo_ok(2, 16, 16, 64, 128, 3, 1, 256, 328) and not R.halo_ok(2, 16, 16, 64, 128, 3, 1, 256, 320)
    assert R.halo_ok(8, 8, 8, 256, 128, 3, 1, 256, 400) and not R.halo_ok(8, 8, 8, 256, 128, 3, 1, 256, 399)
    # LDS of the forms (bytes): halo forms (PF - 1) * BN * 128 + 2 * HL * 128 + 1024; per-tap forms stages * (BM + BN) * 128
    assert R.lds_bytes(R.T64H) == 6 * 64 * 128 + 2 * 320 * 128 + 1024 == 132096
    assert R.lds_bytes(R.P128) == 4 * 256 * 128 == 131072 and R.lds_bytes(R.S128) == 2 * 256 * 128 == 65536
    assert R.lds_bytes(R.H256) == 4 * 128 * 128 + 2 * 328 * 128 + 1024 == 150528
    assert R.resident_cap(R.P128) == 256 and R.resident_cap(R.S128) == 512 and R.resident_cap(R.H256) == 256
    # dispatch_bnf (GEMM terms).  The launches test_conv_gpu.py's decline test expects to be declined:
    assert R.dispatch_bnf(1024, 16, 16, 128, 128, 3) is None                       # 2 048 row tiles: not resident
    assert R.dispatch_bnf(1, 16, 16, 128, 128, 1) is None                          # 4 workgroups: fewer than the barrier's 8 shards
    assert R.dispatch_bnf(8, 32, 32, 64, 64, 3) is None                            # 64 written channels
    # the training step's launches (ResNet-18 at 256 images): 16 x 16 -> 256-row tiles, 8 x 8 -> 256 x 64, 4 x 4 -> 128 x 64
    assert R.dispatch_bnf(256, 16, 16, 128, 128, 3) == R.H256                      # 512 workgroups of 128 rows -> 256 of 256
    assert R.dispatch_bnf(256, 8, 8, 256, 256, 3) == R.N256                        # 256 of 128 x 128 -> 256 of 256 x 64
    assert R.dispatch_bnf(256, 4, 4, 512, 512, 3) == R.N128                        # 256 of 64 x 128 -> 256 of 128 x 64
    assert R.dispatch_bnf(8, 8, 8, 128, 128, 3) == R.T64H and R.dispatch_bnf(8, 8, 8, 128, 128, 1) == R.T64     # 16 of 64 x 64
    assert R.dispatch_bnf(8, 8, 8, 64, 128, 1) == R.P64                            # 64 reduction channels: not the 64 x 64 rule
    assert R.dispatch_bnf(65, 16, 16, 128, 256, 1) == R.S128                       # 260: the four-stage form holds 256
    assert R.dispatch_bnf(8, 8, 8, 256, 128, 3, bsc=True) == R.T64H and R.dispatch_bnf(8, 8, 8, 256, 128, 1, bsc=True) is None
    assert R.dispatch_bnf(8, 8, 8, 256, 128, 3, n_classes=4) == R.P64              # the pair form: per-tap tiles, 32 workgroups
    assert R.dispatch_bnf(8, 8, 8, 64, 128, 3, n_classes=2, multi=True) == R.P64   # two-problem forward: 8 workgroups meet


@pytest.mark.parametrize("backward", [False, True])
def test_tables_reach_the_forms_they_name(backward):
    cases = R.BWD_CASES if backward else R.FWD_CASES
    for c in cases:
        ci, co = R.gemm_dims(c, backward)
        assert R.dispatch_bnf(c.n, c.h, c.h, ci, co, c.k, c.d) == c.form, c.tag
        bm, bn = c.form[0], c.form[1]
        meet = -(-co // bn) * -(-(c.n * c.h * c.h) // bm)
        assert 8 <= meet <= 0.8 * R.resident_cap(c.form), (c.tag, meet)            # the barrier's minimum; at most four fifths of the residency cap
    names = {R.kernel_name("dgrad" if backward else "fwd", c.form) for c in cases}
    want = {k for k in R.FUSED_ALLOWLIST if k.startswith("igemm_dgrad" if backward else "igemm_fwd") and k.endswith("bf1>")}
    assert names == want, (sorted(names - want), sorted(want - names))
    # every instantiation has a case whose written channels span more than one column tile
    for f in {c.form for c in cases}:
        assert any(R.gemm_dims(c, backward)[1] > f[1] for c in cases if c.form == f), f


def test_other_tables_reach_the_forms_they_name():
    for tag, n, ci, co, h, form in R.MULTI_FWD_CASES:
        assert R.dispatch_bnf(n, h // 2, h // 2, ci, co, 3, n_classes=2, multi=True) == form, tag
    for tag, n, ci, co, h, form in R.PAIR_BWD_CASES:
        assert R.dispatch_bnf(n, h // 2, h // 2, co, ci, 3, n_classes=4) == form, tag
    got = set()
    for c in R.GROUPED_CASES:
        f, gs = R.dispatch_grouped_dgrad(c.n, c.h, c.h, c.co, c.ci, c.k)
        assert f == c.form and gs == 1, c.tag                                      # the straddling tile walks twice
        got.add(R.kernel_name("dgrad", f, gs=1, bf=0))
    assert got == {k for k in R.FUSED_ALLOWLIST if ",gs1," in k}
    assert set(R.WGRAD_MULTI_CASES) == {k for k in R.FUSED_ALLOWLIST if k.startswith("wgrad_multi")}
    for name, items in R.WGRAD_MULTI_CASES.items():
        bm, bn, inc = (int(v) for v in name[len("wgrad_multi<"):-1].replace("inc", "").split(","))
        for (n, ci, co, h, k, s, d) in items:
            assert (128 if co % 128 == 0 else 64) == bm and (128 if ci % 128 == 0 else 64) == bn and int(64 % h == 0) == inc, (name, ci, co, h)


def test_allowlist_names_tests_that_exist():
    """FUSED_ALLOWLIST's values are tests of the pinned module, each parametrised over the table that reaches its keys."""
    import test_conv_fused_pinned_gpu as G
    for key, where in R.FUSED_ALLOWLIST.items():
        mod, name = where.split("::")
        assert mod == "tests/test_conv_fused_pinned_gpu.py" and callable(getattr(G, name, None)), (key, where)
