"""The PGD loop that carries sign codes instead of an fp32 iterate (csrc/afan_pgd_packed.hip: afan_pgd_packed_step / afan_pgd_packed_last)
against the launches it replaces, BIT FOR BIT (update_pinned_refs.same_f32 / same_bf16: any NaN equals any NaN, the one permitted
difference being a NaN's payload):

  * entry level: after every step the bf16 shadow, and after the last step x_adv, x32, l2 and linf, equal the existing chain on the
    same inputs on the GPU (ops.pgd_init, ops.pgd_step_ x (K - 1), ops.pgd_step_norms_) and the numpy reference
    (tests/pgd_packed_refs.py; l2, which numpy holds in float64, lies in test_update_pinned_gpu.l2_window of it).  Shapes: 630
    elements with 315 per sample (ragged for every vector width, the scalar norms path); per-sample 5184 (crosses a 4096 slice on the
    vector path); 128 elements; and the second once more through views 2 bytes (codes: 1 byte, fp32: 4 bytes) off alignment, which
    forces the scalar bodies.  bf16 and fp32 gradients seeded with zero, -0.0, NaN and +-inf, starts with -0.0, 1e-30, 3e4 and 1e6;
    gamma = 0.5/255, eps = 2/255, clip off and on, K = 1..5.
  * argument errors return their codes and write nothing.
  * attack_algo.PGD on a ResNet-18 tail (batch 16, K = 2 and 5, with and without grad0): switch on against switch off, torch.equal
    on x_adv, its shadow and the norms; ops.CALLS["pgd_packed"] tells the route; randinit, norm="l2", steps=6 and an fp32 model take
    the old route.
  * one AfanTrainer step, eager and graph-replayed, switch on against off (the pattern of tests/test_tail_end_gpu.py).
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import pgd_packed_refs as P
import update_pinned_refs as R
from test_update_pinned_gpu import l2_window

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
CL = torch.channels_last

SHAPES = {"ragged630": ((2, 5, 7, 9), 0), "slice5184": ((3, 64, 9, 9), 0), "tiny128": ((1, 8, 4, 4), 0), "offset5184": ((3, 64, 9, 9), 1)}


def _dev(a, dt, shape, off, gpu):
    """A numpy array of `dt`-sized patterns as a contiguous device tensor of `shape`, `off` elements into a larger allocation."""
    t = torch.empty(a.size + 16, dtype=dt, device=gpu)
    v = t[off:off + a.size].view(shape)
    raw = {BF16: torch.int16, torch.uint8: torch.uint8, torch.float32: torch.float32}[dt]
    v.view(raw).copy_(torch.from_numpy(np.ascontiguousarray(a).view({BF16: np.int16, torch.uint8: np.uint8, torch.float32: np.float32}[dt])
                                       .reshape(shape)))
    return v


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).ravel()


def _f32(t):
    return t.detach().contiguous().cpu().numpy().ravel()


@pytest.mark.parametrize("steps", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("gdt", [BF16, torch.float32], ids=["gbf16", "gf32"])
@pytest.mark.parametrize("shape_id", list(SHAPES))
def test_packed_steps_equal_the_chain_they_replace(pkg, gpu, shape_id, gdt, clip, steps):
    ops = pkg.ops
    shape, off = SHAPES[shape_id]
    batch, n = shape[0], int(np.prod(shape))
    per = n // batch
    x0_bits, grads = P.inputs(n, steps, seed=17 * steps + len(shape_id))
    want = P.chain(x0_bits, grads, P.GAMMA, P.EPS, clip)
    x0 = _dev(x0_bits, BF16, shape, off, gpu)
    assert (x0.data_ptr() % 16 == 0) == (off == 0)
    g_dev = [_dev(R.bf16_bits(g), BF16, shape, off, gpu) if gdt == BF16 else _dev(g, torch.float32, shape, off, gpu) for g in grads]
    codes = _dev(np.full(n, 0xA5, np.uint8), torch.uint8, shape, off, gpu)          # stale bytes: step 0 must overwrite all of them
    shadow = _dev(np.zeros(n, np.uint16), BF16, shape, off, gpu)
    # the chain the packed launches replace, on the same inputs
    x32_r, xa_r, sh_r = ops.pgd_init(x0, want_shadow=True)
    assert R.same_bf16(_bits(sh_r), x0_bits) is None
    ref_codes = None
    for t in range(steps - 1):
        ops.pgd_step_(xa_r, g_dev[t], float(P.GAMMA), x32_r, float(P.EPS), clip, sh_r)
        ops.pgd_packed_step_(x0, g_dev[t], codes, t, float(P.GAMMA), float(P.EPS), clip, shadow)
        ref_codes, ref_shadow, _ = P.packed_step(x0_bits, grads[t], ref_codes, t, P.GAMMA, P.EPS, clip)
        assert R.same_bf16(_bits(shadow), _bits(sh_r)) is None, f"shadow after step {t} against afan_pgd_step"
        assert R.same_bf16(_bits(shadow), ref_shadow) is None, f"shadow after step {t} against numpy"
        assert R.same_f32(_f32(xa_r), want[t]) is None, f"afan_pgd_step's iterate after step {t} against numpy"
        assert np.array_equal(codes.cpu().numpy().ravel(), ref_codes), f"code bytes after step {t}"
    t = steps - 1
    l2_r, linf_r = ops.pgd_step_norms_(xa_r, g_dev[t], float(P.GAMMA), x32_r, float(P.EPS), clip, sh_r)
    x_adv, x32, l2, linf = ops.pgd_packed_last(x0, g_dev[t], codes if t else None, t, float(P.GAMMA), float(P.EPS), clip, shadow)
    torch.cuda.synchronize()
    assert x_adv.dtype == torch.float32 and x_adv.shape == x0.shape and x32.shape == x0.shape
    for name, got, ref in (("x_adv", x_adv, xa_r), ("x32", x32, x32_r), ("l2", l2, l2_r), ("linf", linf, linf_r)):
        bad = R.same_f32(_f32(got), _f32(ref))
        assert bad is None, f"{name}[{bad}] = {_f32(got)[bad]!r} against the chain's {_f32(ref)[bad]!r}"
    assert R.same_bf16(_bits(shadow), _bits(sh_r)) is None, "shadow after the last step against afan_pgd_step_norms"
    # numpy
    assert R.same_f32(_f32(x_adv), want[t]) is None, "x_adv against numpy"
    assert R.same_f32(_f32(x32), R.bf16_widen(x0_bits)) is None, "x32 against the widened start"
    assert R.same_bf16(_bits(shadow), R.bf16_bits(want[t])) is None, "shadow against numpy"
    with np.errstate(invalid="ignore", over="ignore"):
        linf_n, l2_n, ss_n = R.perturb_norms(want[t].reshape(batch, per), R.bf16_widen(x0_bits).reshape(batch, per))
    assert R.same_f32(_f32(linf), linf_n) is None, "linf against numpy"
    got2 = _f32(l2).astype(np.float64)
    assert np.array_equal(np.isnan(got2), np.isnan(l2_n)), "l2 is NaN exactly for the samples with a NaN gradient"
    assert np.isnan(l2_n).any() and not np.isnan(l2_n).all() or batch == 1
    with np.errstate(invalid="ignore"):
        out = ~np.isnan(l2_n) & ~(np.abs(got2 - l2_n) <= l2_window(per, l2_n, ss_n))
    assert not out.any(), f"l2 outside its window of the float64 norm for samples {np.flatnonzero(out).tolist()}"
    # without the norms and the optional outputs: the same x_adv
    x_adv2, none32, no_l2, no_linf = ops.pgd_packed_last(x0, g_dev[t], codes if t else None, t, float(P.GAMMA), float(P.EPS), clip, None,
                                                         want_x32=False, norms=False)
    assert none32 is None and no_l2 is None and no_linf is None
    assert R.same_f32(_f32(x_adv2), _f32(x_adv)) is None


def test_argument_errors_launch_nothing(pkg, gpu):
    lib = pkg._lib.load()
    n = 64
    sent = lambda dt, v: torch.full((n,), v, dtype=dt, device=gpu)
    x0, g, sh = sent(BF16, 1.0), sent(BF16, 1.0), sent(BF16, 7.0)
    codes, xa, x32, ws, l2, linf = sent(torch.uint8, 0xA5), sent(torch.float32, 7.0), sent(torch.float32, 7.0), sent(torch.float32, 7.0), \
        sent(torch.float32, 7.0), sent(torch.float32, 7.0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    step = lambda x=x0, gr=g, dt=1, c=codes, t=0, nn_=n, s=sh: lib.afan_pgd_packed_step(p(x) if x is not None else None,
        p(gr) if gr is not None else None, dt, p(c) if c is not None else None, t, nn_, 0.1, 0.1, 0, p(s) if s is not None else None, st)
    last = lambda x=x0, gr=g, dt=1, c=codes, t=1, b=2, per=32, a=xa, l=l2, li=linf, w=ws: lib.afan_pgd_packed_last(
        p(x) if x is not None else None, p(gr) if gr is not None else None, dt, p(c) if c is not None else None, t, b, per, 0.1, 0.1, 0,
        p(x32), p(a) if a is not None else None, p(sh), p(w) if w is not None else None, p(l) if l is not None else None,
        p(li) if li is not None else None, st)
    E = R
    assert step(t=4) == E.AFAN_ESHAPE and step(t=-1) == E.AFAN_ESHAPE and step(nn_=-1) == E.AFAN_ESHAPE
    assert step(x=None) == E.AFAN_ENULL and step(c=None) == E.AFAN_ENULL and step(gr=None) == E.AFAN_ENULL and step(s=None) == E.AFAN_ENULL
    assert step(dt=7) == E.AFAN_EDTYPE
    assert step(nn_=0) == E.AFAN_OK
    assert last(t=5) == E.AFAN_ESHAPE and last(t=-1) == E.AFAN_ESHAPE and last(b=65536) == E.AFAN_ESHAPE and last(b=-1) == E.AFAN_ESHAPE
    assert last(per=0) == E.AFAN_ESHAPE
    assert last(x=None) == E.AFAN_ENULL and last(c=None) == E.AFAN_ENULL and last(a=None) == E.AFAN_ENULL and last(gr=None) == E.AFAN_ENULL
    assert last(li=None) == E.AFAN_ENULL and last(w=None) == E.AFAN_ENULL
    assert last(dt=7) == E.AFAN_EDTYPE
    assert last(b=0) == E.AFAN_OK
    torch.cuda.synchronize()
    assert bool((codes == 0xA5).all()) and all(bool((t == 7.0).all()) for t in (sh, xa, x32, ws, l2, linf)), "a refused call wrote something"
    # and the calls these were one argument away from do run
    assert step() == 0 and last() == 0
    torch.cuda.synchronize()
    assert bool((xa != 7.0).all()) and bool((codes != 0xA5).all())


# ---- attack_algo.PGD: the switch on against off ---------------------------------------------------------------------------------------
def _tail_problem(pkg, gpu, dtype=BF16):
    """A freshly built, seeded ResNet-18 (every run starts from the same state, as tests/test_tail_end_gpu.py::_one_step does: a model
    that has already run carries its earlier passes with it), its feature map at block 6 and the gradient there."""
    torch.manual_seed(7)
    model = pkg.resnet_s.resnet18()
    model.set_compute_dtype(dtype).set_channels_last(dtype == BF16).to(gpu).train()
    gen = torch.Generator().manual_seed(8)
    x, y = torch.rand(16, 3, 32, 32, generator=gen).to(gpu), torch.randint(0, 10, (16,), generator=gen).to(gpu)
    pkg.ops.acc_reset(gpu)
    with torch.no_grad():
        fm = model(x, end_point=6, start_point=0)
    xin = fm.detach().requires_grad_(True)
    g0 = pkg.pgd.input_gradient(lambda t: nn.CrossEntropyLoss()(model(t, end_point=model.layer_number, start_point=6).float(), y), xin)
    return model, fm.detach(), y, g0.detach()


def _pgd(pkg, gpu, monkeypatch, packed, steps, with_g0, dtype=BF16, as_float=False, **kw):
    model, fm, y, g0 = _tail_problem(pkg, gpu, dtype)
    monkeypatch.setattr(pkg.attack_algo, "_PGD_PACKED", packed)
    n0 = pkg.ops.CALLS["pgd_packed"]
    adv = pkg.attack_algo.PGD(fm.float() if as_float else fm, nn.CrossEntropyLoss(), y=y, model=model, steps=steps, gamma=0.5 / 255, start_idx=6,
                              layer_number=model.layer_number, eps=2 / 255, clip=True, with_norms=True,
                              grad0=g0 if with_g0 else None, **kw)
    l2, linf = pkg.attack_algo.last_norms()
    torch.cuda.synchronize()
    adv._afan_x = fm
    return adv, l2.clone(), linf.clone(), pkg.ops.CALLS["pgd_packed"] - n0


@pytest.mark.parametrize("with_g0", [True, False], ids=["grad0", "nograd0"])
@pytest.mark.parametrize("steps", [2, 5])
def test_pgd_same_with_and_without_the_packed_route(pkg, gpu, monkeypatch, steps, with_g0):
    a, a_l2, a_linf, a_calls = _pgd(pkg, gpu, monkeypatch, False, steps, with_g0)
    a1 = _pgd(pkg, gpu, monkeypatch, False, steps, with_g0)[0]
    b, b_l2, b_linf, b_calls = _pgd(pkg, gpu, monkeypatch, True, steps, with_g0)
    assert a_calls == 0 and b_calls == steps, "which route ran"
    assert b.requires_grad and b.is_leaf and b.dtype == torch.float32 and b.stride() == a.stride()
    print(f"PGDPACKED PGD K={steps} grad0={with_g0}: elements of x_adv that differ, old route against itself "
          f"{int((a.detach() != a1.detach()).sum())}, against the packed route {int((a.detach() != b.detach()).sum())} of {a.numel()}; "
          f"shadow {int((a._afan_shadow != b._afan_shadow).sum())}, l2 {int((a_l2 != b_l2).sum())}, linf {int((a_linf != b_linf).sum())}")
    assert torch.equal(a.detach(), b.detach()), "x_adv"
    assert torch.equal(a._afan_shadow, b._afan_shadow), "shadow"
    assert torch.equal(a_l2, b_l2) and torch.equal(a_linf, b_linf), "norms"
    fm = b._afan_x
    assert fm.dtype == BF16 and torch.equal(fm, a._afan_x)
    assert torch.equal(b._afan_clean32, fm.float()) and not hasattr(a, "_afan_clean32")
    assert float((b.detach() - fm.float()).abs().max()) > 0


def test_what_the_packed_route_does_not_take(pkg, gpu, monkeypatch):
    torch.manual_seed(3)
    assert _pgd(pkg, gpu, monkeypatch, True, 2, False, randinit=True)[3] == 0
    assert _pgd(pkg, gpu, monkeypatch, True, 2, False, norm="l2")[3] == 0
    assert _pgd(pkg, gpu, monkeypatch, True, 6, False)[3] == 0
    assert _pgd(pkg, gpu, monkeypatch, True, 2, False, as_float=True)[3] == 0        # an fp32 map under the bf16 model
    assert _pgd(pkg, gpu, monkeypatch, True, 2, False, dtype=torch.float32)[3] == 0  # an fp32 model
    assert _pgd(pkg, gpu, monkeypatch, True, 2, False)[3] == 2


# ---- one trainer step, switch on / off ------------------------------------------------------------------------------------------------
def _one_step(pkg, gpu, graph, packed, monkeypatch):
    torch.manual_seed(7)
    model = pkg.resnet_s.resnet18()
    model.set_compute_dtype(BF16).set_channels_last(True).to(gpu).train()
    gen = torch.Generator().manual_seed(8)
    x, y = torch.rand(16, 3, 32, 32, generator=gen).to(gpu), torch.randint(0, 10, (16,), generator=gen).to(gpu)
    monkeypatch.setattr(pkg.attack_algo, "_PGD_PACKED", packed)
    tr = pkg.train_step.AfanTrainer(model, nn.CrossEntropyLoss(), steps=2, gamma=0.5, eps=2.0, perturb_idx=6, lr=0.1, use_graph=graph,
                                    graph_warmup=0)
    n0 = pkg.ops.CALLS["pgd_packed"]
    r = tr.step(x, y)
    torch.cuda.synchronize()
    assert (tr._graph is not None) == graph, getattr(tr, "_graph_failed", None)
    assert pkg.ops.CALLS["pgd_packed"] - n0 == (2 if packed else 0)         # one plain step and the last one
    assert not pkg.ops.grid_barrier_error(gpu)
    assert r["feature_map"].dtype == torch.float32 and r["x_adv"].dtype == torch.float32
    return {"loss_clean": r["loss_clean"].clone(), "loss_adv": r["loss_adv"].clone(), "x_adv": r["x_adv"].clone(),
            "feature_map": r["feature_map"].clone(), "l2": r["l2"].clone(), "linf": r["linf"].clone(),
            "params": tr.arena.param.detach().clone()}


def _maxdiff(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_trainer_step_same_with_and_without_the_packed_route(pkg, gpu, graph, monkeypatch):
    """ResNet-18, batch 16, 32 x 32, K = 2, bf16 channels-last.  The old route is run twice first: where it repeats bit for bit, every
    observable must be bit-equal between the routes; where it does not, the routes may differ by twice its own run-to-run difference."""
    a0 = _one_step(pkg, gpu, graph, False, monkeypatch)
    a1 = _one_step(pkg, gpu, graph, False, monkeypatch)
    b = _one_step(pkg, gpu, graph, True, monkeypatch)
    own = {k: _maxdiff(a0[k], a1[k]) for k in a0}
    got = {k: _maxdiff(a0[k], b[k]) for k in a0}
    print(f"PGDPACKED step {'graph' if graph else 'eager'}: off-vs-off {own}  off-vs-on {got}")
    for k in a0:
        if own[k] == 0.0:
            assert torch.equal(a0[k], b[k]), f"{k}: the old route repeats bit for bit, the routes differ by {got[k]:.3e}"
        else:
            assert got[k] <= 2.0 * own[k], f"{k}: {got[k]:.3e} between the routes > twice the old route's own {own[k]:.3e}"
