"""afan_conv_dgrad_sc_nhwc_bf16 with the walk kernel (csrc/afan_conv_s2walk.hip; afan_conv_s2walk(1), the default) against the same
call with it switched off (the four-class launch of dgrad_impl, pinned to float64 by test_conv_pinned_gpu.py and
test_conv_fused_pinned_gpu.py): the two routes must agree BIT FOR BIT, on every operand case of conv_s2walk_refs.operand_cases, with dx
inside guard bands over a 0xFF and over a 0x00 prefill.  The C ABI is called directly.  One step-level test: a ResNet-18 trainer step,
switch on against switch off, eager and graph-replayed."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import conv_s2walk_refs as R

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
GUARD = 256          # elements on either side of dx

#        n  hi  wi   ci   co
SHAPES = [(2, 4, 4, 64, 64),        # one partial tile; the halo is the image border on every side
          (1, 2, 2, 64, 64),        # one lattice position per image: every shifted view is out of range
          (3, 6, 6, 64, 128),       # 27 positions: a tile that straddles images, ragged tail
          (2, 8, 4, 64, 128),       # Hg != Wg ...
          (2, 4, 8, 64, 128),       # ... and the other way round: swapped row / column shifts
          (5, 16, 16, 128, 192),    # several row tiles, the last one straddling an image boundary; two ci tiles; three co chunks
          (2, 32, 32, 64, 128)]     # the benchmark's spatial shape and channels


def _switch(pkg, on):
    return pkg._lib.load().afan_conv_s2walk(int(on))


def _call(pkg, pair, n, wt10, dxbuf, hi, wi, ci, co, bn_x=None):
    dy, sc = pair[:n], pair[n:]
    dx = dxbuf[GUARD:GUARD + n * hi * wi * ci]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    return pkg._lib.load().afan_conv_dgrad_sc_nhwc_bf16(p(dy), p(sc), p(wt10), p(dx), n, hi, wi, ci, co, p(bn_x), None, 0, None, None, None,
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _run(pkg, gpu, on, pair, n, wt10, hi, wi, ci, co, fill, bn_x=None, walk=True):
    """-> (return code, dx as int16 [numel]); the guard bands are checked here"""
    numel = n * hi * wi * ci
    buf = torch.full((GUARD + numel + GUARD,), fill, dtype=torch.int16, device=gpu)
    old = _switch(pkg, on)
    try:
        with pkg.ops.conv_trace() as tr:
            code = _call(pkg, pair, n, wt10, buf, hi, wi, ci, co, bn_x)
        torch.cuda.synchronize()
    finally:
        _switch(pkg, old)
    # which route ran: dgrad_impl's launches are on the convolution trace, the walk kernel's are not
    assert (len(tr.records) == 0) == bool(on and walk), f"switch {on}: launches on the trace {[r['kernel'] for r in tr.records]}"
    assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + numel:] == fill).all()), f"guard bands written (switch {on}, fill {fill})"
    return code, buf[GUARD:GUARD + numel].clone()


def _pair(dy, sc, gpu):
    return torch.cat([dy, sc], dim=0).contiguous().to(gpu)      # ONE allocation, dy_sc behind dy


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_walk_equals_the_four_class_launch(pkg, gpu, shape):
    n, hi, wi, ci, co = shape
    assert _switch(pkg, 1) == 1, "the walk kernel is the default"
    for name, dy, sc, w in R.operand_cases(n, hi, wi, ci, co, seed=hi * 131 + ci + co):
        pair, wt10 = _pair(dy, sc, gpu), w.to(gpu)
        res = {}
        for on in (0, 1):
            for fill in (-1, 0):
                code, dx = _run(pkg, gpu, on, pair, n, wt10, hi, wi, ci, co, fill)
                assert code == 0, (name, on, fill, code)
                res[on, fill] = dx
        what = f"{shape} {name}"
        assert torch.equal(res[0, -1], res[0, 0]), what + ": the old route depends on what dx held"
        assert torch.equal(res[1, -1], res[1, 0]), what + ": the walk kernel depends on what dx held (elements not written?)"
        assert torch.equal(res[1, 0], res[0, 0]), what + f": {int((res[1, 0] != res[0, 0]).sum())} of {res[0, 0].numel()} elements differ"
        if name == "random":
            assert bool((res[1, 0] != 0).any()), what


@pytest.mark.parametrize("case", ["hi5", "ci96", "bn_x"])
def test_ineligible_calls_fall_through(pkg, gpu, case):
    """switch on: a call the walk kernel does not take returns the old route's code and result"""
    n, hi, wi, ci, co = {"hi5": (2, 5, 4, 64, 64), "ci96": (2, 4, 4, 96, 64), "bn_x": (2, 4, 4, 64, 64)}[case]
    ho, wo = (hi + 1) // 2, (wi + 1) // 2
    g = torch.Generator().manual_seed(17)
    pair = torch.randn(2 * n, ho, wo, co, generator=g).to(BF16).to(gpu)
    wt10 = (torch.randn(ci, 10, co, generator=g) * 0.125).to(BF16).to(gpu)
    bn_x = torch.randn(n, hi, wi, ci, generator=g).to(BF16).to(gpu) if case == "bn_x" else None
    c0, d0 = _run(pkg, gpu, 0, pair, n, wt10, hi, wi, ci, co, -1, bn_x, walk=False)
    c1, d1 = _run(pkg, gpu, 1, pair, n, wt10, hi, wi, ci, co, -1, bn_x, walk=False)
    assert c0 == c1 == 0 and torch.equal(d0, d1)


# ---- one trainer step, switch on / off ------------------------------------------------------------------------------------------------
def _one_step(pkg, gpu, graph, on):
    torch.manual_seed(7)
    model = pkg.resnet_s.resnet18()
    model.set_compute_dtype(BF16).set_channels_last(True).to(gpu).train()
    gen = torch.Generator().manual_seed(8)
    x, y = torch.rand(4, 3, 32, 32, generator=gen).to(gpu), torch.randint(0, 10, (4,), generator=gen).to(gpu)
    old = _switch(pkg, on)
    try:
        tr = pkg.train_step.AfanTrainer(model, nn.CrossEntropyLoss(), steps=2, gamma=0.5, eps=2.0, perturb_idx=6, lr=0.1, use_graph=graph,
                                        graph_warmup=0)
        r = tr.step(x, y)
        torch.cuda.synchronize()
    finally:
        _switch(pkg, old)
    assert (tr._graph is not None) == graph, getattr(tr, "_graph_failed", None)
    assert not pkg.ops.grid_barrier_error(gpu)
    out = {k: v.clone() for k, v in r.items() if torch.is_tensor(v)}
    out["params"] = tr.arena.param.detach().clone()
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_trainer_step_same_with_and_without_the_walk(pkg, gpu, graph):
    """ResNet-18, batch 4, 32 x 32, K = 2, bf16 channels-last: every returned tensor and the parameters, bit for bit."""
    a, b = _one_step(pkg, gpu, graph, 0), _one_step(pkg, gpu, graph, 1)
    assert set(a) == set(b) and "params" in a and len(a) > 1
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: max difference {float((a[k].double() - b[k].double()).abs().max()):.3e}"
