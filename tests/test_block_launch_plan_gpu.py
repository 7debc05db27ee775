"""The residual blocks' launch plan: which kernel instantiation serves which convolution problem, in order, and how many launches of
every kernel one eager training forward + backward through the block fast path (resnet_s._BlockFn) issues, for a small ResNet-18
and a small ResNet-50, against tests/golden/block_launch_plan.json.

Every in-launch BatchNorm form (convolution + train-mode BatchNorm + ReLU as one launch behind a grid barrier) has a two-launch
fallback with the same bits, so a form that silently stops being eligible passes every bit-equality test and only costs time.  The
plan pins the forms themselves: the `bf1` instantiations are the in-launch ones.

The fixture was recorded on an MI355X from the commit BEFORE the launch protocol (ops._grid_launch) and the typed hand-off records
(resnet_s._BlockTail / _GradNote) replaced the hand-written copies; `python tests/test_block_launch_plan_gpu.py` rewrites it from
the code as it stands — for a change that MEANS to alter the plan, never to make this test pass.

Sizes: ResNet-18 at batch 16 of 3x32x32 (identity blocks, projection blocks with the two-problem forward and the stride-2 pair
gradient), ResNet-50 at batch 4 of 3x64x64 (the 1x1 forms, the hand-off across identity and projection blocks).  All launches
are co-resident at these sizes, so the library declines none of the forms: test_fixture_holds_every_in_launch_form checks that on
the recorded file."""
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_launch_plan.json")
CASES = [("resnet18", 16, 32), ("resnet50", 4, 64)]            # (architecture, batch, image side)


def _name(case):
    return "%s_n%d_%d" % case


def launch_plan(pkg, dev, case):
    """{"trace": [[op, problem, kernel], ...] in launch order, "launches": {kernel name: count}} of one forward + backward."""
    arch, batch, side = case
    ops = pkg.ops
    torch.manual_seed(0)
    m = pkg.resnet_s.ARCHS[arch][0](num_classes=10)
    m.set_compute_dtype(torch.bfloat16).set_channels_last(True).to(dev).train()
    arena = pkg.arena.ParamArena(m)
    assert pkg.resnet_s._Flags.param_grads and pkg.resnet_s._Flags.block_fusion
    x = torch.rand(batch, 3, side, side).to(dev)
    arena.zero_grad()
    ops.acc_reset(dev)
    ops.profile_collect()                                       # (drops what an earlier scope may have left)
    ops.profile_enable(True)
    try:
        with ops.conv_trace() as tr:
            y = m(x)
            y.backward(torch.ones_like(y))
        torch.cuda.synchronize(dev)
        prof = ops.profile_collect(256)
    finally:
        ops.profile_enable(False)
    assert not ops.grid_barrier_error(dev)
    return {"trace": [[r["op"], list(r["problem"]), r["kernel"]] for r in tr.records],
            "launches": {k: prof[k]["launches"] for k in sorted(prof)}}


def _forms(trace):
    """Which in-launch (bf1) forms a trace holds: forward, stride-1 input gradient, stride-2 pair input gradient."""
    got = set()
    for op, problem, kernel in trace:
        if kernel.endswith("bf1>"):
            got.add(op if op == "fwd" else "dgrad_s%d" % problem[6])
    return got


def test_fixture_holds_every_in_launch_form():
    """(no GPU) The recorded plan is one in which the launcher declined none of the forms at these sizes."""
    with open(GOLDEN) as f:
        want = json.load(f)
    assert _forms(want[_name(CASES[0])]["trace"]) == {"fwd", "dgrad_s1", "dgrad_s2"}
    assert {"fwd", "dgrad_s1"} <= _forms(want[_name(CASES[1])]["trace"])
    assert any(k == 1 and kern.endswith("bf1>") for _, (*_, k, _, _), kern in want[_name(CASES[1])]["trace"])      # the 1x1 forms


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_name)
def test_block_launch_plan(pkg, gpu, case):
    if not pkg.ops.GRID_BN_ALLOWED:
        pytest.skip("the in-launch BatchNorm is switched off for this process")
    with open(GOLDEN) as f:
        want = json.load(f)[_name(case)]
    got = launch_plan(pkg, gpu, case)
    assert len(got["trace"]) == len(want["trace"])
    for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        assert g == w, "launch %d of the plan" % i
    assert got["launches"] == want["launches"]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import importlib
    pkg_ = importlib.import_module("cv_a-fan_amd")
    out = {_name(c): launch_plan(pkg_, torch.device("cuda:0"), c) for c in CASES}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    for c in CASES:
        print(_name(c), len(out[_name(c)]["trace"]), "trace records;", sorted(_forms(out[_name(c)]["trace"])))
