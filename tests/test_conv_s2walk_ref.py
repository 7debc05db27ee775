"""The CPU side of the walk kernel's tests (csrc/afan_conv_s2walk.hip): the float64 restatement in conv_s2walk_refs.py agrees with
autograd's transposed convolutions, and the order-visible operands of test_conv_s2walk_gpu.py do what they are there for — an fp32
accumulator that takes the same partial products in another order rounds to other bf16 values."""
import torch

import conv_s2walk_refs as R


def _as_conv_weights(wt10):
    """wt10 [ci][10][co] -> the 3x3 weights [co, ci, 3, 3] and the projection's [co, ci, 1, 1]"""
    ci, _, co = wt10.shape
    return wt10[:, :9].permute(2, 0, 1).reshape(co, ci, 3, 3).double(), wt10[:, 9].t().reshape(co, ci, 1, 1).double()


def test_restatement_is_the_two_transposed_convolutions():
    for n, hi, wi, ci, co in [(2, 4, 4, 64, 64), (1, 2, 2, 64, 64), (2, 8, 4, 64, 128), (3, 6, 6, 64, 128)]:
        _, dy, sc, w = next(R.operand_cases(n, hi, wi, ci, co, 11))
        w3, w1 = _as_conv_weights(w)
        sh = (n, ci, hi, wi)
        want = torch.nn.grad.conv2d_input(sh, w3, dy.double().permute(0, 3, 1, 2), 2, 1) + \
            torch.nn.grad.conv2d_input(sh, w1, sc.double().permute(0, 3, 1, 2), 2, 0)
        got = R.restate(dy, sc, w).permute(0, 3, 1, 2)
        assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max()), (n, hi, wi, ci, co)


def test_slot_table():
    assert [R.class_slots(ph, pw) for ph in range(2) for pw in range(2)] == [[4, 9], [3, 5], [1, 7], [0, 2, 6, 8]]
    assert [R.slot_class(s)[2:] for s in range(10)] == [(1, 1), (1, 0), (1, 0), (0, 1), (0, 0), (0, 0), (0, 1), (0, 0), (0, 0), (0, 0)]


def test_order_visible_operands_show_the_order():
    g = torch.Generator().manual_seed(5)
    dy, sc, w = R.order_visible(2, 4, 4, 64, g)
    assert set(torch.log2(dy.double().abs()).floor().flatten().tolist()) >= {8.0} and float(dy.abs().min()) < 2.0 ** -8
    kernel = R.restate(dy, sc, w, R.kernel_order, fp32=True)
    assert torch.equal(kernel, R.restate(dy, sc, w, R.kernel_order, fp32=True))
    for other in (R.tap_outer_order, R.reversed_order):
        got = R.restate(dy, sc, w, other, fp32=True)
        changed = int((got.view(torch.int16) != kernel.view(torch.int16)).sum())
        print(f"S2WALK order-visible operands: {other.__name__} changes {changed} of {kernel.numel()} bf16 results")
        assert changed > kernel.numel() // 100, other.__name__
    # and the plain random operands would NOT have shown it: that is why the case exists
    _, dy, sc, w = next(R.operand_cases(2, 8, 8, 64, 128, 11))
    a, b = R.restate(dy, sc, w, R.kernel_order, fp32=True), R.restate(dy, sc, w, R.reversed_order, fp32=True)
    assert int((a.view(torch.int16) != b.view(torch.int16)).sum()) < a.numel() // 100
