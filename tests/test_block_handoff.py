"""Host logic of the in-launch BatchNorm's wiring, on CPU tensors: the record a consumer block hangs on the gradient it hands back
(resnet_s._GradNote: attach / read, with the two loud refusals no GPU test reaches) and the launch protocol of the four in-launch
forms (ops._grid_launch) against a stand-in launcher."""
import gc
import weakref

import pytest
import torch


def _tail(pkg, done=0):
    t = pkg.resnet_s._BlockTail(None, None, 1, None, True, None)
    t.done = done
    return t


# ------------------------------------------------------------------------------------------------ the hand-off record
def test_done_form_on_an_untouched_tensor(pkg):
    rs = pkg.resnet_s
    g, d_raw, pair = torch.zeros(2, 4, 3, 3), torch.ones(2, 4, 3, 3), torch.ones(4, 4, 3, 3)
    tail = _tail(pkg, done=1)
    assert rs._GradNote.attach(g, d_raw=d_raw, pair=pair) is g
    sums, got_raw, got_pair = rs._GradNote.read(g, tail)
    assert sums is None and got_raw is d_raw and got_pair is pair
    assert tail.done == 0


def test_done_form_modified_on_its_way(pkg):
    rs = pkg.resnet_s
    g = torch.zeros(2, 4, 3, 3)
    tail = _tail(pkg, done=1)
    rs._GradNote.attach(g, d_raw=torch.ones(2, 4, 3, 3), pair=torch.ones(4, 4, 3, 3))
    g.add_(1)
    with pytest.raises(pkg.ops.AfanLibraryError, match="modified on its way"):
        rs._GradNote.read(g, tail)
    assert tail.done == 0


def test_done_but_a_different_tensor_delivered(pkg):
    rs = pkg.resnet_s
    g = torch.zeros(2, 4, 3, 3)
    tail = _tail(pkg, done=1)
    rs._GradNote.attach(g, d_raw=torch.ones(2, 4, 3, 3))
    other = g + 1                                      # what the engine makes of two contributions: a new tensor, no record
    with pytest.raises(pkg.ops.AfanLibraryError, match="delivered a different gradient tensor"):
        rs._GradNote.read(other, tail)
    assert tail.done == 0
    assert rs._GradNote.read(other, tail) == (None, None, None)          # (nothing handed over, nothing pending: the plain backward)


def test_sums_form_fresh_and_stale(pkg):
    rs = pkg.resnet_s
    g = torch.zeros(2, 4, 3, 3)
    sums = pkg.ops.ConvStats(None, 0, None, torch.zeros(8, dtype=torch.float64))
    tail = _tail(pkg)
    rs._GradNote.attach(g, sums=sums)
    assert rs._GradNote.read(g, tail) == (sums, None, None)
    g.mul_(2)                                          # the mark is stale: the sums are of other values
    assert rs._GradNote.read(g, tail) == (None, None, None)


@pytest.mark.parametrize("form", ["sums", "done"])
def test_record_does_not_hold_its_tensor(pkg, form):
    rs = pkg.resnet_s
    g = torch.zeros(2, 4, 3, 3)
    if form == "sums":
        rs._GradNote.attach(g, sums=pkg.ops.ConvStats(None, 0, None, torch.zeros(8, dtype=torch.float64)))
    else:
        rs._GradNote.attach(g, d_raw=torch.ones(2, 4, 3, 3), pair=torch.ones(4, 4, 3, 3))
    note = g._afan_note
    seen, todo = set(), [note]
    while todo:                                        # everything reachable from the record
        o = todo.pop()
        if id(o) in seen or isinstance(o, type):
            continue
        seen.add(id(o))
        assert o is not g
        todo += gc.get_referents(o)
    alive = weakref.ref(g)
    was = gc.isenabled()
    gc.disable()
    try:
        del g, o, todo
        assert alive() is None                         # freed by reference count alone
    finally:
        if was:
            gc.enable()


# ------------------------------------------------------------------------------------------------ the launch protocol
KEY = ("f", 2, 64, 8, 8, 128, 3, 1, None, False)


@pytest.fixture
def arena(pkg, monkeypatch):
    """ops' accumulator arena on a CPU buffer (the real one keys on a HIP stream), not at its start; an empty refused memo."""
    ops = pkg.ops
    a = ops._AccArena(torch.device("cpu"))
    a.off = 2 * ops.acc_block_doubles(64)
    monkeypatch.setattr(ops, "_acc_arena", lambda device: a)
    monkeypatch.setattr(ops, "_grid_refused", set())
    monkeypatch.setattr(ops, "BN_ACC", True)
    monkeypatch.setattr(ops, "_GRID_BN_CHECK", False)
    return a


def test_launch_protocol_when_the_launcher_refuses(pkg, arena):
    ops = pkg.ops
    seen = []

    def refuse(acc, acc2):
        seen.append((acc, acc2))
        return ops.AFAN_ESHAPE, ("never", "returned")

    off0, calls0 = arena.off, dict(ops.CALLS)
    assert ops._grid_launch(KEY, "stand_in", torch.device("cpu"), [64, 128], refuse, n_fwd=2) is None
    (acc, acc2), = seen
    # two different block sizes, taken in the stated order: giving them back in THAT order would leave the first one taken
    assert acc.numel() == ops.acc_block_doubles(64) != acc2.numel() == ops.acc_block_doubles(128)
    assert acc.data_ptr() == arena.buf.data_ptr() + 8 * off0 and acc2.data_ptr() == acc.data_ptr() + 8 * acc.numel()
    assert arena.off == off0
    assert KEY in ops._grid_refused
    assert ops._grid_launch(KEY, "stand_in", torch.device("cpu"), [64, 128], refuse, n_fwd=2) is None
    assert len(seen) == 1                              # remembered: the stand-in was not called again
    assert arena.off == off0 and dict(ops.CALLS) == calls0


def test_launch_protocol_when_the_launcher_succeeds(pkg, arena):
    ops = pkg.ops
    off0, calls0 = arena.off, dict(ops.CALLS)
    out = ops._grid_launch(KEY, "stand_in", torch.device("cpu"), [64, 128], lambda acc, acc2: (0, ("y", acc, acc2)), n_fwd=2, n_dgrad=1)
    assert out[0] == "y" and out[1].numel() == ops.acc_block_doubles(64) and out[2].numel() == ops.acc_block_doubles(128)
    assert arena.off == off0 + ops.acc_block_doubles(64) + ops.acc_block_doubles(128)
    want = dict(calls0, conv_fwd=calls0["conv_fwd"] + 2, conv_dgrad=calls0["conv_dgrad"] + 1, conv_bn_fused=calls0["conv_bn_fused"] + 1)
    assert dict(ops.CALLS) == want
    assert ops._grid_refused == set()


def test_launch_protocol_with_another_error_code(pkg, arena):
    ops = pkg.ops
    calls0 = dict(ops.CALLS)
    with pytest.raises(ops.AfanLibraryError, match="stand_in: AFAN_ENULL"):
        ops._grid_launch(KEY, "stand_in", torch.device("cpu"), [64], lambda acc: (-4, None))
    assert ops._grid_refused == set() and dict(ops.CALLS) == calls0
