"""afan_batch_crop_flip_u8's host-side argument checks (no GPU is touched: every call returns before a launch) and its wrapper."""
import ctypes


def _args(lib):
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return lib.afan_batch_crop_flip_u8, p


def test_argument_errors_without_gpu(pkg):
    f, p = _args(pkg._lib.load())
    ESHAPE, ENULL = -3, -4
    ok = dict(src=p, ls=p, n=5, idx=p, top=p, left=p, flip=p, out=p, lo=p, m=2, c=3, h=4, w=4, pad=1)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["src"], a["ls"], a["n"], a["idx"], a["top"], a["left"], a["flip"], a["out"], a["lo"], a["m"], a["c"], a["h"], a["w"],
                 a["pad"], None)
    for name in ("m", "c", "h", "w", "pad", "n"):
        assert call(**{name: -1}) == ESHAPE, name
    for name in ("src", "idx", "out"):
        assert call(**{name: None}) == ENULL, name
    assert call(ls=None) == ENULL and call(lo=None) == ENULL              # exactly one label pointer
    for sub in (("top",), ("left",), ("flip",), ("top", "left"), ("top", "flip"), ("left", "flip")):
        assert call(**{k: None for k in sub}) == ENULL, sub               # a proper subset of the augmentation pointers
    assert call(n=0) == ESHAPE                                            # nothing to gather from


def test_empty_batch_returns_zero_without_a_launch(pkg):
    f, p = _args(pkg._lib.load())
    assert f(p, p, 5, p, p, p, p, p, p, 0, 3, 4, 4, 1, None) == 0
    assert f(None, None, 0, None, None, None, None, None, None, 0, 3, 32, 32, 4, None) == 0
    assert f(None, p, 0, None, None, None, None, None, None, 0, 3, 32, 32, 4, None) == -4     # argument errors come first


def test_wrapper_exists_and_counts(pkg):
    assert callable(pkg.ops.batch_crop_flip)
    assert pkg.ops.CALLS["batch_crop_flip"] >= 0
    import torch
    import pytest
    with pytest.raises(pkg.AfanLibraryError):                             # no CPU path
        pkg.ops.batch_crop_flip(torch.zeros(1, 1, 4, 4, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64))
