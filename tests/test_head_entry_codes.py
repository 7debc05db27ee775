"""The return code of every classifier-head and loss entry (csrc/afan_head.hip) for calls that end before anything is launched: a
literal table of (entry, arguments) -> code, recorded from the library as of commit 1d575e7, the last one before the head kernels were
reshaped around shared arithmetic, and never regenerated from a later build.  It pins which of AFAN_EDTYPE / AFAN_ESHAPE / AFAN_ENULL /
AFAN_EALIGN wins where several apply, and the value of afan_head_max_classes().  In the manner of tests/test_bn_entry_codes.py.

Every row is one entry's BASE call (bf16, n = 2, c = 64, hw = 16, k = 10: a problem the vector mapping takes) with a few arguments
replaced.  All pointers are host addresses that the library never dereferences, so no GPU is needed.

Rows left out, because the call would go on to a launch:
  * every base call itself, with and without its optional operands (bias; afan_head_ce's acc; afan_head_backward's dbias, and one of
    dx / dweight);
  * afan_head_forward with a misaligned x, with c outside the vector mapping or with hw > 64 (the scalar kernel takes them), and
    afan_head_backward with any such c or hw;
  * the largest problems taken: k = 16, hw = 64 and n * k = 65 536 for afan_head_ce and afan_cross_entropy, n = 65 536 for
    afan_loss_mean, c / 8 = 256 for afan_head_ce;
  * afan_head_ce with acc at + 8 bytes (aligned enough), and with stats / weight / the fp32 outputs at + 2 bytes (not looked at)."""
import ctypes

OK, EDTYPE, EALIGN, ESHAPE, ENULL = 0, -1, -2, -3, -4
F32, BF16 = 0, 1
MAX_CLASSES = 16

# pointer tokens
P = "P"            # aligned to 64 bytes
ODD = "ODD"        # P + 2: a bf16 element boundary, not 16 bytes
ODD4 = "ODD4"      # P + 4: an fp32 element boundary, no fp64 one

_FLOATS = {"root"}

# entry -> (argument names, base call); the C symbol is afan_<entry>
ENTRIES = {
    "head_forward": ("x dtype n c hw weight bias k pooled logits stream", (P, BF16, 2, 64, 16, P, P, 10, P, P, None)),
    "head_backward": ("dlogits weight pooled n c hw k dx dx_dtype dweight dbias accumulate stream",
                      (P, P, P, 2, 64, 16, 10, P, BF16, P, P, 0, None)),
    "cross_entropy": ("logits target n k loss dlogits stream", (P, P, 2, 10, P, P, None)),
    "head_ce": ("out raw dtype n c hw stats weight bias k target root pooled logits loss_row dlogits v acc stream",
                (P, P, BF16, 2, 64, 16, P, P, P, 10, P, 1.0, P, P, P, P, P, P, None)),
    "loss_mean": ("loss_row n loss stream", (P, 2, P, None)),
}

NO_LAUNCH = dict(dx=None, dweight=None)            # afan_head_backward asked for nothing


def _r(entry, code, *overrides, **more):
    args = {}
    for o in overrides:
        args.update(o)
    args.update(more)
    return entry, args, code


ROWS = [
    # ---- afan_head_forward ----
    _r("head_forward", EDTYPE, dtype=7), _r("head_forward", EDTYPE, dtype=-1), _r("head_forward", EDTYPE, dtype=2),
    *[_r("head_forward", ESHAPE, **{a: v}) for a in ("n", "c", "hw", "k") for v in (0, -1)],
    _r("head_forward", ESHAPE, k=17), _r("head_forward", ESHAPE, dtype=F32, k=17),
    *[_r("head_forward", ENULL, **{a: None}) for a in ("x", "weight", "pooled", "logits")],
    _r("head_forward", ENULL, dtype=F32, x=None),
    _r("head_forward", EDTYPE, dtype=7, n=0), _r("head_forward", EDTYPE, dtype=7, x=None), _r("head_forward", ESHAPE, k=17, x=None),
    _r("head_forward", ESHAPE, hw=0, logits=None), _r("head_forward", ENULL, x=ODD, weight=None), _r("head_forward", ENULL, c=12, pooled=None),
    # ---- afan_head_backward ----
    _r("head_backward", EDTYPE, dx_dtype=7), _r("head_backward", EDTYPE, dx_dtype=-1), _r("head_backward", EDTYPE, dx_dtype=7, dweight=None),
    *[_r("head_backward", ESHAPE, **{a: v}) for a in ("n", "c", "hw", "k") for v in (0, -1)],
    _r("head_backward", ESHAPE, k=17), _r("head_backward", ESHAPE, NO_LAUNCH, k=17),
    *[_r("head_backward", ENULL, **{a: None}) for a in ("dlogits", "weight", "pooled")],
    *[_r("head_backward", ENULL, NO_LAUNCH, **{a: None}) for a in ("dlogits", "weight", "pooled")],
    _r("head_backward", OK, NO_LAUNCH), _r("head_backward", OK, NO_LAUNCH, dx_dtype=7), _r("head_backward", OK, NO_LAUNCH, dbias=None),
    _r("head_backward", OK, NO_LAUNCH, accumulate=1),      # (dbias without dweight: nothing written)
    _r("head_backward", EDTYPE, dx_dtype=7, n=0), _r("head_backward", EDTYPE, dx_dtype=7, dlogits=None),
    _r("head_backward", ESHAPE, dx=None, dx_dtype=7, n=0), _r("head_backward", ENULL, dx=None, dx_dtype=7, weight=None),
    _r("head_backward", ESHAPE, n=0, dlogits=None), _r("head_backward", ESHAPE, k=17, pooled=None),
    # ---- afan_cross_entropy ----
    *[_r("cross_entropy", ESHAPE, **{a: v}) for a in ("n", "k") for v in (0, -1)],
    _r("cross_entropy", ESHAPE, n=65537, k=1), _r("cross_entropy", ESHAPE, n=1, k=65537), _r("cross_entropy", ESHAPE, n=1025, k=64),
    _r("cross_entropy", ESHAPE, n=4097, k=16), _r("cross_entropy", ESHAPE, n=-1, k=-1),
    *[_r("cross_entropy", ENULL, **{a: None}) for a in ("logits", "target", "loss", "dlogits")],
    _r("cross_entropy", ENULL, k=64, target=None), _r("cross_entropy", ENULL, n=65536, k=1, loss=None),
    _r("cross_entropy", ESHAPE, n=0, logits=None), _r("cross_entropy", ESHAPE, n=65537, k=1, dlogits=None),
    # ---- afan_head_ce ----
    _r("head_ce", EDTYPE, dtype=F32), _r("head_ce", EDTYPE, dtype=7), _r("head_ce", EDTYPE, dtype=-1),
    *[_r("head_ce", ESHAPE, **{a: v}) for a in ("n", "c", "hw", "k") for v in (0, -1)],
    _r("head_ce", ESHAPE, c=-8), _r("head_ce", ESHAPE, k=17), _r("head_ce", ESHAPE, hw=65),
    _r("head_ce", ESHAPE, n=65537, k=1), _r("head_ce", ESHAPE, n=4097, k=16),
    _r("head_ce", ESHAPE, c=12), _r("head_ce", ESHAPE, c=4), _r("head_ce", ESHAPE, c=2056), _r("head_ce", ESHAPE, c=4096),
    _r("head_ce", ESHAPE, c=24), _r("head_ce", ESHAPE, c=48), _r("head_ce", ESHAPE, c=1536),
    *[_r("head_ce", ENULL, **{a: None}) for a in ("out", "raw", "stats", "weight", "target", "pooled", "logits", "loss_row", "dlogits", "v")],
    *[_r("head_ce", ENULL, acc=None, **{a: None}) for a in ("raw", "stats")],      # required without the sums too
    _r("head_ce", ENULL, bias=None, out=None),
    _r("head_ce", EALIGN, out=ODD), _r("head_ce", EALIGN, raw=ODD), _r("head_ce", EALIGN, v=ODD), _r("head_ce", EALIGN, acc=ODD4),
    _r("head_ce", EALIGN, acc=ODD), _r("head_ce", EALIGN, acc=None, raw=ODD), _r("head_ce", EALIGN, out=ODD4), _r("head_ce", EALIGN, c=512, hw=64, k=16, v=ODD),
    _r("head_ce", EDTYPE, dtype=F32, n=0), _r("head_ce", EDTYPE, dtype=7, out=None), _r("head_ce", EDTYPE, dtype=7, out=ODD),
    _r("head_ce", ESHAPE, n=0, out=None), _r("head_ce", ESHAPE, c=12, out=None), _r("head_ce", ESHAPE, c=24, raw=ODD),
    _r("head_ce", ESHAPE, hw=65, v=ODD), _r("head_ce", ESHAPE, k=17, acc=ODD4), _r("head_ce", ESHAPE, n=65537, k=1, target=None),
    _r("head_ce", ENULL, out=None, raw=ODD), _r("head_ce", ENULL, stats=None, acc=ODD4), _r("head_ce", ENULL, v=None, out=ODD),
    _r("head_ce", ENULL, dlogits=None, acc=ODD4),
    # ---- afan_loss_mean ----
    _r("loss_mean", ESHAPE, n=0), _r("loss_mean", ESHAPE, n=-1), _r("loss_mean", ESHAPE, n=65537), _r("loss_mean", ESHAPE, n=1 << 32),
    _r("loss_mean", ENULL, loss_row=None), _r("loss_mean", ENULL, loss=None), _r("loss_mean", ENULL, n=65536, loss=None),
    _r("loss_mean", ESHAPE, n=0, loss_row=None), _r("loss_mean", ESHAPE, n=65537, loss=None),
]


def _pointers():
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 63) & ~63
    return buf, {P: base, ODD: base + 2, ODD4: base + 4}


def build_call(entry, overrides, ptrs):
    """The ctypes argument list of one row."""
    names, base = ENTRIES[entry]
    names = names.split()
    assert len(names) == len(base) and set(overrides) <= set(names), (entry, overrides)
    args = []
    for name, v in zip(names, base):
        v = overrides.get(name, v)
        if isinstance(v, str):
            v = ctypes.c_void_p(ptrs[v])
        elif name in _FLOATS:
            v = float(v)
        args.append(v)
    return args


def test_every_entry_has_rows():
    assert {r[0] for r in ROWS} == set(ENTRIES) and len(ROWS) > 130
    assert {code for _, _, code in ROWS} == {OK, EDTYPE, EALIGN, ESHAPE, ENULL}
    assert all(entry == "head_backward" and o.get("dx", P) is None and o.get("dweight", P) is None for entry, o, code in ROWS if code == OK)
    assert len({(e, tuple(sorted((k, str(v)) for k, v in o.items()))) for e, o, _ in ROWS}) == len(ROWS), "a row is there twice"


def test_return_codes_of_refused_calls(pkg):
    lib = pkg._lib.load()
    buf, ptrs = _pointers()
    wrong = []
    for entry, overrides, code in ROWS:
        got = getattr(lib, "afan_" + entry)(*build_call(entry, overrides, ptrs))
        if got != code:
            wrong.append((entry, overrides, code, got))
    assert not wrong, "\n".join(f"{e} {o}: {g}, recorded {c}" for e, o, c, g in wrong)


def test_max_classes(pkg):
    assert pkg._lib.load().afan_head_max_classes() == MAX_CLASSES
