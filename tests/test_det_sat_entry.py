"""eval_sat_layers.py without a GPU: its parser against the names and defaults recorded from the reference's own parser
(tests/golden/det_sat_args.json), the two ValueErrors and check_unbuilt's refusals before any device work, the evaluator's constructor,
and afan_sat_points_nhwc's argument errors (decided before any GPU call)."""
import ctypes
import importlib
import json
import os

import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def entry(pkg):
    return importlib.import_module("cv_a-fan_amd.eval_sat_layers")


def _table(parser):
    return [{"dest": a.dest, "flags": list(a.option_strings), "default": a.default} for a in parser._actions if a.dest != "help"]


BASE = ["-s", "voc2007", "-b", "resnet101", "model-1.pth"]


def test_parser_equals_the_references(entry, pkg):
    ref = json.load(open(os.path.join(GOLDEN, "det_sat_args.json")))
    assert len(ref) == 19 and ref[-1] == {"dest": "checkpoint", "flags": [], "default": None}
    assert [r["dest"] for r in ref[:8]] == ["steps", "gamma", "eps", "randinit", "clip", "pertub_idx", "sat_layer", "mix"]
    assert _table(entry.get_argparser(full=False)) == ref          # same options, same order, same defaults
    full = _table(entry.get_argparser())
    assert full[:len(ref)] == ref
    assert tuple(a["dest"] for a in full[len(ref):]) == entry.ADDITIONS == ("synthetic", "dtype", "layout", "table")
    eval_ref = json.load(open(os.path.join(GOLDEN, "det_eval_args.json")))
    assert ref[8:] == eval_ref                                     # eval.py's flags behind the settings
    with pytest.raises(SystemExit):
        entry.get_argparser().parse_args(["-s", "voc2007", "-b", "resnet101"])          # the checkpoint is required


def test_defaults(entry):
    o = entry.get_argparser().parse_args(BASE)
    assert (o.steps, o.gamma, o.eps, o.pertub_idx, o.sat_layer) == (10, 0.5, 2, 0, 1) and isinstance(o.steps, int)
    assert (o.randinit, o.clip, o.mix, o.table) == (False, False, False, False)
    assert (o.synthetic, o.dtype, o.layout, o.checkpoint, o.data_dir) == (0, "bf16", "nhwc", "model-1.pth", "./data")
    o = entry.get_argparser().parse_args(["--pertub_idx", "3", "--sat_layer", "4", "--mix", "--table"] + BASE)
    assert (o.pertub_idx, o.sat_layer, o.mix, o.table) == (3, 4, True, True)


@pytest.mark.parametrize("argv, word", [([], "pertub_idx"), (["--pertub_idx", "0"], "pertub_idx"), (["--pertub_idx", "4"], "pertub_idx"),
                                        (["--pertub_idx", "1", "--sat_layer", "5"], "sat_layer"), (["--pertub_idx", "2", "--sat_layer", "-1"], "sat_layer")])
def test_flag_values_are_refused_before_any_work(entry, argv, word, tmp_path, capsys):
    with pytest.raises(ValueError, match=word):
        entry.main(argv + ["-s", "voc2007", "-b", "resnet101", str(tmp_path / "model-1.pth")])
    assert os.listdir(tmp_path) == []                              # no results directory
    assert "steps" + "." * (80 - len("steps") - 2) + "10" in capsys.readouterr().out       # print_args ran first


@pytest.mark.parametrize("argv, word", [(["-s", "voc2007", "-b", "resnet18"], "BasicBlock"), (["-s", "voc2007", "-b", "resnet50"], "ResNet-101 is pinned"),
                                        (["-s", "coco2017", "-b", "resnet101"], "pycocotools"),
                                        (["-s", "voc2007-cat-dog", "-b", "resnet101"], "cat / dog subset")])
def test_refusals_come_before_any_device_work(entry, argv, word, tmp_path):
    with pytest.raises(NotImplementedError, match=word):
        entry.main(["--pertub_idx", "1"] + argv + [str(tmp_path / "model-1.pth")])
    assert os.listdir(tmp_path) == []


def test_evaluator_constructor(pkg):
    class Loader:
        train, batch, n = False, 1, 2
    de = pkg.det_eval
    gt = (["a", "b"], {})
    ev = de.SatLayerEvaluator(Loader(), gt)
    assert (ev.steps, ev.eps, ev.gamma, ev.pertub_idx, ev.sat_layer, ev.mix, ev.randinit, ev.clip, ev.table) == (10, 2.0, 0.5, 1, 1, False, False, False, False)
    assert de.SAT_TABLE == tuple((j, m) for j in range(5) for m in (False, True))
    with pytest.raises(ValueError, match="pertub_idx"):
        de.SatLayerEvaluator(Loader(), gt, pertub_idx=0)
    with pytest.raises(ValueError, match="sat_layer"):
        de.SatLayerEvaluator(Loader(), gt, sat_layer=5)
    # the hook of Evaluator.detect: today's dict by default
    x = object()
    assert de.Evaluator(Loader(), gt).eval_inputs(None, 0, x, None, None) == {"x": x, "adv": None, "out_idx": None, "flag": 'clean', "min_prob": 0.05}


def test_pgd_takes_a_start(pkg):
    import inspect
    p = inspect.signature(pkg.det_ops.PGD).parameters
    assert list(p)[-1] == "start" and p["start"].default is None
    assert pkg.det_attack_algo.PGD is pkg.det_ops.PGD
    assert pkg.det_attack_algo.SAT_POINTS_FUSED in (True, False)


def test_sat_points_argument_errors_without_gpu(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 16)(*([0.5] * 16))
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.afan_sat_points_nhwc
    w = lambda *v: (ctypes.c_float * len(v))(*v)
    assert f(p, p, p, 0, 4, 4, buf, 0, 0, 1e-5, None) == -3                 # AFAN_ESHAPE: n_points outside 1..10
    assert f(p, p, p, 0, 4, 4, buf, 11, 0, 1e-5, None) == -3
    assert f(p, p, p, 0, 4, 4, w(0.25, 1.5), 2, 0, 1e-5, None) == -3        # a weight outside [0, 1]
    assert f(p, p, p, 0, 4, 4, w(-0.25), 1, 0, 1e-5, None) == -3
    assert f(p, p, p, 0, 4, 4, w(float("nan")), 1, 0, 1e-5, None) == -3
    assert f(p, p, p, 0, 4, 4, buf, 2, 4, 1e-5, None) == -3                 # a mask bit at n_points
    assert f(p, p, p, 0, 4, 0, buf, 2, 1, 1e-5, None) == -3                 # c <= 0
    assert f(p, p, p, 0, -1, 4, buf, 2, 1, 1e-5, None) == -3
    assert f(p, p, p, 7, 4, 4, buf, 2, 1, 1e-5, None) == -1                 # AFAN_EDTYPE
    assert f(None, p, p, 0, 4, 4, buf, 2, 1, 1e-5, None) == -4              # AFAN_ENULL
    assert f(p, None, p, 1, 4, 4, buf, 2, 1, 1e-5, None) == -4
    assert f(p, p, None, 1, 4, 4, buf, 2, 1, 1e-5, None) == -4
    assert f(p, p, p, 0, 4, 4, None, 2, 1, 1e-5, None) == -4
    assert f(p, p, ctypes.c_void_p(p.value + 2), 0, 4, 4, buf, 2, 1, 1e-5, None) == -2      # AFAN_EALIGN: fp32 output at a 2-byte address
    assert f(ctypes.c_void_p(p.value + 2), p, p, 1, 4, 4, buf, 2, 1, 1e-5, None) == -2
    assert f(p, p, ctypes.c_void_p(p.value + 1), 1, 4, 4, buf, 2, 1, 1e-5, None) == -2
    assert f(p, p, p, 0, 0, 4, w(0.0, 1.0), 2, 3, 1e-5, None) == 0          # no pixel: no launch
    assert "sat_points" in pkg.ops.CALLS and "sat_points" not in set(pkg.ops.CALLS)
