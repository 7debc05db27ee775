"""main_inference.py --attack_norm without a GPU: default, parsing, refusal of other values, the documentation, and the clean run's
printed namespace."""
import argparse

import pytest

from conftest import load_pkg


def _mi():
    return __import__(load_pkg().__name__ + ".main_inference", fromlist=["parser"])


def test_attack_norm_default_and_parsing():
    mi = _mi()
    assert mi.parser.parse_args([]).attack_norm == "linf"
    assert mi.parser.parse_args(["--attack_norm", "l2"]).attack_norm == "l2"
    assert mi.parser.parse_args(["--attack_norm", "linf"]).attack_norm == "linf"
    b = mi.parser.parse_args(["--attack_steps", "10", "--attack_eps", "127.5", "--attack_gamma", "25.5", "--attack_norm", "l2"])
    assert (b.attack_steps, b.attack_eps, b.attack_gamma, b.attack_randinit, b.attack_norm) == (10, 127.5, 25.5, False, "l2")


@pytest.mark.parametrize("value", ["l1", "L2", "inf", ""])
def test_other_norms_are_a_parser_error(value, capsys):
    with pytest.raises(SystemExit) as e:
        _mi().parser.parse_args(["--attack_norm", value])
    assert e.value.code == 2 and "--attack_norm" in capsys.readouterr().err


def test_attack_norm_is_documented():
    mi = _mi()
    text = mi.parser.format_help()
    assert "--attack_norm" in text and "linf" in text and "l2" in text and "127.5" in text and "/255" in text
    assert "--attack_norm" in mi.__doc__ and "127.5" in mi.__doc__


def test_clean_run_prints_the_namespace_it_printed_before(monkeypatch, capsys):
    """--attack_steps 0: the printed namespace holds no attack_* entry, the new flag included (main() prints it first)."""
    mi = _mi()

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop

    monkeypatch.setattr(mi.cls_entry, "setup", stop)
    with pytest.raises(Stop):
        mi.main(["--attack_norm", "l2"])
    line = capsys.readouterr().out.strip().splitlines()[0]
    clean = {k: v for k, v in vars(mi.parser.parse_args([])).items() if not k.startswith("attack_")}
    assert line == str(argparse.Namespace(**clean)) and "attack" not in line
    with pytest.raises(Stop):
        mi.main(["--attack_steps", "2", "--attack_norm", "l2"])
    assert "attack_norm='l2'" in capsys.readouterr().out
