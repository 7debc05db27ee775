"""main_inference.py's robust-accuracy flags without a GPU: defaults, parsing and help text."""
from conftest import load_pkg


def _mi():
    return __import__(load_pkg().__name__ + ".main_inference", fromlist=["parser"])


def test_attack_flags_defaults_and_parsing():
    mi = _mi()
    a = mi.parser.parse_args([])
    assert (a.attack_steps, a.attack_eps, a.attack_gamma, a.attack_randinit) == (0, 8.0, 2.0, False)
    # the clean evaluation's flags keep the reference's defaults beside them
    assert (a.data, a.print_freq, a.gpu, a.pretrained, a.batch_size) == ("../data", 50, 0, "res56s_cifar10_baseline", 128)
    b = mi.parser.parse_args(["--attack_steps", "10", "--attack_eps", "4", "--attack_gamma", "0.5", "--attack_randinit"])
    assert (b.attack_steps, b.attack_eps, b.attack_gamma, b.attack_randinit) == (10, 4.0, 0.5, True)


def test_attack_flags_are_documented():
    text = _mi().parser.format_help()
    for flag in ("--attack_steps", "--attack_eps", "--attack_gamma", "--attack_randinit"):
        assert flag in text
    assert "/255" in text and "robust" in text.lower()
    assert callable(_mi().robust_validate)
