"""main_inference.py without a GPU: the reference's flags and defaults, and the CIFAR-10 test-split reader's order."""
import pickle

import numpy as np

from conftest import load_pkg


def test_parser_matches_the_reference():
    mi = __import__(load_pkg().__name__ + ".main_inference", fromlist=["parser"])
    a = mi.parser.parse_args([])
    assert (a.data, a.print_freq, a.gpu, a.pretrained, a.batch_size) == ("../data", 50, 0, "res56s_cifar10_baseline", 128)
    assert (a.arch, a.dtype, a.layout, a.synthetic) == ("resnet56s", "bf16", "nhwc", 0)
    b = mi.parser.parse_args(["--data", "d", "--print_freq", "3", "--gpu", "1", "--pretrained", "p.pt", "--batch_size", "7"])
    assert (b.data, b.print_freq, b.gpu, b.pretrained, b.batch_size) == ("d", 3, 1, "p.pt", 7)


def test_test_split_reader_keeps_file_order(tmp_path):
    mp = __import__(load_pkg().__name__ + ".cls_data", fromlist=["_load_cifar10_test"])
    d = tmp_path / "cifar-10-batches-py"
    d.mkdir()
    data = np.arange(5 * 3072, dtype=np.int64).reshape(5, 3072) % 251
    labels = [3, 1, 4, 1, 5]
    with open(d / "test_batch", "wb") as f:
        pickle.dump({"data": data.astype(np.uint8), "labels": labels}, f)
    for root in (str(tmp_path), str(d)):
        x, y = mp._load_cifar10_test(root)
        assert x.dtype == np.uint8 and x.shape == (5, 3, 32, 32)
        assert np.array_equal(x.reshape(5, -1), data.astype(np.uint8)) and list(y) == labels
