"""Records tests/golden/det_eval_args.json: the names, flags and defaults of the reference's Detection/eval.py parser, read from its
source without importing it, the way tools/gen_det_args.py records the training parser's (same `table`).  It holds settings only.
tests/test_det_eval_entry.py holds det_eval.get_argparser() to it.

    python tools/gen_det_eval_args.py <reference checkout>/Detection/eval.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_det_args import ROOT, table  # noqa: E402


def main():
    rows = table(sys.argv[1])
    path = os.path.join(ROOT, "tests", "golden", "det_eval_args.json")
    with open(path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    print(path, len(rows), "options")


if __name__ == "__main__":
    main()
