"""Records tests/golden/det_args.json: the names, flags and defaults of the reference's Detection parser, read from its source
without importing it (it imports tensorboardX and a compiled extension).  Every `parser.add_argument(...)` call of the file is
re-issued on a fresh argparse parser with its flags, `default` and `action` (literals in the source); the table is that parser's.
It holds settings only.  tests/test_det_entry.py holds det_entry.get_argparser() to it.

    python tools/gen_det_args.py <reference checkout>/Detection/train_aug_sat_muti_advt.py
"""
import argparse
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table(path):
    tree = ast.parse(open(path).read())
    parser = argparse.ArgumentParser()
    for node in ast.walk(tree):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument"):
            continue
        flags = [ast.literal_eval(a) for a in node.args]
        kw = {k.arg: ast.literal_eval(k.value) for k in node.keywords if k.arg in ("default", "action")}
        parser.add_argument(*flags, **kw)
    acts = [a for a in parser._actions if a.dest != "help"]
    # ast.walk is breadth first; the calls are statements of one block, so source order is line order
    return [{"dest": a.dest, "flags": list(a.option_strings), "default": a.default} for a in acts]


def main():
    rows = table(sys.argv[1])
    path = os.path.join(ROOT, "tests", "golden", "det_args.json")
    with open(path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    print(path, len(rows), "options")


if __name__ == "__main__":
    main()
