"""tests/golden/det_final_tiny_readme.npz, det_final_tiny_mixnoise.npz, det_base_tiny.npz — one iteration of the REFERENCE's
Detection/train_aug_final.py (loop body, lines 78-163) and Detection/train_baseline.py (lines 76-89) on oracle.TinyDetNet, and
det_final_args.json / det_base_args.json, the flag tables of the two programs' parsers.

Runs on the CPU, only where the reference lies (AFAN_REFERENCE, default /root/reference).  Its Detection/attack_algo.py is imported
from there at run time with oracle/gen_golden.py's arithmetic-neutral shims (`.cuda()` is the identity).  The two programs cannot be
imported (tensorboardX, the compiled extension), so the lines of their loop bodies are READ from the checkout at run time, dedented
and executed as they stand in a namespace that provides what they name: the model, the optimizer, `args`, the batch, the reference's
attack_algo, f1..f4 as :67-68 compute them, and stand-ins for `scheduler`, `summary_writer` and `losses`.  Only arrays and settings
are written; no line of the reference is.

Model, optimizer and inputs are those of det_step_tiny_s1.npz (oracle/gen_golden.py gen_detection): seed 11, SGD(0.01, 0.9, 5e-4),
two 32 x 32 images drawn from the seeded host generator — which is therefore where a random start or the ROI noise finds it; its
state after the iteration is stored (`rng_state`).

    python tools/gen_det_final_golden.py
"""
import json
import os
import sys
import textwrap
import types
from collections import deque

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import afan_oracle as orc  # noqa: E402
from oracle import gen_golden as gg  # noqa: E402
import gen_det_args  # noqa: E402

FINAL_LINES, BASE_LINES = (78, 163), (76, 89)
SAMPLE = ("stem.0.weight", "layer3.0.weight", "rpn_obj.weight", "hidden.weight", "cls.bias", "layer2.1.running_mean")

CASES = {
    # the README's setting
    "det_final_tiny_readme": dict(pertub_idx_se=2, mix_layer="0011", gamma_se=1.0, gamma_sd=0.1, sd_adv_loss_weight=0.3, only_roi_sd=True,
                                  mix_sd=False, noise_sd=0, randinit=False, clip=False),
    # the other branches: deepest layer, the first two points mixed, mix + noise on the ROI feature, all four losses in its attack, random starts
    "det_final_tiny_mixnoise": dict(pertub_idx_se=3, mix_layer="1100", gamma_se=0.5, gamma_sd=0.1, sd_adv_loss_weight=0.5, only_roi_sd=False,
                                    mix_sd=True, noise_sd=0.01, randinit=True, clip=False),
}


def loop_body(rel, first, last):
    """Lines first..last (1-based, inclusive) of a reference file as a code object."""
    lines = open(os.path.join(gg.REF, rel)).read().split("\n")[first - 1:last]
    return compile(textwrap.dedent("\n".join(lines)), f"<{rel}:{first}-{last}>", "exec")


class _Quiet:
    """scheduler / summary_writer stand-in: every method call is accepted and does nothing."""

    def __getattr__(self, name):
        return lambda *a, **k: None


def setup():
    torch.manual_seed(11)
    model = orc.TinyDetNet()
    model.train()
    optimizer = torch.optim.SGD(model.parameters(), 0.01, momentum=0.9, weight_decay=5e-4)
    image_batch = torch.rand(2, 3, 32, 32)
    bboxes_batch = torch.tensor([[[2., 3., 20., 18.], [10., 12., 30., 31.]], [[0., 0., 15., 15.], [8., 4., 28., 22.]]])
    labels_batch = torch.tensor([[1, 2], [3, 0]])
    return model, optimizer, image_batch, bboxes_batch, labels_batch


def run(code, settings, ref_det):
    model, optimizer, image_batch, bboxes_batch, labels_batch = setup()
    _, c0 = gg._checksums(model)
    args = types.SimpleNamespace(pertub_idx_sd="roi", **settings)
    ns = {"torch": torch, "attack_algo": ref_det, "model": model, "optimizer": optimizer, "args": args, "image_batch": image_batch,
          "bboxes_batch": bboxes_batch, "labels_batch": labels_batch, "scheduler": _Quiet(), "summary_writer": _Quiet(),
          "losses": deque(maxlen=100), "step": 0}
    if "mix_layer" in settings:
        ns["f1"], ns["f2"], ns["f3"], ns["f4"] = (int(c) for c in settings["mix_layer"])
    exec(code, ns)
    k1, c1 = gg._checksums(model)
    sd = model.state_dict()
    rec = {"images": gg._np(image_batch), "bboxes": gg._np(bboxes_batch), "labels": gg._np(labels_batch), "ck0": c0, "ck1": c1,
           "keys": np.array(k1), "loss": gg._np(ns["loss"]), "rng_state": torch.get_rng_state().numpy().copy(),
           **{"sd1/" + k: gg._np(sd[k]) for k in SAMPLE}}
    return rec, ns


def main():
    assert os.path.isdir(gg.REF), f"{gg.REF} not found: this script only runs where the reference lies"
    gg._shims()
    ref_det = gg._load("ref_det_attack_algo", "Detection/attack_algo.py")
    code = loop_body("Detection/train_aug_final.py", *FINAL_LINES)
    for name, settings in CASES.items():
        rec, ns = run(code, settings, ref_det)
        L = [ns[f"loss{i}"] for i in range(6)]
        rec.update(losses=np.array([float(v) for v in L], dtype=np.float32), adv_se=gg._np(ns["feature_adv_se"]),
                   adv_sd=gg._np(ns["adv_feature_map_sd"]), fm_se=gg._np(ns["feature_map_se"]),
                   settings=np.array(json.dumps(settings, sort_keys=True)))
        out = os.path.join(gg.OUT, name + ".npz")
        np.savez_compressed(out, **rec)
        print(name, "loss", float(ns["loss"]), [round(float(v), 5) for v in L], os.path.getsize(out), "bytes")
    rec, ns = run(loop_body("Detection/train_baseline.py", *BASE_LINES), {}, ref_det)
    four = [ns[k] for k in ("anchor_objectness_loss", "anchor_transformer_loss", "proposal_class_loss", "proposal_transformer_loss")]
    rec.update(losses=np.array([float(v) for v in four], dtype=np.float32))
    out = os.path.join(gg.OUT, "det_base_tiny.npz")
    np.savez_compressed(out, **rec)
    print("det_base_tiny loss", float(ns["loss"]), [round(float(v), 5) for v in four], os.path.getsize(out), "bytes")
    for name, rel in (("det_final_args.json", "Detection/train_aug_final.py"), ("det_base_args.json", "Detection/train_baseline.py")):
        rows = gen_det_args.table(os.path.join(gg.REF, rel))
        with open(os.path.join(gg.OUT, name), "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
        print(name, len(rows), "options")


if __name__ == "__main__":
    main()
