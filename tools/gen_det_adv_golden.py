"""tests/golden/det_adv_tiny_plain.npz, det_adv_tiny_rand_clip.npz, det_adv_tiny_rand_clip3.npz — one iteration of the REFERENCE's
Detection/train_baseline_advtrain.py (loop body, lines 75-93: image PGD, one forward on the adversarial batch, backward, the step) on
oracle.TinyDetNet, and det_adv_args.json, the flag table of its parser.

Same method as tools/gen_det_final_golden.py, whose loop_body / setup / _Quiet are imported: runs on the CPU, only where the reference
lies (AFAN_REFERENCE); the program cannot be imported, so the lines of its loop body are READ from the checkout at run time, dedented
and executed as they stand in a namespace that provides what they name.  Only arrays and settings are written; no line of the
reference is.

    plain        steps 1, no random start, no clip
    rand_clip    steps 1, randinit, clip
    rand_clip3   steps 3, randinit, clip — and, for a step-by-step check in which a flipped sign cannot compound, the UN-clamped
                 iterate after each step (`iter1..3`: the reference's adv_input re-run with steps = 1, 2, 3 from the same generator
                 state, its final torch.clamp switched off for those re-runs), the random start itself (`iter0`: steps = 0) and the host
                 generator's state in front of each attack pass (`rng_pass0..2`) and in front of the training forward (`rng_train`)

Every case also runs in float64 (model, images and boxes cast; the random start is the same float32 draw): `ref_flip_share` is the
share of adversarial pixels where the fp32 and the float64 run differ by more than half a step — the reference's own sign-flip
error, asserted here to stay below 1e-2, half the cap the tests hold the product to.

    python tools/gen_det_adv_golden.py
"""
import json
import os
import sys
import types
from collections import deque

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import gen_golden as gg  # noqa: E402
import gen_det_args  # noqa: E402
from gen_det_final_golden import SAMPLE, _Quiet, loop_body, setup  # noqa: E402

ADV_LINES = (75, 93)
REL = "Detection/train_baseline_advtrain.py"
FOUR = ("anchor_objectness_losses1", "anchor_transformer_losses1", "proposal_class_losses1", "proposal_transformer_losses1")

CASES = {
    "det_adv_tiny_plain": dict(steps=1, eps=2.0, gamma=0.5, randinit=False, clip=False),
    "det_adv_tiny_rand_clip": dict(steps=1, eps=2.0, gamma=0.5, randinit=True, clip=True),
    "det_adv_tiny_rand_clip3": dict(steps=3, eps=2.0, gamma=0.5, randinit=True, clip=True),
}


def run(code, settings, ref_det, double=False):
    model, optimizer, image_batch, bboxes_batch, labels_batch = setup()
    _, c0 = gg._checksums(model)
    if double:
        model.double()
        image_batch, bboxes_batch = image_batch.double(), bboxes_batch.double()
    rng0 = torch.get_rng_state()
    states = []
    fwd = model.forward
    model.forward = lambda *a, **k: (states.append(torch.get_rng_state().numpy().copy()), fwd(*a, **k))[1]
    ns = {"torch": torch, "attack_algo": ref_det, "model": model, "optimizer": optimizer, "args": types.SimpleNamespace(**settings),
          "image_batch": image_batch, "bboxes_batch": bboxes_batch, "labels_batch": labels_batch, "scheduler": _Quiet(),
          "summary_writer": _Quiet(), "losses": deque(maxlen=100), "step": 0}
    exec(code, ns)
    model.forward = fwd
    assert len(states) == settings["steps"] + 1
    k1, c1 = gg._checksums(model)
    sd = model.state_dict()
    rec = {"images": gg._np(image_batch), "bboxes": gg._np(bboxes_batch), "labels": gg._np(labels_batch), "ck0": c0, "ck1": c1,
           "keys": np.array(k1), "loss": gg._np(ns["loss"]), "losses": np.array([float(ns[k].detach().mean()) for k in FOUR], dtype=np.float32),
           "adv_image_batch": gg._np(ns["adv_image_batch"]), "rng_state": torch.get_rng_state().numpy().copy(),
           "settings": np.array(json.dumps(settings, sort_keys=True)), **{"sd1/" + k: gg._np(sd[k]) for k in SAMPLE}}
    return rec, ns, rng0, states


def iterates(settings, ref_det, rng0):
    """The un-clamped iterate after 0..steps steps: the reference's adv_input from the same generator state and the same (untouched)
    model, with the module's `torch.clamp` replaced by the identity for these calls."""
    class _NoClamp:
        def __getattr__(self, name):
            return (lambda t, *a, **k: t) if name == "clamp" else getattr(torch, name)
    out = []
    real = ref_det.torch
    try:
        ref_det.torch = _NoClamp()
        for k in range(settings["steps"] + 1):
            model, _, image_batch, bboxes_batch, labels_batch = setup()
            torch.set_rng_state(rng0)
            x = ref_det.adv_input(x=image_batch, y={"bb": bboxes_batch, "lb": labels_batch}, model=model, steps=k, eps=settings["eps"] / 255,
                                  gamma=settings["gamma"] / 255, randinit=settings["randinit"], clip=settings["clip"])
            out.append(gg._np(x))
    finally:
        ref_det.torch = real
    return out


def main():
    assert os.path.isdir(gg.REF), f"{gg.REF} not found: this script only runs where the reference lies"
    gg._shims()
    ref_det = gg._load("ref_det_attack_algo", "Detection/attack_algo.py")
    code = loop_body(REL, *ADV_LINES)
    for name, settings in CASES.items():
        rec, ns, rng0, states = run(code, settings, ref_det)
        rec64, ns64, _, _ = run(code, settings, ref_det, double=True)
        half = 0.5 * settings["gamma"] / 255
        share = float((np.abs(rec["adv_image_batch"].astype(np.float64) - rec64["adv_image_batch"].astype(np.float64)) > half).mean())
        assert share <= 1e-2, (name, share)
        assert float(np.abs(rec["adv_image_batch"] - rec["images"]).max()) > half       # (the fixture moved)
        rec["ref_flip_share"] = np.array(share)
        rec["loss64"] = np.array(float(ns64["loss"]))
        if name.endswith("3"):
            its = iterates(settings, ref_det, rng0)
            np.testing.assert_array_equal(np.clip(its[-1], 0.0, 1.0), rec["adv_image_batch"])      # the re-runs retrace the iteration
            for k, x in enumerate(its):
                rec[f"iter{k}"] = x
            for k, s in enumerate(states[:-1]):
                rec[f"rng_pass{k}"] = s
            rec["rng_train"] = states[-1]
        out = os.path.join(gg.OUT, name + ".npz")
        np.savez_compressed(out, **rec)
        print(name, "loss", float(ns["loss"]), "float64", float(ns64["loss"]), [round(float(v), 5) for v in rec["losses"]],
              "ref_flip_share", share, os.path.getsize(out), "bytes")
    rows = gen_det_args.table(os.path.join(gg.REF, REL))
    with open(os.path.join(gg.OUT, "det_adv_args.json"), "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    print("det_adv_args.json", len(rows), "options")


if __name__ == "__main__":
    main()
