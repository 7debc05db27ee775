"""tests/golden/det_sat_layers_tiny_{clip3,rand_clip3}.npz (one file per case, each under the 1 MiB of a committed file) — the
REFERENCE's Detection/attack_algo.py PGD (:48-74), get_sample_points (:236-245) and mix_feature (:254-265) as evaluator.py:131-180 (`sat_layer_evaluate`) strings them together, on oracle.TinyDetNet — and
tests/golden/det_sat_args.json, the flag table of Detection/eval_sat_layers.py's parser.

Runs on the CPU, only where the reference lies (AFAN_REFERENCE, default /root/reference).  Its attack_algo.py is imported from there at
run time with oracle/gen_golden.py's arithmetic-neutral shims (`.cuda()` is the identity) and called as it stands; what happens
inside a call is observed from outside: the model's forward is wrapped to note the feature it is given and the host generator's state
at that moment, torch.autograd.grad to note the feature gradient it returns.  Only arrays and settings are written.

Model and inputs are those of det_step_tiny_s1.npz (gen_det_final_golden.setup(): seed 11, two 32 x 32 images, two boxes each); the
host generator is seeded 29 before every attack.  Cases `c` = clip3 (steps 3, clip) and rand_clip3 (steps 3, randinit + clip), each
for idx 1 and 2 (keys `c_iN/...`); eps 2 / 255, gamma 0.5 / 255:
    x, bboxes, labels, settings
    fm                     the train-mode `flag: 'head'` feature map behind layer idx, detached
    rng0                   the host generator's state before the call (the random start's draw finds it there)
    rng    [steps, ...]    the generator's state before every step (at the step's forward)
    iter   [steps + 1]     the iterate before step 0 (fm, or fm + the random start) and after every step
    grad   [steps]         the feature gradient of every step, fp32
    grad64 [steps]         the gradient at the SAME iterate from a float64 run of the same function on a float64 copy of the model
    gdiff  [steps]         max |grad - grad64|: the reference's own fp32-against-float64 difference
    thr    [steps]         2 x gdiff: under it a gradient's sign is not decided (the project's ref_det_floor rule)
    adv                    PGD's result
    pt/j      j = 0..4     get_sample_points(fm, adv, 5)[j]
    mixed/j                mix_feature(pt_j, fm) — the evaluation's REVERSED order — in fp32
    mixed64/j              the same formula in float64 on the fp32 point and map
    mdiff/j                max |mixed - mixed64|: the reference's own fp32-against-float64 difference
The tool asserts that at most 1 % of a case's gradient elements fall under the threshold (else: choose other seeds), and that for
j >= 1 max |mixed_j - pt_j| >= 1e-3: a test on the mixed points can tell the mix from its absence.

    python tools/gen_det_sat_golden.py
"""
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import gen_golden as gg  # noqa: E402
import gen_det_args  # noqa: E402
from gen_det_final_golden import setup  # noqa: E402

EPS, GAMMA = 2.0 / 255, 0.5 / 255
CASES = {"clip3": dict(steps=3, randinit=False, clip=True),
         "rand_clip3": dict(steps=3, randinit=True, clip=True)}
IDXS = (1, 2)
UNDER_CAP = 0.01
MIX_MOVES = 1e-3


class Watch:
    """Notes the feature that goes into the model's forward and what torch.autograd.grad hands back while `fn` runs."""

    def __init__(self, model):
        self.model, self.iters, self.rng, self.grads = model, [], [], []

    def __enter__(self):
        self.fwd, self.grad = self.model.forward, torch.autograd.grad

        def forward(d, *a, **k):
            self.iters.append(d["adv"].detach().clone())
            self.rng.append(torch.get_rng_state().numpy().copy())
            return self.fwd(d, *a, **k)

        def grad(*a, **k):
            out = self.grad(*a, **k)
            self.grads.append(out[0].detach().clone())
            return out
        self.model.forward, torch.autograd.grad = forward, grad
        return self

    def __exit__(self, *exc):
        del self.model.forward
        torch.autograd.grad = self.grad
        return False


def main():
    assert os.path.isdir(gg.REF), f"{gg.REF} not found: this script only runs where the reference lies"
    gg._shims()
    ref = gg._load("ref_det_attack_algo", "Detection/attack_algo.py")
    for case, s in CASES.items():
        rec = {}
        for idx in IDXS:
            name = f"{case}_i{idx}"
            model, _, x, bb, lb = setup()
            y = {"bb": bb, "lb": lb}
            fm = model.train().forward({"x": x, "adv": None, "out_idx": idx, "flag": "head"}, bb, lb).detach()
            torch.manual_seed(29)
            rng0 = torch.get_rng_state().numpy().copy()
            with Watch(model) as w:
                adv = ref.PGD(fm, x, y=y, model=model, steps=s["steps"], eps=EPS, gamma=GAMMA, idx=idx, randinit=s["randinit"], clip=s["clip"])
            adv = adv.detach()
            iters = w.iters + [adv.clone()]
            assert len(w.grads) == s["steps"] and len(iters) == s["steps"] + 1
            m64 = copy.deepcopy(model).double()
            g64 = []
            for t in range(s["steps"]):            # the same function, one step, float64, from the fp32 run's own iterate
                with Watch(m64) as w64:
                    ref.PGD(iters[t].double(), x.double(), y={"bb": bb.double(), "lb": lb}, model=m64, steps=1, eps=EPS, gamma=GAMMA, idx=idx)
                g64.append(w64.grads[0])
            grad, grad64 = torch.stack(w.grads), torch.stack(g64)
            gdiff = (grad.double() - grad64).abs().flatten(1).max(dim=1).values
            thr = 2.0 * gdiff
            big = grad.double().abs() > thr[:, None, None, None, None]
            under = float((~big).double().mean())
            assert under <= UNDER_CAP, f"{name}: {under} of the elements lie under the threshold: choose other seeds"
            assert bool((torch.sign(grad.double())[big] == torch.sign(grad64)[big]).all())
            rec.update({f"{name}/x": gg._np(x), f"{name}/bboxes": gg._np(bb), f"{name}/labels": gg._np(lb), f"{name}/fm": gg._np(fm),
                        f"{name}/rng0": rng0, f"{name}/rng": np.stack(w.rng), f"{name}/iter": gg._np(torch.stack(iters)),
                        f"{name}/grad": gg._np(grad), f"{name}/grad64": gg._np(grad64), f"{name}/gdiff": gdiff.numpy(), f"{name}/thr": thr.numpy(),
                        f"{name}/adv": gg._np(adv),
                        f"{name}/settings": np.array(json.dumps(dict(s, eps=EPS, gamma=GAMMA, idx=idx), sort_keys=True))})
            pts = ref.get_sample_points(fm, adv, 5)
            assert len(pts) == 5
            mdiffs, moves = [], []
            for j, pt in enumerate(pts):
                mixed = ref.mix_feature(pt, fm)                       # evaluator.py:159: the reversed order
                mixed64 = ref.mix_feature(pt.double(), fm.double())
                mdiff = float((mixed.double() - mixed64).abs().max())
                mdiffs.append(mdiff)
                moves.append(float((mixed - pt).abs().max()))
                if j >= 1:
                    assert moves[-1] >= MIX_MOVES, f"{name}: the mix moves point {j} by {moves[-1]} only"
                rec.update({f"{name}/pt/{j}": gg._np(pt), f"{name}/mixed/{j}": gg._np(mixed), f"{name}/mixed64/{j}": gg._np(mixed64),
                            f"{name}/mdiff/{j}": np.array(mdiff)})
            print(name, "gdiff", gdiff.tolist(), "under 2 x gdiff:", under, "mdiff", mdiffs, "max |mixed - pt|", moves,
                  "max |mixed64|", float(mixed64.abs().max()))
        out = os.path.join(gg.OUT, f"det_sat_layers_tiny_{case}.npz")          # (one file per case: a committed file stays under 1 MiB)
        np.savez_compressed(out, **rec)
        print(out, os.path.getsize(out), "bytes")
        assert os.path.getsize(out) < (1 << 20)
    rows = gen_det_args.table(os.path.join(gg.REF, "Detection/eval_sat_layers.py"))
    with open(os.path.join(gg.OUT, "det_sat_args.json"), "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    print("det_sat_args.json", len(rows), "options")


if __name__ == "__main__":
    main()
