"""tests/golden/det_eval_pgd_tiny.npz — the REFERENCE's Detection/attack_algo.py eval_PGD (:207-233), the image PGD of its robust
evaluation, on oracle.TinyDetNet — and tests/golden/det_rob_args.json, the flag table of Detection/eval_rob_ori.py's parser.

Runs on the CPU, only where the reference lies (AFAN_REFERENCE, default /root/reference).  Its attack_algo.py is imported from there at
run time with oracle/gen_golden.py's arithmetic-neutral shims (`.cuda()` is the identity) and called as it stands; what happens
inside a call is observed from outside: the model's forward is wrapped to note the iterate it is given and the host generator's state
at that moment, torch.autograd.grad to note the image gradient it returns.  Only arrays and settings are written.

Model and inputs are those of det_step_tiny_s1.npz (seed 11, two 32 x 32 images, two boxes each).  Three cases:
(steps 3, clip), (steps 3, randinit + clip), (steps 2, neither); eps 2 / 255, gamma 0.5 / 255.  Per case `c`:
    c/x, c/bboxes, c/labels, c/settings
    c/rng0                 the host generator's state before the call (the random start's draw finds it there)
    c/rng    [steps, ...]  the generator's state before every step (at the step's forward)
    c/iter   [steps + 1]   the iterate before step 0 (x, or x + the random start) and after every step
    c/grad   [steps]       the image gradient of every step, fp32
    c/grad64 [steps]       the gradient at the SAME iterate from a float64 run of the same function on a float64 copy of the model
    c/gdiff  [steps]       max |grad - grad64|: the reference's own fp32-against-float64 difference
    c/thr    [steps]       2 x gdiff: under it a gradient's sign is not decided (the project's ref_det_floor rule)
The tool asserts that at most 1 % of a case's elements fall under the threshold on these inputs (else: choose other seeds).

    python tools/gen_det_rob_golden.py
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
         "rand_clip3": dict(steps=3, randinit=True, clip=True),
         "plain2": dict(steps=2, randinit=False, clip=False)}
UNDER_CAP = 0.01


class Watch:
    """Notes what goes into the model's forward and what torch.autograd.grad hands back while `fn` runs."""

    def __init__(self, model):
        self.model, self.iters, self.rng, self.grads = model, [], [], []

    def __enter__(self):
        self.fwd, self.grad = self.model.forward, torch.autograd.grad

        def forward(d, *a, **k):
            self.iters.append(d["x"].detach().clone())
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
    rec = {}
    for name, s in CASES.items():
        model, _, x, bb, lb = setup()
        torch.manual_seed(29)
        rng0 = torch.get_rng_state().numpy().copy()
        y = {"bb": bb, "lb": lb}
        with Watch(model) as w:
            out = ref.eval_PGD(x=x, y=y, model=model, steps=s["steps"], eps=EPS, gamma=GAMMA, randinit=s["randinit"], clip=s["clip"])
        iters = w.iters + [out.detach().clone()]
        assert len(w.grads) == s["steps"] and len(iters) == s["steps"] + 1
        m64 = copy.deepcopy(model).double()
        g64 = []
        for t in range(s["steps"]):            # the same function, one step, float64, from the fp32 run's own iterate
            with Watch(m64) as w64:
                ref.eval_PGD(x=iters[t].double(), y={"bb": bb.double(), "lb": lb}, model=m64, steps=1, eps=EPS, gamma=GAMMA)
            g64.append(w64.grads[0])
        grad, grad64 = torch.stack(w.grads), torch.stack(g64)
        gdiff = (grad.double() - grad64).abs().flatten(1).max(dim=1).values
        thr = 2.0 * gdiff
        under = float((grad.double().abs() <= thr[:, None, None, None, None]).double().mean())
        print(name, "gdiff", gdiff.tolist(), "share of elements under 2 x gdiff:", under, "|g| median", float(grad.abs().median()))
        assert under <= UNDER_CAP, f"{name}: {under} of the elements lie under the threshold: choose other seeds"
        # the reference's own fp32 run against its float64 gradients: the signs agree above the threshold (by construction) — checked
        big = grad.double().abs() > thr[:, None, None, None, None]
        assert bool((torch.sign(grad.double())[big] == torch.sign(grad64)[big]).all())
        rec.update({f"{name}/x": gg._np(x), f"{name}/bboxes": gg._np(bb), f"{name}/labels": gg._np(lb), f"{name}/rng0": rng0,
                    f"{name}/rng": np.stack(w.rng), f"{name}/iter": gg._np(torch.stack(iters)), f"{name}/grad": gg._np(grad),
                    f"{name}/grad64": gg._np(grad64), f"{name}/gdiff": gdiff.numpy(), f"{name}/thr": thr.numpy(),
                    f"{name}/settings": np.array(json.dumps(dict(s, eps=EPS, gamma=GAMMA), sort_keys=True))})
    out = os.path.join(gg.OUT, "det_eval_pgd_tiny.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")
    rows = gen_det_args.table(os.path.join(gg.REF, "Detection/eval_rob_ori.py"))
    with open(os.path.join(gg.OUT, "det_rob_args.json"), "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    print("det_rob_args.json", len(rows), "options")


if __name__ == "__main__":
    main()
