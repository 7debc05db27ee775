"""tests/golden/base_r20s.npz — three baseline iterations (Classification/main_base.py:157-162) of the REFERENCE's own ResNet-20s.

Runs on the CPU, only where the reference lies (AFAN_REFERENCE, default /root/reference): its Classification/resnet_s.py is imported
from there at run time with oracle/gen_golden.py's arithmetic-neutral shims; the loop body of main_base.py (which cannot be
imported: top-level torchvision / matplotlib imports) is driven here line by line.  Only arrays are written.

Start: the `sd0/` weights stored in step_r20s_k1.npz (their fingerprint is stored here, not the weights again).  Three seeded
batches of 4 images, fp32, SGD lr 0.1 / momentum 0.9 / weight decay 5e-4.  Stored: the batches, the three losses, out_clean of the
first iteration, the sample of tensors and the per-tensor fingerprints after the third step (layout of the step_* goldens), and
`loss_spread`: per iteration, how far the reference's own loss moves when the same run is done in float64 and in channels-last
(oracle/gen_golden.py lossfloor's `f64` and `cl` variants).

Usage:  python tools/gen_base_golden.py
"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402

SEED, ITERS, BATCH, LN = 11, 3, 4, 16


def run(model0, xs, ys, kind):
    model, (xv,) = gg._to_variant(kind, copy.deepcopy(model0), [xs])
    model.train()
    opt = torch.optim.SGD(model.parameters(), 0.1, momentum=0.9, weight_decay=5e-4)
    crit = nn.CrossEntropyLoss()
    losses, outs = [], []
    for i in range(ITERS):
        xi = xv[i]
        if kind == "cl":
            xi = xi.contiguous(memory_format=torch.channels_last)
        out = model(xi, end_point=LN, start_point=0)
        loss = crit(out, ys[i])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        outs.append(out.detach())
    return losses, outs, model


def main():
    assert os.path.isdir(gg.REF), f"{gg.REF} not found: this script only runs where the reference lies"
    gg._shims()
    ref_resnet = gg._load("ref_cls_resnet_s", "Classification/resnet_s.py")
    g = np.load(os.path.join(gg.OUT, "step_r20s_k1.npz"))
    model0 = ref_resnet.ResNet(ref_resnet.BasicBlock, [3, 3, 3])
    model0.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd0/")})
    k0, c0 = gg._checksums(model0)
    assert np.array_equal(c0, g["ck0"])
    gen = torch.Generator().manual_seed(SEED)
    xs = torch.rand(ITERS, BATCH, 3, 32, 32, generator=gen)
    ys = torch.randint(0, 10, (ITERS, BATCH), generator=gen)
    base, outs, mb = run(model0, xs, ys, "base")
    runs = {k: run(model0, xs, ys, k)[0] for k in ("f64", "cl")}
    spread = np.array([max(abs(runs[k][i] - base[i]) for k in runs) for i in range(ITERS)])
    k1, c1 = gg._checksums(mb)
    assert k0 == k1
    sd = mb.state_dict()
    rec = {"xs": gg._np(xs), "ys": gg._np(ys), "losses": np.array(base, dtype=np.float64), "loss_spread": spread,
           "out_clean": gg._np(outs[0]), "ck0": c0, "ck1": c1, "keys": np.array(k1),
           "hyper": np.array([0.1, 0.9, 5e-4])}
    for k in ("sequential_model.2.running_mean", "sequential_model.2.running_var", "sequential_model.2.num_batches_tracked",
              "sequential_model.7.bn1.running_mean", "sequential_model.7.bn1.running_var", "sequential_model.7.bn1.num_batches_tracked",
              "sequential_model.1.weight", f"sequential_model.{LN - 1}.weight", f"sequential_model.{LN - 1}.bias"):
        rec["sd1/" + k] = gg._np(sd[k])
    out = os.path.join(gg.OUT, "base_r20s.npz")
    np.savez_compressed(out, **rec)
    print("base_r20s losses", base, "spread (f64, cl)", spread.tolist(), {k: v for k, v in runs.items()}, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
