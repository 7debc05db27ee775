"""tests/golden/l2ball_proj.npz — inputs and outputs of the REFERENCE's own l2ball_proj (Classification/attack_algo.py:21-33).

Runs on the CPU, only where a checkout of the reference lies (--reference DIR or AFAN_REFERENCE): its Classification/attack_algo.py is
imported from there at run time, nothing of it is copied.  Only arrays are written: per case k the fp32 `c{k}_center`, `c{k}_t`
([batch, C, H, W], at most 32 elements per sample), the scalar `c{k}_radius` and the reference's `c{k}_out`, and `c{k}_kind` per
sample: 0 far outside the ball (> 1.1 radius), 1 far inside (< 0.9 radius), 2 a zero perturbation (the reference returns NaN).

Usage:  python tools/gen_l2_golden.py --reference DIR
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1, 1), (1, 1, 1, 2), (2, 3, 1, 1), (2, 1, 2, 2), (3, 1, 1, 5), (1, 1, 1, 7), (2, 2, 2, 2), (3, 1, 3, 3), (2, 1, 4, 4),
          (1, 3, 3, 3), (5, 2, 2, 4), (2, 2, 4, 4)]
RADII = [0.5, 8.0 / 255, 3.0]
OUTSIDE, INSIDE, ZERO = 0, 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("AFAN_REFERENCE"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "l2ball_proj.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference DIR (or AFAN_REFERENCE): the reference checkout")
    spec = importlib.util.spec_from_file_location("ref_attack_algo", os.path.join(a.reference, "Classification", "attack_algo.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    rng = np.random.default_rng(20)
    rec, k = {}, 0
    for si, shape in enumerate(SHAPES):
        for ri, radius in enumerate(RADII):
            b, per = shape[0], int(np.prod(shape[1:]))
            center = rng.standard_normal(shape).astype(np.float32)
            direction = rng.standard_normal(shape)
            direction /= np.sqrt((direction.reshape(b, -1) ** 2).sum(axis=1)).reshape(b, 1, 1, 1)
            kind = np.array([(si + ri + j) % 2 for j in range(b)], np.int64)        # outside / inside in turn
            if (si + ri) % 4 == 3:
                kind[(si + ri) % b] = ZERO
            scale = np.where(kind == OUTSIDE, rng.uniform(1.5, 6.0, b), rng.uniform(0.05, 0.7, b)) * radius
            t = (center + direction * scale.reshape(b, 1, 1, 1)).astype(np.float32)
            t[kind == ZERO] = center[kind == ZERO]
            # the kinds as the stored fp32 inputs have them, in float64: far from the ball's edge
            dist = np.sqrt(((t.astype(np.float64) - center.astype(np.float64)).reshape(b, -1) ** 2).sum(axis=1))
            assert all((d > 1.1 * radius) if kd == OUTSIDE else (d < 0.9 * radius) for d, kd in zip(dist, kind)), (shape, radius, dist, kind)
            assert all((d == 0) == (kd == ZERO) for d, kd in zip(dist, kind))
            out = ref.l2ball_proj(torch.from_numpy(center), radius, torch.from_numpy(t.copy()), in_place=False).numpy()
            rec[f"c{k}_center"], rec[f"c{k}_t"], rec[f"c{k}_out"] = center, t, out.astype(np.float32)
            rec[f"c{k}_radius"], rec[f"c{k}_kind"] = np.float32(radius), kind
            k += 1
    rec["cases"] = np.int64(k)
    np.savez_compressed(a.out, **rec)
    print(f"{a.out}: {k} cases, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
