#!/usr/bin/env python3
"""Time of one training step (pesto_amd.training.Trainer.train_step) on the i_v4_1 architecture: one synthetic structure of N atoms
(pesto_amd.topology.synthetic_structure), stacked real i_v4_0 weights as in bench.py. Forward (+ loss), backward and Adam are timed
separately with HIP events inside the library (pesto_train_set_timing); the whole step also with a host clock around a synchronised
call. Device tensors, so no staging copy is inside the timed region. Prints one JSON line and writes it to --out.

    python profiles/train_step.py [--atoms 3000] [--steps 30] [--warmup 5] [--out profiles/train_step.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import load_weights, make_batch  # noqa: E402
from pesto_amd.config import CONFIGS  # noqa: E402
from pesto_amd.training import Trainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=3000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="i_v4_1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step.json"))
    a = ap.parse_args()
    import torch
    config = CONFIGS[a.config]
    sd, weights = load_weights(config)
    X, ids, q, roa, R = make_batch(a.atoms, 1, 1, config["em"]["N0"])
    y = (np.random.default_rng(0).random((R, config["dm"]["N2"])) < 0.2).astype(np.float32)
    dev = torch.device("cuda:0")
    batch = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (X, ids, q, roa.astype(np.int32), y)]
    Xd, idsd, qd, road, yd = batch
    tr = Trainer(config, sd, lr=1e-5).set_timing(True)
    rows, wall = [], []
    for step in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses, _, _ = tr.train_step(Xd, idsd, qd, (road, R), yd)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if step >= a.warmup:
            rows.append(tr.timing())
            wall.append((t1 - t0) * 1e3)
    loss = float(losses.sum())

    def stats(v):
        v = np.sort(np.asarray(v, np.float64))
        return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1])}

    res = {"what": "train_step", "config": a.config, "weights": weights, "atoms": int(X.shape[0]), "residues": int(R), "steps": a.steps, "warmup": a.warmup,
           "forward_ms": stats([r["forward_ms"] for r in rows]), "backward_ms": stats([r["backward_ms"] for r in rows]),
           "adam_ms": stats([r["adam_ms"] for r in rows]), "step_wall_ms": stats(wall),
           "it_per_s": 1e3 / float(np.median(wall)), "final_loss": loss, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
