#!/usr/bin/env python3
"""Time of one training step through pesto_amd.nn.Model against pesto_amd.training.Trainer, on the workload of profiles/train_step.py:
i_v4_1 architecture, one synthetic structure of N atoms, stacked real i_v4_0 weights, device tensors. Four variants, interleaved step by
step in ONE run so that clock and thermal drift hit them alike:

  a  Trainer.train_step of another build of the library (--parent-lib: libpesto_hip.so of the parent commit, built from a checkout of it
     with `python -m pesto_amd.csrc.build`; skipped without it)
  b  Trainer.train_step of this tree
  c  pesto_amd.nn.Model + the reference's loss (model/main.py:49-58, torch ops) + torch.optim.Adam
  d  the same with X.requires_grad (the geometry variant of the layer backward and the backward of the geometry)

Every step is timed with a host clock around a synchronised call. For c and d the shares of torch.cat (the flat parameter tensor and
its backward), of ATen's Adam and of the library calls are timed with HIP events in a second pass. Prints one JSON line, writes --out.

    python profiles/nn_step.py [--atoms 3000] [--steps 30] [--warmup 5] [--parent-lib PATH] [--out profiles/nn_step.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import load_weights, make_batch  # noqa: E402
from pesto_amd import _lib  # noqa: E402
from pesto_amd.config import CONFIGS  # noqa: E402
from pesto_amd.training import MODE_TRAIN, Trainer  # noqa: E402
from pesto_amd.weights import flatten_state_dict  # noqa: E402


class ParentTrainer:
    """train_step of another libpesto_hip.so (the five entry points it needs, bound by hand: the process keeps this tree's library too)"""

    def __init__(self, path, config, sd, lr):
        import torch  # noqa: F401  (one HIP runtime per process, pesto_amd._lib.load)
        self.lib = ctypes.CDLL(path)
        c_p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        self.lib.pesto_train_last_error.restype = ctypes.c_char_p
        self.lib.pesto_train_create.argtypes = [ctypes.POINTER(_lib.PestoConfig), c_p, i64, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.POINTER(c_p)]
        self.lib.pesto_train_destroy.argtypes = [c_p]
        self.lib.pesto_train_step.argtypes = [c_p, i32, i64, i64, i32, i32, c_p, c_p, i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p]
        blob = np.ascontiguousarray(flatten_state_dict(config, sd), np.float32)
        cc = _lib.make_c_config(config, "fp32")
        self.h = ctypes.c_void_p()
        self.check(self.lib.pesto_train_create(ctypes.byref(cc), blob.ctypes.data, blob.size, 0, lr, 0.5, ctypes.byref(self.h)))

    def check(self, rc):
        if rc:
            raise RuntimeError(self.lib.pesto_train_last_error().decode())

    def train_step(self, X, ids, q, roa, R, y, out):
        import torch
        self.check(self.lib.pesto_train_step(self.h, MODE_TRAIN, X.shape[0], R, ids.shape[1], y.shape[1], X.data_ptr(), ids.data_ptr(), _lib.ids_kind(ids),
                                             q.data_ptr(), roa.data_ptr(), y.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None,
                                             _lib.PTR_DEVICE, torch.cuda.current_stream().cuda_stream))

    def close(self):
        self.lib.pesto_train_destroy(self.h)


def reference_loss(z, y, pos_ratios, global_step, f=0.5):
    import torch
    pos_ratios += (torch.mean(y, dim=0).detach() - pos_ratios) / (1.0 + np.sqrt(global_step))
    criterion = torch.nn.BCEWithLogitsLoss(reduction="none")
    criterion.pos_weight = f * (1.0 - pos_ratios) / (pos_ratios + 1e-6)
    dloss = criterion(z, y)
    return ((pos_ratios / torch.sum(pos_ratios)).reshape(1, -1) * dloss) / dloss.shape[0]


def stats(v):
    v = np.sort(np.asarray(v, np.float64))
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=3000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="i_v4_1")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_step.json"))
    a = ap.parse_args()
    import torch
    from pesto_amd.nn import Model
    config = CONFIGS[a.config]
    sd, weights = load_weights(config)
    X, ids, q, roa, R = make_batch(a.atoms, 1, 1, config["em"]["N0"])
    C = config["dm"]["N2"]
    y = (np.random.default_rng(0).random((R, C)) < 0.2).astype(np.float32)
    dev = torch.device("cuda:0")
    Xd, idsd, qd, road, yd = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (X, ids, q, roa.astype(np.int32), y)]
    lr = 1e-5

    tr = Trainer(config, sd, lr=lr)
    parent = ParentTrainer(a.parent_lib, config, sd, lr) if a.parent_lib else None
    out = [torch.empty((R, C), device=dev) for _ in range(3)]

    def module():
        m = Model(config)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=False)
        m.to(dev)
        return m, torch.optim.Adam(m.parameters(), lr=lr), 0.5 * torch.ones(C, device=dev)

    mods = {"c": module(), "d": module()}
    parts = {"c": [], "d": []}

    def nn_step(key, step, events=False):
        m, opt, pos = mods[key]
        Xs = Xd.detach().clone().requires_grad_(key == "d")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if events else None
        opt.zero_grad()
        if ev: ev[0].record()
        z = m(Xs, idsd, qd, (road, R))                      # torch.cat + set_weights + pesto_train_forward
        if ev: ev[1].record()
        loss = torch.sum(reference_loss(z, yd, pos, step))
        if ev: ev[2].record()
        loss.backward()                                      # pesto_train_backward + the backward of torch.cat
        if ev: ev[3].record()
        opt.step()
        if ev:
            ev[4].record()
            torch.cuda.synchronize()
            parts[key].append([ev[i].elapsed_time(ev[i + 1]) for i in range(4)])

    variants = {"b": lambda s: tr.train_step(Xd, idsd, qd, (road, R), yd), "c": lambda s: nn_step("c", s), "d": lambda s: nn_step("d", s)}
    if parent:
        variants = {"a": lambda s: parent.train_step(Xd, idsd, qd, road, R, yd, out), **variants}
    wall = {k: [] for k in variants}
    for step in range(1, a.warmup + a.steps + 1):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(step)
            torch.cuda.synchronize()
            if step > a.warmup:
                wall[k].append((time.perf_counter() - t0) * 1e3)
    # second pass: where c and d spend their step. torch.cat alone (forward + backward of the flat tensor) is timed on the side
    for step in range(a.warmup + a.steps + 1, a.warmup + a.steps + 11):
        nn_step("c", step, events=True)
        nn_step("d", step, events=True)
    m = mods["c"][0]
    cat_ms = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        m.zero_grad()
        e0.record()
        flat = torch.cat([p.reshape(-1) for p in m.parameters()])
        flat.backward(flat.detach())
        e1.record()
        torch.cuda.synchronize()
        cat_ms.append(e0.elapsed_time(e1))

    res = {"what": "nn_step", "config": a.config, "weights": weights, "atoms": int(X.shape[0]), "residues": int(R), "steps": a.steps, "warmup": a.warmup,
           "step_wall_ms": {k: stats(v) for k, v in wall.items()}, "parent_lib": bool(parent),
           "parts_ms": {k: dict(zip(("forward", "loss", "backward", "adam"), np.median(np.asarray(v), 0).tolist())) for k, v in parts.items()},
           "torch_cat_fwd_bwd_ms": stats(cat_ms), "device": torch.cuda.get_device_name(0)}
    if parent:
        sa, sb = res["step_wall_ms"]["a"], res["step_wall_ms"]["b"]
        res["b_within_spread_of_a"] = bool(sa["min"] <= sb["median"] <= sa["max"])
        parent.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
