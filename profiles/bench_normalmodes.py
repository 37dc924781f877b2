#!/usr/bin/env python3
"""Timing of pesto_amd.normalmodes (pesto_enm.hip) beside the routes a user has without it.
usage: python profiles/bench_normalmodes.py [out.json]   (on the GPU box; default profiles/out/normalmodes.json)

Shapes: the 253 CA atoms of tests/golden/io_1thf_D.npz, and seeded self-avoiding 3.8 A chains of 1,000 and 10,000 nodes; the ANM at
cut-off 15 A, gamma 1, p 0, the 20 lowest modes at tol 1e-10. Legs, whole calls on ROCm tensors: network (two calls: the count, then the
fill), hessian where (3n)^2 fits, anm, anm with max_iter = 1 (the list, R, the start block and one Rayleigh-Ritz step), gnm at cut-off
10. Baselines on the same box wherever (3n)^2 <= 2^27: NumPy eigh of the dense Hessian on the host (the thread count is the
environment's; the Hessian itself is not in the time) and torch.linalg.eigh of it on the GPU in float64.
Clock: device events around one whole call (every call of the package synchronises its stream, so the host's enqueue time is inside);
wall clock for the host leg; per call, the median and the range of REPEATS measurements after WARM warm-up ones, the legs of a shape
interleaved. The operator's time is not measured by a kernel trace here but bounded from above: (anm - anm with max_iter 1) / (applies -
1) charges every further Rayleigh-Ritz step, projection and orthonormalisation to the filter's launches. Against it stand the bytes one
application moves: the list (36 bytes an entry through the scalar unit), 3 x 512 bytes gathered per entry (the neighbour's values of
the 64 columns, mostly from L2: the block of n = 10,000 is 15 MB) and the block read twice and written once."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from pesto_amd import normalmodes as nm  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "out", "normalmodes.json")
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
dev = torch.device("cuda:0")
REPEATS, WARM, K, CUTOFF = 5, 1, 20, 15.0


def chain(n, seed, step=3.8, clash=3.7):
    """the generator of tests/test_normalmodes_fixture.py"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 3))
    i = 1
    while i < n:
        u = rng.standard_normal(3)
        p = x[i - 1] + step * u / np.linalg.norm(u)
        if i < 2 or np.linalg.norm(x[:i - 1] - p, axis=1).min() >= clash:
            x[i] = p
            i += 1
    return np.ascontiguousarray(x.astype(np.float32))


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wall_time(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def timed(legs, repeats, warm):
    for _ in range(warm):
        for clock, fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in legs}
    for _ in range(repeats):
        for name, (clock, fn) in legs.items():
            ts[name].append(clock(fn))
    return {name: {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)), "calls": len(t)} for name, t in ts.items()}


def source_hash():
    h = hashlib.sha256()
    for rel in ("pesto_amd/csrc/pesto_enm.hip", "pesto_amd/csrc/pesto_ritz.h", "pesto_amd/csrc/pesto_cellgrid.h", "pesto_amd/normalmodes.py",
                "profiles/bench_normalmodes.py"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "io_1thf_D.npz"))
    shapes = [("1thf_D", np.ascontiguousarray(g["final_xyz"][np.char.strip(g["final_name"].astype(str)) == "CA"], np.float32)),
              ("chain_1000", chain(1000, 71)), ("chain_10000", chain(10000, 72))]
    result = {"device": torch.cuda.get_device_name(0), "source": source_hash(), "threads": os.environ.get("OMP_NUM_THREADS"), "k": K, "cutoff": CUTOFF,
              "shapes": []}
    for name, x in shapes:
        n = len(x)
        d = torch.from_numpy(x).to(dev)
        dense = (3 * n) ** 2 <= nm.MAX_DENSE
        res = nm.anm(d, n_modes=K, cutoff=CUTOFF, scale=1.0)
        one = nm.anm(d, n_modes=K, cutoff=CUTOFF, scale=1.0, max_iter=1)
        gres = nm.gnm(d, n_modes=K, cutoff=10.0, scale=1.0)
        entry = {"name": name, "n": n, "n_springs": res.n_springs, "bound": res.bound, "iterations": res.iterations, "applies": res.applies,
                 "converged": res.converged, "worst_residual_over_b": float(res.residuals.max()) / res.bound, "n_zero": res.n_zero,
                 "lowest_over_b": float(res.eigenvalues[0]) / res.bound,
                 "gnm": {"iterations": gres.iterations, "applies": gres.applies, "converged": gres.converged}}
        gpu = {"network": (event_time, lambda: nm.network(d, cutoff=CUTOFF, scale=1.0)),
               "anm_k20": (event_time, lambda: nm.anm(d, n_modes=K, cutoff=CUTOFF, scale=1.0)),
               "anm_k20_one_step": (event_time, lambda: nm.anm(d, n_modes=K, cutoff=CUTOFF, scale=1.0, max_iter=1)),
               "gnm_k20": (event_time, lambda: nm.gnm(d, n_modes=K, cutoff=10.0, scale=1.0))}
        cpu = {}
        if dense:
            H = nm.hessian(d, cutoff=CUTOFF, scale=1.0)
            Hh = H.cpu().numpy()
            lam = np.linalg.eigvalsh(Hh)
            lam = lam[lam > 1e-10 * res.bound][:K]
            entry["eig_rel_err_vs_eigh"] = float(np.abs(res.eigenvalues.cpu().numpy() - lam).max() / res.bound) if res.n_zero == 0 else None
            gpu["hessian"] = (event_time, lambda: nm.hessian(d, cutoff=CUTOFF, scale=1.0))
            gpu["torch_eigh_of_hessian"] = (event_time, lambda: torch.linalg.eigh(H))
            cpu["numpy_eigh_of_hessian"] = (wall_time, lambda: np.linalg.eigh(Hh))
        t = timed(gpu, REPEATS, WARM)
        t.update(timed(cpu, 2, 0))
        entry["legs"] = t
        if res.applies > 1:
            step_ms = (t["anm_k20"]["median_ms"] - t["anm_k20_one_step"]["median_ms"]) / (res.applies - one.applies)
            entries = 2 * res.n_springs
            gathered, listed, block = entries * 3 * 512, entries * 36, 3 * (3 * n * 64 * 8)
            entry["apply"] = {"ms_upper_bound": step_ms, "bytes_gathered": gathered, "bytes_list": listed, "bytes_block": block,
                              "gb_per_s_lower_bound": (gathered + listed + block) / (step_ms * 1e-3) / 1e9}
        print(json.dumps(entry), flush=True)
        result["shapes"].append(entry)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
