#!/usr/bin/env python3
"""Timing of pesto_amd.dynamics (pesto_dynamics.hip) on seeded frames, beside the routes a user has without it.
usage: python profiles/bench_dynamics.py [out.json] [--trace | --kernel-stats=stats.csv]   (on the GPU box; default profiles/out/dynamics.json)

Shapes (F, n) = (512, 290), (4096, 290), (4096, 1000): frames of one structure with 50 collective modes of decaying amplitude
(0.15 nm x 0.85^i) over thermal noise of 0.01 nm. Legs, whole calls on ROCm tensors: fluctuations, covariance, pca with 10 components.
Baselines on the same box: NumPy float64 on the host (mean, covariance by one matrix product, LAPACK eigh; the thread count is the
environment's), torch.cov + torch.linalg.eigh and torch.pca_lowrank(q = 10, niter = 2) on the GPU in float64 (the cast from float32
inside the timed region, as a user would pay it).
Clock: device events around a batch of BATCH whole calls for the GPU legs shorter than a millisecond (one call between two events would
mostly time the events and the enqueue), around one call for the others (every call of the package synchronises its stream, so the
host's enqueue time is inside); wall clock for the host legs; per call, the median and the range of REPEATS measurements after WARM
warm-up ones, the legs of a shape interleaved. The Gram product's arithmetic as executed: 2 * 64 * 64 * 16 ceil(F / 16) flops per 64 x 64
tile, upper tiles only, the padding counted. Its rate is given twice: against the whole covariance call (pack, mean, product, mirror),
and against the kernel alone from a kernel trace of a SEPARATE run: --trace makes a few covariance calls per shape and times nothing
(run it under the profiler's kernel trace); --kernel-stats=<the trace's kernel csv> then adds the Gram kernel's own time per shape
(its launches in trace order, TRACE_CALLS per shape) to an existing out.json. pca also reports the most sweeps any of its 64 x 64
Jacobi runs took."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch  # noqa: E402

from pesto_amd import dynamics as dy  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
trace = "--trace" in sys.argv
kernel_stats = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--kernel-stats=")), None)
BATCH, TRACE_CALLS = 20, 5
out_path = args[0] if args else os.path.join(ROOT, "profiles", "out", "dynamics.json")
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
dev = torch.device("cuda:0")
REPEATS, WARM = 7, 2
SIZES = [(512, 290), (4096, 290), (4096, 1000)]
K = 10


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def batch_time(fn):
    """per call, BATCH calls between two events"""
    def many():
        for _ in range(BATCH):
            fn()
    return event_time(many) / BATCH


def wall_time(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "calls": len(ts)}


def timed(legs, repeats, warm):
    """legs: name -> (clock, fn); interleaved: every repeat runs each of them once"""
    for _ in range(warm):
        for clock, fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in legs}
    for _ in range(repeats):
        for name, (clock, fn) in legs.items():
            ts[name].append(clock(fn))
    return {name: stats(t) for name, t in ts.items()}


def frames(F, n, seed):
    rng = np.random.default_rng(seed)
    m = 3 * n
    modes = np.linalg.qr(rng.standard_normal((m, 50)))[0]
    x = rng.normal(0.0, 1.0, (1, m)) + (rng.standard_normal((F, 50)) * (0.15 * 0.85 ** np.arange(50))) @ modes.T + 0.01 * rng.standard_normal((F, m))
    return x.astype(np.float32).reshape(F, n, 3)


def gram_flops(F, n):
    T = -(-3 * n // 64)
    return T * (T + 1) // 2 * 2 * 64 * 64 * 16 * -(-F // 16)


def source_hash():
    h = hashlib.sha256()
    for rel in ("pesto_amd/csrc/pesto_dynamics.hip", "pesto_amd/csrc/pesto_geom.h", "pesto_amd/csrc/pesto_mma64.h", "pesto_amd/dynamics.py", "profiles/bench_dynamics.py"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def trace_run():
    for i, (F, n) in enumerate(SIZES):
        d = torch.from_numpy(frames(F, n, 40 + i)).to(dev)
        for _ in range(TRACE_CALLS):
            dy.covariance(d)
    torch.cuda.synchronize()


def add_kernel_stats(path):
    """the Gram kernel's own time from the kernel csv of a --trace run: its launches in order, TRACE_CALLS per shape"""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "k_dyn_mma" in r["Kernel_Name"] and "0" in r["Kernel_Name"].split("k_dyn_mma")[1][:6]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == TRACE_CALLS * len(SIZES), len(rows)
    result = json.load(open(out_path))
    for i, entry in enumerate(result["shapes"]):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[TRACE_CALLS * i:TRACE_CALLS * (i + 1)]]
        entry["gram_kernel_us"] = {"median": float(np.median(us)), "min": min(us), "max": max(us), "launches": len(us)}
        entry["gram_tflops_kernel"] = entry["gram_flops"] / (float(np.median(us)) * 1e-6) / 1e12
        print(entry["F"], entry["n"], entry["gram_kernel_us"], entry["gram_tflops_kernel"])
    json.dump(result, open(out_path, "w"), indent=1)


def main():
    if trace:
        return trace_run()
    if kernel_stats:
        return add_kernel_stats(kernel_stats)
    result = {"device": torch.cuda.get_device_name(0), "source": source_hash(), "threads": os.environ.get("OMP_NUM_THREADS"), "k": K, "shapes": []}
    for i, (F, n) in enumerate(SIZES):
        x = frames(F, n, 40 + i)
        d = torch.from_numpy(x).to(dev)
        res, sweeps = dy._pca(d, None, K, 10.0, 1, 1e-9, 64, None, None)
        lam64 = np.linalg.eigvalsh(100.0 * np.cov(x.reshape(F, -1).astype(np.float64).T))[::-1][:K]
        big = 3 * n > 1500

        def numpy_cov():
            a = x.reshape(F, -1).astype(np.float64)
            a -= a.mean(0)
            return 100.0 * (a.T @ a) / (F - 1)

        def torch_cov_eigh():
            c = torch.cov(d.reshape(F, -1).double().T) * 100.0
            return torch.linalg.eigh(c)

        gpu = {
            "fluctuations": (batch_time, lambda: dy.fluctuations(d)),
            "covariance": (batch_time, lambda: dy.covariance(d)),
            "pca_k10": (event_time, lambda: dy.pca(d, n_components=K)),
            "torch_cov": (batch_time, lambda: torch.cov(d.reshape(F, -1).double().T)),
            "torch_cov_eigh": (event_time, torch_cov_eigh),
            "torch_pca_lowrank": (event_time, lambda: torch.pca_lowrank(d.reshape(F, -1).double(), q=K, center=True, niter=2)),
        }
        cpu = {
            "numpy_fluctuations": (wall_time, lambda: (x.astype(np.float64).mean(0), x.astype(np.float64).std(0))),
            "numpy_cov": (wall_time, numpy_cov),
            "numpy_cov_eigh": (wall_time, lambda: np.linalg.eigh(numpy_cov())),
        }
        t = timed(gpu, 3 if big else REPEATS, 1 if big else WARM)
        t.update(timed(cpu, 1 if big else 3, 0 if big else 1))
        entry = {"F": F, "n": n, "legs": t, "pca_iterations": res.iterations, "pca_converged": res.converged, "pca_max_jacobi_sweeps": sweeps,
                 "pca_eig_rel_err": float(np.abs(res.eigenvalues.cpu().numpy() - lam64).max() / lam64[0]),
                 "gram_flops": gram_flops(F, n),
                 "gram_tflops_whole_call": gram_flops(F, n) / (t["covariance"]["median_ms"] * 1e-3) / 1e12}
        print(json.dumps(entry), flush=True)
        result["shapes"].append(entry)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
