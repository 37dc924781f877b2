#!/usr/bin/env python3
"""Timing of pesto_amd.clustering (pesto_cluster.hip) on seeded frames, beside the only route the package had before it.
usage: python profiles/bench_clustering.py [out.json] [--trace]   (on the GPU box; default profiles/out/clustering.json)

matrix      pairwise_rmsd, self form, at (F, n) = (512, 290), (512, 2030), (4096, 290) on ROCm tensors. The comparator - the yardstick, not
            the new code - is F calls of trajectory.rmsd, frame i the reference of call i (each call refits every frame with one
            workgroup per frame and synchronises). Both are timed in this process, interleaved call by call.
split       the same three sizes with a rectangular call (both pack launches) and with n = 4, where the product is 1 MFMA step per tile
            and the time is the epilogue's (the Jacobi finish of every pair); the kernels' own times come from a kernel trace of a
            separate run (--trace: a few calls of every leg, nothing timed). The covariance kernel's arithmetic as executed:
            2 * 64 * 64 * n_pad flops per 16 x 16-frame tile, the ones row and the zero padding counted, upper tiles only in the self form.
clustering  gromos_clusters at F = 4096 on a seeded symmetric matrix: cutoff at the median entry, and below the smallest (every frame its
            own cluster: the singleton shortcut).
Clock: device events around one whole call (every call synchronises its stream, so the host's enqueue time is inside), the median and the
range of REPEATS calls after WARM warm-up calls."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch  # noqa: E402

from pesto_amd import clustering as C  # noqa: E402
from pesto_amd import trajectory as T  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
trace = "--trace" in sys.argv
out_path = args[0] if args else os.path.join(ROOT, "profiles", "out", "clustering.json")
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
dev = torch.device("cuda:0")
REPEATS, WARM = 7, 2
SIZES = [(512, 290), (512, 2030), (4096, 290)]


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "calls": len(ts)}


def timed(*fns, repeats=REPEATS, warm=WARM):
    """the legs interleaved: every repeat runs each of them once"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            ts[k].append(event_time(fn))
    return [stats(t) for t in ts]


def frames(F, n, seed):
    rng = np.random.default_rng(seed)
    base = rng.normal(0.0, 1.0, (1, n, 3))
    return torch.from_numpy((base + rng.normal(0.0, 0.15, (F, n, 3))).astype(np.float32)).to(dev)


def source_hash():
    h = hashlib.sha256()
    for rel in ("pesto_amd/csrc/pesto_cluster.hip", "pesto_amd/csrc/pesto_geom.h", "pesto_amd/csrc/pesto_mma64.h", "pesto_amd/clustering.py", "profiles/bench_clustering.py"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def cov_flops(F, n, self_form=True):
    tiles_side = -(-F // 16)
    tiles = tiles_side * (tiles_side + 1) // 2 if self_form else tiles_side * tiles_side
    return 2.0 * 64 * 64 * (-(-n // 4) * 4) * tiles


def old_route(x):
    for i in range(x.shape[0]):
        T.rmsd(x[i:i + 1], x)


def symmetric_matrix(F, seed):
    rng = np.random.default_rng(seed)
    U = np.triu(rng.uniform(0.5, 2.0, (F, F)).astype(np.float32), 1)
    return torch.from_numpy(U + U.T).to(dev)


if trace:
    for F, n in SIZES:
        x = frames(F, n, F + n)
        for _ in range(3):
            C.pairwise_rmsd(x)
            C.pairwise_rmsd(x[:, :4].contiguous())
    D = symmetric_matrix(4096, 1)
    for _ in range(3):
        C.gromos_clusters(D, float(D.median()))
        C.gromos_clusters(D, 0.25)
    torch.cuda.synchronize()
    sys.exit(0)

out = {"device": torch.cuda.get_device_name(0), "source": source_hash(),
       "clock": f"device events around one whole call on ROCm tensors, median [min, max] of {REPEATS} calls after {WARM} warm-up calls, legs interleaved",
       "matrix": [], "split": [], "clustering": []}
for F, n in SIZES:
    x = frames(F, n, F + n)
    few = 3 if F > 1000 else REPEATS
    new, old = timed(lambda: C.pairwise_rmsd(x), lambda: old_route(x), repeats=few, warm=1)
    row = {"F": F, "n": n, "pairwise_rmsd_self": new, "F_calls_of_trajectory_rmsd": old, "ratio_of_medians": old["median_ms"] / new["median_ms"]}
    # what is timed is what the tests check: row 0 of the matrix against the old route's call 0
    row["max_abs_difference_row0"] = float((C.pairwise_rmsd(x)[0] - T.rmsd(x[:1], x)).abs().max())
    out["matrix"].append(row)
    print(json.dumps(row), flush=True)
    y = x.clone()
    x4 = x[:, :4].contiguous()
    self_form, rect, finish = timed(lambda: C.pairwise_rmsd(x), lambda: C.pairwise_rmsd(x, y), lambda: C.pairwise_rmsd(x4))
    row = {"F": F, "n": n, "self": self_form, "rectangular": rect, "self_n4_finish_bound": finish,
           "cov_flops_self": cov_flops(F, n), "cov_flops_rectangular": cov_flops(F, n, False),
           "tflops_whole_call_self": cov_flops(F, n) / self_form["median_ms"] / 1e9,
           "tflops_whole_call_rectangular": cov_flops(F, n, False) / rect["median_ms"] / 1e9}
    out["split"].append(row)
    print(json.dumps(row), flush=True)
D = symmetric_matrix(4096, 1)
vals = D[torch.triu(torch.ones_like(D, dtype=torch.bool), 1)]
for label, cut in (("median", float(vals.median())), ("below_minimum", float(vals.min()) / 2)):
    t, = timed(lambda: C.gromos_clusters(D, cut))
    labels, centers, sizes = C.gromos_clusters(D, cut)
    row = {"F": 4096, "cutoff": label, "value": cut, "clusters": int(centers.numel()), "largest": int(sizes[0]), "gromos_clusters": t}
    out["clustering"].append(row)
    print(json.dumps(row), flush=True)
json.dump(out, open(out_path, "w"), indent=1)
