#!/usr/bin/env python3
"""Timing of pesto_amd.peaks (pesto_peaks.hip) on seeded blobs. No earlier route exists in the package, so there is no ratio; the NumPy
definitions of tests/test_peaks_fixture.py are timed on the host at the small shapes as the tests' yardstick only.
usage: python profiles/bench_peaks.py [out.json] [--trace]   (on the GPU box; default profiles/out/peaks.json)

points      distance_quantile (pdc = 2) and density_peaks (d_c given, n_clusters = 3) under both kernels at (n, d) = (512, 3), (4096, 3),
            (65536, 3) on ROCm tensors: three Gaussian blobs of unit variance around centres drawn at scale 6
matrix      the same at n = 4096 over the float32 distance matrix of those points
centers     interface_centers at (F, R) = (512, 290) and (4096, 290)
yardstick   pdist32 + dc_of, peaks_def under both kernels and centers_def in NumPy on the host, at n = 512 and (F, R) = (512, 290)
--trace     a few calls of every leg, nothing timed: for a kernel trace in a separate run
pairs       the pairs an all-pairs pass evaluates: n (n - 1) / 2 + the masked half of the diagonal tiles for a histogram pass (it starts
            each row block at its own tile), n (n - 1) for the density, nearest and border passes
Clock: device events around one whole call (every call synchronises its stream, so the host's enqueue time is inside), the median and the
range of REPEATS calls after WARM warm-up calls, the legs interleaved."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from pesto_amd import peaks as K  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
trace = "--trace" in sys.argv
out_path = args[0] if args else os.path.join(ROOT, "profiles", "out", "peaks.json")
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
dev = torch.device("cuda:0")
REPEATS, WARM = 7, 2
POINTS = [(512, 3), (4096, 3), (65536, 3)]
CENTERS = [(512, 290), (4096, 290)]


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


def host_time(fn, repeats=3):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def blobs(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 6.0, (3, d))
    return (centres[rng.integers(0, 3, n)] + rng.normal(0.0, 1.0, (n, d))).astype(np.float32)


def matrix_of(x):
    """the float32 distance matrix of device points in pdist32's operations (a multiply and an add of one expression are not fused by torch)"""
    s = None
    for c in range(x.shape[1]):
        dx = x[:, None, c] - x[None, :, c]
        s = dx * dx if s is None else s + dx * dx
    return torch.sqrt(s)


def frames(F, R, seed):
    rng = np.random.default_rng(seed)
    Xp = (rng.normal(0.0, 1.5, (1, R, 3)) + rng.normal(0.0, 0.15, (F, R, 3))).astype(np.float32)
    P = rng.uniform(0.0, 1.0, (F, R)).astype(np.float32)
    return torch.from_numpy(Xp).to(dev), torch.from_numpy(P).to(dev)


def source_hash():
    h = hashlib.sha256()
    for rel in ("pesto_amd/csrc/pesto_peaks.hip", "pesto_amd/csrc/pesto_geom.h", "pesto_amd/csrc/pesto_call.h", "pesto_amd/peaks.py", "profiles/bench_peaks.py"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def legs(x=None, D=None):
    src = dict(X=x) if D is None else dict(D=D)
    dc = K.distance_quantile(pdc=2.0, **src)
    return dc, [lambda: K.distance_quantile(pdc=2.0, **src),
                lambda: K.density_peaks(dc=dc, kernel="cutoff", n_clusters=3, **src),
                lambda: K.density_peaks(dc=dc, kernel="gaussian", n_clusters=3, **src)]


if trace:
    for n, d in POINTS:
        x = torch.from_numpy(blobs(n, d, n + d)).to(dev)
        for fn in legs(x)[1]:
            for _ in range(2):
                fn()
    D = matrix_of(torch.from_numpy(blobs(4096, 3, 4099)).to(dev))
    for fn in legs(D=D)[1]:
        for _ in range(2):
            fn()
    for F, R in CENTERS:
        Xp, P = frames(F, R, F + R)
        for _ in range(2):
            K.interface_centers(Xp, P, 0.5)
    torch.cuda.synchronize()
    sys.exit(0)

out = {"device": torch.cuda.get_device_name(0), "source": source_hash(),
       "clock": f"device events around one whole call on ROCm tensors, median [min, max] of {REPEATS} calls after {WARM} warm-up calls, legs interleaved",
       "points": [], "matrix": [], "centers": [], "yardstick_numpy_host": []}
for n, d in POINTS:
    x = torch.from_numpy(blobs(n, d, n + d)).to(dev)
    dc, fns = legs(x)
    few = 3 if n > 10000 else REPEATS
    q, cut, gau = timed(*fns, repeats=few, warm=1 if n > 10000 else WARM)
    res = K.density_peaks(x, dc=dc, kernel="gaussian", n_clusters=3)
    row = {"n": n, "d": d, "dc": dc, "pairs_i_lt_j": n * (n - 1) // 2, "distance_quantile": q, "density_peaks_cutoff": cut, "density_peaks_gaussian": gau,
           "sizes_gaussian": res.sizes.tolist(), "halo_gaussian": int(res.halo.sum()),
           "gpairs_per_s_quantile_3_passes": 3 * (n * (n - 1) / 2) / q["median_ms"] / 1e6,
           "gpairs_per_s_cutoff_3_passes": 3 * n * (n - 1) / cut["median_ms"] / 1e6,
           "gpairs_per_s_gaussian_3_passes": 3 * n * (n - 1) / gau["median_ms"] / 1e6}
    out["points"].append(row)
    print(json.dumps(row), flush=True)
x = torch.from_numpy(blobs(4096, 3, 4099)).to(dev)
D = matrix_of(x)
dc, fns = legs(D=D)
q, cut, gau = timed(*fns)
same = K.density_peaks(x, dc=dc, kernel="gaussian", n_clusters=3)
res = K.density_peaks(D=D, dc=dc, kernel="gaussian", n_clusters=3)
row = {"n": 4096, "dc": dc, "distance_quantile": q, "density_peaks_cutoff": cut, "density_peaks_gaussian": gau,
       "equals_the_points_form": bool(dc == K.distance_quantile(x, pdc=2.0) and all(torch.equal(a, b) for a, b in zip(same[1:], res[1:])))}
out["matrix"].append(row)
print(json.dumps(row), flush=True)
for F, R in CENTERS:
    Xp, P = frames(F, R, F + R)
    t, = timed(lambda: K.interface_centers(Xp, P, 0.5))
    row = {"F": F, "R": R, "interface_centers": t, "bytes_read": F * R * 16 * 2, "gbytes_per_s_whole_call": F * R * 32 / t["median_ms"] / 1e6}
    out["centers"].append(row)
    print(json.dumps(row), flush=True)
# the tests' yardstick, on the host: not a comparison of routes
from test_peaks_fixture import centers_def, dc_of, pdist32, peaks_def, quantile_rank  # noqa: E402
xs = blobs(512, 3, 515)
Ds = pdist32(xs)
dcs = dc_of(Ds, quantile_rank(512, 2.0))
Xp, P = frames(512, 290, 802)
Xh, Th = Xp.cpu().numpy(), (P.cpu().numpy() > np.float32(0.5)).astype(np.float32)
row = {"n": 512, "d": 3, "pdist32_and_dc_of": host_time(lambda: dc_of(pdist32(xs), quantile_rank(512, 2.0))),
       "peaks_def_cutoff": host_time(lambda: peaks_def(Ds, dcs, "cutoff", n_clusters=3)),
       "peaks_def_gaussian": host_time(lambda: peaks_def(Ds, dcs, "gaussian", n_clusters=3)),
       "centers_def_512_290": host_time(lambda: centers_def(Xh, Th), repeats=1)}
out["yardstick_numpy_host"].append(row)
print(json.dumps(row), flush=True)
json.dump(out, open(out_path, "w"), indent=1)
