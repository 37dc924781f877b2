#!/usr/bin/env python3
"""Timing of pesto_amd.surface (pesto_surface.hip) on the stored chains of tests/golden/surface.npz, beside the host restatement.
usage: python profiles/bench_surface.py [out.txt] [--trace]   (on the GPU box; default profiles/out/surface_bench.txt)

Two inputs, on ROCm tensors: one stored chain (the first of the fixture, SPPIDER's atoms), and the three stored chains repeated to 53
structures as one batch - the size of the reference's benchmark. Legs: nearest_atoms; vertex_areas_fixed followed by residue_surface;
benchmark_surfaces (the whole driver with its four ranking calls). nearest_atoms is also timed with other slab sizes, one slab per
structure among them (no split: every vertex tile walks all atoms), to see whether the split is worth its merge.
Clock: device events around one whole call (every call synchronises its stream, so the host's enqueue time is inside), the median and the
range of REPEATS calls after WARM warm-up calls. Beside them the host restatement - the test's yardstick, NOT the reference, whose pyflann
and pymesh cannot be run here: scipy's cKDTree (build and query, at most 16 threads) for the nearest atom, np.bincount for the areas and
the residue sums - on a host clock. With --trace nothing is timed: a few calls of every leg for a kernel trace taken by a profiler around
this script."""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402
from scipy.spatial import cKDTree  # noqa: E402

import test_surface_fixture as T  # noqa: E402
from pesto_amd import surface as S  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
trace = "--trace" in sys.argv
out_path = args[0] if args else os.path.join(ROOT, "profiles", "out", "surface_bench.txt")
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
lines = []
dev = torch.device("cuda:0")
REPEATS, WARM, THREADS = 9, 2, 16


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    """(median, min, max) seconds of one call from device events"""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def host_timed(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), min(ts), max(ts)


def ms(t):
    return f"{1e3 * t[0]:9.3f} ms [{1e3 * t[1]:.3f}, {1e3 * t[2]:.3f}]"


def source_hash():
    h = hashlib.sha256()
    for rel in ("pesto_amd/csrc/pesto_surface.hip", "pesto_amd/csrc/pesto_rank.hip", "pesto_amd/csrc/pesto_scan.h", "pesto_amd/surface.py",
                "profiles/bench_surface.py"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def host_nearest(b):
    out = []
    for s in range(len(b["vo"]) - 1):
        v, x = b["v64"][b["vo"][s]:b["vo"][s + 1]], b["x64"][b["ao"][s]:b["ao"][s + 1]]
        out.append(cKDTree(x).query(v, k=1, workers=THREADS)[1] + b["ao"][s])
    return np.concatenate(out)


def host_tables(b, nearest):
    v, f = b["v64"], b["faces_global"]
    u, w = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    third = 0.5 * np.linalg.norm(np.cross(u, w), axis=1) / 3.0
    area = sum(np.bincount(f[:, c], third, v.shape[0]) for c in range(3))
    res = b["res_of_atom"][nearest]
    R = int(b["ro"][-1])
    n, a, ia = np.bincount(res, minlength=R), np.bincount(res, area, R), np.bincount(res, area * b["iface"], R)
    with np.errstate(invalid="ignore", divide="ignore"):
        return n, a, ia, (ia > 5.0) & (ia / a > 0.04)


def batch_of(names):
    g = np.load(os.path.join(ROOT, "tests", "golden", "surface.npz"))
    chains = {n: T.stored_chain(g, n) for n in set(names)}
    items = []
    for n in names:
        c = chains[n]
        a = c["sppider"]
        p_atom, p_res, valid = T.ca_prediction_def(a["bfactor"], a["ca_index"])
        items.append({"vertices": c["vertices"], "faces": c["faces"], "iface": c["iface"], "xyz": a["xyz"], "atom_residue": a["atom_residue"],
                      "n_residues": a["ca_index"].size, "p_atom": p_atom, "p_res": p_res, "valid": valid})
    vo, ao = S._lib.offsets(it["vertices"].shape[0] for it in items), S._lib.offsets(it["xyz"].shape[0] for it in items)
    fo, ro = S._lib.offsets(it["faces"].shape[0] for it in items), S._lib.offsets(it["n_residues"] for it in items)
    cat = lambda k: np.concatenate([it[k] for it in items])          # noqa: E731
    b = {"items": [{k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in it.items()} for it in items],
         "vo": vo, "ao": ao, "fo": fo, "ro": ro, "v": cat("vertices"), "x": cat("xyz"), "f": cat("faces"), "iface": cat("iface"), "ar": cat("atom_residue")}
    b["v64"], b["x64"] = b["v"].astype(np.float64), b["x"].astype(np.float64)
    b["faces_global"] = np.concatenate([it["faces"].astype(np.int64) + vo[s] for s, it in enumerate(items)])
    b["res_of_atom"] = np.concatenate([it["atom_residue"].astype(np.int64) + ro[s] for s, it in enumerate(items)])
    for k in ("v", "x", "f", "iface", "ar"):
        b["d_" + k] = torch.from_numpy(np.ascontiguousarray(b[k])).to(dev)
    return b


def legs(b):
    near = lambda slab=None: S.nearest_atoms(b["d_v"], b["d_x"], b["vo"], b["ao"], slab=slab)          # noqa: E731
    nearest = near()[0]

    def tables():
        area = S.vertex_areas_fixed(b["d_v"], b["d_f"], b["vo"], b["fo"])
        return S.residue_surface(nearest, b["d_ar"], area, b["d_iface"], None, b["vo"], b["ao"], b["ro"])

    return near, tables, lambda: S.benchmark_surfaces(b["items"])


torch.set_num_threads(THREADS)
names = list(T.CHAINS)
single, batch = batch_of(names[:1]), batch_of([names[i % 3] for i in range(53)])
if trace:
    for b in (single, batch):
        near, tables, driver = legs(b)
        for _ in range(3):
            near(), tables(), driver()
        if b is single:
            for _ in range(3):
                near(2 ** 20)
    torch.cuda.synchronize()
    sys.exit(0)

say(f"device {torch.cuda.get_device_name(0)}; source {source_hash()}; clock: device events around one whole call on ROCm tensors (every call "
    f"synchronises its stream), median [min, max] of {REPEATS} after {WARM} warm-up calls; host rows: time.perf_counter, {THREADS} threads at most")
for label, b in (("one chain", single), ("53 structures", batch)):
    V, N, F, R = (int(b[k][-1]) for k in ("vo", "ao", "fo", "ro"))
    near, tables, driver = legs(b)
    # what is timed is what the tests check: the host restatement's nearest atoms are the device's up to float64 against float32 near-ties
    got, want = near()[0].cpu().numpy(), host_nearest(b)
    say(f"{label}: S = {len(b['vo']) - 1}, V = {V}, N = {N}, F = {F}, R = {R}; pairs in a structure {sum(int(a) * int(c) for a, c in zip(np.diff(b['vo']), np.diff(b['ao']))) / 1e6:.1f} M; "
        f"{int((got != want).sum())} of {V} nearest atoms differ between the float32 definition and the float64 k-d tree")
    t_near, t_tab, t_drv = timed(near), timed(tables), timed(driver)
    say(f"    nearest_atoms                         {ms(t_near)}   2 kernel launches + 1 memset")
    say(f"    vertex_areas_fixed + residue_surface  {ms(t_tab)}   3 kernel launches + 6 memsets, two calls")
    say(f"    benchmark_surfaces                    {ms(t_drv)}   9 kernel launches in five calls of this group, and four ranking.scores calls")
    h_near, h_tab = host_timed(lambda: host_nearest(b)), host_timed(lambda: host_tables(b, want))
    say(f"    host: cKDTree build + query           {ms(h_near)}")
    say(f"    host: np.bincount areas + residues    {ms(h_tab)}")
    for slab in (S.ATOM_TILE, S.SLAB, 2 * S.SLAB, 4 * S.SLAB, 2 ** 20):
        n_wg = sum(-(-int(v) // S.VERTEX_TILE) * -(-int(a) // slab) for v, a in zip(np.diff(b["vo"]), np.diff(b["ao"])))
        say(f"    nearest_atoms, slab {slab:>7d}           {ms(timed(lambda: near(slab)))}   {n_wg} workgroups{' (no split)' if slab == 2 ** 20 else ''}")
open(out_path, "w").write("\n".join(lines) + "\n")
