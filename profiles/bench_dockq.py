#!/usr/bin/env python3
"""Timing of pesto_amd.dockq (pesto_dockq.hip) against the composed route through the package's earlier public functions, on a seeded
complex of two subunits of N / 2 atoms each (residues of 8 atoms, the first 4 their backbone; the last residue of a side takes the rest) and F decoys of it.
usage: python profiles/bench_dockq.py [out.json] [--trace]   (on the GPU box; default profiles/out/dockq.json)

dockq       dockq(ref, xyz, ids_R, ids_L, res_of_atom, bb) on ROCm tensors: the set-up on the reference frame (native pairs, interface,
            the atoms' order by residue) and the one launch over the decoys, all inside the timed call
composed    the same fnat and irmsd by the functions that existed before: residue_contact_maps of the reference and of the decoys over the
            full sides, native_contacts, docking.irmsd. The two sides' coordinates are gathered outside the timed call (in favour of
            this leg), and it has no ligand RMSD, score or class to offer.
--trace     a few calls of both legs, nothing timed: for a kernel trace in a separate run
Shapes (F, N): (64, 2000) and (4096, 5000). Clock: device events around one whole call (every call synchronises its stream, so the
host's enqueue time and the set-up's host arithmetic are inside), the median and the range of REPEATS calls after WARM warm-up calls,
the two legs interleaved. The routes' preserved counts and irmsd bits are compared at every shape."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch  # noqa: E402

from pesto_amd import docking as D  # noqa: E402
from pesto_amd import dockq as Q  # noqa: E402
from pesto_amd import trajectory as T  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
trace = "--trace" in sys.argv
out_path = args[0] if args else os.path.join(ROOT, "profiles", "out", "dockq.json")
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
dev = torch.device("cuda:0")
REPEATS, WARM = 7, 2
SHAPES = [(64, 2000), (4096, 5000)]
PER_RESIDUE = 8


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


def complex_of(F, N, seed):
    """(xyz float32 [F, N, 3] in nanometres, ids_R, ids_L, res_of_atom, bb): two globules of residues 5.5 A apart on a jittered lattice,
    their faces 4 A from each other; decoy 0 is the bound complex, the others move the ligand by up to 0.3 rad and 6 A and every atom by
    0.3 A of noise, as a docking run's poses around the bound one"""
    rng = np.random.default_rng(seed)
    sizes = np.full(-(-(N // 2) // PER_RESIDUE), PER_RESIDUE)
    sizes[-1] -= sizes.sum() - N // 2                  # (the last residue takes what is left of N / 2 atoms)
    n_res = sizes.size
    side = int(np.ceil(n_res ** (1 / 3)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    grid = grid[np.argsort(np.linalg.norm(grid - (side - 1) / 2, axis=1), kind="stable")[:n_res]] * 5.5
    centres = [grid + rng.normal(0, 0.5, grid.shape), grid + rng.normal(0, 0.5, grid.shape)]
    centres[1][:, 2] += centres[0][:, 2].max() - centres[1][:, 2].min() + 4.0
    roa = np.repeat(np.arange(2 * n_res), np.tile(sizes, 2))
    x0 = np.concatenate(centres)[roa] + rng.normal(0, 1.2, (roa.size, 3))
    n = x0.shape[0]
    ids_R, ids_L = np.arange(n // 2), np.arange(n // 2, n)
    bb = np.concatenate([np.arange(z) < 4 for z in np.tile(sizes, 2)])
    xyz = np.empty((F, n, 3), np.float32)
    xyz[0] = x0 * 0.1
    for f in range(1, F):
        a = rng.uniform(0, 1)
        w = rng.normal(size=3)
        w *= 0.3 * a / np.linalg.norm(w)
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / max(th, 1e-30)
        rot = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        x = x0 + rng.normal(0, 0.3, x0.shape)
        cm = x[ids_L].mean(0)
        x[ids_L] = (x[ids_L] - cm) @ rot.T + cm + rng.normal(0, 3.5 * a, 3)
        xyz[f] = x * 0.1
    return xyz, ids_R, ids_L, roa, bb


def source_hash():
    h = hashlib.sha256()
    for rel in ("pesto_amd/csrc/pesto_dockq.hip", "pesto_amd/csrc/pesto_geom.h", "pesto_amd/csrc/pesto_fit.h", "pesto_amd/csrc/pesto_call.h", "pesto_amd/dockq.py", "profiles/bench_dockq.py"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def legs(F, N):
    xyz_h, ids_R, ids_L, roa, bb = complex_of(F, N, F + N)
    xyz = torch.from_numpy(xyz_h).to(dev)
    ref = xyz[:1]
    xa, xb = xyz[:, :ids_R.size].contiguous(), xyz[:, ids_R.size:].contiguous()
    res_a, res_b = roa[ids_R], roa[ids_L] - roa[ids_L].min()

    def fused():
        return Q.dockq(ref, xyz, ids_R, ids_L, roa, bb)

    def composed():
        maps_ref = T.residue_contact_maps(xa[:1], xb[:1], res_a, res_b)
        maps = T.residue_contact_maps(xa, xb, res_a, res_b)
        return T.native_contacts(maps_ref, maps), maps_ref, D.irmsd(ref, xyz, ids_R, ids_L, roa, bb)

    return fused, composed, xyz_h.shape[1]


if trace:
    for F, N in SHAPES:
        fused, composed, _ = legs(F, N)
        for _ in range(2):
            fused()
            composed()
    torch.cuda.synchronize()
    sys.exit(0)

out = {"device": torch.cuda.get_device_name(0), "source": source_hash(),
       "clock": f"device events around one whole call on ROCm tensors, median [min, max] of {REPEATS} calls after {WARM} warm-up calls, legs interleaved",
       "shapes": []}
for F, N in SHAPES:
    fused, composed, n_atoms = legs(F, N)
    a = fused()
    nat, maps_ref, ir = composed()
    same = bool(torch.equal(a.preserved.long(), nat.long()) and int(maps_ref.sum()) == a.n_native and torch.equal(a.irmsd.view(torch.int32), ir.view(torch.int32)))
    tf, tc = timed(fused, composed)
    kept = a.preserved.cpu().numpy()
    row = {"F": F, "N": n_atoms, "atoms_per_side": n_atoms // 2, "n_native": a.n_native, "preserved_min_median_max": [int(kept.min()), float(np.median(kept)), int(kept.max())],
           "capri_counts": np.bincount(a.capri.cpu().numpy(), minlength=4).tolist(), "dockq": tf, "composed": tc,
           "composed_over_dockq": tc["median_ms"] / tf["median_ms"], "routes_agree_preserved_n_native_irmsd_bits": same,
           "atom_pairs_per_frame_composed": (n_atoms // 2) ** 2}
    out["shapes"].append(row)
    print(json.dumps(row), flush=True)
json.dump(out, open(out_path, "w"), indent=1)
