#!/usr/bin/env python3
"""Timing of pesto_amd.poses (pesto_poses.hip) against the only route the package had to the same counts: placing every pose into frames
with torch and running docking.frame_contacts and frame_residue_contacts on them. Two seeded globules of N atoms in residues of 10 atoms
(300 residues a side at N = 3000), F poses: rotation_set(F), the ligand's centre on a sphere around the receptor where the two bodies
overlap by a shell, so that a typical pose has an interface.
usage: python profiles/bench_poses.py [out.json] [F] [N]   (on the GPU box; default profiles/out/poses.json, F = 54000, N = 3000)

scores      pose_scores(...) on ROCm tensors: the grid over the receptor and the one launch over the poses, inside the timed call
slide       slide_to_contact(...) on ROCm tensors, along the line from the receptor's centre through the ligand's
composed    per batch of BATCH poses: torch places the ligand into [B, N, 3] (einsum + add: not the library's rounding, in favour of this
            leg nothing is checked bit for bit), the receptor is expanded to [B, N, 3], then frame_contacts and frame_residue_contacts;
            n_contact and n_pairs are read off the offsets. It has no clash count, residue sets, sums or score to offer.
Clock: device events around one whole leg (every library call synchronises its stream, so the host's enqueue time is inside), the median
and the range of REPEATS runs after WARM warm-up runs, the legs interleaved. The routes' n_contact and n_pairs are compared where the
placement rounds alike (a count of the poses that differ is reported, not asserted). The pair tests of the scoring launch are counted
on the host for a sample of poses from the grid's geometry (placed atoms that pass the box test times the atoms of the 27 cells around
them); the slide tests F N N pairs."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch  # noqa: E402

from pesto_amd import docking as D  # noqa: E402
from pesto_amd import poses as P  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "out", "poses.json")
F = int(args[1]) if len(args) > 1 else 54000
N = int(args[2]) if len(args) > 2 else 3000
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
dev = torch.device("cuda:0")
REPEATS, WARM, BATCH, PER_RESIDUE, SAMPLE = 3, 1, 2000, 10, 32


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "runs": len(ts)}


def globule(n, rng):
    """n atoms in nanometres at 100 atoms / nm^3 in a ball, residues of PER_RESIDUE consecutive atoms around common centres"""
    n_res = -(-n // PER_RESIDUE)
    radius = (3 * n / (4 * np.pi * 100.0)) ** (1 / 3)
    c = rng.normal(size=(n_res, 3))
    c *= (radius * rng.random(n_res) ** (1 / 3) / np.linalg.norm(c, axis=1))[:, None]
    res = np.repeat(np.arange(n_res), PER_RESIDUE)[:n].astype(np.int32)
    return (c[res] + rng.normal(0, 0.15, (n, 3))).astype(np.float32), res, radius


def system():
    rng = np.random.default_rng([F, N])
    xR, res_R, rad_R = globule(N, rng)
    xL, res_L, rad_L = globule(N, rng)
    rot = P.rotation_set(F)
    w = rng.normal(size=(F, 3))
    w /= np.linalg.norm(w, axis=1)[:, None]
    pos = xR.astype(np.float64).mean(0) + w * (rad_R + rad_L - 0.3)
    tr = P.poses_about(rot, xL.astype(np.float64).mean(0), pos)
    p_R, p_L = rng.random(int(res_R.max()) + 1).astype(np.float32), rng.random(int(res_L.max()) + 1).astype(np.float32)
    return dict(xR=xR, xL=xL, res_R=res_R, res_L=res_L, rot=rot, tr=tr, p_R=p_R, p_L=p_L, u=w.astype(np.float32))


def grid_pair_tests(s, r_contact=5.0, scale=10.0):
    """mean pair tests per pose of the scoring launch, from the grid's geometry (pesto_cellgrid.h's cell edge and pesto_poses.hip's box
    test), over SAMPLE poses"""
    xR = s["xR"].astype(np.float64)
    lo, ext = xR.min(0), xR.max(0) - xR.min(0)
    h = max(r_contact / scale * 1.001, ext.max() / 64 * 1.0001)
    while np.prod((ext / h).astype(int) + 1) > 2 * N + 64:
        h *= 1.25
    n = (ext / h).astype(int) + 1
    cell = np.minimum(((xR - lo) / h).astype(int), n - 1)
    cnt = np.zeros(n + 2, np.int64)
    np.add.at(cnt, tuple((cell + 1).T), 1)
    box = sum(np.roll(cnt, (a, b, c), (0, 1, 2)) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1))   # atoms of the 27 cells, padded
    total = 0
    for f in np.linspace(0, F - 1, SAMPLE).astype(int):
        y = s["xL"].astype(np.float64) @ s["rot"][f].astype(np.float64).T + s["tr"][f]
        fx = (y - lo) / h
        keep = ((fx >= -1.5) & (fx <= n + 1.5)).all(1)
        c = np.clip(fx[keep].astype(int), 0, n - 1)
        total += int(box[tuple((c + 1).T)].sum())
    return total / SAMPLE, float(h), n.tolist()


def source_hash():
    h = hashlib.sha256()
    for rel in ("pesto_amd/csrc/pesto_poses.hip", "pesto_amd/csrc/pesto_cellgrid.h", "pesto_amd/csrc/pesto_geom.h", "pesto_amd/csrc/pesto_radix.h",
                "pesto_amd/csrc/pesto_call.h", "pesto_amd/poses.py", "profiles/bench_poses.py"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


s = system()
d = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
state = {}


def scores():
    state["scores"] = P.pose_scores(d["xR"], d["xL"], s["res_R"], s["res_L"], d["rot"], d["tr"], s["p_R"], s["p_L"])


def slide():
    state["slide"] = P.slide_to_contact(d["xR"], d["xL"], d["rot"], d["tr"], d["u"])


def composed():
    nc, npair, k_total = [], [], 0
    for b0 in range(0, F, BATCH):
        R, t = d["rot"][b0:b0 + BATCH], d["tr"][b0:b0 + BATCH]
        y = torch.einsum("fab,nb->fna", R, d["xL"]) + t[:, None, :]
        a = d["xR"][None].expand(y.shape[0], -1, -1).contiguous()
        lists = D.frame_contacts(a, y)
        roff, _, _ = D.frame_residue_contacts(lists, None, s["res_R"], s["res_L"])
        nc.append(lists[0][1:] - lists[0][:-1])
        npair.append(roff[1:] - roff[:-1])
        k_total += int(lists[1].shape[0])
    state["composed"] = (torch.cat(nc), torch.cat(npair), k_total)


legs = (scores, slide, composed)
for _ in range(WARM):
    for fn in legs:
        fn()
torch.cuda.synchronize()
ts = [[] for _ in legs]
for _ in range(REPEATS):
    for k, fn in enumerate(legs):
        ts[k].append(event_time(fn))
t_scores, t_slide, t_composed = (stats(t) for t in ts)
sc, (nc, npair, k_total) = state["scores"], state["composed"]
hits = int((~torch.isnan(state["slide"][0])).sum())
tests, h, cells = grid_pair_tests(s)
n_res = int(s["res_R"].max()) + 1
out = {"device": torch.cuda.get_device_name(0), "source": source_hash(), "F": F, "N_R": N, "N_L": N, "residues_a_side": n_res,
       "clock": f"device events around one whole leg on ROCm tensors, median [min, max] of {REPEATS} runs after {WARM} warm-up, legs interleaved",
       "scores": t_scores, "slide": t_slide, "composed": t_composed, "composed_batch": BATCH,
       "composed_over_scores": t_composed["median_ms"] / t_scores["median_ms"],
       "n_contact_min_median_max": [int(sc.n_contact.min()), float(sc.n_contact.float().median()), int(sc.n_contact.max())],
       "poses_with_clash": int((sc.n_clash > 0).sum()), "slide_hits": hits,
       "poses_where_routes_differ_n_contact": int((sc.n_contact.long() != nc.long()).sum()),
       "poses_where_routes_differ_n_pairs": int((sc.n_pairs.long() != npair.long()).sum()),
       "scores_pair_tests_per_pose_sampled": tests, "scores_pair_tests": tests * F, "grid_cell_nm": h, "grid_cells": cells,
       "scores_pair_tests_per_s": tests * F / (t_scores["median_ms"] * 1e-3),
       "slide_pair_tests": float(F) * N * N, "slide_pair_tests_per_s": float(F) * N * N / (t_slide["median_ms"] * 1e-3),
       "scores_compulsory_bytes": N * 16 + N * 12 + N * 8 + F * 48 + F * (5 * 4 + 3 * 8 + 4),
       "composed_compulsory_bytes": 2 * F * 2 * N * 12 + 2 * k_total * 12 + F * 16, "composed_contacts_listed": k_total,
       "composed_pair_tests": float(F) * N * N}
print(json.dumps(out), flush=True)
json.dump(out, open(out_path, "w"), indent=1)
