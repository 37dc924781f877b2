#!/usr/bin/env python3
"""Timing of pesto_amd.lddt (pesto_lddt.hip) on seeded globules (residues of 8 atoms on a jittered 5.5 A lattice, nanometres, scale 10) whose
frames are the reference plus noise of 0.1 to 1 A, against what a user would write in PyTorch-ROCm on the same GPU.
usage: python profiles/bench_lddt.py [out.json] [--trace]   (on the GPU box; default profiles/out/lddt.json)

one_shot    lddt(ref, xyz, res_of_atom) on ROCm tensors: the index check, the reference list (grid, count, scan, fill) and the scoring,
            all inside the timed call
pairs       lddt(..., pairs=reference_pairs(...)): the index check, the scoring launch and the totals
torch       torch.cdist (exact mode, no matrix product) per chunk of frames (and block of rows: 2^23 outputs per call) against a dense [N, N] reference matrix and mask, the T
            comparisons, a sum over partners and index_add over the residues. The mask and the reference matrix are made outside the timed
            call (in favour of this leg). Its counts are compared with ours at every shape it runs at and the number of differing counts is
            recorded (cdist's own rounding of d may move a pair that sits within a float32 unit of a threshold). Beyond some 2^24 outputs per
            call cdist's exact mode returned wrong distances here, so the leg stays at 2^23 per call.
--trace     a few calls of the first two legs, nothing timed: for a kernel trace in a separate run
Shapes (F, N): an MD run (1024, 3000), a large complex (64, 20000), CA only (10000, 400), and a ragged batch of 256 structures of about
2,000 atoms with one model each (no torch leg: not measured). Clock: device events around one whole call (every call synchronises its
stream, so the host's enqueue time and the call's host arithmetic are inside), the median and the range of REPEATS calls after WARM
warm-up calls, the legs interleaved (the torch leg: TORCH_REPEATS calls after one). For the scoring leg the bytes that one frame must read - the list at 8 B
per entry and the frame's coordinates at 12 B per atom - are recorded against the time per frame, as a rate and as its share of the two
rates of the microarchitecture guide that could bound it: 6.29 TB/s (HBM, measured copy) and 8.6 TB/s (Infinity Cache, gathered rows).
The time is a whole call's, not the kernel's, so the shares are lower bounds of the scoring launch's own."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch  # noqa: E402

from pesto_amd import lddt as L  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
trace = "--trace" in sys.argv
out_path = args[0] if args else os.path.join(ROOT, "profiles", "out", "lddt.json")
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
dev = torch.device("cuda:0")
REPEATS, WARM = 7, 2
TORCH_REPEATS = 2
SHAPES = [("md_run", 1024, 3000), ("large_complex", 64, 20000), ("ca_only", 10000, 400)]
BATCH = (256, 2000)
PER_RESIDUE = 8
THRESHOLDS = (0.5, 1, 2, 4)
HBM_TBS, MALL_TBS = 6.29, 8.6
CDIST_OUTPUTS = 1 << 23


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "calls": len(ts)}


def timed(fns, repeats=REPEATS, warm=WARM):
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


def globule(N, rng, per_residue=PER_RESIDUE, spacing=5.5):
    """(x0 float64 [N, 3] in angstroms, res_of_atom [N]): residues on the lattice points nearest the centre, atoms 1.2 A around them.
    per_residue 1 and spacing 3.8 / 5.5: a CA-like chain of points"""
    n_res = -(-N // per_residue)
    side = int(np.ceil(n_res ** (1 / 3))) + 1
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    grid = grid[np.argsort(np.linalg.norm(grid - (side - 1) / 2, axis=1), kind="stable")[:n_res]] * spacing
    roa = np.repeat(np.arange(n_res), per_residue)[:N]
    return (grid + rng.normal(0, 0.5, grid.shape))[roa] + rng.normal(0, 1.2 if per_residue > 1 else 0.3, (N, 3)), roa


def frames_of(ref, F, seed):
    """float32 [F, N, 3] on the device: frame 0 the reference, frame f the reference plus noise of 0.1 .. 1 A (nanometres)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    sigma = torch.linspace(0.01, 0.1, F, device=dev)[:, None, None]
    xyz = ref[None] + sigma * torch.randn((F,) + tuple(ref.shape), generator=g, device=dev)
    xyz[0] = ref
    return xyz.contiguous()


def source_hash():
    h = hashlib.sha256()
    for rel in ("pesto_amd/csrc/pesto_lddt.hip", "pesto_amd/csrc/pesto_cellgrid.h", "pesto_amd/csrc/pesto_geom.h", "pesto_amd/csrc/pesto_call.h",
                "pesto_amd/lddt.py", "profiles/bench_lddt.py"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def torch_leg(ref, xyz, roa, R):
    """the dense PyTorch route and its set-up (outside the timed call)"""
    N = ref.shape[0]
    res = torch.from_numpy(roa).to(dev)
    mode = "donot_use_mm_for_euclid_dist"
    dref = torch.cat([torch.cdist(ref[None, r0:r0 + CDIST_OUTPUTS // N], ref[None], compute_mode=mode)[0] for r0 in range(0, N, CDIST_OUTPUTS // N)]) * 10.0
    mask = (dref < 15.0) & (res[:, None] != res[None, :])
    thr = [float(t) for t in THRESHOLDS]
    # 2^23 outputs per cdist call (see above): the frames go in chunks and, where one frame's [N, N] is already too much, its rows in blocks
    rows = max(1, min(N, CDIST_OUTPUTS // N))
    chunk = max(1, min(xyz.shape[0], CDIST_OUTPUTS // (rows * N)))

    def run():
        out = torch.zeros((xyz.shape[0], R, len(thr)), dtype=torch.int32, device=dev)
        for f0 in range(0, xyz.shape[0], chunk):
            x = xyz[f0:f0 + chunk]
            for r0 in range(0, N, rows):
                gap = (torch.cdist(x[:, r0:r0 + rows], x, compute_mode=mode) * 10.0 - dref[None, r0:r0 + rows]).abs_()
                m = mask[None, r0:r0 + rows]
                per_atom = torch.stack([((gap < t) & m).sum(2, dtype=torch.int32) for t in thr], 2)
                out[f0:f0 + chunk].index_add_(1, res[r0:r0 + rows], per_atom)
        return out
    return run, int(mask.sum())


def scoring_rates(K, N, F, st):
    """bytes one frame must read over the time per frame of a whole call"""
    per_frame = 8.0 * K + 12.0 * N
    tbs = per_frame * F / (st["median_ms"] * 1e-3) / 1e12
    return {"list_bytes_per_frame": 8.0 * K, "coordinate_bytes_per_frame": 12.0 * N, "ms_per_frame": st["median_ms"] / F,
            "TB_per_s_of_whole_call": tbs, "share_of_hbm_6.29": tbs / HBM_TBS, "share_of_infinity_cache_8.6": tbs / MALL_TBS}


def shape_legs(F, N, ca):
    rng = np.random.default_rng(F + N)
    x0, roa = globule(N, rng, 1 if ca else PER_RESIDUE, 5.0 if ca else 5.5)
    ref = torch.from_numpy((x0 * 0.1).astype(np.float32)).to(dev)
    xyz = frames_of(ref, F, F + N)
    pairs = L.reference_pairs(ref, roa)
    legs = {"one_shot": lambda: L.lddt(ref, xyz, roa, thresholds=THRESHOLDS),
            "pairs": lambda: L.lddt(ref, xyz, roa, thresholds=THRESHOLDS, pairs=pairs)}
    return legs, ref, xyz, roa, int(pairs[1].shape[0])


def batch_legs(B, n):
    rng = np.random.default_rng(B + n)
    sizes = rng.integers(int(0.9 * n), int(1.1 * n) + 1, B)
    xs, rows, start = [], [], 0
    for b in range(B):
        x0, roa = globule(int(sizes[b]), rng)
        xs.append(x0 + 500.0 * rng.normal(size=3))
        rows.append(roa + start)
        start += int(roa.max()) + 1
    roa = np.concatenate(rows)
    ref = torch.from_numpy((np.concatenate(xs) * 0.1).astype(np.float32)).to(dev)
    xyz = frames_of(ref, 2, B)[1:]
    sizes = [int(v) for v in sizes]
    pairs = L.reference_pairs(ref, roa, sizes=sizes)
    legs = {"one_shot": lambda: L.lddt(ref, xyz, roa, thresholds=THRESHOLDS, sizes=sizes),
            "pairs": lambda: L.lddt(ref, xyz, roa, thresholds=THRESHOLDS, sizes=sizes, pairs=pairs)}
    return legs, ref, xyz, roa, int(pairs[1].shape[0]), sizes


if trace:
    for _, F, N in SHAPES:
        legs = shape_legs(F, N, N <= 1000)[0]
        for _ in range(2):
            for fn in legs.values():
                fn()
    torch.cuda.synchronize()
    sys.exit(0)

out = {"device": torch.cuda.get_device_name(0), "source": source_hash(),
       "clock": f"device events around one whole call on ROCm tensors, median [min, max] of {REPEATS} calls after {WARM} warm-up calls, legs interleaved",
       "rates_of_the_guide_TB_per_s": {"hbm_measured_copy": HBM_TBS, "infinity_cache_gathered_rows": MALL_TBS}, "shapes": []}
for name, F, N in SHAPES:
    legs, ref, xyz, roa, K = shape_legs(F, N, name == "ca_only")
    R = int(roa.max()) + 1
    run_torch, n_mask = torch_leg(ref, xyz, roa, R)
    a, b = legs["one_shot"](), legs["pairs"]()
    same = all(torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32)) for k in ("score", "residue", "preserved", "total"))
    theirs = run_torch()
    differing = int((theirs != a.preserved).sum())
    ts = dict(zip(legs, timed(list(legs.values()))))
    ts["torch"] = timed([run_torch], TORCH_REPEATS, 1)[0]
    score = a.score.cpu().numpy()
    row = {"shape": name, "F": F, "N": N, "R": R, "K": K, "partners_per_atom": K / N, "T": len(THRESHOLDS), "score_min_max": [float(score.min()), float(score.max())],
           **ts, "set_up_ms": ts["one_shot"]["median_ms"] - ts["pairs"]["median_ms"], "torch_over_one_shot": ts["torch"]["median_ms"] / ts["one_shot"]["median_ms"],
           "torch_over_pairs": ts["torch"]["median_ms"] / ts["pairs"]["median_ms"],
           "legs_agree_bit_for_bit": bool(same), "torch_mask_pairs": n_mask, "torch_mask_equals_K": n_mask == K,
           "torch_counts_differing": differing, "torch_counts_compared": int(theirs.numel()), "scoring": scoring_rates(K, N, F, ts["pairs"])}
    out["shapes"].append(row)
    print(json.dumps(row), flush=True)
    del legs, ref, xyz, run_torch, theirs, a, b
    torch.cuda.empty_cache()

B, n = BATCH
legs, ref, xyz, roa, K, sizes = batch_legs(B, n)
a, b = legs["one_shot"](), legs["pairs"]()
same = all(torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32)) for k in ("score", "residue", "preserved", "total"))
ts = dict(zip(legs, timed(list(legs.values()))))
N = int(ref.shape[0])
row = {"shape": "ragged_batch", "structures": B, "F": 1, "N": N, "atoms_min_max": [min(sizes), max(sizes)], "R": int(roa.max()) + 1, "K": K, "partners_per_atom": K / N,
       "T": len(THRESHOLDS), **ts, "legs_agree_bit_for_bit": bool(same), "set_up_ms": ts["one_shot"]["median_ms"] - ts["pairs"]["median_ms"], "torch": "not measured", "scoring": scoring_rates(K, N, 1, ts["pairs"])}
out["shapes"].append(row)
print(json.dumps(row), flush=True)
json.dump(out, open(out_path, "w"), indent=1)
