#!/usr/bin/env python3
"""Timing of the sorted ranking path (pesto_amd.ranking.scores, pesto_rank.hip) beside the pairwise one (pesto_amd.evaluate.bc_scoring,
k_bc_scores: every (positive, negative) pair in one workgroup per column) on pooled columns.
usage: python profiles/bench_ranking.py [out.txt]   (on the GPU box; default profiles/out/ranking_bench.txt)

Two pooled columns (S = 1, C = 1), on ROCm tensors:
  pdbs53     the 16,825 residues of tests/golden/eval_scores.npz (pdbs53_logits), as the notebooks pool them
  synthetic  150,000 rows, the size of interface_type_evaluation.ipynb: seeded uniform scores, 10 % positives drawn with probability
             rising in the score
Legs: ranking.scores (keys, the radix passes, the scans, the scores kernel: every launch of one call and its stream synchronisation),
evaluate.bc_scoring (one launch), and ranking.curves with drop_intermediate (the thinned ROC curve). Clock: device events around one whole
call, the two legs alternating inside one repeat loop, the median and the range of REPEATS repeats after WARM warm-up calls of each; every
call synchronises its stream, so the host's enqueue time is inside. The launch count is computed from the call's shape as
pesto_rank.hip's rank_sort launches: 4 + 3 n_pass kernels and one memset, then the leg's own kernels. The float32 rounding of roc_auc is
compared with bc_scoring's auc row before anything is timed."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pesto_amd import evaluate as E  # noqa: E402
from pesto_amd import ranking as R  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "out", "ranking_bench.txt")
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
lines = []
dev = torch.device("cuda:0")
REPEATS, WARM = 15, 3


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fns):
    """per function: (median, min, max) seconds of one call from device events, the functions alternating"""
    for fn in fns:
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(REPEATS):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / 1e3)
    return [(float(np.median(t)), min(t), max(t)) for t in ts]


def source_hash():
    h = hashlib.sha256()
    for rel in ("pesto_amd/csrc/pesto_rank.hip", "pesto_amd/csrc/pesto_eval.hip", "pesto_amd/csrc/pesto_radix.h", "pesto_amd/csrc/pesto_scan.h", "pesto_amd/ranking.py",
                "profiles/bench_ranking.py"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def launches(n_col):
    bits = 33 + max(0, int(n_col - 1).bit_length())
    n_pass = (bits + 7) // 8
    return n_pass, 4 + 3 * n_pass


g = np.load(os.path.join(ROOT, "tests", "golden", "eval_scores.npz"))
rng = np.random.default_rng(150000)
ps = rng.random(150000).astype(np.float32)
ys = (rng.random(150000) < 0.2 * ps).astype(np.uint8)
columns = {"pdbs53": (g["pdbs53_logits_y"][:, 0], g["pdbs53_logits_p"][:, 0]), "synthetic": (ys, ps)}
model = E._scoring_model(0)
say(f"device {torch.cuda.get_device_name(0)}; source {source_hash()}; clock: device events around one whole call (every call synchronises its "
    f"stream), legs alternating, median [min, max] of {REPEATS} after {WARM} warm-up calls each")
rows = {}
for name, (y, p) in columns.items():
    yd, pd = torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev)
    y2, p2 = yd[:, None].contiguous(), pd[:, None].contiguous()
    sc = R.scores(yd, pd, model=model)
    counts, auc = sc["counts"].cpu().numpy()[0, :, 0], sc["scores"].cpu().numpy()[0, :, 0]
    bc = E.bc_scoring(y2, p2, model).cpu().numpy()[6, 0]
    assert np.float32(auc[0]).view(np.uint32) == bc.view(np.uint32), (auc[0], bc)
    n_pass, n_sort = launches(1)
    (t_rank, t_bc, t_roc) = timed([lambda: R.scores(yd, pd, model=model), lambda: E.bc_scoring(y2, p2, model),
                                   lambda: R.curves(yd, pd, True, model=model)])
    rows[name] = (y.size, t_rank[0], t_bc[0])
    say(f"{name}: R = {y.size}, P = {counts[0]}, K = {counts[4]} thresholds, K_roc = {counts[5]}, roc_auc = {auc[0]:.6f} (float32 bits equal "
        f"bc_scoring's), pr_auc = {auc[1]:.6f}")
    say(f"    ranking.scores      {1e3 * t_rank[0]:9.3f} ms [{1e3 * t_rank[1]:.3f}, {1e3 * t_rank[2]:.3f}]   {n_pass} radix passes, "
        f"{n_sort + 1} kernel launches + 1 memset per call")
    say(f"    evaluate.bc_scoring {1e3 * t_bc[0]:9.3f} ms [{1e3 * t_bc[1]:.3f}, {1e3 * t_bc[2]:.3f}]   1 kernel launch per call, "
        f"{counts[0] * counts[1] / 1e9:.3f} G pairs")
    say(f"    ranking.curves(drop_intermediate) {1e3 * t_roc[0]:9.3f} ms [{1e3 * t_roc[1]:.3f}, {1e3 * t_roc[2]:.3f}]   {n_sort + 3} kernel launches "
        f"+ 1 memset per call")
(n0, r0, b0), (n1, r1, b1) = rows["pdbs53"], rows["synthetic"]
say(f"growth from R = {n0} to R = {n1} (x{n1 / n0:.2f} rows, x{(n1 / n0) ** 2:.1f} squared): ranking.scores x{r1 / r0:.2f}, evaluate.bc_scoring x{b1 / b0:.2f}")
open(out_path, "w").write("\n".join(lines) + "\n")
