#!/usr/bin/env python3
"""Timing of the evaluation kernels (pesto_interface_labels, pesto_bc_scores) beside the reference's method on the same GPU.
usage: python profiles/bench_eval.py [out.txt]   (on the GPU box; default profiles/out/r07_eval.txt)

labels: 6NFU.pdb1 (16,192 atoms after preprocessing, 24 subunits) and all 16 assemblies of tests/golden/eval_labels.npz in one launch,
        device pointers (the call synchronises) - vs the reference's locate_contacts: a dense torch distance matrix per pair of subunits
        on the GPU plus the per-residue OR of the typed contacts (src/data_encoding.py:116-176; the contacts_types maps are not timed).
scores: 53 structures (the pdbs_test residue counts) and 10,000 structures (R uniform in 50 - 600) x 5 classes, ROCm tensors in one
        launch - vs bc_scoring's method: torch counts on the GPU + sklearn roc_auc_score on the host per structure (src/scoring.py:77-96;
        for the 10,000 it is timed on the first 500 and scaled).
The gfx clock is sampled (torch.cuda.clock_rate, amdsmi) around each GPU timing and printed with it."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from sklearn.metrics import roc_auc_score  # noqa: E402

from conftest import golden  # noqa: E402
from pesto_amd import Model  # noqa: E402
from pesto_amd.config import CONFIGS  # noqa: E402
from pesto_amd.evaluate import bc_scores_batch, contact_labels, resname_masks  # noqa: E402
from pesto_amd.weights import synthetic_state_dict  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "out", "r07_eval.txt")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def clock():
    try:
        return float(torch.cuda.clock_rate(0)) / 1e3
    except Exception:      # noqa: BLE001 - no amdsmi
        return float("nan")


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    clk = [clock()]
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    clk.append(clock())
    return dt, np.nanmean(clk)


dev = torch.device("cuda:0")
m = Model(CONFIGS["i_v4_0"]).to(dev)
m.load_state_dict(synthetic_state_dict(CONFIGS["i_v4_0"]))
say(f"device {torch.cuda.get_device_name(0)}; times are wall clock per call after 3 warm-up calls; clock = gfx clock sampled before / after")

# ---------------------------------------------------------------- labels
g = golden("eval_labels")
names = list(g["names"].astype(str))
table = g["resname_table"].astype(str)
rec_all, mask_all = resname_masks(table[g["atom_resname"]])


def labels_case(idx):
    sel = np.concatenate([np.arange(g["atom_offsets"][a], g["atom_offsets"][a + 1]) for a in idx])
    sizes = [int(g["atom_offsets"][a + 1] - g["atom_offsets"][a]) for a in idx]
    sub = g["atom_sub"][sel].astype(np.int32)
    res = g["atom_res"][sel] + g["res_offsets"][sub]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = (t(g["X"][sel]), t(sub), t(res.astype(np.int32)), t(rec_all[sel]), t(mask_all[sel].view(np.int32)))
    n_res = int(g["res_offsets"][-1])
    return sel, sizes, args, n_res


def reference_labels(sel, idx):
    """locate_contacts for every pair of subunits (dense torch.norm on the GPU) + the per-residue OR of the partners' class bits"""
    X = torch.from_numpy(g["X"]).to(dev)
    mask = torch.from_numpy(mask_all.astype(np.int64)).to(dev)
    rec = torch.from_numpy(rec_all.astype(bool)).to(dev)
    res = torch.from_numpy((g["atom_res"] + g["res_offsets"][g["atom_sub"]]).astype(np.int64)).to(dev)
    y = torch.zeros(int(g["res_offsets"][-1]), dtype=torch.int64, device=dev)
    for a in idx:
        ks = np.where(g["sub_assembly"] == a)[0]
        rng = [torch.from_numpy(np.where(g["atom_sub"] == k)[0]).to(dev) for k in ks]
        for i in range(len(ks)):
            for j in range(i + 1, len(ks)):
                D = torch.norm(X[rng[i]].unsqueeze(1) - X[rng[j]].unsqueeze(0), dim=2)
                ii, jj = torch.where(D < 5.0)
                for r, o in ((rng[i][ii], rng[j][jj]), (rng[j][jj], rng[i][ii])):
                    keep = rec[r]
                    y.index_put_((res[r[keep]],), mask[o[keep]], accumulate=True)      # (a sum: > 0 where the OR is set)
    return y


for label, idx in (("6NFU.pdb1 (24 subunits)", [names.index("6NFU")]), ("all 16 assemblies, one launch", list(range(16)))):
    sel, sizes, args, n_res = labels_case(idx)
    dt, clk = timed(lambda: contact_labels(m, *args, sizes, n_res), 20)
    dtr, clkr = timed(lambda: reference_labels(sel, idx), 3)
    say(f"labels  {label}: {sel.size} atoms  k_contact_labels path {dt * 1e3:.3f} ms ({clk:.2f} GHz)   "
        f"reference method (dense torch.norm per subunit pair, GPU) {dtr * 1e3:.1f} ms ({clkr:.2f} GHz)   x{dtr / dt:.0f}")

# ---------------------------------------------------------------- scores
rng = np.random.default_rng(3)


def score_case(sizes):
    ys = [torch.from_numpy((rng.uniform(size=(r, 5)) < 0.15).astype(np.uint8)).to(dev) for r in sizes]
    ps = [torch.from_numpy(np.clip(rng.normal(0.3, 0.25, (r, 5)), 0, 1).astype(np.float32)).to(dev) for r in sizes]
    return ys, ps


def reference_scores(ys, ps):
    for y, p in zip(ys, ps):
        y = y.float()
        q = torch.round(p)
        TP, FP = torch.sum(q * y, 0), torch.sum(q * (1 - y), 0)
        P = torch.sum(y, 0)
        N = torch.sum(1 - y, 0)
        mk = ((P > 0) & (N > 0)).cpu().numpy()
        if mk.any():
            roc_auc_score(y[:, mk].cpu().numpy(), p[:, mk].cpu().numpy(), average=None)
        torch.std(p, 0).cpu()


sizes53 = golden("pdbs_test_sizes")["residues"]
for label, sizes, n_ref in (("53 structures x 5", [int(v) for v in sizes53], None),
                            ("10,000 structures x 5", [int(v) for v in rng.integers(50, 601, 10000)], 500)):
    ys, ps = score_case(sizes)
    dt, clk = timed(lambda: bc_scores_batch(m, ys, ps), 10)
    k = n_ref or len(sizes)
    dtr, clkr = timed(lambda: reference_scores(ys[:k], ps[:k]), 1)
    dtr *= len(sizes) / k
    say(f"scores  {label} ({sum(sizes)} rows): k_bc_scores path {dt * 1e3:.3f} ms ({clk:.2f} GHz)   reference method (torch counts on the GPU + "
        f"sklearn AUC per structure{'' if n_ref is None else f', timed on {n_ref}, scaled'}) {dtr * 1e3:.1f} ms   x{dtr / dt:.0f}")
open(out_path, "w").write("\n".join(lines) + "\n")
