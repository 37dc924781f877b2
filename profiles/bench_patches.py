#!/usr/bin/env python3
"""Timing of the interface-patch kernels (pesto_interface_patches) beside a host baseline.
usage: python profiles/bench_patches.py [out.txt]   (on the GPU box; default profiles/out/r07_patches.txt)

Legs, every one x 15 selections (cluster_multi_interfaces' class pairs) in ONE launch, thresholds (70, 0.5, 10):
  af1000   1,000 AlphaFold-like synthetic proteins: R uniform in 100 - 2,700, a helix-like CA trace of 3.8 A steps folded into a ball,
           p and pLDDT from smooth random fields over space
  pdbs53   the 53 pdbs_test chains of tests/golden/patches.npz
  big      one 20,000-residue structure built like af1000's (large-structure path)
GPU times: patch_labels with ROCm tensors (device pointers; the call synchronises) and interface_patches_batch (the same plus the host
lists of the reference's layout). Host baseline: a NumPy float32 distance matrix plus scipy.sparse.csgraph.connected_components per
structure and selection - a lower bound on the reference's Python-set method (follow_rabbits); for af1000 it is timed on the first 50
proteins and scaled. Without scipy the baseline is skipped and the output says so.
The gfx clock is sampled (torch.cuda.clock_rate, amdsmi) around each GPU timing and printed with it."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from conftest import golden  # noqa: E402
from pesto_amd import Model  # noqa: E402
from pesto_amd.config import CONFIGS  # noqa: E402
from pesto_amd.patches import interface_patches_batch, patch_labels, selections  # noqa: E402
from pesto_amd.weights import synthetic_state_dict  # noqa: E402

try:
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
except ImportError:          # the baseline needs scipy
    connected_components = None

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "out", "r07_patches.txt")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
lines = []
SEL = selections(5, True)
THR = (70.0, 0.5, 10.0)


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


def af_like(R, rng):
    """(xyz [R,3], p [R,5], afs [R]) float32: a persistent 3.8 A walk pulled into a ball, smooth random fields for p and pLDDT"""
    r_ball = 3.8 * 1.6 * R ** (1 / 3)
    x = np.zeros((R, 3))
    d = rng.standard_normal(3)
    d /= np.linalg.norm(d)
    noise = rng.standard_normal((R, 3))
    for i in range(1, R):
        d = 0.8 * d + 0.45 * noise[i] - 0.35 * x[i - 1] / r_ball
        d /= np.linalg.norm(d)
        x[i] = x[i - 1] + 3.8 * d

    def field(k):
        c = x[rng.integers(0, R, k)]
        w = rng.standard_normal(k)
        return (w[None] * np.exp(-np.sum((x[:, None] - c[None]) ** 2, 2) / (2 * 12.0 ** 2))).sum(1)
    p = np.stack([1 / (1 + np.exp(-(2.5 * field(24) - b))) for b in (0.5, 2.5, 2.0, 1.5, 3.0)], 1)
    afs = 50 + 50 / (1 + np.exp(-2 * field(12)))
    return x.astype(np.float32), p.astype(np.float32), afs.astype(np.float32)


def host_baseline(xyz, p, afs):
    afs_thr, p_thr, d_thr = (np.float32(v) for v in THR)
    for i, j in SEL:
        m = (afs > afs_thr) & (p[:, i] > p_thr) & (p[:, j] > p_thr)
        x = xyz[m]
        D = np.sqrt(np.sum(np.square(x[None] - x[:, None]), axis=2))
        connected_components(csr_matrix(D < d_thr), directed=False)


def leg(name, items, base_n=None):
    ps = [torch.from_numpy(p).to(dev) for _, p, _ in items]
    xs = [torch.from_numpy(x).to(dev) for x, _, _ in items]
    afss = [torch.from_numpy(a).to(dev) for _, _, a in items]
    R = sum(len(x) for x, _, _ in items)
    n_items = len(items) * len(SEL)
    reps = 5 if R > 100000 else 20
    t_k, c_k = timed(lambda: patch_labels(m, ps, xs, afss, sel=SEL, afs_thr=THR[0], p_thr=THR[1], d_thr=THR[2]), reps)
    t_l, c_l = timed(lambda: interface_patches_batch(m, ps, xs, afss), max(2, reps // 4))
    po, npch, _, _, _ = patch_labels(m, ps, xs, afss, sel=SEL)
    nodes = int((po >= 0).sum())
    s = (f"{name}: {len(items)} structures x 15 selections ({R} rows, {nodes} nodes, {int(npch.sum())} patches)  patch_labels {1e3 * t_k:.3f} ms "
         f"({1e6 * t_k / n_items:.2f} us per structure x selection, {c_k:.2f} GHz)   interface_patches_batch (+ host lists) {1e3 * t_l:.3f} ms "
         f"({c_l:.2f} GHz)")
    if connected_components is None:
        s += "   host baseline: not measured (no scipy)"
    else:
        sub = items if base_n is None else items[:base_n]
        t0 = time.perf_counter()
        for it in sub:
            host_baseline(*it)
        tb = (time.perf_counter() - t0) * len(items) / len(sub)
        s += (f"   host baseline (NumPy float32 distance matrix + scipy connected_components{'' if base_n is None else f', timed on {base_n}, scaled'}) "
              f"{1e3 * tb:.1f} ms ({1e6 * tb / n_items:.1f} us per structure x selection)   x{tb / t_k:.0f}")
    say(s)


dev = torch.device("cuda:0")
m = Model(CONFIGS["i_v4_0"]).to(dev)
m.load_state_dict(synthetic_state_dict(CONFIGS["i_v4_0"]))
say(f"device {torch.cuda.get_device_name(0)}; times are wall clock per call after 3 warm-up calls; clock = gfx clock sampled before / after")
rng = np.random.default_rng(1000)
af = [af_like(int(r), rng) for r in rng.integers(100, 2701, 1000)]
leg("af1000", af, base_n=50)
g = golden("patches")
offs = g["pdbs53_offsets"]
leg("pdbs53", [(g["pdbs53_xyz"][offs[s]:offs[s + 1]], g["pdbs53_p"][offs[s]:offs[s + 1]], g["pdbs53_afs"][offs[s]:offs[s + 1]]) for s in range(53)])
leg("big", [af_like(20000, rng)])
open(out_path, "w").write("\n".join(lines) + "\n")
