#!/usr/bin/env python3
"""Timing of the structure alignment (pesto_amd.structalign, pesto_structalign.hip) and of the sequence clustering whose wave recursion it
shares (pesto_alignwave.h).
usage: python profiles/bench_structalign.py [out.txt] [--sequences-only]   (on the GPU box; default profiles/out/structalign_bench.txt)

Legs:
  cluster_sequences   DESIGN.md 4.25's two figures (S = 2048, L = 300 and S = 256, L = 2000; BLOSUM62 11 / 1, global), FIVE single calls
                      each after a warm-up call, all five printed: run at the parent commit and at this one in the same session, the new
                      median must lie within the spread of the parent's five (--sequences-only runs on a tree without the new module)
  align_structures    all pairs of 64 chains of 300 residues (8 families of 8: a CA-like trace, 1 A of noise, a hinged second half),
                      one pair of 2000 x 2000, and two calls shaped so that one form of k_sa_dp dominates: rounds = 1 with 16 fragment
                      starts (scores only: 289 fragment pairs a pair against 5 traced DPs) and frag_starts = 2 with 20 rounds (traced)
A cell update is one (i, j) of one DP. GPU times are device events around whole calls on device tensors: allocation, set-up, the per-round
readbacks and the stream synchronisation are inside, so the rates are lower bounds on the kernel's own. A record, not a bar."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pesto_amd import _lib, sequences as sq  # noqa: E402
from pesto_amd.patches import _default_model  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "out", "structalign_bench.txt")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
lines = []
dev = torch.device("cuda:0")


def say(s):
    print(s, flush=True)
    lines.append(s)


def five(fn):
    """seconds of five single calls after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / 1e3)
    return out


def report(name, fn, cells, what="cell updates"):
    t = five(fn)
    s = sorted(t)
    say(f"{name}: {', '.join(f'{1e3 * v:.2f}' for v in t)} ms; median {1e3 * s[2]:.2f} [{1e3 * s[0]:.2f}, {1e3 * s[4]:.2f}] ms   "
        f"{cells:.3e} {what}, {cells / s[2] / 1e9:.1f} G / s at the median")


m = _default_model(0)
rng = np.random.RandomState(0)
say(f"device {torch.cuda.get_device_name(0)}; five single calls after a warm-up call, device events around each whole call")
for S, L in ((2048, 300), (256, 2000)):
    codes = torch.from_numpy(rng.randint(0, 20, S * L).astype(np.uint8)).to(dev)
    offs = _lib.offsets([L] * S)
    report(f"cluster_sequences, S = {S}, L = {L}", lambda: sq.cluster_sequences((codes, offs), model=m, _reduce=False), S * (S - 1) / 2 * L * L)

if "--sequences-only" not in sys.argv:
    from pesto_amd import structalign as sa

    def trace(gen, L):
        step = gen.normal(size=(L, 3))
        for k in range(1, L):
            step[k] += 0.8 * step[k - 1]
            step[k] /= np.linalg.norm(step[k])
        step[0] /= np.linalg.norm(step[0])
        return np.cumsum(3.8 * step, 0)

    def member(gen, base):
        x = base + gen.normal(size=base.shape)
        h = base.shape[0] // 2
        a = gen.normal(size=3)
        a /= np.linalg.norm(a)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        ang = np.deg2rad(gen.uniform(10, 40))
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        c = x[h:].mean(0)
        x[h:] = (x[h:] - c) @ R + c
        return (0.1 * x).astype(np.float32)

    gen = np.random.default_rng(0)
    chains = []
    for _ in range(8):
        base = trace(gen, 300)
        chains += [member(gen, base) for _ in range(8)]
    xyz = torch.from_numpy(np.concatenate(chains)).to(dev)
    sizes = [300] * 64
    P, cell = 64 * 63 // 2, 300 * 300

    def dp_cells(out, n_pairs, frags, cells_of_pair):
        """(scores-only, traced) cell updates of a call: the fragment pairs; I2's alignment and every (unit, round) that ran"""
        ran = int(np.isfinite(_lib.host(out.history)[..., 0]).sum())
        return n_pairs * frags * cells_of_pair, (n_pairs + ran) * cells_of_pair

    out = sa.align_structures(xyz, sizes, model=m)
    so, tr = dp_cells(out, P, 17 * 17, cell)
    tm = _lib.host(out.tm_a)
    say(f"all pairs of 64 chains of 300: {so:.3e} scores-only and {tr:.3e} traced cell updates; tm_a within a family "
        f"{np.median([tm[p] for p, (i, j) in enumerate((i, j) for i in range(64) for j in range(i + 1, 64)) if i // 8 == j // 8]):.3f} (median), across "
        f"{np.median([tm[p] for p, (i, j) in enumerate((i, j) for i in range(64) for j in range(i + 1, 64)) if i // 8 != j // 8]):.3f}")
    report("align_structures, all pairs of 64 x 300, defaults", lambda: sa.align_structures(xyz, sizes, model=m), so + tr)
    out = sa.align_structures(xyz, sizes, rounds=1, model=m)
    so, tr = dp_cells(out, P, 17 * 17, cell)
    report(f"  rounds = 1 (scores-only {so:.3e}, traced {tr:.3e}): k_sa_dp<false> dominates", lambda: sa.align_structures(xyz, sizes, rounds=1, model=m), so)
    out = sa.align_structures(xyz, sizes, frag_starts=2, model=m)
    so, tr = dp_cells(out, P, 4, cell)
    report(f"  frag_starts = 2 (scores-only {so:.3e}, traced {tr:.3e}): k_sa_dp<true> dominates", lambda: sa.align_structures(xyz, sizes, frag_starts=2, model=m), tr)
    big = trace(gen, 2000)
    two = torch.from_numpy(np.concatenate([member(gen, big), (0.1 * big).astype(np.float32)])).to(dev)
    out = sa.align_structures(two, [2000, 2000], model=m)
    so, tr = dp_cells(out, 1, 16 * 16, 4e6)
    say(f"one pair of 2000 x 2000: tm {float(_lib.host(out.tm_a)[0]):.3f}, rounds run per unit {np.isfinite(_lib.host(out.history)[0, :, :, 0]).sum(1).tolist()}")
    report("align_structures, one pair of 2000 x 2000, defaults", lambda: sa.align_structures(two, [2000, 2000], model=m), so + tr)
open(out_path, "w").write("\n".join(lines) + "\n")
