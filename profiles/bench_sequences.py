#!/usr/bin/env python3
"""Timing of the sequence alignment kernels (pesto_amd.sequences, pesto_align.hip).
usage: python profiles/bench_sequences.py [out.txt]   (on the GPU box; default profiles/out/sequences_bench.txt)

Legs, on seeded random 20-letter sequences under BLOSUM62 (11 / 1), "global":
  align_scores        all against all at S = 2048 sequences of length 300 and at S = 256 of length 2000 (four column blocks each)
  cluster_sequences   the same two sets through the clustering call (the links in the scoring launch, no per-pair output)
  align_maps          64 pairs of length 300
A cell update is one (i, j) of one pair: its three states. GPU times are device events around a synchronised window of WHOLE calls after
warm-up calls, on device tensors: the call's allocation, the code check, the launch, the labels and the stream synchronisation are inside,
so the rates are lower bounds on the kernel's own. The host line is the NumPy definition of tests/test_sequences_fixture.py (align_diag)
on one pair, for scale only. A record, not a bar."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from pesto_amd import _lib, sequences as sq  # noqa: E402
from pesto_amd.patches import _default_model  # noqa: E402
from test_sequences_fixture import align_diag  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "out", "sequences_bench.txt")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
lines = []
dev = torch.device("cuda:0")


def say(s):
    print(s, flush=True)
    lines.append(s)


def clock():
    try:
        return float(torch.cuda.clock_rate(0)) / 1e3
    except Exception:      # noqa: BLE001 - no amdsmi
        return float("nan")


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    clk = [clock()]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    clk.append(clock())
    return e0.elapsed_time(e1) / 1e3 / reps, float(np.nanmean(clk))


def report(name, fn, reps, cells):
    runs = sorted(timed(fn, reps) for _ in range(3))
    t, c = runs[1]
    at = f"{c:.2f} GHz" if np.isfinite(c) else "an unsampled clock"
    say(f"{name}: {1e3 * t:.2f} [{1e3 * runs[0][0]:.2f}, {1e3 * runs[-1][0]:.2f}] ms per call (median [min, max] of 3 windows of {reps} calls) at {at}   "
        f"{cells:.3e} cell updates, {cells / t / 1e9:.1f} G cell updates / s")


m = _default_model(0)
rng = np.random.RandomState(0)
say(f"device {torch.cuda.get_device_name(0)}; GPU times: device events around a window of whole calls after a warm-up call (every call "
    f"synchronises its stream); clock = gfx clock sampled before / after; BLOSUM62, 11 / 1, global")
for S, L, reps in ((2048, 300, 3), (256, 2000, 3)):
    codes = torch.from_numpy(rng.randint(0, 20, S * L).astype(np.uint8)).to(dev)
    offs = _lib.offsets([L] * S)
    cells = S * (S - 1) / 2 * L * L
    report(f"align_scores all against all, S = {S}, L = {L}", lambda: sq.align_scores((codes, offs), model=m), reps, cells)
    report(f"cluster_sequences, S = {S}, L = {L}", lambda: sq.cluster_sequences((codes, offs), model=m, _reduce=False), reps, cells)
L = 300
codes = torch.from_numpy(rng.randint(0, 20, 128 * L).astype(np.uint8)).to(dev)
offs = _lib.offsets([L] * 128)
pairs = np.arange(128, dtype=np.int32).reshape(64, 2)
report(f"align_maps, 64 pairs, L = {L}", lambda: sq.align_maps((codes, offs), pairs, model=m), 20, 64 * L * L)
a, b = rng.randint(0, 20, 2000), rng.randint(0, 20, 2000)
t0 = time.perf_counter()
align_diag(a, b, sq.BLOSUM62, 11, 1, "global", 20)
t = time.perf_counter() - t0
say(f"host, for scale: the NumPy definition (align_diag) on one 2000 x 2000 pair: {t:.2f} s, {4e6 / t / 1e6:.1f} M cell updates / s")
open(out_path, "w").write("\n".join(lines) + "\n")
