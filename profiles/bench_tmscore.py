#!/usr/bin/env python3
"""Timing of the TM-score / GDT search (pesto_amd.tmscore, pesto_tmscore.hip).
usage: python profiles/bench_tmscore.py [out.txt]   (on the GPU box; default profiles/out/tmscore_bench.txt)

Legs: the seeded system of tests/test_tmscore_fixture.py at L = 300 (a CA-like trace, every frame with 1 A of noise and its second half
moved as a rigid domain), step 1, n_iter 20 - 1,514 seeds per frame:
  one model   F = 1: the seeds of one frame shared out over the device
  a run       F = 1,000 frames in one call
GPU times are device events around a synchronised window of WHOLE calls after warm-up calls, on device tensors: the call's allocation,
the index check, the search, the maximum over the shares, the RMSD launch and the stream synchronisation are inside, so they are upper
bounds on the kernels' own times. The work is double-precision vector arithmetic on LDS-resident points with a data-dependent number of
fits per seed, so no floor is derived from the shapes; the time per seed search is printed instead. A record, not a bar."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from pesto_amd import tmscore as T  # noqa: E402
from pesto_amd.patches import _default_model  # noqa: E402
from test_tmscore_fixture import sweep_system  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "out", "tmscore_bench.txt")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
lines = []
dev = torch.device("cuda:0")
L = 300


def say(s):
    print(s, flush=True)
    lines.append(s)


def clock():
    try:
        return float(torch.cuda.clock_rate(0)) / 1e3
    except Exception:      # noqa: BLE001 - no amdsmi
        return float("nan")


def timed(fn, reps, warm=2):
    """(seconds per call from device events, mean gfx clock in GHz sampled before / after the window)"""
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


m = _default_model(0)
n_seeds = int(T.seed_windows(L, 1).shape[0])
say(f"device {torch.cuda.get_device_name(0)}; GPU times: device events around a window of whole calls after 2 warm-up calls (every call "
    f"synchronises its stream); clock = gfx clock sampled before / after; L = {L}, step 1, n_iter 20: {n_seeds} seeds per frame")
for F, reps in ((1, 1000), (1000, 8)):                  # windows of about half a second, so that the clock has settled
    s = sweep_system(L, F, 0)
    y, x = torch.from_numpy(s["ref"]).to(dev), torch.from_numpy(s["xyz"]).to(dev)
    runs = sorted(timed(lambda: T.tm_score(y, x, model=m), reps) for _ in range(5))
    t, c = runs[2]
    out = T.tm_score(y, x, model=m)
    at = f"{c:.2f} GHz" if np.isfinite(c) else "an unsampled clock"
    say(f"tm_score L = {L}, F = {F}: {1e3 * t:.3f} [{1e3 * runs[0][0]:.3f}, {1e3 * runs[-1][0]:.3f}] ms per call (median [min, max] of 5 windows of "
        f"{reps} calls) at {at}   {F * n_seeds} seed searches, {1e9 * t / (F * n_seeds):.0f} ns each   "
        f"tm {float(out.tm.min()):.3f} .. {float(out.tm.max()):.3f}, gdt_ts {float(out.gdt_ts.min()):.3f} .. {float(out.gdt_ts.max()):.3f}, "
        f"rmsd of the one global fit {float(out.rmsd.min()):.2f} .. {float(out.rmsd.max()):.2f} A")
open(out_path, "w").write("\n".join(lines) + "\n")
