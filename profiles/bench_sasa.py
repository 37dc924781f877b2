#!/usr/bin/env python3
"""Timing of the solvent-accessible-surface-area kernels (pesto_amd.sasa, pesto_sasa.hip).
usage: python profiles/bench_sasa.py [out.txt]   (on the GPU box; default profiles/out/sasa_bench.txt)

Legs (960 sphere points, 1.4 A probe, radii from the element table; inputs on the device):
  md       the 29 frames x 2,030 atoms of tests/golden/frames_md_1JTG_uL.npz tiled to 1,024 frames, one call: us per frame, ns per atom
  batch    the four structures of the golden's batch case, sixteen times over: a ragged batch of 64 structures in one call, structures/s
  cloud    one synthetic cloud of 20,000 atoms (topology.synthetic_cloud, 0.05 atoms / A^3), radius 1.7 + 1.4
Every time is of WHOLE calls: device events around a window of calls after warm-up calls; allocation, the six launches and the stream
synchronisation of each call are inside. The split: the same call stopped after the grid build (PESTO_SASA_DEBUG=1: sigma, setup, count,
scan, scatter) is timed in the same way and the point pass (with the area kernel) is the difference. The ordering choice: the call as
shipped beside the call without the kernel's occluder-ordering step (PESTO_SASA_DEBUG=2, see pesto_sasa.hip), alternating, with equal
counts asserted. No CPU library is timed: mdtraj is not available here, and the NumPy restatement of the tests is not a competitor.
The number of executed point-occluder tests is not counted (no debug build counts them); the all-pairs figure without early exit comes
from the candidate lists of the golden generator (960 x N x mean candidates)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from conftest import golden  # noqa: E402
from pesto_amd import sasa as SA  # noqa: E402
from pesto_amd.patches import _default_model  # noqa: E402
from pesto_amd.topology import synthetic_cloud  # noqa: E402
from test_sasa_fixture import batch_structures  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "out", "sasa_bench.txt")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
lines = []
dev = torch.device("cuda:0")
PROBE = np.float32(1.4)


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps, warm=2):
    """seconds per call from device events around `reps` calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / reps


def mode(bits):
    if bits:
        os.environ["PESTO_SASA_DEBUG"] = str(bits)
    else:
        os.environ.pop("PESTO_SASA_DEBUG", None)


def leg(name, x, r, sizes, reps, unit):
    """whole call, grid build alone, and the call without the occluder-ordering step (three rounds, alternating)"""
    call = lambda: SA.shrake_rupley(x, radii=r, probe_radius=0.0, sizes=sizes, model=m, return_counts=True)      # noqa: E731
    mode(0)
    counts = call()[1]
    mode(2)
    assert torch.equal(call()[1], counts), "the counts depend on the occluder order"
    t_all, t_grid, t_plain = [], [], []
    for _ in range(3):
        mode(0)
        t_all.append(timed(call, reps))
        mode(1)
        t_grid.append(timed(call, reps))
        mode(2)
        t_plain.append(timed(call, reps))
    mode(0)
    F, N = (1, int(x.shape[0])) if x.dim() == 2 else (int(x.shape[0]), int(x.shape[1]))
    ta, tg, tp = min(t_all), min(t_grid), min(t_plain)
    say(f"{name}: F = {F}, N = {N}, {len(sizes) if sizes else 1} structure(s) per frame; whole call {1e3 * ta:.3f} ms "
        f"(three rounds: {', '.join(f'{1e3 * t:.3f}' for t in t_all)}), grid build {1e3 * tg:.3f} ms, point pass + areas {1e3 * (ta - tg):.3f} ms")
    say(f"    {unit(ta)}; {1e9 * ta / (F * N):.2f} ns per atom, {1e9 * (ta - tg) / (F * N):.2f} ns per atom in the point pass; "
        f"mean exposed points {float(counts.float().mean()):.1f} of 960")
    say(f"    without the occluder-ordering step: whole call {1e3 * tp:.3f} ms ({', '.join(f'{1e3 * t:.3f}' for t in t_plain)}): "
        f"the step is x{tp / ta:.3f} on the call, x{(tp - tg) / (ta - tg):.3f} on the point pass")


m = _default_model(0)
say(f"device {torch.cuda.get_device_name(0)}; whole calls, device events around a window of calls after 2 warm-up calls; best of three "
    f"alternating rounds; P = 960")

f = golden("frames_md_1JTG_uL")
g = golden("sasa")
X = np.tile(f["X_frames"], (36, 1, 1))[:1024]
leg("md", torch.from_numpy(np.ascontiguousarray(X)).to(dev), torch.from_numpy(g["md_R"]).to(dev), None, 5,
    lambda t: f"{1e6 * t / 1024:.2f} us per frame")

structs = batch_structures(g)
xs = np.concatenate([s[1] for s in structs] * 16)
rs = np.concatenate([SA.atomic_radii(s[2]) + PROBE for s in structs] * 16)
sizes = [s[1].shape[0] for s in structs] * 16
leg("batch", torch.from_numpy(xs).to(dev), torch.from_numpy(rs).to(dev), sizes, 20, lambda t: f"{64 / t:.0f} structures per second")

xc = synthetic_cloud(20000)
leg("cloud", torch.from_numpy(xc).to(dev), torch.full((20000,), float(np.float32(1.7) + PROBE), device=dev), None, 20,
    lambda t: f"{1e3 * t:.3f} ms per cloud")
open(out_path, "w").write("\n".join(lines) + "\n")
