#!/usr/bin/env python3
"""Timing of the docking kernels (pesto_amd.docking, pesto_docking.hip) beside extract_all_contacts_batch on the same frames.
usage: python profiles/bench_docking.py [out.txt]   (on the GPU box; default profiles/out/docking_bench.txt)

The ensemble: the 2,030 atoms of tests/golden/frames_md_1JTG_uL.npz (frame 0, angstroms) as subunit A and a rotated copy of them docked
beside it (closest atoms 3 A apart) as subunit B, F = 1,000 frames of per-atom Gaussian noise (0.3 A), made on the device from a seed.
Legs, r_thr = 5 A, scale 1:
  frame_contacts    the whole call on ROCm tensors (tiled brute force: count, two scans, emit, the count's synchronisation), contacts per
                    second, and the same call with a capacity of one row - the emit pass returns at once, so what is left is the count
                    pass, the scans and the synchronisation on the count: its share of the whole call
  pesto_contacts    the dataset module's cell-grid contact search on the same frames, each frame an assembly of two subunits:
                    dataset._contacts_call (pesto_contacts: grid build, count, emit, regroup and typed keys; its input is host arrays,
                    uploaded inside the call) and, with the reference-shaped dicts built from it, extract_all_contacts_batch's work
  residue pairs, interface, irmsd, pose     the other entry points on the same ensemble
GPU times are device events around a synchronised window of whole calls after warm-up calls, so they include allocation, every launch
and the stream synchronisation of a call; a kernel trace gives the kernels' own times. The pair-test count comes from the shapes
(OPS_PAIR); the floor is VALU issue at the sampled gfx clock."""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from conftest import golden  # noqa: E402
from pesto_amd import _lib, dataset  # noqa: E402
from pesto_amd import docking as D  # noqa: E402
from pesto_amd.patches import _default_model  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "out", "docking_bench.txt")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
lines = []
dev = torch.device("cuda:0")
N_CU, LANES_PER_CU_CLK, NOMINAL_GHZ = 256, 128, 2.4         # MI355X: 4 SIMDs x 32 lanes per clock
OPS_PAIR = 9                                                # per pair and pass: 3 sub, 3 mul, 2 add, 1 compare (two passes: count, emit)
F, R_THR = 1000, 5.0


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


def source_hash():
    h = hashlib.sha256()
    for rel in ("pesto_amd/csrc/pesto_docking.hip", "pesto_amd/csrc/pesto_geom.h", "pesto_amd/csrc/pesto_fit.h", "pesto_amd/docking.py", "profiles/bench_docking.py"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def docked_pair():
    """(A, B) float32 [N, 3]: the molecule and a rotated copy moved along x until their closest atoms are 3 A apart"""
    a = golden("frames_md_1JTG_uL")["X_frames"][0].astype(np.float64)
    a -= a.mean(0)
    c, s = np.cos(2.0), np.sin(2.0)
    b = a @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    lo, hi = 0.0, 200.0                                     # the closest distance grows with the shift once the copies are apart
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        gap = float(torch.cdist(ta, tb + torch.tensor([mid, 0.0, 0.0], device=dev, dtype=ta.dtype)).min())
        lo, hi = (mid, hi) if gap < 3.0 else (lo, mid)
    return a.astype(np.float32), (b + np.array([hi, 0.0, 0.0])).astype(np.float32)


def ensemble(x0, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.from_numpy(x0).to(dev)[None] + 0.3 * torch.randn((F,) + x0.shape, generator=g, device=dev)).contiguous()


m = _default_model(0)
say(f"device {torch.cuda.get_device_name(0)}; source {source_hash()}; GPU times: device events around a window of whole calls after 2 warm-up "
    f"calls (every call synchronises its stream); clock = gfx clock sampled before / after")
a0, b0 = docked_pair()
xa, xb = ensemble(a0, 1), ensemble(b0, 2)
Na, Nb = a0.shape[0], b0.shape[0]

# ---- frame_contacts: the whole call, and the call whose emit pass has nothing to do
off, pairs, d = D.frame_contacts(xa, xb, R_THR, 1.0, model=m)
K = int(pairs.shape[0])
t, c = timed(lambda: D.frame_contacts(xa, xb, R_THR, 1.0, model=m), 10)
ghz = c if np.isfinite(c) else NOMINAL_GHZ
fl = 2 * F * Na * Nb * OPS_PAIR / (N_CU * LANES_PER_CU_CLK * ghz * 1e9)
say(f"frame_contacts {Na} x {Nb}, F = {F}, r_thr {R_THR} A (tiled brute force): {1e3 * t:.3f} ms per call at {c:.2f} GHz, K = {K} contacts "
    f"({K / F:.0f} per frame), {K / t / 1e6:.1f} M contacts/s, {F * Na * Nb / t / 1e9:.1f} G pair tests/s per pass pair; "
    f"VALU-issue floor {1e3 * fl:.3f} ms ({100 * fl / t:.1f} % of it)")
side = _lib.Side(xa, m._gpu)
lib = _lib.load()
o1, p1, d1, sz = side.empty((F + 1,), np.int64), side.empty((1, 2), np.int32), side.empty((1,), np.float32), np.zeros(1, np.int64)


def count_only():
    _lib.check(lib.pesto_frame_contacts(m.handle, F, Na, Nb, side.ptr(xa), side.ptr(xb), R_THR, 1.0, 1, side.ptr(o1), side.ptr(p1), side.ptr(d1),
                                        sz.ctypes.data, side.kind, side.stream), lib.pesto_docking_last_error)


tc, _ = timed(count_only, 10)
assert int(sz[0]) == K
say(f"    the same call with a capacity of 1 row (count pass, scans, the synchronisation on the count; the emit pass returns at once): "
    f"{1e3 * tc:.3f} ms = {100 * tc / t:.0f} % of the whole call")

# ---- pesto_contacts on the same frames: every frame an assembly of two subunits
ha, hb = xa.cpu().numpy(), xb.cpu().numpy()
za, zb, ta_, tb_ = np.zeros(Na, np.int32), np.zeros(Nb, np.int32), np.full(Na, -1, np.int32), np.full(Nb, -1, np.int32)
rows = [[("A", ha[f], za, ta_, 1), ("B", hb[f], zb, tb_, 1)] for f in range(F)]
out, meta = dataset._contacts_call(m, rows, R_THR, dataset.MOLECULE_IDS, True)
torch.cuda.synchronize()
t0 = time.perf_counter()
out, meta = dataset._contacts_call(m, rows, R_THR, dataset.MOLECULE_IDS, True)
torch.cuda.synchronize()
tg = time.perf_counter() - t0
t0 = time.perf_counter()
dataset._contact_dicts(out, meta)
torch.cuda.synchronize()
td = time.perf_counter() - t0
say(f"pesto_contacts (cell grid; on {F} assemblies of {Na} + {Nb} atoms, host arrays in, ROCm tensors out): {1e3 * tg:.1f} ms per call, "
    f"K = {out['K']} (torch.norm's rounding)  x{tg / t:.1f}; with the reference-shaped dicts of extract_all_contacts_batch: "
    f"{1e3 * (tg + td):.1f} ms  x{(tg + td) / t:.1f}")
del rows, out, meta

# ---- the other entry points
res_a = np.arange(Na) // 8
res_b = np.arange(Nb) // 8
t2, _ = timed(lambda: D.frame_residue_contacts((off, pairs, d), res_a=res_a, res_b=res_b, model=m), 10)
U = int(D.frame_residue_contacts((off, pairs, d), res_a=res_a, res_b=res_b, model=m)[1].shape[0])
say(f"frame_residue_contacts from those lists ({res_a.max() + 1} x {res_b.max() + 1} residues): {1e3 * t2:.3f} ms per call, U = {U} residue pairs")
X = torch.cat([xa, xb], 1).contiguous()
ids_a, ids_b, roa = np.arange(Na), Na + np.arange(Nb), np.concatenate([res_a, res_a.max() + 1 + res_b])
ca = np.zeros(Na + Nb, bool)
ca[1::8] = True
t3, _ = timed(lambda: D.interface_atoms(X, ids_a, ids_b, roa, 10.0, 1.0, model=m), 10)
t4, _ = timed(lambda: D.irmsd(X[:1], X, ids_a, ids_b, roa, ca, 10.0, 1.0, model=m), 10)
t5, _ = timed(lambda: D.interface_rigid_docking(X[:1], X, ids_a, ids_b, roa, 10.0, 1.0, model=m), 10)
ira, irb = D.interface_atoms(X, ids_a, ids_b, roa, 10.0, 1.0, model=m)
say(f"interface_atoms ({Na + Nb} atoms): {1e3 * t3:.3f} ms -> {ira.numel()} + {irb.numel()} atoms; irmsd F = {F}: {1e3 * t4:.3f} ms; "
    f"interface_rigid_docking F = {F}: {1e3 * t5:.3f} ms (each includes its interface_atoms call)")
open(out_path, "w").write("\n".join(lines) + "\n")
