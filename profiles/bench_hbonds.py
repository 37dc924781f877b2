#!/usr/bin/env python3
"""Timing of the hydrogen-bond and unwrapping kernels (pesto_amd.hbonds, pesto_hbonds.hip) beside their NumPy restatements on the host.
usage: python profiles/bench_hbonds.py [out.txt]   (on the GPU box; default profiles/out/hbonds_bench.txt)

Two systems, F = 512 frames each (frame 0 of tests/golden/pdb/6I9F.pdb.gz in nanometres plus per-atom Gaussian noise of 0.15 A, made on
the device from a seed):
  6I9F      the whole structure, hydrogens included: 2,546 atoms, hbond_tables' 320 donor pairs x 476 acceptors
  6I9F x8   eight copies on a 2 x 2 x 2 lattice 6 nm apart, the tables repeated per copy: 20,368 atoms, 2,560 x 3,808
Legs, at the defaults (r_thr 2.5 A, angle 120 degrees, scale 10):
  frame_hbonds      the whole call on ROCm tensors (index check, count, two scans, emit, the count's synchronisation)
  baker_hubbard     the whole call at freq = 0.1 (index check, count over the frames, two scans, emit: the frames are walked twice)
  unwrap_pbc        the whole call; the molecules are the two residue halves (6I9F) or the eight copies (x8), each but the first
                    displaced by a seeded periodic image; unit masses
GPU times are device events around one whole call, after 2 warm-up calls, the median of 9 repeats; they include the call's allocation,
every launch and its stream synchronisation. The distance-test rate is the kernel's own count, F * P * A tests per pass over the
candidates (two passes per call), divided by the call's time. The NumPy column times the restatements of tests/test_hbonds_fixture.py
(the definitions the GPU tests compare against, vectorised per frame on [P, A] arrays) on the first HOST_FRAMES frames with
time.perf_counter and scales to F frames; it is the yardstick on the host, not the reference: mdtraj is not available here."""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from test_hbonds_fixture import IMAGES, frame_hbonds_def, occupancy_def, read_structure, unwrap_def  # noqa: E402
from pesto_amd import hbonds as H  # noqa: E402
from pesto_amd.patches import _default_model  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "out", "hbonds_bench.txt")
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
lines = []
dev = torch.device("cuda:0")
F, REPEATS, WARM = 512, 9, 2
HOST_FRAMES = {"6I9F": 16, "6I9F x8": 2}


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    """median seconds of one call, from device events"""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    return float(np.median(ts))


def host_timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def source_hash():
    h = hashlib.sha256()
    for rel in ("pesto_amd/csrc/pesto_hbonds.hip", "pesto_amd/csrc/pesto_geom.h", "pesto_amd/csrc/pesto_scan.h", "pesto_amd/hbonds.py",
                "profiles/bench_hbonds.py"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def ensemble(x0, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.from_numpy(x0).to(dev)[None].repeat(F, 1, 1)
    x[1:] += 0.015 * torch.randn((F - 1,) + x0.shape, generator=g, device=dev)
    return x.contiguous()


m = _default_model(0)
say(f"device {torch.cuda.get_device_name(0)}; source {source_hash()}; F = {F}; GPU times: device events around one whole call, median of {REPEATS} "
    f"after {WARM} warm-up calls (every call synchronises its stream)")
st = read_structure("6I9F.pdb")
dh1, acc1 = H.hbond_tables(st)
x1 = (st["xyz"].astype(np.float64) - np.round(st["xyz"].astype(np.float64).mean(0))).astype(np.float32) * np.float32(0.1)
n1 = x1.shape[0]
half = (st["resid"] >= np.median(np.unique(st["resid"]))).astype(np.int32)
lattice = np.array([(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float32) * np.float32(6.0)
systems = {
    "6I9F": (x1, dh1, acc1, half),
    "6I9F x8": (np.concatenate([x1 + s for s in lattice]), np.concatenate([dh1 + c * n1 for c in range(8)]).astype(np.int32),
                np.concatenate([acc1 + c * n1 for c in range(8)]).astype(np.int32), np.repeat(np.arange(8, dtype=np.int32), n1)),
}
rng = np.random.default_rng(11)
for name, (x0, dh, acc, mol) in systems.items():
    N, P, A, M = x0.shape[0], dh.shape[0], acc.shape[0], int(mol.max()) + 1
    xyz = ensemble(x0, 5)
    dh_d, acc_d = torch.from_numpy(dh).to(dev), torch.from_numpy(acc).to(dev)
    hf = HOST_FRAMES[name]
    xh = xyz[:hf].cpu().numpy()
    tests = F * P * A
    say(f"{name}: N = {N} atoms, P = {P} donor pairs, A = {A} acceptors, {P * A / 1e6:.2f} M candidates per frame")

    off, trip, d = H.frame_hbonds(xyz, dh_d, acc_d, model=m)
    K = int(trip.shape[0])
    t = timed(lambda: H.frame_hbonds(xyz, dh_d, acc_d, model=m))
    th = host_timed(lambda: frame_hbonds_def(xh, dh, acc)) * F / hf
    w_off = frame_hbonds_def(xh, dh, acc)[0]
    assert np.array_equal(off[:hf + 1].cpu().numpy(), w_off)
    say(f"    frame_hbonds   {1e3 * t:9.3f} ms per call, K = {K} bonds ({K / F:.0f} per frame), {2 * tests / t / 1e9:.1f} G distance tests/s "
        f"(2 passes of {tests / 1e9:.3f} G); NumPy restatement {th:.2f} s for {F} frames (timed on {hf})  x{th / t:.0f}")

    tr, cn = H.baker_hubbard(xyz, dh_d, acc_d, 0.1, model=m, return_counts=True)
    t = timed(lambda: H.baker_hubbard(xyz, dh_d, acc_d, 0.1, model=m))
    th = host_timed(lambda: occupancy_def(xh, dh, acc, 0.1)) * F / hf
    say(f"    baker_hubbard  {1e3 * t:9.3f} ms per call, {int(tr.shape[0])} triplets above freq 0.1, {2 * tests / t / 1e9:.1f} G distance tests/s "
        f"(2 passes of {tests / 1e9:.3f} G); NumPy restatement {th:.2f} s for {F} frames (timed on {hf})  x{th / t:.0f}")

    box = np.tile(np.array([[14.0, 15.0, 16.0]], np.float32), (F, 1))
    images = rng.integers(0, 27, (F, M))
    images[:, 0] = 0
    shift = torch.from_numpy((box[:, None, :] * IMAGES[images].astype(np.float32))[:, mol]).to(dev)
    wrapped = (xyz - shift).contiguous()
    box_d, mol_d, mass_d = torch.from_numpy(box).to(dev), torch.from_numpy(mol).to(dev), torch.ones(N, dtype=torch.float64, device=dev)
    out, img = H.unwrap_pbc(wrapped, box_d, mol_d, mass_d, model=m, return_images=True)
    assert np.array_equal(img.cpu().numpy(), images)
    t = timed(lambda: H.unwrap_pbc(wrapped, box_d, mol_d, mass_d, model=m))
    wh = wrapped[:hf].cpu().numpy()
    th = host_timed(lambda: unwrap_def(wh, box[:hf], mol, np.ones(N))) * F / hf
    say(f"    unwrap_pbc     {1e3 * t:9.3f} ms per call, M = {M} molecules, {F * N * 24 / t / 1e9:.1f} GB/s of coordinates read and written "
        f"(the mol table goes through the host); NumPy restatement {th:.2f} s for {F} frames (timed on {hf})  x{th / t:.0f}")
    del xyz, wrapped, shift, out
open(out_path, "w").write("\n".join(lines) + "\n")
