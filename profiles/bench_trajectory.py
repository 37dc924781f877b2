#!/usr/bin/env python3
"""Timing of the MD-analysis kernels (pesto_amd.trajectory, pesto_trajectory.hip) beside the reference's formulation.
usage: python profiles/bench_trajectory.py [out.txt]   (on the GPU box; default profiles/out/trajectory_bench.txt)

Legs (seeded synthetic ensembles shaped like tests/golden/trajectory.npz: frame 0 of the fixture plus Gaussian noise of 0.3 A per atom and
a drift of the second side by 0 to 6 A, made on the device):
  iface      274 x 285 interface atoms, F = 5,000 and F = 50,000, 20 bins: contacts_distribution (fit) and loglikelihood
  self       1,235 x 1,235 atoms (a chain against itself), F = 500, 20 bins: contacts_distribution
  maps       707 x 701 atoms in 91 x 87 residues, F = 5,000: residue_contact_maps and fnat
  superpose  3,265 atoms, F = 5,000: superpose onto frame 0 (fit on every 7th atom) and residue_centroids
Beside each: the method a user of the reference has today, restated here in this project's own code. For the contacts model that is a
per-frame loop of torch operations on the SAME GPU that builds a dense [Na, Nb, bins] mask per frame (what contacts_distribution and
loglikelihood of statistical_contacts_model.py do), timed on a subset of the frames and scaled where the output says so; for the centroids
a dense [N, R] matrix product in torch on the same GPU; for fnat NumPy on the host, one distance tensor per residue pair (timed on a
subset of the frames and scaled); for the superposition NumPy on the host in float32 with a batched SVD (the difference printed beside
it is that float32 evaluation's own error at these coordinates).
GPU times are device events around a synchronised window of WHOLE calls after warm-up calls: allocation, the threshold-table upload, every
launch of the call and its stream synchronisation are inside, so they are upper bounds on the kernels' own times (a kernel trace gives
those). Operation and byte counts come from the shapes (OPS_PAIR and the byte expressions below); the floor is the larger of the two at
the sampled gfx clock and names which one binds."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from conftest import golden  # noqa: E402
from pesto_amd import trajectory as T  # noqa: E402
from pesto_amd.patches import _default_model  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "out", "trajectory_bench.txt")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
lines = []
dev = torch.device("cuda:0")
BINS = np.linspace(0.0, 10.0, 21)
N_CU, LANES_PER_CU_CLK, HBM_BPS = 256, 128, 8.0e12          # MI355X: 4 SIMDs x 32 lanes per clock (a wave64 VALU instruction issues over 2 cycles); 8 TB/s HBM3E
# per pair-frame: 3 sub, 3 mul, 2 add, 2 range compares (the bin search and the counter update run on the hits only)
OPS_PAIR = 10
NOMINAL_GHZ = 2.4


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


def floor(ops, nbytes, ghz):
    ghz = ghz if np.isfinite(ghz) else NOMINAL_GHZ           # (report() says so when the clock could not be sampled)
    t_ops, t_mem = ops / (N_CU * LANES_PER_CU_CLK * ghz * 1e9), nbytes / HBM_BPS
    return (t_ops, "VALU issue") if t_ops >= t_mem else (t_mem, "HBM bandwidth")


def report(name, t, ghz, ops, nbytes, base=None, base_name="", base_note=""):
    fl, which = floor(ops, nbytes, ghz)
    at = f"{ghz:.2f} GHz" if np.isfinite(ghz) else f"an unsampled clock (floor at the nominal {NOMINAL_GHZ} GHz)"
    s = (f"{name}: {1e3 * t:.3f} ms at {at}   {ops / 1e9:.2f} Gop, {nbytes / 1e6:.1f} MB -> floor {1e3 * fl:.3f} ms ({which}), "
         f"{100 * fl / t:.1f} % of it")
    if base is not None:
        s += f"   {base_name}{base_note}: {1e3 * base:.1f} ms  x{base / t:.1f}"
    say(s)


def ensemble(x0, F, seed, drift_axis=None):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.from_numpy(x0).to(dev)[None] + 0.3 * torch.randn((F,) + x0.shape, generator=g, device=dev)
    if drift_axis is not None:
        x = x + torch.linspace(0.0, 6.0, F, device=dev)[:, None, None] * torch.from_numpy(drift_axis.astype(np.float32)).to(dev)[None, None]
    return x.contiguous()


def frame_onehot(fa, fb, lower, upper):
    """[Na, Nb, B] float mask of ONE frame: which bin each pair's distance is in (the dense per-frame tensor the per-frame method builds)"""
    delta = fa[:, None, :] - fb[None, :, :]
    dist = (delta * delta).sum(-1).sqrt()[..., None]
    return ((dist >= lower) & (dist < upper)).to(torch.float32)


def edges_on_device(bins):
    e = torch.as_tensor(np.asarray(bins), device=dev)
    return e[:-1].view(1, 1, -1), e[1:].view(1, 1, -1)


def loop_distribution(fa, fb, bins):
    """the per-frame method: one dense [Na, Nb, B] mask per frame, accumulated, then normalised"""
    lower, upper = edges_on_device(bins)
    total = torch.zeros((fa.shape[1], fb.shape[1], len(bins) - 1), device=dev)
    for f in range(fa.shape[0]):
        total += frame_onehot(fa[f], fb[f], lower, upper)
    return total / (total.sum(-1, keepdim=True) + 1e-6)


def loop_loglikelihood(fa, fb, bins, P):
    """the per-frame method: the dense mask of each frame selects its P entries, -mean(log(1 - p + floor(p))) per frame"""
    lower, upper = edges_on_device(bins)
    out = torch.empty(fa.shape[0], device=dev)
    for f in range(fa.shape[0]):
        picked = P * frame_onehot(fa[f], fb[f], lower, upper)
        out[f] = -(1.0 - picked + picked.floor()).log().mean()
    return out


def scaled(fn, F, sub):
    """fn(sub frames) timed once after one warm-up on 8 frames, scaled to F frames"""
    fn(8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(sub)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * F / sub, ("" if sub == F else f", timed on {sub} frames and scaled")


def from256(q):
    return (q.astype(np.float64) / 256.0).astype(np.float32)


m = _default_model(0)
g = golden("trajectory")
say(f"device {torch.cuda.get_device_name(0)}; GPU times: device events around a window of calls after 2 warm-up calls (every call synchronises its "
    f"stream); clock = gfx clock sampled before / after; floors at {N_CU} CUs x {LANES_PER_CU_CLK} fp32 lanes per clock and {HBM_BPS / 1e12:.0f} TB/s")

# ---- iface
a0, b0 = from256(g["iface_a256"][0]), from256(g["iface_b256"][0])
axis = b0.mean(0) - a0.mean(0)
axis /= np.linalg.norm(axis)
for F in (5000, 50000):
    xa, xb = ensemble(a0, F, 1), ensemble(b0, F, 2, axis)
    Na, Nb, B = a0.shape[0], b0.shape[0], 20
    t, c = timed(lambda: T.contacts_distribution(xa, xb, BINS, model=m), 5)
    tb, note = scaled(lambda n: loop_distribution(xa[:n], xb[:n], BINS), F, 1000)
    report(f"iface {Na} x {Nb}, F = {F}: contacts_distribution", t, c, F * Na * Nb * OPS_PAIR, F * (Na + Nb) * 12 + Na * Nb * B * 8, tb,
           "per-frame loop in torch on this GPU", note)
    P = T.contacts_distribution(xa, xb, BINS, model=m)
    t, c = timed(lambda: T._loglik(xa, xb, BINS, P, m), 5)
    tb, note = scaled(lambda n: loop_loglikelihood(xa[:n], xb[:n], BINS, P), F, 1000)
    report(f"iface {Na} x {Nb}, F = {F}: loglikelihood", t, c, F * Na * Nb * OPS_PAIR, F * (Na + Nb) * 12 + Na * Nb * B * 4 + F * 4, tb,
           "per-frame loop in torch on this GPU", note)
    del xa, xb, P

# ---- self
c0 = from256(g["chain1_256"][0])
F, N, B = 500, c0.shape[0], 20
xs = ensemble(c0, F, 3)
t, c = timed(lambda: T.contacts_distribution(xs, xs, BINS, model=m), 5)
tb, note = scaled(lambda n: loop_distribution(xs[:n], xs[:n], BINS), F, 100)
report(f"self {N} x {N}, F = {F}: contacts_distribution", t, c, F * N * N * OPS_PAIR, F * N * 12 + N * N * B * 8, tb,
       "per-frame loop in torch on this GPU", note)
del xs

# ---- maps + fnat
a0, b0 = from256(g["iface10_a256"][0]) * np.float32(0.1), from256(g["iface10_b256"][0]) * np.float32(0.1)
ra, rb = g["iface10_res_a"].astype(np.int64), g["iface10_res_b"].astype(np.int64)
F, Na, Nb = 5000, a0.shape[0], b0.shape[0]
axis = b0.mean(0) - a0.mean(0)
axis /= np.linalg.norm(axis)
xa = torch.from_numpy(a0).to(dev)[None] + 0.1 * (ensemble(a0 * 10, F, 4) - torch.from_numpy(a0 * 10).to(dev)[None])
xb = torch.from_numpy(b0).to(dev)[None] + 0.1 * (ensemble(b0 * 10, F, 5, axis) - torch.from_numpy(b0 * 10).to(dev)[None])
xa, xb = xa.contiguous(), xb.contiguous()


def maps_fnat():
    mp = T.residue_contact_maps(xa, xb, ra, rb, model=m)
    return T.fnat(mp[:1], mp, model=m)


t, c = timed(maps_fnat, 5)
sub = 50
ha, hb = xa[:sub].cpu().numpy(), xb[:sub].cpu().numpy()
groups_a = [np.nonzero(ra == r)[0] for r in range(int(ra.max()) + 1)]
groups_b = [np.nonzero(rb == r)[0] for r in range(int(rb.max()) + 1)]
t0 = time.perf_counter()
touch = np.zeros((sub, len(groups_a), len(groups_b)), bool)
for r, ia in enumerate(groups_a):                 # the host method: one small distance tensor over all frames per residue pair
    pa = ha[:, ia, None, :]
    for q, ib in enumerate(groups_b):
        gap = pa - hb[:, None, ib, :]
        touch[:, r, q] = (np.sqrt((gap * gap).sum(-1)) * 10.0 < 5.0).reshape(sub, -1).any(-1)
fn = (touch & touch[:1]).sum((1, 2)) / touch[:1].sum()
tb = (time.perf_counter() - t0) * F / sub
assert np.array_equal(fn, maps_fnat()[:sub].cpu().numpy())
report(f"maps {Na} x {Nb} atoms, {len(groups_a)} x {len(groups_b)} residues, F = {F}: residue_contact_maps + fnat", t, c, F * Na * Nb * 9,
       F * (Na + Nb) * 12 + 2 * F * len(groups_a) * len(groups_b), tb, "NumPy on the host (a loop over residue pairs)",
       f", timed on {sub} frames and scaled; an early exit per residue pair skips most of the counted operations")
del xa, xb

# ---- superposition and centroids
f = golden("frames_md_1JTG_uL")
x0 = np.concatenate([f["X_frames"][0], c0 + np.float32(60.0)])
roa = np.concatenate([f["res_of_atom"].astype(np.int64), int(f["res_of_atom"].max()) + 1 + np.arange(c0.shape[0]) // 8])
F, N, R = 5000, x0.shape[0], int(roa.max()) + 1
X = ensemble(x0, F, 6)
sel = np.arange(1, N, 7)
t, c = timed(lambda: T.superpose(X[:1], X, sel, sel, model=m), 5)
Xh = X.cpu().numpy()
t0 = time.perf_counter()
mov, fix = Xh[:, sel], Xh[:1, sel]               # the host method: float32 means and covariance, LAPACK's batched SVD
c_mov, c_fix = mov.mean(1, keepdims=True), fix.mean(1, keepdims=True)
cov = np.einsum("fna,fnb->fab", fix - c_fix, mov - c_mov)
Uh, _, Wh = np.linalg.svd(cov)
Wh[:, 2] *= np.sign(np.linalg.det(Uh) * np.linalg.det(Wh))[:, None]
rot = np.einsum("fka,fbk->fab", Wh, Uh)
sup = (np.einsum("fna,fac->fnc", Xh - c_mov, rot) + c_fix).astype(np.float32)
tb = time.perf_counter() - t0
err = float(np.abs(sup - T.superpose(X[:1], X, sel, sel, model=m).cpu().numpy()).max())
report(f"superpose {N} atoms (fit on {sel.size}), F = {F}", t, c, F * (sel.size * 50 + N * 18), F * (sel.size * 3 + 2 * N) * 12, tb,
       "NumPy on the host (float32, batched SVD)", f"; max |difference| {err:.1e}")
t, c = timed(lambda: T.residue_centroids(X, roa, R, model=m), 5)
onehot = torch.nn.functional.one_hot(torch.from_numpy(roa).to(dev), R).to(torch.float32)      # [N, R]: the dense residue matrix
size = onehot.sum(0)
tb, _ = timed(lambda: torch.einsum("fnc,nr->frc", X, onehot) / size[None, :, None], 5)
report(f"residue_centroids {N} atoms -> {R} residues, F = {F}", t, c, F * N * 3, F * (N + R) * 12, tb, "a dense [N, R] matrix product in torch on this GPU", "")
open(out_path, "w").write("\n".join(lines) + "\n")
