#!/usr/bin/env python3
"""Generate the MD-analysis golden (tests/golden/trajectory.npz) by IMPORTING the reference's own md_analysis/mdtraj_utils modules
(statistical_contacts_model.py, trajectory_utils.py) from /root/reference (build container only; nothing under tests/ reads the
reference at run time). mdtraj is stubbed (no function that is called needs it) and the two modules are imported as submodules of a stub
package, because the package's own __init__ also wants parmed. Everything runs on the CPU.

Cases
  iface     1JTG_C.pdb (md_analysis/pdbs_clusters, chains 0 and 1) read with the package's own reader; the atoms of the residues with an
            atom within 5 A of the other chain (interface_residues_within's rule restated); F = 64 frames = frame 0 plus per-atom Gaussian
            noise (sigma 0.3 A) and a rigid drift of chain 1 away from chain 0 (0 to 6 A along the line between the interface centroids).
            A second ensemble of the same atoms (24 frames, another seed, sigma 0.6 A, no drift) plays the other side for L and KL.
            Coordinates are multiples of 1/256 A, stored as int16 offsets from the interface's centre (<case>_xyz256).
  iface10   the same at 10 A, F = 32, in nanometres (float32(A) * float32(0.1)), with res_a / res_b, for the contact maps (r_thr 5 and 4.1)
  planted   distances exactly on a bin edge and one float32 ulp either side, on r_thr / scale and one ulp either side, 0, NaN, beyond the
            last edge; B = 64 with the edges 0.1 * k (not float32 values) and B = 1; a single-atom residue, non-contiguous residue rows
  superpose the 29 frames of frames_md_1JTG_uL.npz (referenced, not duplicated) onto frame 0, on all atoms and on a selection (every
            CA-like 7th atom), plus frame 5 mirrored; residue centroids of the 29 frames (no reference function can be
            imported for them: a float32 restatement, torch.index_add_ over the residue sizes, stands for the notebook's expression)
Recorded: the inputs, the reference's outputs (P as integer counts: the generator asserts that float32(count) / (float32(sum) + 1e-6f)
reproduces the reference's P bit for bit), for every floating-point output a float64 restatement of the definition on the same float32
inputs (for the two large ones, superposed coordinates and centroids, the float64 t, R, t_ref and the test's own restatement stand in)
and e_ref, the reference's maximum deviation from it. Asserted about the inputs: the reference's counts (torch's CPU sqrt, not correctly
rounded) equal the definition's (correctly rounded sqrt) on every case; no superposition frame is degenerate.

Usage:  python tests/golden/make_trajectory_golden.py
"""
import importlib
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
SEEDS = {"iface": 7, "iface_other": 11, "iface10": 13}
BINS = np.linspace(0.0, 10.0, 21)


def import_reference():
    import torch
    sys.modules.setdefault("mdtraj", types.ModuleType("mdtraj"))
    pkg = types.ModuleType("mdtraj_utils")
    pkg.__path__ = [os.path.join(REF, "md_analysis", "mdtraj_utils")]
    sys.modules["mdtraj_utils"] = pkg
    tu = importlib.import_module("mdtraj_utils.trajectory_utils")
    scm = importlib.import_module("mdtraj_utils.statistical_contacts_model")
    return tu, scm, torch


class Traj:
    def __init__(self, xyz):
        self.xyz = xyz


# ------------------------------------------------------------------ the definitions (NumPy; correctly rounded float32 sqrt)
def dist(x0, x1):
    return np.sqrt(np.sum(np.square(x0[:, :, None, :] - x1[:, None, :, :]), -1))


def hits(x0, x1, bins):
    """int [F, Na, Nb]: the bin of every pair-frame, -1 for none"""
    d = dist(x0, x1).astype(np.float64)
    b = np.searchsorted(bins, d, side="right") - 1
    return np.where((d >= bins[0]) & (d < bins[-1]), b, -1)


def counts_def(x0, x1, bins):
    h = hits(x0, x1, bins)
    B = len(bins) - 1
    c = np.zeros(h.shape[1:] + (B,), np.int64)
    for b in range(B):
        c[..., b] = (h == b).sum(0)
    return c


def p_of_counts(c):
    return c.astype(np.float32) / (c.sum(-1).astype(np.float32) + np.float32(1e-6))[..., None]


def loglik64(x0, x1, bins, P):
    h = hits(x0, x1, bins)
    p = np.take_along_axis(P.astype(np.float64)[None], np.maximum(h, 0)[..., None], -1)[..., 0]
    term = np.where(h >= 0, np.log(1.0 - p + np.floor(p)), 0.0)
    return -term.sum((1, 2)) / (P.size)


def kl64(P, Q):
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    R = Q / (P + np.float64(np.float32(1e-6)))
    R[R < np.float64(np.float32(1e-6))] = 1.0
    return -np.sum(P * np.log(R), -1)


def superpose64(ref, xyz):
    ref, xyz = ref.astype(np.float64), xyz.astype(np.float64)
    t, tr = xyz.mean(1, keepdims=True), ref.mean(1, keepdims=True)
    U, S, Vt = np.linalg.svd(np.einsum("fna,fnb->fab", ref - tr, xyz - t))
    Vt[:, 2] *= np.sign(np.linalg.det(U) * np.linalg.det(Vt))[:, None]                   # the reflection folded into the last right vector
    return t, np.einsum("fka,fbk->fab", Vt, U), tr, S


def maps_def(xa, xb, res_a, res_b, r_thr, scale):
    c = dist(xa, xb) * np.float32(scale) < np.float32(r_thr)
    Ra, Rb = res_a.max() + 1, res_b.max() + 1
    m = np.zeros((xa.shape[0], Ra, Rb), bool)
    for r in range(Ra):
        rows = c[:, res_a == r].any(1)
        for s in range(Rb):
            m[:, r, s] = rows[:, res_b == s].any(1)
    return m.astype(np.uint8)


# ------------------------------------------------------------------ cases
def interface(r_cut):
    from pesto_amd.structure_io import Structure
    d = Structure.read_pdb(os.path.join(REF, "md_analysis", "pdbs_clusters", "1JTG_C.pdb")).to_dict()
    xyz, chain, resid = d["xyz"].astype(np.float32), d["chain_name"].astype(str), d["resid"]
    assert not np.any(np.char.upper(d["element"].astype(str)) == "H")
    chain = np.char.partition(chain, ":")[:, 0]                        # (the reader appends the model number)
    ia, ib = np.nonzero(chain == "0")[0], np.nonzero(chain == "1")[0]
    assert ia.size == 2030 and ib.size == 1235
    D = np.sqrt(np.sum(np.square(xyz[ia][:, None] - xyz[ib][None]), -1))
    ca, cb = np.nonzero(D <= r_cut)
    sel_a = ia[np.isin(resid[ia], np.unique(resid[ia][ca]))]
    sel_b = ib[np.isin(resid[ib], np.unique(resid[ib][cb]))]
    res_a = np.unique(resid[sel_a], return_inverse=True)[1]
    res_b = np.unique(resid[sel_b], return_inverse=True)[1]
    return xyz[sel_a], xyz[sel_b], res_a.astype(np.int16), res_b.astype(np.int16), xyz[ib]


def ensemble(x0a, x0b, F, seed, sigma, drift):
    """int16 [F, N, 3] pairs: multiples of 1/256 A around the interface's centre; frame 0 is the structure itself"""
    rng = np.random.default_rng(seed)
    centre = np.round(np.concatenate([x0a, x0b]).mean(0))
    axis = x0b.mean(0) - x0a.mean(0)
    axis /= np.linalg.norm(axis)
    out = []
    for x0, moves in ((x0a, 0.0), (x0b, 1.0)):
        x = np.repeat((x0 - centre)[None].astype(np.float64), F, 0)
        x[1:] += rng.normal(0.0, sigma, x[1:].shape)
        x += (np.linspace(0.0, drift, F) * moves)[:, None, None] * axis[None, None]
        q = np.round(x * 256.0)
        assert np.abs(q).max() < 32768
        out.append(q.astype(np.int16))
    return out


def from256(q, nm=False):
    x = (q.astype(np.float64) / 256.0).astype(np.float32)
    return x * np.float32(0.1) if nm else x


def plant(target, torch):
    """a float32 point whose float32 distance from the origin is exactly ``target`` under NumPy's sqrt and torch's CPU sqrt"""
    target = np.float32(target)
    if np.isnan(target):
        return np.array([np.nan, 0, 0], np.float32)
    for y in [0.0] + [float(target) * k / 16 for k in range(1, 16)]:
        x = np.float32(np.sqrt(max(float(target) ** 2 - y * y, 0.0)))
        for dx in range(-3, 4):
            xx = x
            for _ in range(abs(dx)):
                xx = np.nextafter(xx, np.float32(np.inf if dx > 0 else -np.inf))
            p = np.array([xx, np.float32(y), 0], np.float32)
            d_np = np.sqrt(np.sum(np.square(p)))
            d_pt = torch.sqrt(torch.sum(torch.pow(torch.from_numpy(p), 2))).numpy()
            if d_np == target and d_pt == target:
                return p
    raise AssertionError(f"no placement for {target!r}")


def ulps(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def ceil32(e):
    v = np.float32(e)
    return np.nextafter(v, np.float32(np.inf)) if float(v) < e else v


def main():
    tu, scm, torch = import_reference()
    cpu = torch.device("cpu")
    out, e_ref = {}, {}

    def floats(key, ref, f64, store64=True):
        e = float(np.max(np.abs(np.asarray(ref, np.float64) - f64)))
        out[key + "_ref"] = np.asarray(ref) if np.asarray(ref).size < 4096 else np.asarray(ref, np.float32)    # (R comes as float64)
        if store64:
            out[key + "_f64"] = np.asarray(f64, np.float64)
        out[key + "_eref"] = np.float64(e)
        e_ref[key] = e

    def contacts_case(name, x0, x1, bins, self_=False):
        P_ref = scm.contacts_distribution(x0, x0 if self_ else x1, bins, device=cpu)
        c = counts_def(x0, x0 if self_ else x1, bins)
        assert np.array_equal(P_ref, p_of_counts(c)), name        # the reference's counts are the definition's, and P is its formula
        assert c.max() < 256
        out[name + "_counts"] = c.astype(np.uint8)
        out[name + "_bins"] = np.asarray(bins, np.float64)
        return P_ref, c

    # ---- iface
    xa0, xb0, _, _, _ = interface(5.0)
    assert (xa0.shape[0], xb0.shape[0]) == (274, 285)
    qa, qb = ensemble(xa0, xb0, 64, SEEDS["iface"], 0.3, 6.0)
    ua, ub = ensemble(xa0, xb0, 24, SEEDS["iface_other"], 0.6, 0.0)
    out.update(iface_a256=qa, iface_b256=qb, iface_other_a256=ua, iface_other_b256=ub)
    xa, xb, ya, yb = from256(qa), from256(qb), from256(ua), from256(ub)
    P_bnd, c = contacts_case("iface", xa, xb, BINS)
    hit = c.sum(-1) > 0
    two = (c > 0).sum(-1) >= 2
    assert hit.mean() >= 0.1 and two.sum() >= 0.5 * hit.sum(), (hit.mean(), two.sum() / hit.sum())
    P_oth, _ = contacts_case("iface_other", ya, yb, BINS)
    m = scm.StatisticalContactsModel(0.0, 10.0, 21, device_name="cpu")
    m.fit(Traj(xa), Traj(xb))
    assert np.array_equal(m.P, P_bnd) and np.array_equal(m.bins, BINS)
    L0, L = m.loglikelihood(Traj(xa), Traj(xb)), m.loglikelihood(Traj(ya), Traj(yb))
    L0_64, L_64 = loglik64(xa, xb, BINS, P_bnd), loglik64(ya, yb, BINS, P_bnd)
    floats("iface_L0", L0, L0_64)
    floats("iface_L", L, L_64)
    floats("iface_Lrel", L / np.mean(L0), L_64 / np.mean(L0_64))
    floats("iface_KL", scm.div_KL(P_oth, P_bnd), kl64(P_oth, P_bnd))
    print(f"iface: {hit.mean():.3f} of the pairs hit a bin, {two.sum() / hit.sum():.3f} of those two or more; L0 {L0_64.min():.3e}..{L0_64.max():.3e}")

    # ---- iface10: contact maps and fnat in nanometres
    xa0, xb0, res_a, res_b, chain_b = interface(10.0)
    assert (xa0.shape[0], xb0.shape[0]) == (707, 701)
    qa, qb = ensemble(xa0, xb0, 32, SEEDS["iface10"], 0.3, 6.0)
    out.update(iface10_a256=qa, iface10_b256=qb, iface10_res_a=res_a, iface10_res_b=res_b)
    xa, xb = from256(qa, True), from256(qb, True)
    both = Traj(np.concatenate([xa, xb], 1))
    D = tu.pairwise_distance_matrix(both, np.arange(707), 707 + np.arange(701))         # the reference's float32 distances * 1e1
    for tag, r_thr in (("t5", 5.0), ("t41", 4.1)):
        c = D < r_thr                                                                    # fnat's test, then its any() per residue pair
        ref = np.zeros((32, res_a.max() + 1, res_b.max() + 1), bool)
        for r in range(ref.shape[1]):
            rows = c[:, res_a == r].any(1)
            for s in range(ref.shape[2]):
                ref[:, r, s] = rows[:, res_b == s].any(1)
        assert np.array_equal(ref, maps_def(xa, xb, res_a, res_b, r_thr, 10.0) != 0)
        out[f"iface10_{tag}_maps"] = ref.astype(np.uint8)
        nat = (ref & ref[:1]).sum((1, 2))
        out[f"iface10_{tag}_native"] = nat.astype(np.int64)
        out[f"iface10_{tag}_fnat"] = nat / ref[:1].sum()
        print(f"iface10 {tag}: fnat {out[f'iface10_{tag}_fnat'][0]:.2f} -> {out[f'iface10_{tag}_fnat'][-1]:.2f}, "
              f"{np.unique(out[f'iface10_{tag}_fnat']).size} distinct values")
        assert np.unique(out[f"iface10_{tag}_fnat"]).size >= 8
    # the large self-distribution's source: all of chain 1, 1/256 A, 8 frames
    big = ensemble(chain_b, chain_b[:1], 8, 17, 0.3, 0.0)[0]
    out["chain1_256"] = big

    # ---- planted
    e64 = 0.1 * np.arange(65)
    targets = [0.0, np.nan, 100.0]
    for k in (3, 5, 7, 10, 30, 64):
        targets += ulps(ceil32(e64[k]))
    targets += ulps(1.0) + ulps(2.5)
    pts = np.stack([plant(t, torch) for t in targets])
    xb = np.stack([np.roll(pts, f, 0) for f in range(3)])                                # [3, n, 3]: every atom visits three distances
    xa = np.zeros((3, 3, 3), np.float32)
    xa[:, 1] = np.nan
    xa[:, 2] = (0, 0, 1000)
    out.update(planted_a=xa, planted_b=xb, planted_targets=np.array(targets, np.float32))
    for name, bins in (("planted_b64", e64), ("planted_b1", np.array([1.0, 2.5]))):
        contacts_case(name, xa, xb, bins)
    contacts_case("planted_self", xb, None, e64, self_=True)
    mt = ulps(0.5) + ulps(ceil32(0.41)) + [0.0, np.nan, 50.0]
    mb = np.stack([plant(t, torch) for t in mt])[None].repeat(2, 0)
    mb[1] = np.roll(mb[1], 1, 0)
    ma = np.zeros((2, 2, 3), np.float32)
    ma[:, 1] = (0, 0, 1000)
    rb = np.array([0, 1, 2, 3, 4, 5, 6, 6, 2], np.int16)                                  # rows 2 and 6 hold two atoms, not adjacent for 2
    out.update(plantedmap_targets=np.array(mt, np.float32), plantedmap_a=ma, plantedmap_b=mb, plantedmap_res_a=np.array([0, 1], np.int16), plantedmap_res_b=rb)
    for tag, r_thr in (("t5", 5.0), ("t41", 4.1)):
        D = tu.pairwise_distance_matrix(Traj(np.concatenate([ma, mb], 1)), np.arange(2), 2 + np.arange(9))
        c = D < r_thr
        ref = np.stack([[[c[f, res_i][:, rb == s].any() for s in range(7)] for res_i in ([0], [1])] for f in range(2)])
        assert np.array_equal(ref, maps_def(ma, mb, np.array([0, 1]), rb, r_thr, 10.0) != 0)
        out[f"plantedmap_{tag}_maps"] = ref.astype(np.uint8)

    # ---- superposition (frames_md_1JTG_uL.npz) and centroids
    g = np.load(os.path.join(OUT, "frames_md_1JTG_uL.npz"))
    X, roa = g["X_frames"], g["res_of_atom"].astype(np.int64)
    sel = np.arange(1, X.shape[1], 7)
    mirrored = X[5:6] * np.array([1, 1, -1], np.float32)
    out["superpose_sel"] = sel.astype(np.int32)
    for tag, ref_xyz, xyz, s in (("all", X[:1], X, None), ("sel", X[:1], X, sel), ("mirror", X[:1], mirrored, None)):
        yr, xr = (ref_xyz, xyz) if s is None else (ref_xyz[:, s], xyz[:, s])
        t, R, tr = tu.superpose_transform(yr, xr)
        t64, R64, tr64, S = superpose64(yr, xr)
        assert S[:, 2].min() > 1e-3 * S[:, 0].max() and (S[:, 1] - S[:, 2]).min() > 1e-3 * S[:, 0].max(), tag     # not degenerate
        dR = np.abs(R - R64).reshape(len(R), -1).max(1)
        assert dR.max() < 20 * np.median(dR) + 1e-6, (tag, dR)
        pick = slice(None) if s is None else s
        sup = (np.einsum("fna,fac->fnc", xyz - t, R) + tr).astype(np.float32)           # the reference's t, R, t_ref applied; float32 as mdtraj keeps xyz
        sup64 = np.einsum("fna,fac->fnc", xyz.astype(np.float64) - t64, R64) + tr64
        gap, gap64 = sup[:, pick] - yr, sup64[:, pick] - yr.astype(np.float64)
        rm, rm64 = np.sqrt((gap * gap).sum(-1).mean(-1)) * np.float32(10.0), np.sqrt((gap64 * gap64).sum(-1).mean(-1)) * 10.0
        floats(f"superpose_{tag}_t", t, t64)
        floats(f"superpose_{tag}_R", R, R64)
        floats(f"superpose_{tag}_tref", tr, tr64)
        floats(f"superpose_{tag}_rmsd", rm, rm64)
        floats(f"superpose_{tag}_xyz", sup[:, ::32], sup64[:, ::32], store64=False)       # (every 32nd atom of the reference's output)
        out[f"superpose_{tag}_xyz_eref"] = np.float64(np.abs(sup - sup64).max())
        e_ref[f"superpose_{tag}_xyz"] = float(np.abs(sup - sup64).max())
        if tag == "mirror":
            assert np.linalg.det(R64)[0] > 0 and rm64[0] > 1.0                          # a proper rotation cannot undo the mirror
    Rn = int(roa.max()) + 1
    # no importable reference function: the notebook divides a float32 product of the coordinates with the dense residue matrix by the
    # residues' sizes; restated here as a float32 sum per residue (torch.index_add_) over the size
    acc = torch.zeros((X.shape[0], Rn, 3)).index_add_(1, torch.from_numpy(roa), torch.from_numpy(X))
    Xp = (acc / torch.bincount(torch.from_numpy(roa), minlength=Rn).to(torch.float32)[None, :, None]).numpy()
    acc64 = np.zeros((X.shape[0], Rn, 3))
    np.add.at(acc64, (slice(None), roa), X.astype(np.float64))
    Xp64 = acc64 / np.bincount(roa, minlength=Rn)[None, :, None]
    floats("centroids", Xp, Xp64, store64=False)

    out["seeds"] = np.array(sorted(SEEDS.items()), dtype="S")
    path = os.path.join(OUT, "trajectory.npz")
    np.savez_compressed(path, **out)
    print("e_ref (the reference's maximum deviation from the float64 restatement):")
    for k, v in e_ref.items():
        print(f"    {k:24s} {v:.2e}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
