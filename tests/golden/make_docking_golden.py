#!/usr/bin/env python3
"""Generate the docking golden (tests/golden/docking.npz) by IMPORTING the reference's own md_analysis/mdtraj_utils/trajectory_utils.py
from /root/reference (build container only; nothing under tests/ reads the reference at run time), the way make_trajectory_golden.py
does: mdtraj is stubbed and the module is imported as a submodule of a stub package. Added here: a minimal stand-in trajectory (xyz,
topology.atoms with .residue.index and .name, topology.select for "all", "not type H" and "name CA", atom_slice, __getitem__) and
trajectory_utils.align replaced by the identity pairing - chain alignment stays with mdtraj. contacts is called with device_name="cpu";
everything runs on the CPU. The definitions are those of tests/test_docking_fixture.py (the GPU tests' yardsticks), imported from there.

Systems (xyz in nanometres, scale 10; ids_a / ids_b the two subunits, roa the residue row and ca the CA flag of every atom)
  iface     1JTG_C.pdb (md_analysis/pdbs_clusters, chains 0 and 1): the atoms of the residues with an atom within 10 A of the other chain,
            as in the trajectory golden; 32 frames = frame 0, then per-atom Gaussian noise (sigma 0.3 A), a rigid drift of chain 1 (0 to
            6 A along the line between the centroids) and a rotation of chain 1 about its centroid growing to 2.3 rad. Multiples of
            1/256 A stored as int16 (iface_xyz256); the contact counts are also recorded at r_thr 4.1 and in angstroms with scale 1.
  planted   one atom of A at the origin and atoms of B at exactly r_thr / scale and one float32 ulp either side for r_thr 5 (out of
            contacts at and above) and 10 (in the interface at and below), at 0 and at NaN, each visiting three distances over F = 3; a
            NaN atom and a far single-atom residue of A; residue rows that are not contiguous; an atom of the first residue that is in
            neither subunit
  e0 e1 e2  planted frames with a frame without any contact first, in the middle and last
  single    Na = Nb = 1: coincident (d = 0), then apart;   far: the subunits far apart, every list empty
  size      300 x 12 atoms, F = 4: all 3,600 pairs in contact, about half, none, all - more contacts in a frame than the scan block of
            pesto_docking.hip (1,024) and more than three blocks in all
  rigid     24 + 24 interface atoms of iface: the reference itself (t = r = 0), a rotated and shifted ligand, that frame mirrored, noise
Recorded: the inputs; the definitions' contact lists, residue pairs, d, dmin and interface atoms; for irmsd, t and r (iface, rigid) the
reference's float32 outputs, the float64 restatement on the same float32 inputs and e_ref, the reference's maximum deviation from it.
Asserted here: the reference's pair lists, residue pairs and interface_residues_within indices equal the definitions' on every system; its
d is fl32(root' * 10) for a root' within one float32 ulp of the correctly rounded root (torch's CPU sqrt is not correctly rounded: the
share of roots one ulp off is printed for random inputs; the product by 10 can make that two ulps of d and dmin; membership at r_thr
4.1, 5 and 10 is unaffected); no superposition frame is degenerate; every planted rotation angle is below 2.5 rad.

Usage:  python tests/golden/make_docking_golden.py
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), OUT]

from make_trajectory_golden import import_reference, interface, plant, ulps  # noqa: E402
from test_docking_fixture import (SCAN_BLOCK, contacts_def, dist_def, docking64, interface_def, irmsd64, residue_contacts_def,  # noqa: E402
                                  superpose64, ulp_apart)

SEED = 23


# ------------------------------------------------------------------ a stand-in for md.Trajectory
class _Residue:
    def __init__(self, index):
        self.index = index


class _Atom:
    def __init__(self, residue, name):
        self.residue, self.name = _Residue(int(residue)), name


class _Topology:
    def __init__(self, roa, ca):
        self.roa, self.ca = np.asarray(roa), np.asarray(ca, bool)

    @property
    def atoms(self):
        return [_Atom(r, "CA" if c else "X") for r, c in zip(self.roa, self.ca)]

    def select(self, selection):
        if selection in ("all", "not type H"):
            return np.arange(self.roa.size)
        assert selection == "name CA", selection
        return np.nonzero(self.ca)[0]


class Traj:
    """xyz [F, N, 3] with a topology; ``ids``: for a subunit, its atoms' indices in the complex (what align would find)"""

    def __init__(self, xyz, roa, ca, ids=None):
        self.xyz, self.topology, self.ids = xyz, _Topology(roa, ca), ids

    def atom_slice(self, ids):
        return Traj(self.xyz[:, ids], self.topology.roa[ids], self.topology.ca[ids])

    def __getitem__(self, key):
        xyz = self.xyz[key]
        return Traj((xyz[None] if xyz.ndim == 2 else xyz).copy(), self.topology.roa, self.topology.ca, self.ids)


def identity_align(traj_ref, *trajs, selection="all"):
    """align without chain identification: a subunit pairs with its own atoms of the complex, a trajectory with itself"""
    if traj_ref.ids is not None:
        return np.stack([np.arange(traj_ref.ids.size)] + [traj_ref.ids] * len(trajs), 1)
    return np.stack([traj_ref.topology.select(selection)] * (1 + len(trajs)), 1)


# ------------------------------------------------------------------ systems
def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def iface_system(rng):
    xa0, xb0, res_a, res_b, _ = interface(10.0)
    F, na = 32, xa0.shape[0]
    centre = np.round(np.concatenate([xa0, xb0]).mean(0))
    a0, b0 = (xa0 - centre).astype(np.float64), (xb0 - centre).astype(np.float64)
    axis = b0.mean(0) - a0.mean(0)
    axis /= np.linalg.norm(axis)
    angles = np.linspace(0.0, 2.3, F)
    xyz = np.zeros((F, na + xb0.shape[0], 3))
    for f in range(F):
        R = rotation([0.3, -0.5, 0.8], angles[f])
        xyz[f, :na] = a0
        xyz[f, na:] = (b0 - b0.mean(0)) @ R.T + b0.mean(0) + 6.0 * f / (F - 1) * axis
    xyz[1:] += rng.normal(0.0, 0.3, xyz[1:].shape)
    q = np.round(xyz * 256.0)
    assert np.abs(q).max() < 32768 and angles.max() < 2.5
    roa = np.concatenate([res_a.astype(np.int64), res_a.max() + 1 + res_b.astype(np.int64)])
    ca = np.zeros(roa.size, bool)
    ca[np.unique(roa, return_index=True)[1] + 1] = True                 # the second atom of every residue (N, CA, ...)
    assert np.all(roa[np.nonzero(ca)[0]] == np.arange(roa.max() + 1))
    return dict(xyz256=q.astype(np.int16), ids_a=np.arange(na), ids_b=np.arange(na, roa.size), roa=roa, ca=ca)


def planted_system(torch):
    half, one = np.float32(0.5), np.float32(1.0)
    targets = ulps(half) + ulps(one) + [np.float32(0.0), np.float32(np.nan), np.float32(0.25), np.float32(0.75), np.float32(3.0)]
    pts = np.stack([plant(t, torch) for t in targets])
    nb = len(targets)
    # topology: a0 | NaN atom of A | far atom of A (its own residue) | B ... | an atom of a0's residue that is in neither subunit
    F = 3
    xyz = np.zeros((F, 3 + nb + 1, 3), np.float32)
    xyz[:, 1] = np.nan
    xyz[:, 2] = (0, 0, 100)
    for f in range(F):
        xyz[f, 3:3 + nb] = np.roll(pts, f, 0)
    xyz[:, -1] = (0, 50, 0)
    roa = np.array([0, 1, 2] + [3 + r for r in (0, 1, 2, 3, 4, 5, 6, 6, 2, 7, 8)] + [0])
    assert len(roa) == xyz.shape[1] and nb == 11
    top = dict(ids_a=np.arange(3), ids_b=np.arange(3, 3 + nb), roa=roa, ca=np.zeros(roa.size, bool))
    empty = xyz[0].copy()
    empty[3:3 + nb, 2] += 500
    banks = dict(e0=[empty, xyz[0], xyz[1]], e1=[xyz[0], empty, xyz[1]], e2=[xyz[0], xyz[1], empty])
    return dict(xyz=xyz, **top), {k: np.stack(v) for k, v in banks.items()}, np.array(targets, np.float32)


def size_system(rng):
    def ball(n, radius):
        v = rng.normal(size=(n, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True) * radius * rng.random((n, 1)) ** (1 / 3)
    a, b = ball(300, 2.4), ball(12, 2.4)                                 # angstroms: every pair within 4.8
    frames = [np.concatenate([a * s, b * s + shift]) for s, shift in ((1, 0), (1.9, 0), (1, 100), (1, 0))]
    q = np.round(np.stack(frames) * 256.0)
    assert np.abs(q).max() < 32768
    roa = np.concatenate([np.arange(300) // 3, 100 + np.arange(12) // 4])
    return dict(xyz256=q.astype(np.int16), ids_a=np.arange(300), ids_b=np.arange(300, 312), roa=roa, ca=np.zeros(312, bool))


def rigid_system(iface, rng):
    x0 = iface["xyz256"][0].astype(np.float64) / 256.0
    na = iface["ids_a"].size
    D = np.linalg.norm(x0[:na, None] - x0[None, na:], axis=-1)
    pa, pb = np.sort(np.argsort(D.min(1))[:24]), na + np.sort(np.argsort(D.min(0))[:24])
    keep = np.concatenate([pa, pb])
    x0 = x0[keep] - np.round(x0[keep].mean(0))
    lig = np.arange(24, 48)
    moved = x0.copy()
    moved[lig] = (x0[lig] - x0[lig].mean(0)) @ rotation([1, 2, -1], 0.9).T + x0[lig].mean(0) + (1.5, -0.5, 2.0)
    noisy = x0 + rng.normal(0.0, 0.3, x0.shape)
    q = np.round(np.stack([x0, moved, moved * (1, 1, -1), noisy]) * 256.0)
    roa = np.unique(iface["roa"][keep], return_inverse=True)[1]
    ca = np.zeros(48, bool)
    ca[::3] = True
    return dict(xyz256=q.astype(np.int16), ids_a=np.arange(24), ids_b=lig, roa=roa, ca=ca)


def root_one_ulp_off(d_ref, xa, xb, offsets, pairs):
    """the reference's d is fl32(root' * 10) for a root' within one float32 ulp of the correctly rounded root (torch's CPU sqrt); the
    product by 10 can carry that to two ulps of d"""
    f = np.repeat(np.arange(offsets.size - 1), np.diff(offsets))
    root = dist_def(xa, xb, 1.0)[f, pairs[:, 0], pairs[:, 1]]
    ten = np.float32(10.0)
    near = [np.nextafter(root, np.float32(-np.inf)) * ten, root * ten, np.nextafter(root, np.float32(np.inf)) * ten]
    return bool(np.all((d_ref == near[0]) | (d_ref == near[1]) | (d_ref == near[2]))) and ulp_apart(d_ref, near[1]) <= 2


def nm(sysd):
    if "xyz256" in sysd:
        return (sysd["xyz256"].astype(np.float64) / 256.0).astype(np.float32) * np.float32(0.1)
    return sysd["xyz"]


def main():
    tu, _, torch = import_reference()
    tu.align = identity_align
    rng = np.random.default_rng(SEED)
    out, e_ref = {}, {}

    # torch's CPU sqrt against the correctly rounded one, on random inputs
    s = rng.random(1 << 20, dtype=np.float32) * np.float32(4.0)
    off = np.abs(torch.sqrt(torch.from_numpy(s)).numpy().view(np.int32) - np.sqrt(s).view(np.int32))
    assert off.max() <= 1
    print(f"torch's CPU sqrt: {100.0 * off.mean():.2f} % of 2^20 random inputs one float32 ulp off the correctly rounded root")

    iface = iface_system(rng)
    planted, banks, targets = planted_system(torch)
    systems = dict(iface=iface, planted=planted)
    for k, xyz in banks.items():
        systems[k] = dict(xyz=xyz, top="planted")
    one = dict(ids_a=np.array([0]), ids_b=np.array([1]), roa=np.array([0, 1]), ca=np.zeros(2, bool))
    systems["single"] = dict(xyz=np.array([[[1, 2, 3], [1, 2, 3]], [[1, 2, 3], [1, 2, 4]]], np.float32), **one)
    far = planted["xyz"].copy()
    far[:, 3:14, 2] += 500
    far[:, 1] = (0, 0, -100)
    systems["far"] = dict(xyz=far, top="planted")
    systems["size"] = size_system(rng)
    systems["rigid"] = rigid_system(iface, rng)
    out["planted_targets"] = targets

    def floats(key, ref, f64):
        e = float(np.max(np.abs(np.asarray(ref, np.float64) - f64)))
        out[key + "_ref"], out[key + "_f64"], out[key + "_eref"] = np.asarray(ref), np.asarray(f64, np.float64), np.float64(e)      # (float64 where R made it so)
        e_ref[key] = e

    for name, sysd in systems.items():
        topd = systems[sysd["top"]] if "top" in sysd else sysd
        xyz = nm(sysd)
        ids_a, ids_b, roa, ca = (np.asarray(topd[k]) for k in ("ids_a", "ids_b", "roa", "ca"))
        for k in ("xyz256", "xyz"):
            if k in sysd:
                out[f"{name}_{k}"] = sysd[k]
        if "top" in sysd:
            out[name + "_top"] = np.array(sysd["top"])
        else:
            small = np.int16 if roa.size < 32768 else np.int32
            out.update({f"{name}_ids_a": ids_a.astype(small), f"{name}_ids_b": ids_b.astype(small), f"{name}_roa": roa.astype(small), f"{name}_ca": ca})
        xa, xb = xyz[:, ids_a], xyz[:, ids_b]
        res_a, res_b = np.unique(roa[ids_a], return_inverse=True)[1], np.unique(roa[ids_b], return_inverse=True)[1]
        F = xyz.shape[0]
        full = Traj(xyz, roa, ca)
        sub_a, sub_b = Traj(xa, roa[ids_a], ca[ids_a], ids_a), Traj(xb, roa[ids_b], ca[ids_b], ids_b)

        # ---- contacts and residue contacts: the reference's lists are the definition's, d within one ulp
        for r_thr in ((5.0, 4.1) if name == "iface" else (5.0,)):
            offd, pairs, d = contacts_def(xa, xb, r_thr)
            with np.errstate(invalid="ignore"):
                ref = tu.contacts(sub_a, sub_b, full, r_thr=r_thr, device_name="cpu")
            assert len(ref) == F
            ic = [np.asarray(c[1]).reshape(-1, 2) for c in ref]
            assert np.array_equal(np.cumsum([0] + [len(c) for c in ic]), offd), (name, r_thr)
            assert np.array_equal(np.concatenate(ic), np.stack([ids_a[pairs[:, 0]], ids_b[pairs[:, 1]]], 1)), (name, r_thr)
            d_ref = np.concatenate([c[0] for c in ref]).astype(np.float32)
            assert root_one_ulp_off(d_ref, xa, xb, offd, pairs), (name, r_thr)
            if r_thr != 5.0:
                out[f"{name}_off41"] = offd
                continue
            roff, rpairs, dmin = residue_contacts_def(offd, pairs, d, res_a, res_b)
            rr, dr = tu.atoms_to_residue_contacts(full.topology, ic, [c[0] for c in ref])
            rank = {int(r): k for k, r in enumerate(np.unique(roa))}          # the reference numbers the residues of the whole topology
            ra_of = np.array([rank[int(r)] for r in np.unique(roa[ids_a])])
            rb_of = np.array([rank[int(r)] for r in np.unique(roa[ids_b])])
            for f in range(F):
                want = rpairs[roff[f]:roff[f + 1]]
                got = np.asarray(rr[f]).reshape(-1, 2)
                assert np.array_equal(got, np.stack([ra_of[want[:, 0]], rb_of[want[:, 1]]], 1)), (name, f)
                assert ulp_apart(np.asarray(dr[f], np.float32), dmin[roff[f]:roff[f + 1]]) <= 2, (name, f)     # (a minimum of such d)
            assert pairs.max(initial=0) < 65536 and rpairs.max(initial=0) < 65536
            out.update({f"{name}_off": offd, f"{name}_pairs": pairs.astype(np.uint16), f"{name}_d": d, f"{name}_roff": roff,
                        f"{name}_rpairs": rpairs.astype(np.uint16), f"{name}_dmin": dmin})
            print(f"{name}: F {F}, Na {xa.shape[1]}, Nb {xb.shape[1]}, contacts per frame {np.diff(offd).min()}..{np.diff(offd).max()}, K {offd[-1]}, "
                  f"U {roff[-1]}, d one ulp off in {100.0 * np.mean(d_ref.view(np.int32) != d.view(np.int32)) if d.size else 0.0:.2f} %")
        if name == "iface":
            ang = (sysd["xyz256"].astype(np.float64) / 256.0).astype(np.float32)
            out["iface_off_angstrom"] = contacts_def(ang[:, ids_a], ang[:, ids_b], 5.0, 1.0)[0]

        # ---- interface atoms
        ira, irb = interface_def(xyz[0], ids_a, ids_b, roa)
        with np.errstate(invalid="ignore"):
            ra_ref, rb_ref = tu.interface_residues_within(sub_a, sub_b, 10.0, full)
        assert np.array_equal(ra_ref[:, 0], ira) and np.array_equal(rb_ref[:, 0], irb), name
        out.update({f"{name}_ira": ira.astype(np.int32), f"{name}_irb": irb.astype(np.int32)})

        # ---- irmsd, t, r
        if name not in ("iface", "rigid"):
            continue
        ref_traj = full[0]
        rm64, sel = irmsd64(xyz[:1], xyz, ids_a, ids_b, roa, ca)
        (rm_ref,) = tu.irmsd(ref_traj, sub_a, sub_b, full, r_thr=10.0)
        t64, r64, R2 = docking64(xyz[:1], xyz, ids_a, ids_b, roa)
        t_ref, r_ref = tu.interface_rigid_docking(sub_a, sub_b, ref_traj, full, r_thr=10.0)
        floats(name + "_irmsd", rm_ref, rm64)
        floats(name + "_t", np.reshape(t_ref, (F, 3)), t64)
        floats(name + "_r", np.reshape(r_ref, (F, 3)), r64)
        # no fit is degenerate: the selection's CA atoms, the receptor's and the ligand's interface
        for pick in (sel, ira, irb):
            ref64, x64 = xyz[:1, pick].astype(np.float64), xyz[:, pick].astype(np.float64)
            S = np.linalg.svd(np.einsum("fna,fnb->fab", ref64 - ref64.mean(1, keepdims=True), x64 - x64.mean(1, keepdims=True)), compute_uv=False)
            assert S[:, 2].min() > 1e-3 * S[:, 0].max() and (S[:, 1] - S[:, 2]).min() > 1e-3 * S[:, 0].max(), name
        ang = np.linalg.norm(r64, axis=1)
        assert ang.max() < 2.5, (name, ang.max())
        print(f"{name}: {sel.size} CA atoms, irmsd {rm64.min():.3f}..{rm64.max():.3f} A, |t| up to {np.abs(t64).max():.3f} nm, angle up to {ang.max():.3f} rad")

    n = np.diff(out["size_off"])
    assert n.max() > SCAN_BLOCK and n.sum() >= 3 * SCAN_BLOCK
    out["seed"] = np.array(SEED)
    path = os.path.join(OUT, "docking.npz")
    np.savez_compressed(path, **out)
    print("e_ref (the reference's maximum deviation from the float64 restatement):")
    for k, v in e_ref.items():
        print(f"    {k:24s} {v:.2e}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
