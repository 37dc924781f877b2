"""CPU checks of the definitions behind pesto_amd.dockq and of its host side: the NumPy statements of the native pairs, the preserved
count, the ligand RMSD (float64), the DockQ score and the CAPRI class are pinned by hand-worked cases on a complex of 2 + 2 residues whose
coordinates are multiples of 1/256 A, agree with the recorded contact lists and interface selections of the docking fixture
(tests/golden/docking.npz), bad arguments raise ValueError without a GPU, and the header's new symbols are exported and bound. The
definitions are the yardsticks of the GPU tests (tests/test_dockq.py), which also draws its seeded systems from here."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
from test_docking_fixture import DOCKING, contacts_def, dist_def, interface_def, irmsd64, residue_contacts_def, system
from test_trajectory_fixture import superpose64


# ------------------------------------------------------------------ the definitions (NumPy)
def native_pairs_def(xyz0, ids_R, ids_L, roa, r_contact=5.0, scale=10.0):
    """int32 [P, 2]: the residue pairs (r, s) with an atom pair d < r_contact in the frame xyz0 [N, 3], ascending by (r, s)"""
    D = dist_def(xyz0[None, ids_R], xyz0[None, ids_L], scale)[0]
    with np.errstate(invalid="ignore"):
        i, j = np.nonzero(D < np.float32(r_contact))
    if i.size == 0:
        return np.zeros((0, 2), np.int32)
    return np.unique(np.stack([roa[ids_R[i]], roa[ids_L[j]]], 1), axis=0).astype(np.int32)


def preserved_def(xyz, pairs, ids_R, ids_L, roa, r_contact=5.0, scale=10.0):
    """int32 [F]: the pairs with an atom pair d < r_contact in every frame of xyz [F, N, 3] (frame by frame, on dist_def)"""
    uR, dR = np.unique(roa[ids_R], return_inverse=True)
    uL, dL = np.unique(roa[ids_L], return_inverse=True)
    oneR = (dR.reshape(-1)[:, None] == np.arange(uR.size)[None]).astype(np.float32)
    oneL = (dL.reshape(-1)[:, None] == np.arange(uL.size)[None]).astype(np.float32)
    r, s = np.searchsorted(uR, pairs[:, 0]), np.searchsorted(uL, pairs[:, 1])
    out = np.zeros(xyz.shape[0], np.int32)
    for f in range(xyz.shape[0]):
        D = dist_def(xyz[f:f + 1, ids_R], xyz[f:f + 1, ids_L], scale)[0]
        with np.errstate(invalid="ignore"):
            hit = (D < np.float32(r_contact)).astype(np.float32)
        out[f] = int(((oneR.T @ hit @ oneL)[r, s] > 0).sum())               # (counts below 2^24: exact in float32)
    return out


def backbone_def(ids_R, ids_L, bb):
    """(S_R, S_L): the backbone atoms of the two subunits, ascending"""
    R, L = np.unique(ids_R), np.unique(ids_L)
    return R[bb[R]], L[bb[L]]


def interface_sel_def(xyz0, ids_R, ids_L, roa, bb, r_interface=10.0, scale=10.0):
    """the backbone atoms of the interface (interface_def of both sides), ascending"""
    both = np.union1d(*interface_def(xyz0, ids_R, ids_L, roa, r_interface, scale))
    return both[bb[both]]


def fit_rmsd_def(xyz_ref, xyz, sel_fit, sel_measure, scale=10.0):
    """float64 [F]: the frames fitted onto the reference on sel_fit, the RMSD over sel_measure times scale"""
    t, R, tr = superpose64(xyz_ref[:, sel_fit], xyz[:, sel_fit])
    gap = (xyz[:, sel_measure].astype(np.float64) - t) @ R + tr - xyz_ref[:, sel_measure].astype(np.float64)
    return np.sqrt(np.mean(np.sum(gap * gap, 2), 1)) * scale


def lrmsd_def(xyz_ref, xyz, ids_R, ids_L, bb, scale=10.0):
    return fit_rmsd_def(xyz_ref, xyz, *backbone_def(ids_R, ids_L, bb), scale)


def dockq_def(fnat, irmsd, lrmsd):
    """float32: the score in double from the three float32 values, every operation as written"""
    f, i, l = (np.asarray(v, np.float32).astype(np.float64) for v in (fnat, irmsd, lrmsd))
    a, b = i / 1.5, l / 8.5
    return ((f + 1.0 / (1.0 + a * a) + 1.0 / (1.0 + b * b)) / 3.0).astype(np.float32)


def capri_def(preserved, n_native, irmsd, lrmsd):
    """uint8: the highest class whose condition holds, one decoy at a time, the fnat conditions on the integers"""
    out = []
    for k, i, l in zip(np.asarray(preserved).tolist(), np.asarray(irmsd, np.float32).tolist(), np.asarray(lrmsd, np.float32).tolist()):
        if 2 * k >= n_native and (l <= 1.0 or i <= 1.0):
            out.append(3)
        elif 10 * k >= 3 * n_native and (l <= 5.0 or i <= 2.0):
            out.append(2)
        elif 10 * k >= n_native and (l <= 10.0 or i <= 4.0):
            out.append(1)
        else:
            out.append(0)
    return np.array(out, np.uint8)


def scores_def(xyz_ref, xyz, ids_R, ids_L, roa, bb, r_contact=5.0, r_interface=10.0, scale=10.0):
    """dict of the whole definition in its widest precision: pairs, preserved, fnat (float32), irmsd and lrmsd (float64)"""
    pairs = native_pairs_def(xyz_ref[0], ids_R, ids_L, roa, r_contact, scale)
    kept = preserved_def(xyz, pairs, ids_R, ids_L, roa, r_contact, scale)
    sel = interface_sel_def(xyz_ref[0], ids_R, ids_L, roa, bb, r_interface, scale)
    return dict(pairs=pairs, preserved=kept, fnat=(kept.astype(np.float64) / pairs.shape[0]).astype(np.float32),
                irmsd=fit_rmsd_def(xyz_ref, xyz, sel, sel, scale), lrmsd=lrmsd_def(xyz_ref, xyz, ids_R, ids_L, bb, scale), sel=sel)


# ------------------------------------------------------------------ the hand-worked complex: 2 + 2 residues, multiples of 1/256 A
STEP = 1.0 / 256.0
RESIDUE = np.array([[0, 0, 0], [1, 0.5, 0], [0.5, 1, 0.25], [0, 0.5, 1]], np.float64)       # four atoms; the last is the side chain


def tiny():
    """dict: xyz0 float32 [16, 3] in angstroms (scale 1), ids_R (residues 0 and 1), ids_L (residues 2 and 3), roa, bb. Receptor residue
    0 sits at the origin and 1 at (0, 8, 0.5); ligand residue 2 at (4, 0, 0) faces residue 0 and residue 3 at (4, 8, 0.5) faces 1."""
    origins = np.array([[0, 0, 0], [0, 8, 0.5], [4, 0, 0], [4, 8, 0.5]], np.float64)
    xyz0 = (origins[:, None] + RESIDUE[None]).reshape(16, 3).astype(np.float32)
    assert np.array_equal(xyz0 * 256, np.round(xyz0 * 256))
    return dict(xyz0=xyz0, ids_R=np.arange(8), ids_L=np.arange(8, 16), roa=np.repeat(np.arange(4), 4), bb=np.tile([True, True, True, False], 4))


def tiny_decoys():
    """(xyz float32 [6, 16, 3], names): the reference; the ligand moved by t = (0.75, 1, 0); the ligand out of reach; residue 3 far away
    but for its first atom at exactly 5 A from the first atom of residue 1, and one step of 1/256 A closer; the ligand moved by 8 t (10 A)"""
    c = tiny()
    t = np.array([0.75, 1.0, 0.0], np.float32)
    frames = [c["xyz0"].copy() for _ in range(6)]
    frames[1][8:] += t
    frames[2][8:] += np.array([100, 0, 0], np.float32)
    for f, dx in ((3, 0.0), (4, STEP)):
        frames[f][12:] += np.array([100, 0, 0], np.float32)
        frames[f][12] = c["xyz0"][4] + np.array([-3 + dx, -4, 0], np.float32)
    frames[5][8:] += 8 * t
    return np.stack(frames), ["reference", "moved", "far", "at_r_contact", "one_step_closer", "moved_far"]


def test_hand_worked_cases_pin_the_definitions():
    c = tiny()
    xyz, _ = tiny_decoys()
    args = (c["ids_R"], c["ids_L"], c["roa"])
    pairs = native_pairs_def(c["xyz0"], *args, 5.0, 1.0)
    assert pairs.tolist() == [[0, 2], [1, 3]]                    # the facing residues: 4 A apart; the diagonal ones sqrt(80) A
    assert native_pairs_def(c["xyz0"], *args, 3.0, 1.0).shape == (0, 2)                        # their closest atoms: (3, 0.5, 0) apart
    kept = preserved_def(xyz, pairs, *args, 5.0, 1.0)
    ref = c["xyz0"][None]
    lr = lrmsd_def(ref, xyz, c["ids_R"], c["ids_L"], c["bb"], 1.0)
    sel = interface_sel_def(c["xyz0"], *args, c["bb"], 10.0, 1.0)
    assert sel.tolist() == [i for i in range(16) if i % 4 != 3]                                # every residue lies within 10 A: all backbone atoms
    ir = fit_rmsd_def(ref, xyz, sel, sel, 1.0)
    # decoy = reference: (1, 0, 0, 1.0, class 3)
    assert kept[0] == 2 and abs(ir[0]) < 1e-12 and abs(lr[0]) < 1e-12
    assert dockq_def(1.0, 0.0, 0.0) == np.float32(1.0) and capri_def([2], 2, [0.0], [0.0]).tolist() == [3]
    # the ligand moved rigidly by t with the receptor fixed: lrmsd = |t| scale = 1.25, and ten times that at scale 10
    assert kept[1] == 2 and abs(lr[1] - 1.25) < 1e-12 and abs(lr[5] - 10.0) < 1e-12 and kept[5] == 0             # (10 A away: out of reach too)
    assert abs(lrmsd_def(ref, xyz, c["ids_R"], c["ids_L"], c["bb"], 10.0)[1] - 12.5) < 1e-11
    assert 0 < ir[1] < lr[1]                                                                   # the interface fit shares the motion out
    # out of reach
    assert kept[2] == 0 and capri_def([0], 2, [0.0], [0.0]).tolist() == [0]
    # exactly d = r_contact is no contact; one step of 1/256 A closer is one
    d = dist_def(xyz[3:5, 4:8], xyz[3:5, 12:16], 1.0)
    assert d[0].min() == np.float32(5.0) and d[0, 0, 0] == np.float32(5.0) and (d[0].ravel() <= 5).sum() == 1          # 3-4-5
    assert d[1, 0, 0] < np.float32(5.0) and (d[1].ravel() < 5).sum() == 1 and np.float32(25.0) - d[1, 0, 0] ** 2 < 0.03
    assert kept[3] == 1 and kept[4] == 2
    # the score of a hand-worked triple: fnat 0.5, irmsd 1.5, lrmsd 8.5 -> (0.5 + 0.5 + 0.5) / 3
    assert dockq_def(0.5, 1.5, 8.5) == np.float32(0.5)
    assert dockq_def(0.0, np.inf, np.inf) == 0 and np.isnan(dockq_def(0.5, np.nan, 1.0))


def test_every_class_boundary_from_both_sides():
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    big = 100.0
    cases = [  # (preserved of 10, irmsd, lrmsd, class)
        (5, big, 1.0, 3), (4, big, 1.0, 2), (5, big, up(1.0), 2), (5, 1.0, big, 3), (5, up(1.0), big, 2),
        (3, big, 5.0, 2), (2, big, 5.0, 1), (3, big, up(5.0), 1), (3, 2.0, big, 2), (3, up(2.0), big, 1), (10, big, up(5.0), 1),
        (1, big, 10.0, 1), (0, big, 10.0, 0), (1, big, up(10.0), 0), (1, 4.0, big, 1), (1, up(4.0), big, 0), (10, up(4.0), up(10.0), 0),
        (10, 0.0, 0.0, 3), (0, 0.0, 0.0, 0), (10, np.nan, np.nan, 0), (10, np.nan, 0.5, 3), (10, 0.5, np.nan, 3),
    ]
    k, ir, lr, want = (np.array(v) for v in zip(*cases))
    assert capri_def(k, 10, ir, lr).tolist() == want.tolist()
    # the integers decide: 3 of 9 is a third, above 0.3 - and 0.3 itself is 3 of 10, which float32(3 / 10) < 0.3 would miss
    assert capri_def([3, 3], 9, [2.0, 2.0], [big, big]).tolist() == [2, 2] and capri_def([299], 1000, [2.0], [big]).tolist() == [1]
    # the package's host function is the same cascade
    from pesto_amd.dockq import capri_class
    got = capri_class(k, 10, ir.astype(np.float32), lr.astype(np.float32))
    assert got.dtype == np.uint8 and got.tolist() == want.tolist()
    rng = np.random.default_rng(7)
    kk, ii, ll = rng.integers(0, 41, 4000), rng.choice([0.5, 1, 1.5, 2, 3, 4, 5], 4000), rng.choice([0.5, 1, 3, 5, 7, 10, 12], 4000)
    assert np.array_equal(capri_class(kk, 40, ii, ll), capri_def(kk, 40, ii, ll)) and set(capri_def(kk, 40, ii, ll).tolist()) == {0, 1, 2, 3}
    with pytest.raises(ValueError):
        capri_class([3], 2, [1.0], [1.0])
    with pytest.raises(ValueError):
        capri_class([0], 0, [1.0], [1.0])


# ------------------------------------------------------------------ against the recorded lists of the docking fixture
@pytest.mark.parametrize("name", DOCKING)
def test_definitions_agree_with_the_recorded_lists(name):
    g = golden("docking")
    s = system(g, name)
    args = (s["ids_a"], s["ids_b"], s["roa"])
    pairs = native_pairs_def(s["xyz"][0], *args)
    kept = preserved_def(s["xyz"], pairs, *args)
    # the same count from the recorded residue pairs of every frame (dense rows of each side in the order of the topology's rows)
    roff, rp = g[name + "_roff"], g[name + "_rpairs"].astype(np.int64)
    ua, ub = np.unique(s["roa"][s["ids_a"]]), np.unique(s["roa"][s["ids_b"]])
    native = {(int(a), int(b)) for a, b in rp[roff[0]:roff[1]]}
    assert pairs.tolist() == [[int(ua[a]), int(ub[b])] for a, b in sorted(native)] and len(native) >= 20
    want = [len(native & {(int(a), int(b)) for a, b in rp[roff[f]:roff[f + 1]]}) for f in range(roff.size - 1)]
    assert kept.tolist() == want and kept[0] == len(native) and kept.min() < kept.max()
    # ... and from maps made of contacts_def / residue_contacts_def here, for two frames
    off, prs, d = contacts_def(s["xa"][:2], s["xb"][:2])
    roff2, rp2, _ = residue_contacts_def(off, prs, d, s["res_a"], s["res_b"])
    assert np.array_equal(roff2, roff[:3]) and np.array_equal(rp2, rp[:roff[2]])
    # with bb = ca the interface selection is the one the recorded irmsd used
    rm, sel = irmsd64(s["xyz"][:1], s["xyz"], *args, s["ca"])
    assert np.array_equal(interface_sel_def(s["xyz"][0], *args, s["ca"]), sel)
    assert np.allclose(fit_rmsd_def(s["xyz"][:1], s["xyz"], sel, sel), g[name + "_irmsd_f64"], rtol=1e-9, atol=1e-11) and np.allclose(rm, g[name + "_irmsd_f64"], rtol=1e-9, atol=1e-11)
    # the ligand RMSD of the recorded frames: 0 for the frame that is its reference, above the interface RMSD's scale elsewhere
    lr = lrmsd_def(s["xyz"][:1], s["xyz"], s["ids_a"], s["ids_b"], s["ca"])
    assert lr[0] < 1e-9 and lr[1:].min() > 0.1 and np.isfinite(lr).all()


# ------------------------------------------------------------------ the seeded systems of the GPU sweep
@functools.lru_cache(maxsize=None)
def sweep_system(P, F, n_SR, n_SL, seed=0):
    """dict of a seeded complex with exactly P native pairs (asserted by the callers through native_pairs_def), F decoys and n_SR / n_SL
    backbone atoms on the receptor / ligand: two layers of residues facing each other, the receptor's in the plane z = 0 and the ligand's
    above it. A column holds one receptor residue under one ligand residue 4 A above it (one pair), or two receptor residues 6 A apart
    under one ligand residue between them (two pairs); columns are 24 A apart, and unpaired residues far from every partner fill the
    sides up. Residues have 1 to 6 atoms within 0.4 A of their centre, one receptor residue of a pair has 70 (more than a wave); rows and
    the atom order are shuffled, so neither side is contiguous. Coordinates are nanometres (scale 10). Decoy 0 is the reference; the
    others move the ligand rigidly by a growing rotation and shift and every atom by noise, so preserved runs from P down to 0."""
    rng = np.random.default_rng([P, F, n_SR, n_SL, seed])
    doubles = P // 3
    columns = P - doubles                                # singles + doubles columns give singles + 2 doubles = P pairs
    centres, owner, paired = [], [], []                  # per residue: centre, side (0 receptor, 1 ligand), in a pair
    for c in range(columns):
        base = np.array([24.0 * (c % 20), 24.0 * (c // 20), 0.0])
        if c < doubles:
            centres += [base, base + [6.0, 0, 0], base + [3.0, 0, 2.5]]
            owner += [0, 0, 1]
        else:
            centres += [base, base + [0, 0, 4.0]]
            owner += [0, 1]
    paired = [True] * len(centres)
    sizes = rng.integers(1, 7, len(centres)).tolist()
    sizes[0] = 70
    if len(sizes) > 3:
        sizes[-1] = sizes[-2] = 1
    need = max(n_SR, n_SL) + 8
    k = 0
    while sum(z for z, o in zip(sizes, owner) if o == 0) < need or sum(z for z, o in zip(sizes, owner) if o == 1) < need:
        side = 0 if sum(z for z, o in zip(sizes, owner) if o == 0) < need else 1
        centres.append(np.array([24.0 * (k % 20) + 12.0, -40.0 - 24.0 * (k // 20), 30.0 * side]))          # far from every column
        owner.append(side)
        paired.append(False)
        sizes.append(int(rng.integers(1, 7)))
        k += 1
    R = len(centres)
    row = rng.permutation(R)
    atoms, res, sideof, inpair = [], [], [], []
    for r in range(R):
        u = rng.normal(size=(sizes[r], 3))
        u *= (0.4 * rng.uniform(0, 1, (sizes[r], 1)) ** (1 / 3)) / np.linalg.norm(u, axis=1, keepdims=True)
        atoms.append(centres[r] + u)
        res += [row[r]] * sizes[r]
        sideof += [owner[r]] * sizes[r]
        inpair += [paired[r]] * sizes[r]
    order = rng.permutation(len(res))
    x0 = np.concatenate(atoms)[order]
    res, sideof, inpair = np.array(res)[order], np.array(sideof)[order], np.array(inpair)[order]
    ids_R, ids_L = np.nonzero(sideof == 0)[0], np.nonzero(sideof == 1)[0]
    bb = np.zeros(len(res), bool)
    for ids, n in ((ids_R, n_SR), (ids_L, n_SL)):       # the paired residues' atoms first, so the interface always holds backbone atoms
        first = np.concatenate([ids[inpair[ids]], ids[~inpair[ids]]])
        bb[first[:n]] = True
    frames = [x0]
    for f in range(1, F):
        a = (f / max(F - 1, 1)) ** 2
        w = rng.normal(size=3)
        w *= 0.5 * a / np.linalg.norm(w)
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / max(th, 1e-30)
        Rot = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        x = x0 + rng.normal(0, 0.15 * a + 0.02, x0.shape)
        cm = x[ids_L].mean(0)
        x[ids_L] = (x[ids_L] - cm) @ Rot.T + cm + a * np.array([1.0, -0.5, 2.5]) * rng.uniform(0.5, 1.0)
        frames.append(x)
    xyz = (np.stack(frames).astype(np.float32) * np.float32(0.1))
    return dict(xyz=xyz, ids_R=ids_R.astype(np.int64), ids_L=ids_L.astype(np.int64), roa=res.astype(np.int64), bb=bb, P=P)


@functools.lru_cache(maxsize=None)
def sweep_definition(P, F, n_SR, n_SL, seed=0):
    s = sweep_system(P, F, n_SR, n_SL, seed)
    return scores_def(s["xyz"][:1], s["xyz"], s["ids_R"], s["ids_L"], s["roa"], s["bb"])


def test_the_sweep_generator_gives_what_it_promises():
    for P, F, n_SR, n_SL in ((1, 2, 3, 3), (65, 3, 257, 255)):
        s = sweep_system(P, F, n_SR, n_SL)
        d = sweep_definition(P, F, n_SR, n_SL)
        S_R, S_L = backbone_def(s["ids_R"], s["ids_L"], s["bb"])
        assert d["pairs"].shape == (P, 2) and S_R.size == n_SR and S_L.size == n_SL and d["sel"].size >= 3
        assert d["preserved"][0] == P and d["preserved"].dtype == np.int32 and np.bincount(s["roa"]).max() == 70
        assert s["xyz"].dtype == np.float32 and s["xyz"].shape[0] == F
        if P > 2:                                       # a ligand residue in two pairs; single-atom residues; rows not contiguous
            assert np.bincount(d["pairs"][:, 1]).max() == 2 and np.bincount(s["roa"]).min() == 1 and np.any(np.diff(s["roa"][s["ids_R"]]) < 0)


# ------------------------------------------------------------------ the host side of pesto_amd.dockq
def test_arguments_raise_before_any_launch(monkeypatch):
    from pesto_amd import dockq as Q
    m = object()                # no handle: the checks must come first
    c = tiny()
    x = np.repeat(c["xyz0"][None], 3, 0)
    base = dict(xyz_ref=c["xyz0"], xyz=x, ids_R=c["ids_R"], ids_L=c["ids_L"], res_of_atom=c["roa"], bb=c["bb"], scale=1.0, model=m)
    few = np.zeros(16, bool)
    few[[0, 1, 8, 9, 10]] = True                        # two backbone atoms on the receptor
    none_L = np.zeros(16, bool)
    none_L[:8] = True
    for kw in (dict(xyz_ref=x[:2]), dict(xyz_ref=c["xyz0"][:15]), dict(xyz=x[:, :, :2]), dict(xyz=x[:, :15]), dict(xyz=np.zeros((0, 16, 3), np.float32)),
               dict(ids_R=[0, 16]), dict(ids_L=[-1, 9]), dict(ids_R=[]), dict(ids_L=np.zeros(8)), dict(res_of_atom=c["roa"][:15]),
               dict(res_of_atom=c["roa"] * 1.0), dict(res_of_atom=-c["roa"]), dict(res_of_atom=c["roa"] + 13), dict(bb=c["bb"][:15]),
               dict(bb=c["bb"] * 0.5), dict(bb=few), dict(bb=none_L), dict(r_contact=np.nan), dict(r_contact=np.inf), dict(r_interface=np.nan),
               dict(r_interface=-np.inf), dict(scale=0.0), dict(scale=-1.0), dict(scale=np.inf), dict(scale=np.nan)):
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError):
            Q.dockq(**args)
        if not set(kw) & {"xyz", "bb", "r_interface"}:
            a = {k: v for k, v in args.items() if k not in ("xyz", "bb", "r_interface")}
            with pytest.raises(ValueError):
                Q.native_pairs(**a)
        if not set(kw) & {"res_of_atom", "r_contact", "r_interface"}:
            a = {k: v for k, v in args.items() if k not in ("res_of_atom", "r_contact", "r_interface")}
            with pytest.raises(ValueError):
                Q.lrmsd(**a)
    long = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2 ** 23 + 1, 16, 3), (0, 0, 0))       # shapes alone decide this
    with pytest.raises(ValueError, match="frames"):
        Q.dockq(**dict(base, xyz=long))
    with pytest.raises(ValueError, match="frames"):
        Q.fit_rmsd(c["xyz0"], long, [0, 1, 2], [8], model=m)
    for kw in (dict(sel_fit=[0, 1]), dict(sel_fit=[0, 1, 16]), dict(sel_measure=[]), dict(sel_measure=[-1]), dict(sel_fit=None), dict(sel_measure=None),
               dict(scale=0.0), dict(scale=-2.0), dict(scale=np.nan), dict(xyz_ref=x[:2]), dict(xyz_ref=c["xyz0"][:15]), dict(sel_fit=np.ones(15, bool))):
        args = dict(xyz_ref=c["xyz0"], xyz=x, sel_fit=[0, 1, 2], sel_measure=[8, 9], model=m)
        args.update(kw)
        with pytest.raises(ValueError):
            Q.fit_rmsd(**args)
    # the two checks that follow the set-up launches, with what those launches would return
    monkeypatch.setattr(Q, "_native_rows", lambda *a: np.zeros((0, 2), np.int32))
    with pytest.raises(ValueError, match="no native pair"):
        Q.dockq(**base)
    with pytest.raises(ValueError, match="no native pair"):
        Q.native_pairs(c["xyz0"], c["ids_R"], c["ids_L"], c["roa"], scale=1.0, model=m)
    monkeypatch.setattr(Q, "_native_rows", lambda *a: np.array([[0, 0], [1, 1]], np.int32))
    monkeypatch.setattr(Q, "_interface_lists", lambda *a: (np.array([0, 1, 3], np.int32), np.array([11], np.int32), 16, None))
    with pytest.raises(ValueError, match="interface holds 2 backbone"):
        Q.dockq(**base)
    # the set-up's index arithmetic, without a launch: the pairs in the topology's rows, the atoms by residue, a range pair per pair
    pairs, ranges, perm = Q._native(c["xyz0"][None], c["ids_R"].astype(np.int32), c["ids_L"].astype(np.int32), c["roa"], 5.0, 1.0, m)
    assert pairs.tolist() == [[0, 2], [1, 3]] and perm.tolist() == list(range(16)) and ranges.tolist() == [[0, 4, 8, 12], [4, 8, 12, 16]]
    assert pairs.dtype == ranges.dtype == perm.dtype == np.int32


def test_new_symbols_are_declared_exported_and_bound():
    from pesto_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    new = ["pesto_dockq_last_error", "pesto_dockq", "pesto_fit_rmsd"]
    lib = _lib.load()
    for name in new:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.pesto_dockq_last_error.restype is not None
    for name in new[1:]:                                # each entry point cites what it replaces
        decl = hdr[:hdr.index(f"int {name}(")]
        assert "trajectory_utils.py:" in decl[decl.rindex("/*"):] and "replaces" in decl[decl.rindex("/*"):], name
    assert int(re.search(r"PESTO_DOCKQ_MAX_FRAMES = 1 << (\d+)", hdr).group(1)) == 23
    assert int(re.search(r"PESTO_DOCKQ_MAX_PAIRS = 1 << (\d+)", hdr).group(1)) == 24
    import pesto_amd
    from pesto_amd import dockq
    assert dockq.MAX_PAIRS == 2 ** 24 and pesto_amd.dockq is dockq and pesto_amd.lrmsd is dockq.lrmsd and pesto_amd.fit_rmsd is dockq.fit_rmsd
    assert pesto_amd.native_pairs is dockq.native_pairs and pesto_amd.capri_class is dockq.capri_class
    assert "pesto_dockq.hip" in open(os.path.join(ROOT, "pesto_amd", "csrc", "build.py")).read()
