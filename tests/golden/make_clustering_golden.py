#!/usr/bin/env python3
"""Generate the clustering golden (tests/golden/clustering.npz) by IMPORTING the reference's own md_analysis/mdtraj_utils/trajectory_utils.py
from /root/reference (build container only; nothing under tests/ reads the reference at run time). mdtraj is stubbed (no function that
is called needs it) and the module is imported as a submodule of a stub package, as make_trajectory_golden.py does. Everything runs on
the CPU.

RMSD cases (the 29 frames are those of frames_md_1JTG_uL.npz, [29, 2030, 3] in angstrom, so scale = 1; referenced by index, not copied)
  md29_all   the 29 frames against themselves, all atoms
  md29_sel   the same on sel = arange(0, 2030, 7), n = 290
  md29_rect  frames 0..4 against frames 3..28: frames 3 and 4 are on both sides, so two pairs are exact duplicates
  mirror     frame 5 of md29_sel against its mirror image (z negated): a proper rotation cannot undo it
  near       frame 0 against itself plus Gaussian noise of sigma 1e-6, 1e-4 and 1e-2 A, each randomly rotated and shifted by some
             tens of angstrom (a few nm): the cancellation case
  tiny       rank-deficient covariances: n = 1 (all zeros), n = 2, n = 3 collinear, n = 4 planar; 2 x 3 frames each (tiny_n1 .. tiny_n4,
             one e_ref for the four)
Recorded per case: the reference's float32 result, superpose_transform + the expression of rmsd pair by pair (the superposed frame
kept in float32, as mdtraj keeps xyz); the float64 restatement (explicit superposition by np.linalg.svd, then the coordinate
differences); e_ref = max |reference - restatement|.

Clustering: for the float64 md29_all matrix the cutoffs 1.36675, 1.47542 and 1.55823 with the labels, centres and sizes of the integer
definition (gromos_def). Asserted: around each cutoff the matrix has a gap of more than 100 x the RMSD tolerance of md29_all and no entry
within that tolerance, so every matrix within tolerance has the same adjacency and the same clusters.

Usage:  python tests/golden/make_clustering_golden.py
"""
import importlib
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
EPS32 = float(np.finfo(np.float32).eps)
SEEDS = {"near": 23, "tiny": 29}
CUTOFFS = (1.36675, 1.47542, 1.55823)


def import_reference():
    sys.modules.setdefault("mdtraj", types.ModuleType("mdtraj"))
    pkg = types.ModuleType("mdtraj_utils")
    pkg.__path__ = [os.path.join(REF, "md_analysis", "mdtraj_utils")]
    sys.modules["mdtraj_utils"] = pkg
    return importlib.import_module("mdtraj_utils.trajectory_utils")


def reference_rmsd(tu, a, b, scale):
    """float32 [Fa, Fb]: the reference's superpose_transform, its transform as superpose applies it, the last line of its rmsd"""
    D = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for i in range(a.shape[0]):
        ref = a[i:i + 1]
        t, R, tr = tu.superpose_transform(ref, b)
        sup = (np.matmul(b - t, R) + tr).astype(np.float32)
        D[i] = np.sqrt(np.mean(np.sum(np.square(sup - ref), axis=2), axis=1)) * np.float32(scale)
    return D


def pairwise_rmsd64(a, b, scale):
    """float64 [Fa, Fb]: explicit optimal proper rotation of every b_j onto every a_i, then the RMS coordinate difference"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    a, b = a - a.mean(1, keepdims=True), b - b.mean(1, keepdims=True)
    D = np.zeros((a.shape[0], b.shape[0]))
    for i in range(a.shape[0]):
        U, _, Vt = np.linalg.svd(np.einsum("na,fnb->fab", a[i], b))
        Vt[:, 2] *= np.sign(np.linalg.det(U) * np.linalg.det(Vt))[:, None]
        R = np.einsum("fka,fbk->fab", Vt, U)                                    # b R lies on a
        gap = np.einsum("fna,fac->fnc", b, R) - a[i][None]
        D[i] = np.sqrt((gap * gap).sum(-1).mean(-1)) * scale
    return D


def gromos_def(D, cutoff):
    """(labels, centers, sizes) of the integer definition"""
    F = D.shape[0]
    adj = (D <= np.float32(cutoff)) | np.eye(F, dtype=bool)
    active, labels, centers, sizes = np.ones(F, bool), np.full(F, -1, np.int32), [], []
    while active.any():
        cnt = np.where(active, (adj & active[None]).sum(1), -1)
        c = int(np.argmax(cnt))                                                 # the first of the largest
        mem = adj[c] & active
        labels[mem] = len(centers)
        centers.append(c)
        sizes.append(int(mem.sum()))
        active &= ~mem
    return labels, np.array(centers, np.int32), np.array(sizes, np.int32)


def rg_of(*frames):
    """the largest RMS radius of the frames' atoms about their mean"""
    out = 0.0
    for x in frames:
        x = x.astype(np.float64)
        out = max(out, float(np.sqrt(np.square(x - x.mean(1, keepdims=True)).sum(-1).mean(-1)).max()))
    return out


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def main():
    tu = import_reference()
    X = np.load(os.path.join(OUT, "frames_md_1JTG_uL.npz"))["X_frames"]
    assert X.shape == (29, 2030, 3) and X.dtype == np.float32
    sel = np.arange(0, 2030, 7)
    out, e_ref = {"sel7": sel.astype(np.int32)}, {}

    def record(case, a, b, scale, group=None):
        ref, f64 = reference_rmsd(tu, a, b, scale), pairwise_rmsd64(a, b, scale)
        out[case + "_ref"], out[case + "_f64"] = ref, f64
        e = float(np.abs(ref.astype(np.float64) - f64).max())
        e_ref[group or case] = max(e_ref.get(group or case, 0.0), e)
        return f64

    D_all = record("md29_all", X, X, 1.0)
    record("md29_sel", X[:, sel], X[:, sel], 1.0)
    out["md29_rect_ia"], out["md29_rect_ib"] = np.arange(0, 5, dtype=np.int32), np.arange(3, 29, dtype=np.int32)
    record("md29_rect", X[0:5], X[3:29], 1.0)
    mirrored = X[5:6, sel] * np.array([1, 1, -1], np.float32)
    d = record("mirror", X[5:6, sel], mirrored, 1.0)
    assert d[0, 0] > 1.0
    rng = np.random.default_rng(SEEDS["near"])
    near = []
    for sigma in (1e-6, 1e-4, 1e-2):
        x = X[0].astype(np.float64) + rng.normal(0.0, sigma, X[0].shape)
        near.append((x @ random_rotation(rng) + rng.uniform(-40.0, 40.0, 3)).astype(np.float32))
    out["near_b"] = np.stack(near)
    d = record("near", X[0:1], out["near_b"], 1.0)
    print("near:", d[0])
    rng = np.random.default_rng(SEEDS["tiny"])
    axis, u, v = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3)
    tiny = {
        "tiny_n1": lambda: np.zeros((1, 3)),
        "tiny_n2": lambda: rng.normal(0.0, 2.0, (2, 3)),
        "tiny_n3": lambda: rng.normal(0.0, 2.0, (3, 1)) * axis[None] + rng.normal(0.0, 5.0, 3),            # collinear
        "tiny_n4": lambda: rng.normal(0.0, 2.0, (4, 1)) * u[None] + rng.normal(0.0, 2.0, (4, 1)) * v[None],   # planar, through the origin
    }
    for case, make in tiny.items():
        a = np.stack([make() for _ in range(2)]).astype(np.float32)
        b = np.stack([make() @ random_rotation(rng) for _ in range(3)]).astype(np.float32)
        out[case + "_a"], out[case + "_b"] = a, b
        record(case, a, b, 1.0, group="tiny")
    for case in list(tiny):
        out[case + "_eref"] = np.float64(e_ref["tiny"])
    for case in ("md29_all", "md29_sel", "md29_rect", "mirror", "near"):
        out[case + "_eref"] = np.float64(e_ref[case])
    out["e_floor"] = np.float64(min(e_ref.values()))
    assert out["e_floor"] > 0

    # ---- clustering of the float64 md29_all matrix
    tol = max(4.0 * e_ref["md29_all"], 4.0 * EPS32 * max(float(D_all.max()), rg_of(X)))
    entries = np.sort(D_all[np.triu_indices(29, 1)])
    out["cutoffs"] = np.array(CUTOFFS, np.float64)
    for k, cut in enumerate(CUTOFFS):
        below, above = entries[entries <= cut].max(), entries[entries > cut].min()
        print(f"cutoff {cut}: gap {above - below:.3e} ({below:.5f} .. {above:.5f}), tolerance {tol:.2e}")
        assert above - below > 100.0 * tol and min(cut - below, above - cut) > tol, (cut, below, above, tol)
        labels, centers, sizes = gromos_def(D_all.astype(np.float32), cut)
        assert all(np.array_equal(v, w) for v, w in zip(gromos_def(D_all, cut), (labels, centers, sizes)))
        out[f"cl{k}_labels"], out[f"cl{k}_centers"], out[f"cl{k}_sizes"] = labels, centers, sizes
        print(f"    {len(centers)} clusters, sizes {sizes}, centres {centers}")

    out["seeds"] = np.array(sorted(SEEDS.items()), dtype="S")
    path = os.path.join(OUT, "clustering.npz")
    np.savez_compressed(path, **out)
    print("e_ref (the reference's maximum deviation from the float64 restatement):")
    for k, v in e_ref.items():
        print(f"    {k:12s} {v:.2e}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
