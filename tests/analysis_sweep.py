"""Deterministic case generators of the analysis sweeps (a plain module: tests/test_analysis_sweep_fixture.py checks the generators without a
GPU, tests/test_analysis_sweep.py puts every case through its entry point on one).

A case is a tuple (family, seed, shape). The lists below are fixed, so a failure names its case and two runs execute the same cases.
``build(entry, case)`` returns the case's inputs and the expected outputs of the definitions the fixture modules already hold
(test_trajectory_fixture, test_docking_fixture, test_hbonds_fixture, test_sasa_fixture; test_cellgrid's brute force), all pinned to the
reference project's recorded outputs by the CPU suite. Inputs come from numpy.random.default_rng([seed, attempt]): a builder draws again
(attempt 0, 1, ...) until the properties it promises hold - a hit, an empty and a crowded frame, the 1 % cap of the cell-grid cases - which
are properties of the definitions alone, asserted by the fixture test; no builder looks at the library.

family = kind [+flag ...]:
    lattice     coordinates are multiples of 1/16 with |x| < 32 in angstroms (``scale`` 1 where an entry point has a scale): every
                coordinate difference is a multiple of 1/16 below 64, every squared distance an integer multiple of 2^-8 below 2^14 and
                exact in float32 in any order of summation, fused or not. Thresholds lie on attained distances (3-4-5 offsets: d = 5 and
                d = 2.5), bin edges on attained float32 distances, so the strict / non-strict comparison is decided by the definition.
    graze       (hbonds, docking) a lattice case with one planted pair whose float32 squared distance lies one unit BELOW r_thr^2 while
                its correctly rounded root is r_thr itself: d < r_thr fails though s < r_thr^2 holds. The kernels compare s with a
                threshold s* derived on the host; this pair has s == s*, so `s < s*` against `s <= s*` is decided here and nowhere else
    rough       full-mantissa float32 coordinates (nanometres and scale 10 where an entry point has a scale)
    rough9k     the same, translated by (9000, -9000, 9000) angstroms (PDB's coordinate range): differences are no longer exact
    +nan +inf   one coordinate is NaN / infinite, where the group's documentation says it is harmless      +group   (hbonds) a group filter
Edge sets (the constants are read from the sources named; tests assert the coverage table built from the lists, REQUIRED below):
    pesto_trajectory.hip  CT = 16 (count tile), CF = 32 frames staged, FU = 4 frames side by side, LT = 32, LF = 64, JU = 4, bins: B with
                          top < B and an empty bin
    pesto_hbonds.hip      HB_ROWS = 8, HB_TILE = 32 (= hbonds.DONOR_TILE), 64-lane acceptor walk, NT = 256 (k_frame_scan over P and over the
                          acceptor blocks), LIST_SCAN_NT = 1024 (pesto_scan.h: frames of frame_hbonds, donor pairs of the occupancy list)
    pesto_docking.hip     FC_ROWS = 8, FC_TILE = 32, 64-lane partner walk, NT = 256 (k_frame_scan over Na), SCAN_NT = 1024 (over F)
    pesto_sasa.hip        NT = 256, WAVES = 4 atoms per workgroup, TILE = 256 candidate records, MB = 64 points per mask
    pesto_fit.h           NT = 256 threads stride a selection (the superposition fit of the trajectory, docking and DockQ groups), 64-lane waves
    pesto_cellgrid.h      GRID_MAX = 64 cells per axis, 2 N + 64 cells, h *= 1.25f, 256-thread setup / count, 1024-thread k_grid_scan
"""
import functools
import math

import numpy as np

from test_cellgrid import RES_ATOMS
from test_docking_fixture import contacts_def, dist_def, docking64, interface_def, irmsd64, residue_contacts_def
from test_hbonds_fixture import bonded_def, frame_hbonds_def, hydrogen_bonds_def, occupancy_def, unwrap_def
from test_sasa_fixture import areas_of, group_sums
from test_trajectory_fixture import centroids64, counts_def, dist, kl64, loglik64, maps_def, p_of_counts, superpose64

EPS32 = float(np.finfo(np.float32).eps)
FAR = np.array([9000.0, -9000.0, 9000.0], np.float32)


def case_id(case):
    family, seed, shape = case
    flat = []
    for v in shape:
        flat.append("-".join(f"{a}{b}" for a, b in v) if isinstance(v, tuple) and v and isinstance(v[0], tuple) else
                    "-".join(str(a) for a in v) if isinstance(v, tuple) else str(v))
    return f"{family}_s{seed}_" + "x".join(flat)


def parse(family):
    kind, *flags = family.split("+")
    return kind, set(flags)


def lattice_points(rng, shape, span):
    """float32 multiples of 1/16 in [-span, span]"""
    return (rng.integers(-int(16 * span), int(16 * span) + 1, shape) / 16.0).astype(np.float32)


def rough_points(rng, shape, span):
    return rng.uniform(-span, span, shape).astype(np.float32)


def points(rng, kind, shape, span):
    return lattice_points(rng, shape, span) if kind == "lattice" else rough_points(rng, shape, span)


def drawn(draw, seed, tries=400):
    """the first draw(rng) of attempts 0, 1, ... that is not None"""
    for attempt in range(tries):
        c = draw(np.random.default_rng([seed, attempt]))
        if c is not None:
            c["attempt"] = attempt
            return c
    raise AssertionError(f"seed {seed}: no draw in {tries} attempts has the promised properties")


def rows_of(rng, n, layout):
    """int32 [n] dense residue rows, not contiguous: 'one' atom per residue, 'all' atoms in one residue, 'mixed'"""
    if layout == "one":
        r = np.arange(n)
    elif layout == "all":
        r = np.zeros(n, np.int64)
    else:
        r = np.unique(rng.integers(0, max(1, n // 3), n), return_inverse=True)[1].reshape(-1)
    return rng.permutation(r).astype(np.int32)


def ulps_apart(a, b):
    """float32 units between two arrays of non-negative finite floats (int64)"""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(0, 1, (3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


# ================================================================== pesto_trajectory.hip: counts, P, log-likelihood, KL, maps, centroids
# shape (Na, Nb, F, B, frame_splits); Nb = 0: the trajectory against itself (xyz1=None); frame_splits 0: None
COUNTS = (
    ("lattice", 11, (1, 1, 1, 1, 0)),
    ("lattice", 12, (15, 17, 3, 2, 2)),
    ("lattice+nan", 13, (16, 16, 4, 3, 3)),
    ("lattice", 14, (17, 33, 5, 20, 5)),
    ("lattice", 15, (33, 15, 31, 64, 0)),
    ("lattice", 16, (33, 0, 32, 20, 2)),
    ("rough", 17, (16, 1, 33, 3, 3)),
    ("rough9k", 18, (17, 16, 65, 64, 65)),
    ("rough+nan", 19, (1, 33, 65, 20, 2)),
    ("rough+inf", 20, (15, 15, 32, 2, 3)),
    ("rough", 21, (33, 33, 4, 1, 0)),
    ("lattice+nan", 22, (16, 17, 65, 3, 3)),
)
# shape (Na, Nb, F, B)
LOGLIK = (
    ("rough", 31, (1, 1, 1, 3)),
    ("rough", 32, (3, 5, 63, 20)),
    ("rough+nan", 33, (4, 31, 64, 20)),
    ("rough", 34, (5, 32, 65, 3)),
    ("lattice", 35, (31, 4, 1, 20)),
    ("rough9k", 36, (32, 33, 65, 20)),
    ("rough+inf", 37, (33, 3, 64, 64)),
    ("lattice", 38, (33, 33, 63, 2)),
)
# shape (Na, Nb, F, residue layout)
MAPS = (
    ("lattice", 41, (1, 1, 1, "one")),
    ("lattice", 42, (15, 33, 3, "mixed")),
    ("lattice+nan", 43, (64, 65, 2, "all")),
    ("rough", 44, (63, 17, 5, "one")),
    ("rough9k", 45, (33, 64, 3, "mixed")),
    ("rough+inf", 46, (16, 16, 2, "mixed")),
)
# shape (N, F, residue layout)
CENTROIDS = (
    ("lattice", 51, (1, 1, "one")),
    ("rough", 52, (255, 3, "mixed")),
    ("rough9k", 53, (257, 2, "all")),
    ("rough+nan", 54, (64, 5, "mixed")),
)


def _nonfinite(flags, rng, arrays):
    """one NaN or infinite coordinate in the first array that has more than one atom (else the first)"""
    if not flags & {"nan", "inf"}:
        return
    a = next((v for v in arrays if v is not None and v.shape[1] > 1), arrays[0])
    a[int(rng.integers(0, a.shape[0])), a.shape[1] - 1, int(rng.integers(0, 3))] = np.nan if "nan" in flags else np.inf


def _pair_clouds(rng, kind, Na, Nb, F, span=4.0):
    x0 = points(rng, kind, (F, Na, 3), span)
    x1 = None if Nb == 0 else points(rng, kind, (F, Nb, 3), span)
    if kind == "lattice" and x1 is not None:
        x1[0, 0] = x0[0, 0] + np.array([0.75, 1.0, 0.0], np.float32)          # a 3-4-5 pair: d = 1.25 exactly
    if kind == "rough9k":
        x0 += FAR
        if x1 is not None:
            x1 += FAR
    return x0, x1


def _attained(x0, x1):
    d = dist(x0, x0 if x1 is None else x1)
    return np.unique(d[np.isfinite(d)]).astype(np.float64)


def _edges(kind, att, B):
    """(B + 1 float64 edges, the two synthetic edges of the empty bin or ()). lattice: every edge is an attained float32 distance, but
    for B = 20, where two edges one and two float64 units above an attained distance e make the bin [e, e+) that holds exactly d == e
    and the bin behind it that nothing can fall into (two equal edges are refused: this is as near as edges get); when a case attains
    fewer than B + 1 distances the last ones are whole numbers behind the largest. rough: an even grid that no float32 value lies on."""
    if kind != "lattice":
        return np.linspace(0.3141, float(np.quantile(att, 0.8)) + 0.2718, B + 1), ()
    need = B + 1 - (2 if B == 20 else 0)
    if att.size >= need:
        e = att[np.linspace(0, att.size - 1, need).round().astype(np.int64)]
    else:
        e = np.concatenate([att, att[-1] + np.arange(1, need - att.size + 1)])
    if B != 20:
        return e, ()
    s1 = np.nextafter(e[need // 2], np.inf)
    s2 = np.nextafter(s1, np.inf)
    return np.sort(np.concatenate([e, [s1, s2]])), (float(s1), float(s2))


def build_counts(case):
    family, seed, (Na, Nb, F, B, splits) = case
    kind, flags = parse(family)

    def draw(rng):
        x0, x1 = _pair_clouds(rng, kind, Na, Nb, F)
        _nonfinite(flags, rng, [x1, x0])
        bins, synthetic = _edges(kind, _attained(x0, x1), B)
        counts = counts_def(x0, x1, bins)
        if counts.sum() == 0:
            return None
        return dict(x0=x0, x1=x1, bins=bins, synthetic=synthetic, frame_splits=splits or None, counts=counts.astype(np.uint32),
                    P=p_of_counts(counts.astype(np.uint32)))
    return drawn(draw, seed)


def build_loglik(case):
    family, seed, (Na, Nb, F, B) = case
    kind, flags = parse(family)

    def draw(rng):
        x0, x1 = _pair_clouds(rng, kind, Na, Nb, F)
        y0, y1 = _pair_clouds(rng, kind, Na, Nb, F)
        _nonfinite(flags, rng, [x1, x0])
        bins, synthetic = _edges(kind, _attained(x0, x1), B)
        cp, cq = counts_def(x0, x1, bins), counts_def(y0, y1, bins)
        if cp.sum() == 0 or cq.sum() == 0:
            return None
        P, Q = p_of_counts(cp.astype(np.uint32)), p_of_counts(cq.astype(np.uint32))
        if not np.abs(kl64(Q, P)).max() > 0:
            return None
        return dict(x0=x0, x1=x1, y0=y0, y1=y1, bins=bins, synthetic=synthetic, P=P, Q=Q, L=loglik64(x0, x1, bins, P),
                    L_other=loglik64(y0, y1, bins, P), KL=kl64(Q, P))
    return drawn(draw, seed)


def _scaled(kind, rng, *arrays):
    """(arrays, scale, unit): lattice stays in angstroms with scale 1; rough goes to nanometres (scale 10) with a full mantissa"""
    if kind in ("lattice", "graze"):
        return arrays, 1.0
    out = []
    for a in arrays:
        b = (a.astype(np.float64) * 0.1 + rng.normal(0, 2e-4, a.shape)).astype(np.float32)
        out.append(b + FAR * np.float32(0.1) if kind == "rough9k" else b)
    return out, 10.0


def build_maps(case):
    family, seed, (Na, Nb, F, layout) = case
    kind, flags = parse(family)

    def draw(rng):
        side = min(60.0, max(6.0, (523.0 * Nb) ** (1.0 / 3.0)))
        xa, xb = lattice_points(rng, (F, Na, 3), side / 2), lattice_points(rng, (F, Nb, 3), side / 2)
        xb[0, 0] = xa[0, 0] + np.array([3.0, 4.0, 0.0], np.float32)           # d = 5 = r_thr exactly: not a contact (strict)
        (xa, xb), scale = _scaled(kind, rng, xa, xb)
        _nonfinite(flags, rng, [xb, xa])
        ra, rb = rows_of(rng, Na, layout), rows_of(rng, Nb, layout)
        maps = maps_def(xa, xb, ra, rb, 5.0, scale)
        if maps[0].sum() == 0 and Na * Nb > 1:
            return None
        if Na * Nb == 1:                                                       # the single pair: one step inside
            xb[0, 0] = xa[0, 0] + np.array([3.0, 3.9375, 0.0], np.float32)
            maps = maps_def(xa, xb, ra, rb, 5.0, scale)
        nat = (maps & maps[:1]).sum((1, 2)).astype(np.int64)
        return dict(xa=xa, xb=xb, res_a=ra, res_b=rb, r_thr=5.0, scale=scale, maps=maps, native=nat, fnat=nat / maps[:1].sum())
    return drawn(draw, seed)


def build_centroids(case):
    family, seed, (N, F, layout) = case
    kind, flags = parse(family)
    rng = np.random.default_rng([seed, 0])
    x = points(rng, kind, (F, N, 3), 16.0)
    if kind == "rough9k":
        x += FAR
    roa = rows_of(rng, N, layout)
    if "nan" in flags:
        x[0, 0, 1] = np.nan
    return dict(x=x, roa=roa, R=int(roa.max()) + 1, want=centroids64(x, roa), attempt=0)


# ================================================================== pesto_hbonds.hip
# shape (P, A, F)
HBONDS = (
    ("lattice", 61, (1, 63, 2)),
    ("lattice+group", 62, (7, 64, 1)),
    ("lattice+nan", 63, (8, 65, 2)),
    ("lattice+group", 64, (9, 129, 1)),
    ("rough", 65, (31, 1, 257)),
    ("rough+group+nan", 66, (32, 63, 2)),
    ("rough9k", 67, (33, 64, 1)),
    ("rough+group+inf", 68, (65, 65, 2)),
    ("lattice+group+nan", 69, (33, 129, 3)),
    ("rough", 70, (8, 8, 1025)),
    ("lattice", 71, (1030, 5, 2)),
    ("graze", 72, (9, 65, 2)),
)
# shape (molecule sizes, F)
UNWRAP = (
    ("lattice", 81, ((1,), 1)),
    ("lattice", 82, ((255, 1, 257), 2)),
    ("lattice+tie", 83, ((1, 1, 1, 2), 2)),
    ("rough", 84, ((256, 600, 2, 3, 1), 3)),
    ("rough+nan", 85, ((5, 257, 256), 3)),
    ("lattice+inf", 86, ((3, 4), 2)),
)
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)


def build_hbonds(case):
    """Donor atoms carry two hydrogens each (donor pairs 2 k and 2 k + 1), one angstrom away along different axes; a quarter of the
    acceptor table are donor atoms themselves (j != don[r]), the others atoms of their own that move from frame to frame. The last
    frame (F >= 2) puts every hydrogen on its donor (uu = 0: no bond in that frame). lattice: the first acceptor of its own sits, in
    frame 0, 2.5 from the hydrogen of donor pair 0 at 126.9 degrees: on the threshold, and out by the strict comparison alone."""
    family, seed, (P, A, F) = case
    kind, flags = parse(family)

    def draw(rng):
        nD = (P + 1) // 2
        shared = min(A // 4, nD)
        nX = A - shared
        N = nD + P + nX
        side = max(3.0, (16.4 * A / 1.2) ** (1.0 / 3.0))
        don = np.arange(P) // 2
        e = AXES[2 * (np.arange(P) % 2) + rng.integers(0, 2, P)]
        D = lattice_points(rng, (nD, 3), side / 2).astype(np.float64)
        if kind == "graze":
            D[0, 2] = -0.5                              # (so that the grazing coordinate below, 1.5 - 2^-23, is a float32 value)
        X = lattice_points(rng, (nX, 3), side / 2).astype(np.float64)
        xyz = np.repeat(np.concatenate([D, D[don] + e, X])[None], F, 0)
        xyz[:, nD + P:] += rng.integers(-8, 9, (F, nX, 3)) / 16.0
        if kind in ("lattice", "graze"):                # (pair 0's axis is +-x) graze: s = 2.25 + (4 - 2^-21) = 6.25 - one unit, its root 2.5
            xyz[0, nD + P] = xyz[0, nD] + 1.5 * e[0] + (2.0 - (2.0 ** -23 if kind == "graze" else 0.0)) * AXES[4]
        if F >= 2:
            xyz[F - 1, nD:nD + P] = xyz[F - 1, don]
        xyz = xyz.astype(np.float32)
        (xyz,), scale = _scaled(kind, rng, xyz)
        if F >= 2:
            xyz[F - 1, nD:nD + P] = xyz[F - 1, don]
        if flags & {"nan", "inf"}:
            xyz[0 if nX > 1 else F - 1, N - 1, 1] = np.nan if "nan" in flags else np.inf
        relabel = rng.permutation(N)
        out = np.empty_like(xyz)
        out[:, relabel] = xyz
        dh = relabel[np.stack([don, nD + np.arange(P)], 1)].astype(np.int32)
        acc = relabel[np.concatenate([rng.choice(nD, shared, replace=False), nD + P + np.arange(nX)])].astype(np.int32)
        group = rng.integers(0, 3, N).astype(np.int8) if "group" in flags else None
        crit = dict(r_thr=2.5, angle=120.0, scale=scale)
        off, trip, d = frame_hbonds_def(out, dh, acc, group=None, **crit)
        if off[-1] == 0:
            return None
        per_frame = np.diff(off)
        per_pair = np.zeros((F, P), np.int64)
        key = {(int(a), int(b)): k for k, (a, b) in enumerate(dh)}
        for f in range(F):
            for a, b, _ in trip[off[f]:off[f + 1]]:
                per_pair[f, key[(int(a), int(b))]] += 1
        if P * A >= 2 and not ((per_pair == 0).any() and (per_frame >= 2).any()):
            return None
        c = dict(xyz=out, dh=dh, acc=acc, group=group, off=off, trip=trip, d=d, per_pair=per_pair, **crit)
        if group is not None:
            if not ((group == 1).any() and (group == 2).any()):
                return None
            c["goff"], c["gtrip"], c["gd"] = frame_hbonds_def(out, dh, acc, group=group, **crit)
            if c["goff"][-1] == 0:
                return None
            c["nhb"], rows = hydrogen_bonds_def(out, dh, acc, group, **crit)
            c["rows"] = np.concatenate(rows).astype(np.int32).reshape(-1, 3)
        _, n0 = occupancy_def(out, dh, acc, 0.0, **crit)
        n0 = n0[n0 > 0]
        c["freq"] = float(n0.min()) / float(F) if n0.max() > n0.min() else 0.0      # a tie of the strict float(n) / float(F) > freq
        c["occ_trip"], c["occ_n"] = occupancy_def(out, dh, acc, c["freq"], **crit)
        return c
    return drawn(draw, seed)


def build_unwrap(case):
    """Molecule m >= 1 is drawn around molecule 0 and then moved by a whole number of box lengths along every axis. lattice: box lengths
    and coordinates are multiples of 1/16 and the masses small integers, so every centre of mass is one correctly rounded division of
    exact sums, whatever the order of the sum. +tie: single atoms half a box away from molecule 0: two images at the same distance."""
    family, seed, (sizes, F) = case
    kind, flags = parse(family)

    def draw(rng):
        M, N = len(sizes), int(sum(sizes))
        mol = rng.permutation(np.repeat(np.arange(M), sizes)).astype(np.int32)
        box = np.tile(np.array([[20.0, 24.5, 30.25]]), (F, 1)) + (rng.integers(0, 16, (F, 3)) / 16.0)
        base = lattice_points(rng, (F, N, 3), 2.0).astype(np.float64)
        img = rng.integers(-1, 2, (F, M, 3))
        img[:, 0] = 0
        centre = lattice_points(rng, (F, M, 3), 3.0).astype(np.float64)
        centre[:, 0] = 0
        if "tie" in flags:
            box = np.round(box * 8) / 8
            base[:], img[:] = 0.0, 0
            centre[:, 1] = box * [-0.5, 0, 0]
            centre[:, 2] = box * [0, 0.5, 0]
        xyz = base + (centre + img * box[:, None, :])[:, mol]
        if kind != "lattice":
            xyz = xyz + rng.normal(0, 1e-3, xyz.shape)
            box = box + rng.normal(0, 1e-3, box.shape)
        xyz, box = xyz.astype(np.float32), box.astype(np.float32)
        masses = rng.integers(1, 17, N).astype(np.float64) if kind == "lattice" else rng.uniform(1.0, 60.0, N)
        if "nan" in flags:
            xyz[1, int(np.nonzero(mol == M - 1)[0][0]), 2] = np.nan
            box[2, 0] = np.nan
        if "inf" in flags:
            xyz[0, int(np.nonzero(mol == M - 1)[0][0]), 0] = np.inf
        with np.errstate(invalid="ignore"):
            out, image, gap = unwrap_def(xyz, box, mol, masses)
        planted = "tie" in flags
        with np.errstate(invalid="ignore"):
            close = gap <= 1e-6
        if (close.any() and not planted) or (M > 1 and not planted and not image.any()):
            return None
        return dict(xyz=xyz, box=box, mol=mol, masses=masses, out=out, image=image, gap=gap)
    return drawn(draw, seed)


# ================================================================== pesto_docking.hip
# shape (Na, Nb, F, residue layout)
DOCKING = (
    ("lattice", 91, (1, 63, 2, "one")),
    ("lattice", 92, (31, 64, 1, "mixed")),
    ("lattice+nan", 93, (32, 65, 2, "all")),
    ("rough", 94, (33, 129, 3, "mixed")),
    ("rough9k", 95, (65, 1, 2, "one")),
    ("rough+nan", 96, (257, 33, 2, "mixed")),
    ("rough", 97, (3, 4, 1023, "mixed")),
    ("lattice", 98, (2, 3, 1024, "one")),
    ("rough+inf", 99, (4, 2, 1025, "all")),
    ("lattice+nan", 100, (255, 7, 1, "mixed")),
    ("rough", 101, (256, 5, 2, "one")),
    ("rough", 102, (5, 3, 255, "mixed")),
    ("lattice", 103, (3, 5, 256, "all")),
    ("rough+nan", 104, (7, 8, 257, "mixed")),
    ("lattice", 105, (8, 9, 3, "mixed")),
    ("rough", 106, (9, 31, 2, "mixed")),
    ("graze", 107, (33, 65, 2, "mixed")),
)


def build_docking(case):
    """Two clouds in one box, fresh in every frame; the last frame (F >= 2) gathers side B in a point 6 beyond the box: no contact there.
    lattice: atom 0 of B sits exactly 5 (r_thr) from atom 0 of A in frame 0: out of the contacts (<), inside the interface (<=). The
    topology of the interface functions: the atoms of A, those of B, and one atom of neither side in the residue of A's atom 0."""
    family, seed, (Na, Nb, F, layout) = case
    kind, flags = parse(family)

    def draw(rng):
        side = min(40.0, max(6.0, (523.0 * Nb) ** (1.0 / 3.0)))
        xa, xb = lattice_points(rng, (F, Na, 3), side / 2), lattice_points(rng, (F, Nb, 3), side / 2)
        xb[0, 0] = xa[0, 0] + np.array([3.0, 4.0, 0.0], np.float32)
        if kind == "graze":                             # s = 9 + (16 - 2^-19) = 25 - one unit, its root 5: no contact by d < r_thr
            xa[0, 0, 1] = -1.0
            xb[0, 0] = xa[0, 0] + np.array([3.0, 4.0 - 2.0 ** -22, 0.0], np.float32)
        if F >= 2:
            xb[F - 1] = np.float32(math.ceil(side / 2) + 6)
        extra = np.full((F, 1, 3), -np.float32(math.ceil(side / 2) + 11), np.float32)
        (xa, xb, extra), scale = _scaled(kind, rng, xa, xb, extra)
        _nonfinite(flags, rng, [xb, xa])
        ra, rb = rows_of(rng, Na, layout), rows_of(rng, Nb, layout)
        off, pairs, d = contacts_def(xa, xb, 5.0, scale)
        if off[-1] == 0:
            return None
        per_atom = np.zeros((F, Na), np.int64)
        np.add.at(per_atom, (np.repeat(np.arange(F), np.diff(off)), pairs[:, 0]), 1)
        if Na * Nb >= 2 and not ((per_atom == 0).any() and (np.diff(off) >= 2).any()):
            return None
        roff, rpairs, dmin = residue_contacts_def(off, pairs, d, ra, rb)
        xyz = np.ascontiguousarray(np.concatenate([xa, xb, extra], 1))
        ids_a, ids_b = np.arange(Na), Na + np.arange(Nb)
        roa = np.concatenate([ra, int(ra.max()) + 1 + rb, ra[:1]]).astype(np.int64)
        with np.errstate(invalid="ignore"):
            ira, irb = interface_def(xyz[0], ids_a, ids_b, roa, 5.0, scale)
        if ira.size == 0 or irb.size == 0:
            return None
        return dict(xa=xa, xb=xb, res_a=ra, res_b=rb, r_thr=5.0, scale=scale, off=off, pairs=pairs, d=d, roff=roff, rpairs=rpairs, dmin=dmin,
                    xyz=xyz, ids_a=ids_a, ids_b=ids_b, roa=roa, ira=ira, irb=irb, per_atom=per_atom)
    return drawn(draw, seed)


# ================================================================== pesto_sasa.hip
# shape (structure sizes, F, sphere points)
SASA = (
    ("lattice", 111, ((1, 2), 1, 1)),
    ("lattice+nan", 112, ((2, 63), 3, 64)),
    ("rough", 113, ((64, 65, 1, 2, 63), 1, 96)),
    ("rough+nan", 114, ((257, 2), 1, 100)),
    ("rough9k", 115, ((65, 64, 1), 3, 64)),
    ("rough+inf", 116, ((63, 257), 1, 96)),
    ("rough", 117, ((300,), 1, 64)),            # every atom within reach of every other: 299 candidate records > TILE = 256
)


def sasa_counts(X, R, S, sizes):
    """int64 [N] of one frame: test_sasa_fixture.definition_counts with the loops over i and j as array axes (the same float32
    operations in the same order; the fixture test holds the two against each other)"""
    X, R, S = np.asarray(X, np.float32), np.asarray(R, np.float32), np.asarray(S, np.float32)
    out = np.full(X.shape[0], S.shape[0], np.int64)
    start = 0
    with np.errstate(all="ignore"):
        for n in sizes:
            x, r = X[start:start + n], R[start:start + n]
            ok = np.isfinite(x).all(1) & np.isfinite(r)
            rr = r * r
            for i0 in range(0, n, 32):
                i = np.arange(i0, min(n, i0 + 32))
                t = x[i][:, None, :] + r[i][:, None, None] * S[None]                             # [i, P, 3]
                d = t[:, :, None, :] - x[None, None, :, :]                                         # [i, P, j, 3]
                q = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                use = ok[None, :] & (np.arange(n)[None, :] != i[:, None])                          # [i, j]
                buried = ((q < rr[None, None, :]) & use[:, None, :]).any(2)
                out[start + i] = S.shape[0] - buried.sum(1)
            start += n
    return out


def build_sasa(case):
    family, seed, (sizes, F, P) = case
    kind, flags = parse(family)
    from pesto_amd.sasa import sphere_points
    S = sphere_points(P)

    def draw(rng):
        X, rows, base = [], [], 0
        for n in sizes:
            side = 3.0 if n == 300 else max(2.0, (20.0 * n) ** (1.0 / 3.0))
            X.append(points(rng, kind, (1, n, 3), side / 2))
            rows.append(base + rows_of(rng, n, "mixed"))
            base = int(rows[-1].max()) + 1
        X = np.concatenate(X, 1)
        X = np.repeat(X, F, 0) + points(rng, kind, (F,) + X.shape[1:], 0.5)
        if kind == "rough9k":
            X += FAR
        N = X.shape[1]
        R = (rng.integers(24, 57, N) / 16.0).astype(np.float32) if kind == "lattice" else rng.uniform(1.5, 3.5, N).astype(np.float32)
        if flags & {"nan", "inf"}:
            X[0, N - 1, 0] = np.nan if "nan" in flags else np.inf
        counts = np.stack([sasa_counts(X[f], R, S, sizes) for f in range(F)])
        if not (counts < P).any():
            return None
        rows = np.concatenate(rows).astype(np.int32)
        with np.errstate(all="ignore"):
            return dict(X=X, R=R, S=S, P=P, sizes=list(sizes), rows=rows, counts=counts.astype(np.int32), areas=areas_of(counts, R, P),
                        sums=group_sums(counts, R, P, rows))
    return drawn(draw, seed)


# ================================================================== pesto_cellgrid.h through its two users
R_THR = 5.0
BAND = 1e-3
# shape: ((kind of assembly, atoms), ...): 1 to 6 assemblies of two subunits each
CELLGRID = (
    ("lattice", 121, (("cube", 3),)),
    ("lattice", 122, (("cube", 257), ("slab", 256), ("point", 3), ("corner", 255), ("big", 600))),
    ("lattice+nan", 123, (("slab", 3), ("cube", 600), ("point", 2))),
    ("rough", 124, (("cube", 256), ("rod", 257), ("slab", 255), ("point", 3), ("corner", 600), ("budget", 2))),
    ("rough9k", 125, (("cube", 255), ("budget", 256), ("rod", 600), ("corner", 3))),
    ("rough+nan", 126, (("big", 600), ("cube", 2), ("budget", 257), ("slab", 3))),
    ("rough+inf", 127, (("cube", 257), ("cube", 3))),
)


def _assembly(rng, kind, shape, n):
    """(xyz float32 [n, 3], atoms of the first subunit). cube; rod: 400 long, more than 64 x r_thr x 1.001, so the 64-cells-per-axis cap
    sets the cell edge; slab; point: all atoms coincident (extent 0); corner: a cube with its last atom on the maximum corner of the
    bounding box; budget: tight pairs scattered through a 250 cube, whose cells at the r_thr edge exceed 2 N + 64 many times over
    (h *= 1.25f several times); big: 54.875 x 49.875 x 49.875 with atoms on both extreme corners: 11 x 10 x 10 = 1100 cells at the
    r_thr edge, within 2 N + 64 = 1264 and more than the 1024 threads of k_grid_scan (per > 1)."""
    n0 = max(1, n // 2)
    dense = min(30.0, max(6.0, (60.0 * n) ** (1.0 / 3.0)))
    if kind == "point":
        x = np.repeat(points(rng, shape, (1, 3), 8.0), n, 0)
    elif kind == "budget":
        c = points(rng, shape, (n0, 3), 125.0)
        x = np.concatenate([c, np.resize(c, (n - n0, 3)) + points(rng, shape, (n - n0, 3), 2.5)])
    else:
        ext = dict(cube=(dense,) * 3, corner=(dense,) * 3, slab=(dense * 1.4, dense * 1.4, 3.0), rod=(4.0, 4.0, 400.0),
                   big=(54.875, 49.875, 49.875))[kind]
        x = points(rng, shape, (n, 3), 1.0) * (np.array(ext, np.float32) / 2)
        if kind in ("corner", "big"):
            x[n - 1] = np.array(ext, np.float32) / 2
        if kind == "big":
            x[0] = -np.array(ext, np.float32) / 2
        if shape == "lattice":
            x = np.round(x * 16) / 16
    return np.ascontiguousarray(x, np.float32), n0


def chain_dist(xa, xb):
    """float32 [na, nb]: dist() of pesto_cellgrid.h - the differences rounded to float32, then sqrt(fma(z, z, fma(y, y, x * x))): the
    fused steps in float64 (exact products) rounded once each, as pesto_amd/topology.py emulates them"""
    from pesto_amd.topology import _fma_round_f32
    with np.errstate(all="ignore"):
        r = xb[None, :, :] - xa[:, None, :]
        x, y, z = (r[..., c].astype(np.float64) for c in range(3))
        t = (x * x).astype(np.float32).astype(np.float64)
        t = _fma_round_f32(y * y, t).astype(np.float64)
        return np.sqrt(_fma_round_f32(z * z, t))


def cellgrid_expected(asm):
    """From the float32 chain: pairs int64 [K, 2] (per assembly, a then b ascending), d float32 [K], ties uint8 [N], labelled residues
    bool [n_res]; from test_cellgrid's float64 brute force: pairs64 [K64, 2], near64 bool [K64]: within BAND of r_thr, band_pairs: every
    pair within BAND of r_thr, contact or not, n_near: their number"""
    pairs, d, ties, p64, near64, band_pairs, base = [], [], [], [], [], [], 0
    thr = np.float32(R_THR)
    for xyz, n0 in asm:
        D = chain_dist(xyz[:n0], xyz[n0:])
        with np.errstate(invalid="ignore"):
            ia, ib = np.where(D < thr)
            t = D == thr
        pairs.append(np.stack([ia + base, ib + base + n0], 1))
        d.append(D[ia, ib])
        ties.append(np.concatenate([t.any(1), t.any(0)]))
        x = xyz.astype(np.float64)
        with np.errstate(invalid="ignore"):
            D64 = np.sqrt(((x[:n0, None, :] - x[None, n0:, :]) ** 2).sum(-1))
            ja, jb = np.where(D64 < R_THR)
            band = np.abs(D64 - R_THR) <= BAND
        p64.append(np.stack([ja + base, jb + base + n0], 1))
        near64.append(band[ja, jb])
        band_pairs.append(np.stack(np.nonzero(band), 1) + [base, base + n0])
        base += xyz.shape[0]
    pairs = np.concatenate(pairs).astype(np.int64)
    res, n_res = atom_residues(asm)
    labelled = np.zeros(n_res, bool)
    labelled[res[pairs.reshape(-1)]] = True
    return dict(pairs=pairs, d=np.concatenate(d).astype(np.float32), ties=np.concatenate(ties).astype(np.uint8), labelled=labelled,
                pairs64=np.concatenate(p64).astype(np.int64), near64=np.concatenate(near64), band_pairs=np.concatenate(band_pairs).astype(np.int64),
                n_near=sum(b.shape[0] for b in band_pairs))


def atom_residues(asm):
    """test_cellgrid._atom_residues: RES_ATOMS consecutive atoms of a subunit form a residue"""
    res, r_base = [], 0
    for xyz, n0 in asm:
        for n in (n0, xyz.shape[0] - n0):
            res.append(np.arange(n) // RES_ATOMS + r_base)
            r_base += (n + RES_ATOMS - 1) // RES_ATOMS
    return np.concatenate(res).astype(np.int32), r_base


def build_cellgrid(case):
    family, seed, shape = case
    kind, flags = parse(family)

    def draw(rng):
        asm = []
        for a_kind, n in shape:
            x, n0 = _assembly(rng, a_kind, "lattice" if kind == "lattice" else "rough", n)
            if kind == "lattice" and a_kind != "point" and n >= 3:
                x[n0] = x[0] + np.array([3.0, 4.0, 0.0], np.float32) * (-1 if x[0, 0] > 0 else 1)      # d = r_thr exactly: a tie, no contact
            if kind == "rough9k":
                x = x + FAR
            asm.append((x, n0))
        if flags & {"nan", "inf"}:
            x, n0 = asm[0]
            x[1 if x.shape[0] > 2 else 0, 1] = np.nan if "nan" in flags else np.inf
        want = cellgrid_expected(asm)
        k64 = want["pairs64"].shape[0]
        if k64 == 0 or want["pairs"].shape[0] == 0:
            return None
        if kind != "lattice" and want["n_near"] > 0.01 * k64:
            return None
        return dict(asm=asm, **want)
    return drawn(draw, seed)


# ================================================================== kabsch_rotation through the one fit (pesto_fit.h) and its three users
# shape (selected atoms, F, 'one' reference frame | a reference 'per' frame)
SUPERPOSE = (
    ("generic", 201, (3, 1, "one")),
    ("generic", 202, (65, 5, "per")),
    ("rot180", 203, (4, 5, "one")),
    ("rot180", 204, (300, 5, "per")),
    ("identity", 205, (64, 1, "one")),
    ("identity", 206, (3, 5, "per")),
    ("mirror", 207, (65, 5, "one")),
    ("mirror+noise", 208, (4, 5, "per")),
    ("planar", 209, (64, 5, "one")),
    ("planar+mirror", 210, (300, 1, "one")),
    ("planar+mirror+noise", 211, (3, 5, "per")),
    ("slab2", 212, (65, 5, "one")),
    ("slab4+mirror", 213, (64, 5, "per")),
    ("slab7", 214, (300, 5, "one")),
    ("slab7+mirror", 215, (4, 1, "one")),
    ("collinear", 216, (64, 5, "per")),
    ("collinear", 217, (4, 5, "per")),
    ("square", 218, (4, 5, "one")),
    ("tetrahedron", 219, (4, 5, "per")),
    ("cube", 220, (8, 5, "one")),
    ("far9k", 221, (65, 5, "one")),
    ("far9k", 222, (3, 1, "one")),
    ("small", 223, (64, 5, "per")),
    ("small", 224, (300, 1, "one")),
    ("generic", 225, (255, 2, "one")),          # the workgroup edge (NT = 256 threads stride the selection): one short of it,
    ("generic", 226, (256, 2, "per")),          # ... on it,
    ("generic", 227, (257, 2, "one")),          # ... and one thread with a second atom
)
SYMMETRIC = dict(square=[(1, 1, 0), (-1, 1, 0), (-1, -1, 0), (1, -1, 0)], tetrahedron=[(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)],
                 cube=[(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)])
DEGENERATE = {"collinear": (0,), "tetrahedron": (2,), "cube": (2,)}          # family -> the frames built to leave the rotation undetermined
EXTRA = 7               # atoms outside the selection: the ligand of the rigid docking, and the unselected atoms of superpose


def determined(ref_sel, xyz_sel):
    """bool [F]: the float64 covariance H = sum (y - ty)^T (x - tx) fixes the rotation: s2 + d s3 >= 1e-6 s1, d = sign(det U det V)"""
    y, x = ref_sel.astype(np.float64), xyz_sel.astype(np.float64)
    H = np.einsum("fna,fnb->fab", y - y.mean(1, keepdims=True), x - x.mean(1, keepdims=True))
    U, s, Vt = np.linalg.svd(H)
    dsign = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    return s[:, 1] + dsign * s[:, 2] >= 1e-6 * s[:, 0]


def build_superpose(case):
    """ref [Fr, N, 3], xyz [F, N, 3] with N = n + EXTRA atoms, the family's point set in the selected rows ``sel`` (ascending), a generic
    cloud in the others. Every frame of xyz is the reference moved by a rigid motion of its own (rot180: the exact half turns about x, y, z
    and two random axes, no translation; identity: none at all; mirror: reflected first), the unselected atoms by a second motion on top
    (the ligand's own: angle 0.3 .. 2 rad), so the rigid docking has a translation and a rotation vector well away from 0 and pi."""
    family, seed, (n, F, mode) = case
    return drawn(lambda rng: _superpose_case(rng, family, n, F, mode), seed)


def _superpose_case(rng, family, n, F, mode):
    kind, flags = parse(family)
    N = n + EXTRA
    sel = np.sort(rng.choice(N, n, replace=False))
    rest = np.setdiff1d(np.arange(N), sel)
    Fr = F if mode == "per" else 1

    shaped = kind in ("planar", "collinear") or kind.startswith("slab")         # families whose property every reference frame keeps
    mirror, noisy = "mirror" in family, "noise" in family
    unit = 1e-3 if kind == "small" else 1.0

    def selected():
        if kind in SYMMETRIC:
            return 3.0 * np.array(SYMMETRIC[kind], np.float64)
        if kind == "collinear":
            return rng.uniform(-10, 10, (n, 1)) * random_rotation(rng)[0][None] + rng.normal(0, 1e-3, (n, 3))
        s = rng.normal(0, 3.0, (n, 3))
        if kind == "planar":
            s[:, 2] = 0.0
        if kind.startswith("slab"):
            s[:, 2] *= 10.0 ** -int(kind[4:])
        return s @ random_rotation(rng) if shaped else s

    base = selected()
    ref = np.zeros((Fr, N, 3))
    for f in range(Fr):
        if f == 0 or kind in SYMMETRIC:
            s = base
        elif kind == "collinear":
            s = rng.normal(0, 3.0, (n, 3))               # only frame 0 is collinear
        else:
            s = selected() if shaped else base + rng.normal(0, 0.3, base.shape)
        ref[f, sel], ref[f, rest] = s, rng.normal(0, 3.0, (EXTRA, 3)) + [12.0, 0, 0]
    ref *= unit
    if kind == "far9k":
        ref += FAR.astype(np.float64)
    ref = ref.astype(np.float32)
    xyz = np.zeros((F, N, 3))
    half_turns = [np.diag([1.0, -1, -1]), np.diag([-1.0, 1, -1]), np.diag([-1.0, -1, 1])]
    for f in range(F):
        y = ref[f if mode == "per" else 0].astype(np.float64)
        Q, t, noise = random_rotation(rng), rng.normal(0, 5.0, 3) * unit, 0.01 * unit
        if kind == "identity":
            Q, t, noise = np.eye(3), np.zeros(3), 0.0
        elif kind == "rot180":
            u = rng.normal(0, 1, 3)
            u /= np.linalg.norm(u)
            Q, t, noise = (half_turns[f] if f < 3 else 2.0 * np.outer(u, u) - np.eye(3)), np.zeros(3), 0.0
        elif kind in SYMMETRIC:                         # exact | perturbed | mirrored exact | mirrored perturbed | an exact half turn
            noise = (0.0, 3e-3, 0.0, 3e-3, 0.0)[f]
            Q = half_turns[0] if f == 4 else Q
        elif mirror and not noisy:
            noise = 0.0
        elif kind == "collinear" and f == 0:
            noise = 1e-3
        c = np.zeros(3) if kind == "rot180" else y[sel].mean(0)
        m = y - c
        if mirror or (kind in SYMMETRIC and f in (2, 3)):
            m = m * [1.0, 1.0, -1.0]
        x = m @ Q + c + t
        x[sel] += rng.normal(0, 1.0, (n, 3)) * noise
        # the ligand's own motion about its centroid
        angle, axis = rng.uniform(0.3, 2.0), rng.normal(0, 1, 3)
        axis /= np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        QL = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K
        lc = x[rest].mean(0)
        x[rest] = (x[rest] - lc) @ QL + lc + rng.normal(0, 2.0, 3) * unit + rng.normal(0, 0.01, (EXTRA, 3)) * unit
        xyz[f] = x
    xyz = xyz.astype(np.float32)
    if kind == "identity":
        xyz[:, sel] = ref[:, sel] if mode == "per" else np.repeat(ref[:, sel], F, 0)
    yr, xr = ref[:, sel], xyz[:, sel]
    t64, R64, tr64 = superpose64(yr, xr)
    sup64 = (xyz.astype(np.float64) - t64) @ R64 + tr64
    gap = sup64[:, sel] - yr.astype(np.float64)
    ok = determined(yr if mode == "per" else np.repeat(yr, F, 0), xr)
    design = np.ones(F, bool)
    design[[f for f in DEGENERATE.get(kind, ()) if f < F]] = False
    # the docking topology: every atom a residue of its own; selected atoms = receptor, the others = ligand; a threshold beyond every
    # distance makes all of them interface atoms, and the CA mask picks the selection for irmsd
    roa = np.arange(N, dtype=np.int64)
    ca = np.zeros(N, bool)
    ca[sel] = True
    half = N // 2
    irmsd_want, irmsd_sel = irmsd64(ref, xyz, np.arange(half), np.arange(half, N), roa, ca, 1e6, 1.0)
    assert np.array_equal(irmsd_sel, sel)
    dock_t, dock_r, _ = docking64(ref, xyz, sel, rest, roa, 1e6, 1.0)
    if np.linalg.norm(dock_r[design], axis=1).max() >= 2.5:      # (near pi the sign of the axis is rounding's: r and -r are one rotation)
        return None
    return dict(ref=ref, xyz=xyz, sel=sel, rest=rest, t64=t64, R64=R64, tr64=tr64, sup64=sup64, rmsd64=np.sqrt((gap * gap).sum(-1).mean(-1)),
                determined=ok, design=design, roa=roa, ca=ca, half=half, irmsd64=irmsd_want, dock_t=dock_t, dock_r=dock_r)


# ================================================================== the registry
CASES = dict(counts=COUNTS, loglik=LOGLIK, maps=MAPS, centroids=CENTROIDS, hbonds=HBONDS, unwrap=UNWRAP, docking=DOCKING, sasa=SASA,
             cellgrid=CELLGRID, superpose=SUPERPOSE)
BUILDERS = dict(counts=build_counts, loglik=build_loglik, maps=build_maps, centroids=build_centroids, hbonds=build_hbonds, unwrap=build_unwrap,
                docking=build_docking, sasa=build_sasa, cellgrid=build_cellgrid, superpose=build_superpose)
# the library entry points every case of a list goes through
ENTRY_POINTS = dict(counts=("contact_counts", "contacts_distribution"), loglik=("StatisticalContactsModel.loglikelihood", "div_KL"),
                    maps=("residue_contact_maps", "native_contacts", "fnat"), centroids=("residue_centroids",),
                    hbonds=("frame_hbonds", "baker_hubbard", "hydrogen_bonds"), unwrap=("unwrap_pbc",),
                    docking=("frame_contacts", "contacts", "frame_residue_contacts", "interface_atoms"), sasa=("shrake_rupley",),
                    cellgrid=("dataset._contacts_call", "evaluate.contact_labels"),
                    superpose=("superpose_transform", "superpose", "rmsd", "irmsd", "interface_rigid_docking"))


@functools.lru_cache(maxsize=None)
def build(entry, case):
    return BUILDERS[entry](case)


def all_cases():
    return [(entry, case) for entry, cases in CASES.items() for case in cases]


def every_third(entry, case):
    """the cases that also run from host arrays"""
    return CASES[entry].index(case) % 3 == 0


def coverage():
    """{(case list, constant): the set of values the list's shapes hit}"""
    t = {}

    def hit(entry, name, values):
        t.setdefault((entry, name), set()).update(values)
    for _, _, (Na, Nb, F, B, splits) in COUNTS:
        hit("counts", "CT:Na", [Na]); hit("counts", "CT:Nb", [Nb or Na]); hit("counts", "CF,FU:F", [F]); hit("counts", "B", [B])
        hit("counts", "frame_splits", ["None" if not splits else "F" if splits == F else splits])
    for _, _, (Na, Nb, F, B) in LOGLIK:
        hit("loglik", "LT,JU:Na", [Na]); hit("loglik", "LT,JU:Nb", [Nb]); hit("loglik", "LF:F", [F])
    for family, _, (P, A, F) in HBONDS:
        hit("hbonds", "HB_ROWS,HB_TILE:P", [P]); hit("hbonds", "lanes:A", [A]); hit("hbonds", "F", [F])
        hit("hbonds", "group", ["group" in family]); hit("hbonds", "P>LIST_SCAN_NT", [P > 1024])
    for _, _, (sizes, F) in UNWRAP:
        hit("unwrap", "NT:molecule", sizes); hit("unwrap", "F", [F]); hit("unwrap", "M", [len(sizes)])
    for _, _, (Na, Nb, F, layout) in DOCKING:
        hit("docking", "FC_ROWS,FC_TILE,NT:Na", [Na]); hit("docking", "lanes:Nb", [Nb]); hit("docking", "NT,SCAN_NT:F", [F]); hit("docking", "residues", [layout])
    for _, _, (sizes, F, P) in SASA:
        hit("sasa", "sizes", sizes); hit("sasa", "structures", [len(sizes)]); hit("sasa", "F", [F]); hit("sasa", "points", [P])
    for _, _, shape in CELLGRID:
        hit("cellgrid", "assemblies", [len(shape)]); hit("cellgrid", "kind", [k for k, _ in shape]); hit("cellgrid", "atoms", [n for _, n in shape])
    for family, _, (n, F, mode) in SUPERPOSE:
        hit("superpose", "family", [family]); hit("superpose", "atoms", [n]); hit("superpose", "F", [F]); hit("superpose", "reference", [mode])
    return t


REQUIRED = {
    ("counts", "CT:Na"): {1, 15, 16, 17, 33}, ("counts", "CT:Nb"): {1, 15, 16, 17, 33}, ("counts", "CF,FU:F"): {1, 3, 4, 5, 31, 32, 33, 65},
    ("counts", "frame_splits"): {"None", 2, 3, "F"}, ("counts", "B"): {1, 2, 3, 20, 64},
    ("loglik", "LT,JU:Na"): {1, 3, 4, 5, 31, 32, 33}, ("loglik", "LT,JU:Nb"): {1, 3, 4, 5, 31, 32, 33}, ("loglik", "LF:F"): {1, 63, 64, 65},
    ("hbonds", "HB_ROWS,HB_TILE:P"): {1, 7, 8, 9, 31, 32, 33, 65}, ("hbonds", "lanes:A"): {1, 63, 64, 65, 129}, ("hbonds", "F"): {1, 2, 257, 1025},
    ("hbonds", "group"): {False, True}, ("hbonds", "P>LIST_SCAN_NT"): {False, True},
    ("unwrap", "NT:molecule"): {1, 255, 256, 257, 600}, ("unwrap", "F"): {1, 2, 3}, ("unwrap", "M"): {1, 2, 5},
    ("docking", "FC_ROWS,FC_TILE,NT:Na"): {1, 7, 8, 9, 31, 32, 33, 65, 255, 256, 257}, ("docking", "lanes:Nb"): {1, 63, 64, 65, 129},
    ("docking", "NT,SCAN_NT:F"): {1, 255, 256, 257, 1023, 1024, 1025}, ("docking", "residues"): {"one", "all", "mixed"},
    ("sasa", "sizes"): {1, 2, 63, 64, 65, 257, 300}, ("sasa", "structures"): {1, 2, 3, 5}, ("sasa", "F"): {1, 3}, ("sasa", "points"): {1, 64, 96, 100},
    ("cellgrid", "assemblies"): {1, 3, 4, 5, 6, 2}, ("cellgrid", "kind"): {"cube", "rod", "slab", "point", "corner", "budget", "big"},
    ("cellgrid", "atoms"): {2, 3, 255, 256, 257, 600},
    ("superpose", "atoms"): {3, 4, 64, 65, 255, 256, 257, 300}, ("superpose", "F"): {1, 2, 5}, ("superpose", "reference"): {"one", "per"},
    ("superpose", "family"): {"generic", "rot180", "identity", "mirror", "mirror+noise", "planar", "planar+mirror", "slab2", "slab4+mirror", "slab7",
                              "collinear", "square", "tetrahedron", "cube", "far9k", "small"},
}
