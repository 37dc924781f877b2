"""The NumPy definitions of pesto_amd.poses (place_def, scores_def, slide_def, top_def), the hand-worked cases that pin them, the host
helpers (rotation_set, poses_about), the seeded sweep systems the GPU tests draw too - with the asserts, on the definition alone, that
the sweep cannot pass vacuously - and the host side of the module: every ValueError without a GPU, the exports. No GPU here."""
import functools
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_docking_fixture import dist_def

EPS32 = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------ the definitions
def place_def(xyz_L, rotations, translations):
    """float32 [F, N_L, 3]: y_a = ((R[a,0]*x_0 + R[a,1]*x_1) + R[a,2]*x_2) + t_a, every operation a float32 one"""
    x, R, t = (np.asarray(v, np.float32) for v in (xyz_L, rotations, translations))
    with np.errstate(invalid="ignore", over="ignore"):
        return ((R[:, None, :, 0] * x[None, :, None, 0] + R[:, None, :, 1] * x[None, :, None, 1]) + R[:, None, :, 2] * x[None, :, None, 2]) + t[:, None, :]


def bits_def(member, R):
    """uint32 [ceil(R / 32)] of a boolean [R]"""
    words = np.zeros(-(-R // 32), np.uint32)
    for r in np.nonzero(member)[0]:
        words[r // 32] |= np.uint32(1) << np.uint32(r % 32)
    return words


def scores_def(xyz_R, xyz_L, res_R, res_L, rotations, translations, p_R, p_L, r_contact=5.0, r_clash=3.0, scale=10.0):
    """dict of the fields of PoseScores and masks, by the definition: the double sums are exactly rounded (math.fsum), and n_w_* hold the
    number of their terms (all terms are >= 0, so a sum is its own sum of absolute values)"""
    xR, pR, pL = np.asarray(xyz_R, np.float32), np.asarray(p_R, np.float32), np.asarray(p_L, np.float32)
    y = place_def(xyz_L, rotations, translations)
    F, R_R, R_L = y.shape[0], int(res_R.max()) + 1, int(res_L.max()) + 1
    D = dist_def(np.repeat(xR[None], F, 0), y, scale)                       # [F, N_R, N_L]
    with np.errstate(invalid="ignore"):
        hit, clash = D < np.float32(r_contact), D < np.float32(r_clash)
    out = dict(n_contact=hit.sum((1, 2)).astype(np.int32), n_clash=clash.sum((1, 2)).astype(np.int32))
    keys = ("n_res_R", "n_res_L", "n_pairs", "w_R", "w_L", "w_pair", "score", "masks")
    rows = {k: [] for k in keys}
    P_R, P_L = math.fsum(pR.astype(np.float64)), math.fsum(pL.astype(np.float64))
    for f in range(F):
        i, j = np.nonzero(hit[f])
        I_R, I_L = np.zeros(R_R, bool), np.zeros(R_L, bool)
        I_R[res_R[i]] = True
        I_L[res_L[j]] = True
        C = np.unique(np.stack([res_R[i], res_L[j]], 1), axis=0) if i.size else np.zeros((0, 2), np.int64)
        w_R, w_L = math.fsum(pR[I_R].astype(np.float64)), math.fsum(pL[I_L].astype(np.float64))
        w_pair = math.fsum(pR[C[:, 0]].astype(np.float64) * pL[C[:, 1]].astype(np.float64))
        n_R, n_L = int(I_R.sum()), int(I_L.sum())
        dice_R = 2.0 * w_R / (n_R + P_R) if n_R + P_R != 0 else 0.0
        dice_L = 2.0 * w_L / (n_L + P_L) if n_L + P_L != 0 else 0.0
        for k, v in zip(keys, (n_R, n_L, C.shape[0], w_R, w_L, w_pair, np.float32((dice_R + dice_L) / 2.0),
                               np.concatenate([bits_def(I_R, R_R), bits_def(I_L, R_L)]))):
            rows[k].append(v)
    for k in keys[:3]:
        out[k] = np.array(rows[k], np.int32)
    for k in keys[3:6]:
        out[k] = np.array(rows[k], np.float64)
    out["score"], out["masks"] = np.array(rows["score"], np.float32), np.stack(rows["masks"])
    out["n_w_R"], out["n_w_L"], out["n_w_pair"] = out["n_res_R"], out["n_res_L"], out["n_pairs"]
    return out


def slide_def(xyz_R, xyz_L, rotations, origins, directions, r_touch=3.5, scale=10.0):
    """(s float64 [F], translations float32 [F, 3], pair int32 [F, 2]) in NumPy float64, every operation rounded as written"""
    xR = np.asarray(xyz_R, np.float32).astype(np.float64)
    y = place_def(xyz_L, rotations, origins).astype(np.float64)
    o, U = np.asarray(origins, np.float32).astype(np.float64), np.asarray(directions, np.float32).astype(np.float64)
    rho = float(np.float32(r_touch)) / float(np.float32(scale))
    F = y.shape[0]
    s, t, pair = np.full(F, np.nan), np.full((F, 3), np.nan, np.float32), np.full((F, 2), -1, np.int32)
    for f in range(F):
        u = U[f]
        with np.errstate(invalid="ignore", over="ignore"):
            w = y[f][None, :, :] - xR[:, None, :]                          # [N_R, N_L, 3]
            b = (w[..., 0] * u[0] + w[..., 1] * u[1]) + w[..., 2] * u[2]
            c = ((w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]) - b * b
            disc = rho * rho - c
            counts = (disc > 0) & np.isfinite(w).all(-1)
            sij = np.where(counts, -b + np.sqrt(np.where(counts, disc, 0.0)), -np.inf)
        if counts.any():
            k = int(np.argmax(sij))                                        # the first maximum in (i, j) order
            s[f] = sij.reshape(-1)[k]
            pair[f] = divmod(k, sij.shape[1])
            t[f] = (o[f] + s[f] * u).astype(np.float32)
    return s, t, pair


def top_def(score, k, n_clash=None, max_clash=0):
    """int32 [min(k, eligible)]: by score descending, ties by index ascending, NaN scores and poses over max_clash left out"""
    score = np.asarray(score, np.float32)
    ok = ~np.isnan(score)
    if n_clash is not None:
        ok &= np.asarray(n_clash) <= max_clash
    idx = np.nonzero(ok)[0]
    return idx[np.argsort(-score[idx].astype(np.float64), kind="stable")][:k].astype(np.int32)


# ------------------------------------------------------------------ the hand-worked cases
def tiny():
    """2 + 2 residues in angstroms (scale = 1), coordinates multiples of 1 / 256. Receptor: A0 (residue 0), A1, A2 (residue 1); ligand:
    L0, L1 (residue 0), L2, L3 (residue 1). In the identity pose |A0 L0| = 5 exactly (a 3-4-5 offset: no contact), |A0 L1| = 3 exactly
    (a contact, no clash), |A1 L2| = 2 and |A2 L2| = sqrt(5) (clashes), everything else is far."""
    e = 1.0 / 256.0
    turn = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]                              # (x, y, z) -> (-y, x, z)
    return dict(xyz_R=np.array([[0, 0, 0], [20, 0, 0], [20, 1, 0]], np.float32), res_R=np.array([0, 1, 1], np.int32),
                xyz_L=np.array([[3, 4, 0], [0, 0, 3], [20, 0, 2], [40, 0, 0]], np.float32), res_L=np.array([0, 0, 1, 1], np.int32),
                p_R=np.array([0.5, 0.25], np.float32), p_L=np.array([0.75, 0.125], np.float32),
                rotations=np.array([np.eye(3), np.eye(3), turn, np.eye(3), np.eye(3)], np.float32),
                translations=np.array([[0, 0, 0], [0, 0, -e], [0, 0, 0], [1000, 0, 0], [-e, 0, 0]], np.float32))


# what the five poses of tiny() give, written out by hand:
#   0  identity            contacts A0-L1, A1-L2, A2-L2; the last two clash; both residues of both sides; pairs (0, 0), (1, 1)
#   1  1 / 256 down in z   L1 now clashes with A0 as well; L0 is still farther than 5
#   2  a quarter turn      L0 -> (-4, 3, 0): still exactly 5; L1 stays; L2 -> (0, 20, 2) is far: one contact, pair (0, 0)
#   3  1000 away           nothing
#   4  1 / 256 back in x   A0-L0 becomes a contact; A0-L1 moves beyond 3 but stays a contact
TINY = dict(n_contact=[3, 3, 1, 0, 4], n_clash=[2, 3, 0, 0, 2], n_res_R=[2, 2, 1, 0, 2], n_res_L=[2, 2, 1, 0, 2], n_pairs=[2, 2, 1, 0, 2],
            w_R=[0.75, 0.75, 0.5, 0.0, 0.75], w_L=[0.875, 0.875, 0.75, 0.0, 0.875], w_pair=[0.40625, 0.40625, 0.375, 0.0, 0.40625],
            masks=[[3, 3], [3, 3], [1, 1], [0, 0], [3, 3]])
# dice_R = 2 w_R / (n_res_R + 0.75), dice_L = 2 w_L / (n_res_L + 0.875)
TINY_SCORE = [(1.5 / 2.75 + 1.75 / 2.875) / 2, (1.5 / 2.75 + 1.75 / 2.875) / 2, (1.0 / 1.75 + 1.5 / 1.875) / 2, 0.0, (1.5 / 2.75 + 1.75 / 2.875) / 2]


def tiny_args(c):
    return (c["xyz_R"], c["xyz_L"], c["res_R"], c["res_L"], c["rotations"], c["translations"], c["p_R"], c["p_L"])


def test_hand_worked_case_pins_the_definition():
    from pesto_amd import poses as P
    c = tiny()
    got = scores_def(*tiny_args(c), r_contact=5.0, r_clash=3.0, scale=1.0)
    assert set(P.PoseScores._fields) == set(TINY) | {"score"}           # the hand-worked table names every field of the result
    # the five translations as poses_about gives them: L0 = (3, 4, 0) turned with the pose lands where the table says
    landed = place_def(c["xyz_L"][:1], c["rotations"], c["translations"])[:, 0].astype(np.float64)
    assert np.array_equal(P.poses_about(c["rotations"], c["xyz_L"][0], landed), c["translations"])
    for k, v in TINY.items():
        assert got[k].tolist() == v, k
    assert got["score"].tolist() == [float(np.float32(v)) for v in TINY_SCORE]
    assert got["masks"].dtype == np.uint32 and got["score"].dtype == np.float32 and got["w_pair"].dtype == np.float64
    # the same poses read as nanometres
    nm = scores_def(c["xyz_R"] / 16, c["xyz_L"] / 16, c["res_R"], c["res_L"], c["rotations"], c["translations"] / 16, c["p_R"], c["p_L"], 5.0, 3.0, 16.0)
    assert all(np.array_equal(nm[k], got[k]) for k in got)
    # the placement itself: a quarter turn and a shift, exact
    y = place_def(c["xyz_L"], c["rotations"], c["translations"])
    assert y.dtype == np.float32 and y[2, 0].tolist() == [-4, 3, 0] and y[1, 1].tolist() == [0, 0, 3 - 1 / 256] and y[3, 3].tolist() == [1040, 0, 0]


def tiny_slides():
    """three one-pose systems with rho = 2 (r_touch = 2, scale = 1), the ligand withdrawn along +x: (xyz_R, xyz_L, s, pair)"""
    head_on = (np.zeros((1, 3), np.float32), np.array([[10, 0, 0]], np.float32), -8.0, [0, 0])                      # s = rho - gap = 2 - 10
    sideways = (np.zeros((1, 3), np.float32), np.array([[10, 3, 0]], np.float32), np.nan, [-1, -1])                 # 3 > rho: a miss
    lattice = (np.array([[0, 0, 0], [0, 4, 0]], np.float32), np.array([[10, 4, 0], [10, 0, 0]], np.float32), -8.0, [0, 1])   # (0, 1) and (1, 0) tie
    return head_on, sideways, lattice


def test_hand_worked_slides():
    eye, o, u = np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32), np.array([[1, 0, 0]], np.float32)
    for xR, xL, want, pair in tiny_slides():
        s, t, p = slide_def(xR, xL, eye, o, u, r_touch=2.0, scale=1.0)
        assert p.tolist() == [pair] and s.dtype == np.float64 and t.dtype == np.float32 and p.dtype == np.int32
        if np.isnan(want):
            assert np.isnan(s[0]) and np.isnan(t).all()
        else:
            assert s[0] == want and t.tolist() == [[want, 0, 0]]
    # an origin shifted along the direction (poses_about: the ligand's atom put on (11.5, 0, 0)) moves s by as much and the contact pose
    # not at all
    from pesto_amd import poses as P
    shifted = P.poses_about(eye, [10, 0, 0], [11.5, 0, 0])
    assert shifted.tolist() == [[1.5, 0, 0]]
    s, t, p = slide_def(*tiny_slides()[0][:2], eye, shifted, u, r_touch=2.0, scale=1.0)
    assert s[0] == -9.5 and t.tolist() == [[-8, 0, 0]] and p.tolist() == [[0, 0]]


# ------------------------------------------------------------------ the host helpers
@pytest.mark.parametrize("n", [1, 2, 512])
def test_rotation_set(n):
    from pesto_amd import poses as P
    R = P.rotation_set(n)
    assert R.dtype == np.float32 and R.shape == (n, 3, 3) and np.array_equal(R, P.rotation_set(n))
    R64 = R.astype(np.float64)
    assert np.abs(np.swapaxes(R64, 1, 2) @ R64 - np.eye(3)).max() <= 4 * EPS32 and (np.linalg.det(R64) > 0).all()
    if n == 512:                                        # distinct, and spread: no two rotations closer than 15 degrees
        tr = np.einsum("aij,bij->ab", R64, R64)
        ang = np.degrees(np.arccos(np.clip((tr - 1) / 2, -1, 1)))
        np.fill_diagonal(ang, 180.0)
        assert ang.min() > 15.0
    # poses_about: the centre lands on the position, to float32 rounding
    rng = np.random.default_rng(n)
    c, pos = rng.normal(size=3) * 3, rng.normal(size=(n, 3)) * 5
    t = P.poses_about(R, c, pos)
    assert t.dtype == np.float32 and t.shape == (n, 3)
    landed = R64 @ c + t.astype(np.float64)
    assert np.abs(landed - pos).max() <= EPS32 * (np.abs(pos).max() + np.abs(c).sum() * 2)
    assert np.array_equal(P.poses_about(R, c, pos[0])[0], t[0])


def test_top_def():
    nan = np.nan
    score = np.array([0.5, nan, 0.75, 0.5, -1.0, 0.75, nan, 0.0, -0.0, 0.5], np.float32)
    assert top_def(score, 100).tolist() == [2, 5, 0, 3, 9, 7, 8, 4]                     # duplicates by index, NaN left out, k above the count
    assert top_def(score, 0).tolist() == [] and top_def(score, 3).tolist() == [2, 5, 0] and top_def(score, 3).dtype == np.int32
    clash = np.array([0, 0, 3, 1, 0, 0, 0, 2, 0, 0], np.int32)
    assert top_def(score, 100, clash).tolist() == [5, 0, 9, 8, 4]
    assert top_def(score, 100, clash, max_clash=2).tolist() == [5, 0, 3, 9, 7, 8, 4]
    assert top_def(score, 2, clash, max_clash=-1).tolist() == []
    # the arguments top_def takes are those top_poses checks before any launch
    from pesto_amd import poses as P
    for k, kw in ((-1, {}), (2.5, {}), (2, dict(n_clash=clash[:9])), (2, dict(n_clash=clash, max_clash=2 ** 31))):
        with pytest.raises(ValueError):
            P.top_poses(score, k, model=object(), **kw)


# ------------------------------------------------------------------ the seeded sweep systems
# (F poses, N_R, N_L atoms, R_R, R_L residues): every F of {1, 2, 65, 257}, every N_R and every N_L of {1, 63, 64, 65, 255, 256, 257} and
# every residue count of {1, 31, 32, 33, 65} on each side; the cases with F >= 65 keep both bodies at 63 atoms or more
SWEEP = [(1, 1, 257, 1, 65), (2, 63, 64, 31, 32), (65, 64, 255, 32, 33), (257, 255, 256, 33, 31), (65, 256, 63, 65, 1), (65, 257, 65, 1, 33),
         (2, 65, 1, 33, 1)]


def residue_rows(N, R, rng):
    """int32 [N]: dense rows 0 .. R - 1, not contiguous; where N allows, one residue of 70 atoms and one of a single atom"""
    sizes = np.ones(R, np.int64)
    spare = N - R
    if R > 1 and spare >= 69:
        sizes[0] += 69
        spare -= 69
        extra = rng.multinomial(spare, np.ones(R - 2) / (R - 2)) if R > 2 else np.array([], np.int64)
        sizes[2:] += extra
        sizes[0] += spare - int(extra.sum())
    else:
        sizes += rng.multinomial(spare, np.ones(R) / R)
    return rng.permutation(np.repeat(np.arange(R), sizes)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def sweep_system(F, N_R, N_L, R_R, R_L, seed=0):
    """a seeded system in nanometres (scale 10): two random bodies at protein-like density, and F poses - rotations of rotation_set, the
    ligand's centre led from the receptor's centre outwards (deep overlap to out of reach); with F >= 65 the last poses put the ligand's
    centre on the centre of each face of the receptor's box, then far outside it. Also origins / directions for the slide."""
    from pesto_amd.poses import poses_about, rotation_set
    rng = np.random.default_rng([seed, F, N_R, N_L, R_R, R_L])
    side = lambda n: max((n / 60.0) ** (1.0 / 3.0), 0.6)
    xyz_R = ((rng.random((N_R, 3)) - 0.5) * side(N_R) + np.array([3.0, -2.0, 1.0])).astype(np.float32)
    xyz_L = ((rng.random((N_L, 3)) - 0.5) * side(N_L) + np.array([-1.0, 0.5, 4.0])).astype(np.float32)
    lo, hi = xyz_R.astype(np.float64).min(0), xyz_R.astype(np.float64).max(0)
    mid, c_L = (lo + hi) / 2, xyz_L.astype(np.float64).mean(0)
    reach = (side(N_R) + side(N_L)) * 0.9 + 0.5
    w = rng.normal(size=(F, 3))
    pos = mid + w / np.linalg.norm(w, axis=1)[:, None] * (np.arange(F) / max(F - 1, 1) * reach)[:, None]
    if F >= 65:
        for a in range(3):
            for k, end in enumerate((lo, hi)):
                pos[F - 8 + 2 * a + k] = mid
                pos[F - 8 + 2 * a + k, a] = end[a]
        pos[F - 2] = mid + np.array([100.0, 0.0, 0.0])
        pos[F - 1] = mid - np.array([0.0, side(N_R) + side(N_L) + 1.0, 0.0])
    rot = rotation_set(F)
    d = rng.normal(size=(F, 3))
    return dict(xyz_R=xyz_R, xyz_L=xyz_L, res_R=residue_rows(N_R, R_R, rng), res_L=residue_rows(N_L, R_L, rng), rotations=rot,
                translations=poses_about(rot, c_L, pos), p_R=(rng.random(R_R) * (rng.random(R_R) > 0.2)).astype(np.float32),
                p_L=(rng.random(R_L) * (rng.random(R_L) > 0.2)).astype(np.float32),
                directions=(d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32))


def sweep_args(s):
    return (s["xyz_R"], s["xyz_L"], s["res_R"], s["res_L"], s["rotations"], s["translations"], s["p_R"], s["p_L"])


@functools.lru_cache(maxsize=None)
def sweep_definition(*case):
    return scores_def(*sweep_args(sweep_system(*case)))


@functools.lru_cache(maxsize=None)
def sweep_slide(*case):
    s = sweep_system(*case)
    return slide_def(s["xyz_R"], s["xyz_L"], s["rotations"], s["translations"], s["directions"])


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "F%d-NR%d-NL%d-RR%d-RL%d" % c)
def test_the_sweep_cannot_pass_vacuously(case):
    F, N_R, N_L, R_R, R_L = case
    s, d = sweep_system(*case), sweep_definition(*case)
    assert s["xyz_R"].shape == (N_R, 3) and s["xyz_L"].shape == (N_L, 3) and s["rotations"].shape == (F, 3, 3) and s["translations"].shape == (F, 3)
    for res, N, R in ((s["res_R"], N_R, R_R), (s["res_L"], N_L, R_L)):
        cnt = np.bincount(res, minlength=R)
        assert cnt.size == R and cnt.min() >= 1
        if R > 1 and N - R >= 69:
            assert cnt.max() >= 70 and cnt.min() == 1 and np.any(np.diff(res) < 0)
    assert d["masks"].shape == (F, -(-R_R // 32) + -(-R_L // 32))
    assert np.array_equal(np.array([[bin(int(w)).count("1") for w in row] for row in d["masks"]]).sum(1), d["n_res_R"] + d["n_res_L"])
    if F < 65:
        return
    assert np.unique(d["n_contact"]).size > 20 and d["n_contact"].min() == 0 and d["n_clash"].max() > 0 and d["n_pairs"].max() > 1
    y = place_def(s["xyz_L"], s["rotations"], s["translations"])
    lo, hi = s["xyz_R"].min(0), s["xyz_R"].max(0)
    inside = ((y >= lo) & (y <= hi)).all(2)                                # [F, N_L]: the placed atom lies in the receptor's box
    assert (~inside).all(1).any()                                          # a pose wholly outside the box
    for a in range(3):                                                     # a pose with atoms on both sides of each of the six faces
        assert ((y[..., a] < lo[a]).any(1) & (y[..., a] > lo[a]).any(1) & inside.any(1)).any()
        assert ((y[..., a] > hi[a]).any(1) & (y[..., a] < hi[a]).any(1) & inside.any(1)).any()
    sl = sweep_slide(*case)[0]
    assert np.isnan(sl).any() and (~np.isnan(sl)).sum() > F // 4


# ------------------------------------------------------------------ the host side of pesto_amd.poses
def test_arguments_raise_before_any_launch():
    from pesto_amd import poses as P
    m = object()                # no handle: the checks must come first
    c = tiny()
    F = 5
    base = dict(xyz_R=c["xyz_R"], xyz_L=c["xyz_L"], res_R=c["res_R"], res_L=c["res_L"], rotations=c["rotations"], translations=c["translations"],
                p_R=c["p_R"], p_L=c["p_L"], scale=1.0, model=m)
    bad_rot, bad_t = c["rotations"].copy(), c["translations"].copy()
    bad_rot[3, 1, 2], bad_t[0, 0] = np.inf, np.nan
    for kw in (dict(xyz_R=c["xyz_R"][:, :2]), dict(xyz_L=np.zeros((0, 3), np.float32)), dict(xyz_R=np.zeros((2, 3, 3), np.float32)),
               dict(res_R=c["res_R"][:2]), dict(res_R=c["res_R"] * 1.0), dict(res_R=-c["res_R"]), dict(res_R=c["res_R"] * 2), dict(res_L=c["res_L"] + 1),
               dict(rotations=c["rotations"][:, :2]), dict(rotations=bad_rot), dict(translations=bad_t), dict(translations=c["translations"][:4]),
               dict(p_R=c["p_R"][:1]), dict(p_L=[0.5, -0.25]), dict(p_L=[0.5, np.nan]), dict(p_R=[np.inf, 0.0]), dict(r_contact=np.nan),
               dict(r_clash=np.inf), dict(r_clash=6.0), dict(r_clash=-1.0), dict(scale=0.0), dict(scale=-1.0), dict(scale=np.nan)):
        with pytest.raises(ValueError):
            P.pose_scores(**dict(base, **kw))
    many = np.arange(P.MAX_RESIDUES + 1, dtype=np.int32)
    with pytest.raises(ValueError, match="residues"):
        P.pose_scores(**dict(base, xyz_R=np.zeros((many.size, 3), np.float32), res_R=many, p_R=np.zeros(many.size, np.float32)))
    wide = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2 ** 16, 3), (0, 0))                # shapes alone decide these
    with pytest.raises(ValueError, match="atom pairs"):
        P.pose_scores(**dict(base, xyz_R=wide, xyz_L=wide))
    long_rot = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2 ** 23 + 1, 3, 3), (0, 0, 0))
    with pytest.raises(ValueError, match="poses"):
        P.pose_scores(**dict(base, rotations=long_rot))
    u = np.tile(np.array([1, 0, 0], np.float32), (F, 1))
    slide = dict(xyz_R=c["xyz_R"], xyz_L=c["xyz_L"], rotations=c["rotations"], origins=c["translations"], directions=u, scale=1.0, model=m)
    for kw in (dict(directions=u * np.float32(1.001)), dict(directions=u * 0), dict(directions=u[:4]), dict(origins=bad_t), dict(rotations=bad_rot),
               dict(directions=np.where(np.arange(F)[:, None] == 2, np.nan, u).astype(np.float32)), dict(r_touch=np.nan), dict(r_touch=-1.0),
               dict(scale=0.0), dict(xyz_R=wide, xyz_L=wide), dict(xyz_L=c["xyz_L"][:, :2])):
        with pytest.raises(ValueError):
            P.slide_to_contact(**dict(slide, **kw))
    for kw in (dict(rotations=bad_rot), dict(translations=bad_t), dict(translations=c["translations"][:2]), dict(xyz_L=c["xyz_L"].T),
               dict(xyz_R=c["xyz_R"][:, :1]), dict(rotations=long_rot)):
        with pytest.raises(ValueError):
            P.materialize(**dict(dict(xyz_L=c["xyz_L"], rotations=c["rotations"], translations=c["translations"], xyz_R=c["xyz_R"], model=m), **kw))
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2 ** 20, 3, 3), (0, 0, 0))
    with pytest.raises(ValueError, match="batches"):
        P.materialize(wide, big, np.zeros((2 ** 20, 3), np.float32), model=m)
    score = np.zeros(4, np.float32)
    for a, kw in (((score, -1), {}), ((score, 1.5), {}), ((score[:0], 1), {}), ((score[None], 1), {}), ((score, 1), dict(n_clash=np.zeros(3, np.int32))),
                  ((score, 1), dict(n_clash=np.zeros(4, np.int32), max_clash=2 ** 31)), ((np.zeros(2 ** 23 + 1, np.float32), 1), {})):
        with pytest.raises(ValueError):
            P.top_poses(*a, model=m, **kw)
    for n in (0, -3, 1.5):
        with pytest.raises(ValueError):
            P.rotation_set(n)
    with pytest.raises(ValueError):
        P.poses_about(c["rotations"], [0, 0], [0, 0, 0])
    with pytest.raises(ValueError):
        P.poses_about(c["rotations"], [0, 0, 0], np.zeros((4, 3)))
    # guided_dock: a weighted centre that is undefined, and one that is the centroid itself
    dock = dict(xyz_R=c["xyz_R"], xyz_L=c["xyz_L"], res_R=c["res_R"], res_L=c["res_L"], p_R=c["p_R"], p_L=c["p_L"], n_rot=16, scale=1.0, model=m)
    with pytest.raises(ValueError, match="sum of p is 0"):
        P.guided_dock(**dict(dock, p_R=[0.0, 0.0]))
    with pytest.raises(ValueError, match="sum of p is 0"):
        P.guided_dock(**dict(dock, p_L=[0.0, 0.0]))
    square = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0]], np.float32)                          # two residues with one centroid
    with pytest.raises(ValueError, match="equals the centroid"):
        P.guided_dock(**dict(dock, xyz_L=square, res_L=np.array([0, 1, 1, 0], np.int32), p_L=[0.5, 0.25]))
    with pytest.raises(ValueError):
        P.guided_dock(**dict(dock, cone=0.0))
    with pytest.raises(ValueError):
        P.guided_dock(**dict(dock, p_R=[0.5]))


def test_the_cone_filter_keeps_what_it_says():
    from pesto_amd import poses as P
    axis, u = np.array([0.3, -1.0, 0.2]), np.array([0.0, 0.6, 0.8])
    rots, keep = P.cone_filter(512, axis, u, 60.0)
    assert rots.dtype == np.float32 and np.array_equal(rots, P.rotation_set(512)[keep]) and 0 < keep.size < 512
    v = P.rotation_set(512).astype(np.float64) @ axis
    ang = np.degrees(np.arccos(np.clip(-(v @ u) / np.linalg.norm(v, axis=1), -1, 1)))
    assert (ang[keep] <= 60.0 + 1e-9).all() and (np.delete(ang, keep) >= 60.0 - 1e-9).all()
    assert abs(keep.size / 512 - 0.25) < 0.05                              # a cone of 60 degrees holds a quarter of the sphere
    assert P.cone_filter(512, axis, u, 180.0)[1].size == 512


def test_new_symbols_are_declared_exported_and_bound():
    from pesto_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    new = ["pesto_poses_last_error", "pesto_poses_scores", "pesto_poses_slide", "pesto_poses_materialize", "pesto_poses_top"]
    lib = _lib.load()
    for name in new:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.pesto_poses_last_error.restype is not None
    import pesto_amd
    from pesto_amd import poses
    assert int(re.search(r"PESTO_POSES_MAX_FRAMES = 1 << (\d+)", hdr).group(1)) == 23 and poses.MAX_FRAMES == 2 ** 23
    assert int(re.search(r"PESTO_POSES_MAX_RESIDUES = (\d+)", hdr).group(1)) == poses.MAX_RESIDUES >= 4096
    assert int(re.search(r"PESTO_POSES_MAX_PAIRS = (0x[0-9a-f]+)", hdr).group(1), 16) == poses.MAX_PAIRS == 2 ** 31 - 1
    assert int(re.search(r"PESTO_POSES_MAX_PLACED = (0x[0-9a-f]+)", hdr).group(1), 16) == poses.MAX_PLACED
    assert pesto_amd.poses is poses
    for name in ("pose_scores", "slide_to_contact", "materialize", "top_poses", "rotation_set", "poses_about", "guided_dock", "PoseScores"):
        assert getattr(pesto_amd, name) is getattr(poses, name) and name in pesto_amd.__all__, name
    src = open(os.path.join(ROOT, "pesto_amd", "csrc", "build.py")).read()
    assert '"pesto_poses.hip"' in src
    for header in ("pesto_call.h", "pesto_cellgrid.h"):                 # the shared headers name their users
        assert "poses" in open(os.path.join(ROOT, "pesto_amd", "csrc", header)).read().split("#pragma once")[0], header
