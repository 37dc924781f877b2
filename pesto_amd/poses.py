"""Rigid poses of a ligand on a receptor on the GPU: the step between the interface prediction and the scoring of finished complexes.

The package predicts interfaces (Model, patches, peaks) and judges complexes (docking, dockq, lddt, tmscore, qsscore); those take
materialised frames [F, N, 3]. Here a pose is a transform, nothing is materialised unless asked for, and the poses are ranked by how well
they agree with the two predicted interfaces (pesto_poses.hip):
    pose_scores          per pose: contacts, clashes, the posed interfaces, their residue pairs, probability sums and a soft Dice score
    slide_to_contact     per pose: push the ligand along a direction until it first touches the receptor
    materialize          the placed frames [F, N, 3], the bridge to dockq.dockq, lddt and tm_score
    top_poses            the best k eligible poses by score
    rotation_set         n rotations that cover SO(3) evenly (host)
    poses_about          the translations that turn the ligand about a centre and put that centre on given positions (host)
    guided_dock          everything in a row: poses sampled around the predicted patches, slid to contact, scored and ranked
The lead coordinate argument decides where a call runs (_lib.Side): NumPy in, NumPy out; ROCm tensors in, ROCm tensors out on torch's
current stream. ``model`` lends its device handle; without one a weightless handle is used. There is no CPU or PyTorch fallback. Arguments
are checked on the host before any launch (ValueError).

Definitions. They are this package's own. Units and distance are docking.py's, so results feed dockq directly: scale (default 10.0) and
the thresholds are rounded to float32, d = fl32(sqrt_rn((dx*dx + dy*dy) + dz*dz)) * fl32(scale), and a NaN distance passes no test.
    pose f         (R_f float32 [3, 3] row-major, t_f float32 [3]), both finite (ValueError otherwise). R_f is NOT required to be
                   orthonormal: any finite matrix is applied as it is.
    placement      ligand atom x has in pose f the coordinates y_a = ((R[a,0]*x_0 + R[a,1]*x_1) + R[a,2]*x_2) + t_a, in float32, every
                   operation rounded as written, no contraction. Every function sees the ligand through this placement and nothing else.
    residues       res_R [N_R], res_L [N_L]: dense residue rows 0 .. R - 1, every row holding an atom; p_R [R_R], p_L [R_L]: float32,
                   finite and >= 0, the predicted interface probability of every residue.
pose_scores, per pose: n_contact / n_clash are the atom pairs (receptor atom, placed ligand atom) with d < r_contact / d < r_clash;
I_R and I_L the residues of either side with a contact pair (n_res_R, n_res_L), C the distinct residue pairs (r, s) with one (n_pairs);
w_R = sum over I_R of p_R[r], w_L likewise, w_pair = sum over C of double(p_R[r]) * double(p_L[s]), in double in a fixed order that
depends on the pose's sets alone; score = float32((dice_R + dice_L) / 2) with dice_R = 2 w_R / (n_res_R + P_R), P_R = sum of p_R in
double, 0 where the denominator is 0: the soft Dice overlap of the predicted and the posed interface.
slide_to_contact, per pose, with t = origin_f and the direction u_f used as given (| |u|^2 - 1 | <= 1e-3 in double, else ValueError),
in double, every operation rounded as written, over every atom pair (i of the receptor, j of the ligand):
    w = double(y_j) - double(x_i);  b = (w0*u0 + w1*u1) + w2*u2;  c = ((w0*w0 + w1*w1) + w2*w2) - b*b
    rho = double(fl32(r_touch)) / double(fl32(scale));  disc = rho*rho - c;  a pair counts where disc > 0;  s_ij = -b + sqrt(disc)
s[f] is the maximum of s_ij (the ligand, withdrawn along +u and pushed back, first touches the receptor there), pair[f] the (i, j) that
attains it (the smallest (i, then j) among ties), translations[f] = fl32(double(origin) + s * u) per component; where no pair counts (the
ray misses; a non-finite w counts for nothing) s and the translation are NaN and the pair is (-1, -1).
Every output is bit-identical from call to call, between host and device inputs, and for a pose alone or inside a batch.

Limits: F <= MAX_FRAMES = 2**23 poses, N_R * N_L < 2**31, at most MAX_RESIDUES = 4096 residues a side, F * (N_R + N_L) < 2**31 atoms
out of materialize. Every excess raises ValueError before any launch.
"""
import ctypes
from collections import namedtuple

import numpy as np

from . import _lib
from .docking import _cutoff, _residue_rows
from .trajectory import _model_of, _residue_order

MAX_FRAMES = 2 ** 23            # PESTO_POSES_MAX_FRAMES
MAX_RESIDUES = 4096             # PESTO_POSES_MAX_RESIDUES
MAX_PAIRS = 2 ** 31 - 1         # PESTO_POSES_MAX_PAIRS: N_R * N_L
MAX_PLACED = 2 ** 31 - 1        # PESTO_POSES_MAX_PLACED: F * (N_R + N_L) of materialize

PoseScores = namedtuple("PoseScores", "n_contact n_clash n_res_R n_res_L n_pairs w_R w_L w_pair score masks", defaults=(None,))
GuidedDock = namedtuple("GuidedDock", "rotations translations scores index n_sampled")


def _body(x, name):
    """the one conformation [N, 3] of a coordinate argument ([1, N, 3] is taken as [N, 3]), on its own side"""
    a = getattr(x, "xyz", x)
    if not (_lib.is_torch(a) or isinstance(a, np.ndarray)):
        a = np.asarray(a, np.float32)
    if len(a.shape) == 3 and int(a.shape[0]) == 1:
        a = a[0]
    if len(a.shape) != 2 or int(a.shape[1]) != 3 or int(a.shape[0]) < 1:
        raise ValueError(f"{name} must be [N >= 1, 3] (or [1, N, 3]), got {list(a.shape)}")
    return a


def _vectors(v, F, name):
    """v [F, 3] (F None: any F >= 1), finite; returns (v on its side, host float32 copy)"""
    h = _lib.host(v)
    if h.ndim != 2 or h.shape[1] != 3 or h.shape[0] < 1 or (F is not None and h.shape[0] != F):
        raise ValueError(f"{name} must be [{'F' if F is None else F}, 3], got {list(h.shape)}")
    h = h.astype(np.float32)
    if not np.isfinite(h).all():
        raise ValueError(f"{name} must be finite")
    return (v if _lib.is_torch(v) else h), h


def _rotations(rotations):
    """rotations [F, 3, 3] finite; returns (rotations on their side, F)"""
    h = _lib.host(rotations)
    if h.ndim != 3 or tuple(h.shape[1:]) != (3, 3) or h.shape[0] < 1:
        raise ValueError(f"rotations must be [F >= 1, 3, 3], got {list(h.shape)}")
    if h.shape[0] > MAX_FRAMES:
        raise ValueError(f"at most 2**23 poses, got {h.shape[0]}")
    if not np.isfinite(h.astype(np.float32)).all():
        raise ValueError("rotations must be finite")
    return (rotations if _lib.is_torch(rotations) else h.astype(np.float32)), int(h.shape[0])


def _pair_limit(N_R, N_L):
    if N_R * N_L > MAX_PAIRS:
        raise ValueError(f"too many atom pairs per pose: N_R * N_L = {N_R} * {N_L} must stay below 2**31")


def _probabilities(p, R, name):
    h = _lib.host(p).reshape(-1)
    if h.size != R:
        raise ValueError(f"{name} must hold one probability per residue, {R}, got {h.size}")
    h = h.astype(np.float32)
    if not (np.isfinite(h).all() and (h >= 0).all()):
        raise ValueError(f"{name} must be finite and >= 0")
    return h


def pose_scores(xyz_R, xyz_L, res_R, res_L, rotations, translations, p_R, p_L, r_contact=5.0, r_clash=3.0, scale=10.0, masks=False, model=None):
    """PoseScores(n_contact, n_clash, n_res_R, n_res_L, n_pairs int32 [F], w_R, w_L, w_pair float64 [F], score float32 [F], masks) of the
    F poses (rotations [F, 3, 3], translations [F, 3]) of the ligand xyz_L [N_L, 3] on the receptor xyz_R [N_R, 3]: see the module's
    definition. 0 <= r_clash <= r_contact. masks=True also gives masks uint32 [F, ceil(R_R / 32) + ceil(R_L / 32)]: bit r % 32 of word
    r // 32 is set for r in I_R(f), and the ligand's words follow the receptor's (None otherwise). One cell grid over the receptor per
    call and one launch over the poses; no frame and no pair list is written."""
    xR, xL = _body(xyz_R, "xyz_R"), _body(xyz_L, "xyz_L")
    N_R, N_L = int(xR.shape[0]), int(xL.shape[0])
    _pair_limit(N_R, N_L)
    rR, R_R = _residue_rows(res_R, N_R, "res_R")
    perm, off, R_L = _residue_order(res_L, N_L, "res_L")
    if R_R > MAX_RESIDUES or R_L > MAX_RESIDUES:
        raise ValueError(f"at most {MAX_RESIDUES} residues a side, got {R_R} and {R_L}")
    rot, F = _rotations(rotations)
    tr, _ = _vectors(translations, F, "translations")
    pR, pL = _probabilities(p_R, R_R, "p_R"), _probabilities(p_L, R_L, "p_L")
    thr, sc = _cutoff(r_contact, scale)
    clash, _ = _cutoff(r_clash, scale)
    if not 0 <= np.float32(clash) <= np.float32(thr) or not np.isfinite(np.float32(thr) / np.float32(sc)):
        raise ValueError(f"0 <= r_clash <= r_contact expected, got {r_clash!r} and {r_contact!r}")
    model = _model_of(model, xR)
    h = model.handle
    side = _lib.Side(xR, model._gpu)
    xr, xl = side.put(xR, np.float32), side.put(xL, np.float32)
    rd, pm, of = side.put(rR, np.int32), side.put(perm, np.int32), side.put(off, np.int32)
    ro, td = side.put(rot, np.float32), side.put(tr, np.float32)
    prd, pld = side.put(pR, np.float32), side.put(pL, np.float32)
    counts = [side.empty((F,), np.int32) for _ in range(5)]
    sums = [side.empty((F,), np.float64) for _ in range(3)]
    score = side.empty((F,), np.float32)
    mk = side.empty((F, -(-R_R // 32) + -(-R_L // 32)), np.uint32) if masks else None
    lib = _lib.load()
    _lib.check(lib.pesto_poses_scores(h, F, N_R, N_L, R_R, R_L, side.ptr(xr), side.ptr(xl), side.ptr(rd), side.ptr(pm), side.ptr(of), side.ptr(ro),
                                      side.ptr(td), side.ptr(prd), side.ptr(pld), thr, clash, sc, *(side.ptr(v) for v in counts),
                                      *(side.ptr(v) for v in sums), side.ptr(score), side.ptr(mk), side.kind, side.stream),
               lib.pesto_poses_last_error)
    return PoseScores(*counts, *sums, score, mk)


def slide_to_contact(xyz_R, xyz_L, rotations, origins, directions, r_touch=3.5, scale=10.0, model=None):
    """(s float64 [F], translations float32 [F, 3], pair int32 [F, 2]): the ligand placed with t = origins[f], withdrawn along
    +directions[f] and pushed back until its first atom comes within r_touch of a receptor atom - see the module's definition. A pose
    whose ray misses the receptor has s = NaN, a NaN translation and the pair (-1, -1). All atom pairs of every pose, one launch."""
    xR, xL = _body(xyz_R, "xyz_R"), _body(xyz_L, "xyz_L")
    N_R, N_L = int(xR.shape[0]), int(xL.shape[0])
    _pair_limit(N_R, N_L)
    rot, F = _rotations(rotations)
    org, _ = _vectors(origins, F, "origins")
    dirs, u = _vectors(directions, F, "directions")
    u = u.astype(np.float64)
    if not (np.abs(((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]) - 1.0) <= 1e-3).all():
        raise ValueError("directions must have unit length: | |u|^2 - 1 | <= 1e-3")
    thr, sc = _cutoff(r_touch, scale)
    if not thr >= 0:
        raise ValueError(f"r_touch must be >= 0, got {r_touch!r}")
    model = _model_of(model, xR)
    h = model.handle
    side = _lib.Side(xR, model._gpu)
    xr, xl = side.put(xR, np.float32), side.put(xL, np.float32)
    ro, od, dd = side.put(rot, np.float32), side.put(org, np.float32), side.put(dirs, np.float32)
    s, t, pair = side.empty((F,), np.float64), side.empty((F, 3), np.float32), side.empty((F, 2), np.int32)
    lib = _lib.load()
    _lib.check(lib.pesto_poses_slide(h, F, N_R, N_L, side.ptr(xr), side.ptr(xl), side.ptr(ro), side.ptr(od), side.ptr(dd), thr, sc, side.ptr(s),
                                     side.ptr(t), side.ptr(pair), side.kind, side.stream), lib.pesto_poses_last_error)
    return s, t, pair


def materialize(xyz_L, rotations, translations, xyz_R=None, model=None):
    """float32 [F, N_L, 3]: the ligand in every pose, the placement bit for bit. With xyz_R [N_R, 3] the result is [F, N_R + N_L, 3], the
    receptor's rows first (copied): the frames dockq.dockq, lddt and tm_score take."""
    xL = _body(xyz_L, "xyz_L")
    N_L, N_R = int(xL.shape[0]), 0
    xR = None
    if xyz_R is not None:
        xR = _body(xyz_R, "xyz_R")
        N_R = int(xR.shape[0])
    rot, F = _rotations(rotations)
    tr, _ = _vectors(translations, F, "translations")
    if F * (N_R + N_L) > MAX_PLACED:
        raise ValueError(f"too many atoms to write: F * (N_R + N_L) = {F} * {N_R + N_L} must stay below 2**31, pass the poses in batches")
    model = _model_of(model, xL)
    h = model.handle
    side = _lib.Side(xL, model._gpu)
    xl, xr = side.put(xL, np.float32), None if xR is None else side.put(xR, np.float32)
    ro, td = side.put(rot, np.float32), side.put(tr, np.float32)
    out = side.empty((F, N_R + N_L, 3), np.float32)
    lib = _lib.load()
    _lib.check(lib.pesto_poses_materialize(h, F, N_R, N_L, side.ptr(xr), side.ptr(xl), side.ptr(ro), side.ptr(td), side.ptr(out), side.kind,
                                           side.stream), lib.pesto_poses_last_error)
    return out


def top_poses(score, k, n_clash=None, max_clash=0, model=None):
    """int32 [min(k, eligible)]: the indices of the best poses. Eligible are the poses whose score [F] is not a NaN and, if n_clash [F] is
    given, has n_clash <= max_clash; they come by score descending (-0.0 equals 0.0), ties by index ascending. k >= 0. One radix sort
    of 64-bit keys on the device; nothing is sorted on the host."""
    if not _lib.is_torch(score):
        score = np.asarray(score)
    if n_clash is not None and not _lib.is_torch(n_clash):
        n_clash = np.asarray(n_clash)
    if len(score.shape) != 1 or int(score.shape[0]) < 1:
        raise ValueError(f"score must be [F >= 1], got {list(score.shape)}")
    F = int(score.shape[0])
    if F > MAX_FRAMES:
        raise ValueError(f"at most 2**23 poses, got {F}")
    if int(k) != k or k < 0:
        raise ValueError(f"k must be an integer >= 0, got {k!r}")
    if n_clash is not None and tuple(n_clash.shape) != (F,):
        raise ValueError(f"n_clash must be [{F}], got {list(n_clash.shape)}")
    if int(max_clash) != max_clash or not -2 ** 31 <= max_clash < 2 ** 31:
        raise ValueError(f"max_clash must be an int32, got {max_clash!r}")
    model = _model_of(model, score)
    h = model.handle
    side = _lib.Side(score, model._gpu)
    sd = side.put(score, np.float32)
    cd = None if n_clash is None else side.put(n_clash, np.int32)
    cap = min(int(k), F)
    index = side.empty((cap,), np.int32)
    n = ctypes.c_int64(0)
    lib = _lib.load()
    _lib.check(lib.pesto_poses_top(h, F, int(k), side.ptr(sd), side.ptr(cd), int(max_clash), side.ptr(index) if cap else None, ctypes.byref(n),
                                   side.kind, side.stream), lib.pesto_poses_last_error)
    return index[:int(n.value)]


# ------------------------------------------------------------------ host helpers (NumPy float64, rounded once to float32, no launch)
_PSI = 1.533751168755204288118041


def rotation_set(n):
    """float32 [n, 3, 3]: n rotations that cover SO(3) evenly, deterministic, n >= 1 - the super-Fibonacci quaternion spiral (Alexa 2022):
    with s = i + 1/2, r = sqrt(s / n), R = sqrt(1 - s / n), alpha = 2 pi s / sqrt(2), beta = 2 pi s / 1.533751168755204288118041, the
    quaternion q = (x, y, z, w) = (r sin alpha, r cos alpha, R sin beta, R cos beta). Built in float64 and rounded once."""
    if int(n) != n or n < 1:
        raise ValueError(f"n must be an integer >= 1, got {n!r}")
    n = int(n)
    s = np.arange(n, dtype=np.float64) + 0.5
    r, R = np.sqrt(s / n), np.sqrt(1.0 - s / n)
    alpha, beta = 2.0 * np.pi * s / np.sqrt(2.0), 2.0 * np.pi * s / _PSI
    q = np.stack([r * np.sin(alpha), r * np.cos(alpha), R * np.sin(beta), R * np.cos(beta)], 1)
    q /= np.sqrt((q * q).sum(1))[:, None]
    x, y, z, w = q.T
    m = np.empty((n, 3, 3), np.float64)
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    return m.astype(np.float32)


def poses_about(rotations, center, positions):
    """float32 [F, 3]: the translations position - R center, so that the ligand turns about ``center`` [3] and ``center`` lands on
    ``positions`` ([3], or [F, 3]: one per rotation). In float64 from the float32 rotations, rounded once."""
    R = _lib.host(rotations).astype(np.float32).astype(np.float64)
    c, p = np.asarray(_lib.host(center), np.float64).reshape(-1), np.asarray(_lib.host(positions), np.float64)
    if R.ndim != 3 or R.shape[1:] != (3, 3) or c.size != 3 or p.shape not in ((3,), (R.shape[0], 3)):
        raise ValueError(f"rotations [F, 3, 3], center [3] and positions [3] or [F, 3] expected, got {list(R.shape)}, {list(c.shape)}, {list(p.shape)}")
    t = np.broadcast_to(p, (R.shape[0], 3)) - R @ c
    if not np.isfinite(t).all():
        raise ValueError("rotations, center and positions must be finite")
    return t.astype(np.float32)


def _centres(xyz, res, R, p, name):
    """(c_if, c) in float64: the p-weighted mean of the residue centroids, and the plain centroid of the atoms"""
    x = xyz.astype(np.float64)
    cnt = np.bincount(res, minlength=R).astype(np.float64)
    cen = np.stack([np.bincount(res, weights=x[:, a], minlength=R) for a in range(3)], 1) / cnt[:, None]
    P = float(p.astype(np.float64).sum())
    if not P > 0:
        raise ValueError(f"{name}: the weighted centre is undefined, sum of p is 0")
    c_if, c = (p.astype(np.float64)[:, None] * cen).sum(0) / P, x.mean(0)
    if not (np.isfinite(c_if).all() and np.isfinite(c).all()):
        raise ValueError(f"{name}: coordinates must be finite")
    if np.array_equal(c_if, c):
        raise ValueError(f"{name}: the weighted centre equals the centroid, there is no direction to the interface")
    return c_if, c


def cone_filter(n_rot, axis_L, u, cone):
    """(rotations float32 [n, 3, 3], their indices in rotation_set(n_rot)): the rotations R whose R axis_L lies within ``cone`` degrees of
    -u (float64 from the float32 rotations)"""
    rots = rotation_set(n_rot)
    v = rots.astype(np.float64) @ np.asarray(axis_L, np.float64)
    cos = -(v @ np.asarray(u, np.float64)) / np.sqrt((v * v).sum(1))
    keep = np.nonzero(cos >= np.cos(np.deg2rad(float(cone))))[0]
    return rots[keep], keep


def _rows(a, idx):
    """a[idx] on a's side (idx: host integers)"""
    if a is None:
        return None
    if _lib.is_torch(a):
        import torch
        return a[torch.from_numpy(np.asarray(idx, np.int64)).to(a.device)]
    return a[np.asarray(idx, np.int64)]


def guided_dock(xyz_R, xyz_L, res_R, res_L, p_R, p_L, n_rot=4096, cone=60.0, top=100, r_touch=3.5, r_contact=5.0, r_clash=3.0, scale=10.0,
                model=None):
    """GuidedDock(rotations [K, 3, 3], translations [K, 3], scores PoseScores of the K kept poses in rank order, index int32 [K] into the
    cone-filtered set, n_sampled): poses sampled around the two predicted patches.
        centres      c_if: the p-weighted mean of a side's residue centroids; c: the side's plain centroid (host NumPy, float64)
        approach     u = unit(c_if_R - c_R); the origin is c_if_R
        cone filter  of rotation_set(n_rot), the rotations whose R (c_if_L - c_L) lies within ``cone`` degrees of -u: n_sampled of them
        poses        poses_about(rotations, c_L, origin), then slide_to_contact along u (float32), then pose_scores of the poses that
                     touch, then top_poses(score, top, n_clash, max_clash=0)
    ValueError where a weighted centre is undefined (sum p = 0), where c_if == c on either side, where no rotation passes the cone or
    where no sampled pose touches the receptor."""
    xR, xL = _body(xyz_R, "xyz_R"), _body(xyz_L, "xyz_L")
    N_R, N_L = int(xR.shape[0]), int(xL.shape[0])
    rR, R_R = _residue_rows(res_R, N_R, "res_R")
    rL, R_L = _residue_rows(res_L, N_L, "res_L")
    pR, pL = _probabilities(p_R, R_R, "p_R"), _probabilities(p_L, R_L, "p_L")
    if not 0 < float(cone) <= 180:
        raise ValueError(f"cone must lie in (0, 180] degrees, got {cone!r}")
    cif_R, c_R = _centres(_lib.host(xR), rR, R_R, pR, "receptor")
    cif_L, c_L = _centres(_lib.host(xL), rL, R_L, pL, "ligand")
    u = cif_R - c_R
    u = u / np.sqrt((u * u).sum())
    rots, _ = cone_filter(n_rot, cif_L - c_L, u, cone)
    n_sampled = int(rots.shape[0])
    if n_sampled == 0:
        raise ValueError("no rotation passes the cone filter")
    origins = poses_about(rots, c_L, cif_R)
    dirs = np.tile(u.astype(np.float32), (n_sampled, 1))
    s, trans, _ = slide_to_contact(xR, xL, rots, origins, dirs, r_touch, scale, model)
    hits = np.nonzero(~np.isnan(_lib.host(s)))[0]
    if hits.size == 0:
        raise ValueError("no sampled pose touches the receptor")
    rot_h, trans_h = rots[hits], _rows(trans, hits)
    sc = pose_scores(xR, xL, rR, rL, rot_h, trans_h, pR, pL, r_contact, r_clash, scale, False, model)
    best = _lib.host(top_poses(sc.score, top, sc.n_clash, 0, model)).astype(np.int64)
    side = _lib.Side(xR, _model_of(model, xR)._gpu)
    index = side.put(hits[best].astype(np.int32), np.int32)
    return GuidedDock(side.put(rot_h[best], np.float32), _rows(trans_h, best), PoseScores(*(_rows(v, best) for v in sc)), index, n_sampled)
