"""Hydrogen bonds and periodic unwrapping on the GPU: the last two array functions of the reference's MD toolkit.

The reference (md_analysis/mdtraj_utils/trajectory_utils.py) calls ``md.baker_hubbard(traj[k], periodic=False)`` once per frame in a Python
loop and filters the triplets with ``np.isin`` (``hydrogen_bonds``), and loops over chains and their 27 periodic images in NumPy
(``unwrap_pbc``). Here every function is one launch sequence over all frames (pesto_hbonds.hip):
    frame_hbonds                         the bonded (donor, hydrogen, acceptor) triplets of every frame, with their H .. A distances
    baker_hubbard                        the triplets bonded in more than ``freq`` of the frames, with the number of frames
    hydrogen_bonds                       the reference's form: the bonds between two subunits, per frame
    unwrap_pbc                           every molecule shifted to its periodic image nearest to molecule 0
    atomic_masses / hbond_tables         the host-side tables: standard atomic weights, donor pairs and acceptors of a structure
Coordinates are float32 [F, N, 3] arrays, or [N, 3] where a single frame is meant. The lead argument decides where a call runs
(_lib.Side): ROCm tensors stay on the device (device pointers, torch's current stream, ROCm tensors out); NumPy arrays are staged and NumPy
arrays come back. ``model`` lends its device handle; without one a weightless handle is used. Arguments are checked before any launch
(ValueError). There is no CPU or PyTorch fallback.

Definitions. mdtraj is not part of this project's environment; what follows restates what md.baker_hubbard documents in this project's own
arithmetic, and can differ from mdtraj's float32 / acos evaluation only for decisions within rounding of a threshold.

Tables (topology, host side): ``dh`` int32 [P, 2], rows (donor atom, hydrogen atom); ``acc`` int32 [A], the acceptor atoms. The candidates
are all triplets (dh[p, 0], dh[p, 1], acc[a]) with acc[a] != dh[p, 0] (mdtraj filters out only this self pairing), in the order p
ascending, then a ascending (mdtraj's Cartesian-product order).

Distance. Between H and A, the float32 distance of the docking module, scale and r_thr rounded to float32:
    d = fl32(sqrt_rn((dx*dx + dy*dy) + dz*dz)) * fl32(scale)       every operation rounded as written, the root correctly rounded
tested as d < r_thr (defaults scale = 10 and r_thr = 2.5: mdtraj's 0.25 nm on nanometre input).

Angle. The D-H-A angle must exceed ``angle`` degrees (default 120; allowed [90, 180)). It is evaluated in double from the float32
coordinates, without acos or root: u = D - H, v = A - H,
    c = (ux*vx + uy*vy) + uz*vz,   uu and vv likewise,   k = cos(radians(angle))**2 (on the host, in double)
    bonded iff c < 0 and c*c > k * (uu*vv)                         every operation rounded as written
A NaN, uu = 0 and vv = 0 all fail the test.

Occupancy. n[p, a] is the number of frames in which the triplet is bonded; it is reported iff float(n) / float(F) > freq (strict; mdtraj's
default freq = 0.1; freq must not be negative).

unwrap_pbc. xyz float32 [F, N, 3]; unitcell_lengths float32 [F, 3]; mol int32 [N], dense molecule rows 0 .. M - 1 (not necessarily
contiguous, every row non-empty); masses float64 [N], positive and finite. com[f, m] is the mass-weighted mean in double. For every
molecule m >= 1 and frame f, the 27 image vectors dV[k] = (gx, gy, gz), g drawn from (0, 1, -1), are enumerated with y slowest, then x,
then z fastest (the reference's np.meshgrid(dgrid, dgrid, dgrid) with default indexing, ravelled); the distance is
|com[f, m] + L[f] * dV[k] - com[f, 0]| in double, sqrt((tx*tx + ty*ty) + tz*tz); the image is the first k of minimum distance; the shifted
coordinates are fl32(float64(x) + float64(L[f, c]) * dV[k][c]) for every atom of m. Molecule 0 is never moved. A NaN centre of mass (of m
or of molecule 0) or box length leaves that molecule's frame unshifted (a copy), with k = 0.

Every output is bit-identical from call to call and between host and device inputs.
"""
import math

import numpy as np

from . import _lib
from .docking import _frames, _sized
from .trajectory import F32_MAX, _model_of, _residue_order, _selection, _xyz

MAX_FRAMES = 2 ** 23            # PESTO_HBONDS_MAX_FRAMES
MAX_PAIRS = 2 ** 31 - 1         # PESTO_HBONDS_MAX_PAIRS: P * A
MAX_LIST = 2 ** 30 - 1          # PESTO_HBONDS_MAX_LIST: entries of one list
DONOR_TILE = 32                 # PESTO_HBONDS_DONOR_TILE: donor pairs of one workgroup

WATER = ("HOH", "DOD", "WAT", "H2O", "SOL", "TIP3", "TIP4")
# standard atomic weights (IUPAC 2021 abridged values; D: the deuterium isotope)
ATOMIC_WEIGHTS = {
    "H": 1.008, "D": 2.014, "HE": 4.0026, "LI": 6.94, "B": 10.81, "C": 12.011, "N": 14.007, "O": 15.999, "F": 18.998, "NA": 22.990,
    "MG": 24.305, "AL": 26.982, "SI": 28.085, "P": 30.974, "S": 32.06, "CL": 35.45, "K": 39.098, "CA": 40.078, "MN": 54.938, "FE": 55.845,
    "CO": 58.933, "NI": 58.693, "CU": 63.546, "ZN": 65.38, "SE": 78.971, "BR": 79.904, "I": 126.90,
}


def atomic_masses(elements):
    """float64 [N]: the standard atomic weight of every element symbol (any letter case, surrounding blanks ignored). An unknown element
    raises ValueError."""
    out = np.empty(len(elements), np.float64)
    for i, e in enumerate(elements):
        key = str(e).strip().upper()
        if key not in ATOMIC_WEIGHTS:
            raise ValueError(f"atomic_masses: no atomic weight for element {e!r} (atom {i})")
        out[i] = ATOMIC_WEIGHTS[key]
    return out


def hbond_tables(structure, exclude_water=True, max_bond=1.3):
    """(dh int32 [P, 2], acc int32 [A]) of a structure dict as structure_io.read_pdb returns it (before clean_structure, which drops the
    hydrogens). In the place of mdtraj's residue templates, a geometric rule: a hydrogen (element H or D) is bonded to the nearest
    non-hydrogen atom of its own residue (same chain, resid and icode) by float64 distance, ties to the lower index, and only when that
    distance is <= max_bond. Donor pairs are those whose heavy atom is N or O, ordered by (donor, hydrogen); acceptors are all N and O
    atoms, ascending. With exclude_water, residues named HOH, DOD, WAT, H2O, SOL, TIP3 or TIP4 are in neither table."""
    xyz = np.asarray(structure["xyz"], np.float64)
    n = xyz.shape[0]
    el = np.char.upper(np.char.strip(np.asarray(structure["element"]).astype(str)))
    if xyz.ndim != 2 or xyz.shape[1] != 3 or el.shape != (n,):
        raise ValueError(f"structure: xyz [N, 3] and element [N] expected, got {list(xyz.shape)} and {list(el.shape)}")
    if not (float(max_bond) > 0):
        raise ValueError(f"max_bond must be positive, got {max_bond!r}")
    keys = [np.asarray(structure[k]).astype(str) if k in structure else np.zeros(n, str) for k in ("chain_name", "icode")]
    resid = np.asarray(structure["resid"])
    keep = np.ones(n, bool)
    if exclude_water:
        keep = ~np.isin(np.char.upper(np.char.strip(np.asarray(structure["resname"]).astype(str))), WATER)
    is_h = (el == "H") | (el == "D")
    # residues: runs of equal (chain, resid, icode) are not assumed; group by the key itself
    _, res = np.unique(np.stack([keys[0], resid.astype(str), keys[1]], 1), axis=0, return_inverse=True)
    res = np.asarray(res).reshape(-1)
    order = np.argsort(res, kind="stable")
    bounds = np.flatnonzero(np.diff(res[order])) + 1
    dh = []
    for members in np.split(order, bounds):
        hs, heavy = members[is_h[members] & keep[members]], members[~is_h[members]]
        if hs.size == 0 or heavy.size == 0:
            continue
        dist = np.sqrt(np.sum(np.square(xyz[hs][:, None] - xyz[heavy][None]), -1))
        near = np.argmin(dist, 1)                       # (the first minimum: heavy is ascending, so ties go to the lower index)
        for h, j, dmin in zip(hs, heavy[near], dist[np.arange(hs.size), near]):
            if dmin <= max_bond and el[j] in ("N", "O"):
                dh.append((int(j), int(h)))
    dh = np.array(sorted(dh), np.int32).reshape(-1, 2)
    acc = np.flatnonzero(((el == "N") | (el == "O")) & keep).astype(np.int32)
    return dh, acc


# ------------------------------------------------------------------ argument checks (all before any launch)
def _indices(a, n_atoms, name, width=None):
    """int32 array of atom indices in [0, n_atoms), [n] or [n, width]"""
    v = _lib.host(a)
    if width is not None and (v.ndim != 2 or v.shape[1] != width):
        raise ValueError(f"{name} must be [P, {width}], got {list(v.shape)}")
    if width is None:
        if v.ndim != 1:
            raise ValueError(f"{name} must be one-dimensional, got {list(v.shape)}")
    if v.shape[0] < 1:
        raise ValueError(f"{name} must not be empty")
    if not np.issubdtype(v.dtype, np.integer):
        raise ValueError(f"{name} must hold integer atom indices, got {v.dtype}")
    if v.min() < 0 or v.max() >= n_atoms:
        raise ValueError(f"{name}: atom indices must lie in 0 .. {n_atoms - 1}")
    return np.ascontiguousarray(v, np.int32)


def _criteria(r_thr, angle, scale):
    thr, sc, ang = float(r_thr), float(scale), float(angle)
    if not (0 < thr <= F32_MAX and np.float32(thr) > 0) or not (0 < sc <= F32_MAX and np.float32(sc) > 0):
        raise ValueError(f"r_thr and scale must be positive and finite, got {r_thr!r}, {scale!r}")
    if not 90.0 <= ang < 180.0:
        raise ValueError(f"angle must lie in [90, 180) degrees, got {angle!r}")
    return thr, sc, math.cos(math.radians(ang)) ** 2


def _tables(xyz, dh, acc):
    x = _frames(xyz, "xyz")
    F, N = int(x.shape[0]), int(x.shape[1])
    if F > MAX_FRAMES:
        raise ValueError(f"at most 2**23 frames, got {F}")
    dh_h, acc_h = _indices(dh, N, "dh", 2), _indices(acc, N, "acc")
    P, A = dh_h.shape[0], acc_h.shape[0]
    if P * A > MAX_PAIRS:
        raise ValueError(f"too many candidate triplets per frame: P * A = {P} * {A} must stay below 2**31")
    return x, F, N, P, A, dh_h, acc_h


def _capacity(capacity, default):
    cap = default if capacity is None else int(capacity)
    if not 1 <= cap <= MAX_LIST:
        raise ValueError(f"capacity must be in 1 .. 2**30 - 1, got {capacity!r}")
    return cap


def frame_hbonds(xyz, dh, acc, r_thr=2.5, angle=120.0, scale=10.0, group=None, model=None, capacity=None):
    """(offsets int64 [F + 1], triplets int32 [K, 3], d float32 [K]): frame f owns the rows offsets[f]:offsets[f + 1], exactly the
    candidate triplets (donor, hydrogen, acceptor atom) bonded in that frame, in candidate order, with their H .. A distance d. The [P, A]
    candidates are never stored. group int8 [N] (None: no filter): only triplets whose donor and acceptor atoms carry different non-zero
    groups are listed (0 = in neither subunit). capacity: the rows to allocate for the first attempt (default: 2 F (P + A), at least
    4096); the call is repeated once with the exact count if it was too small."""
    x, F, N, P, A, dh_h, acc_h = _tables(xyz, dh, acc)
    if F * -(-P // DONOR_TILE) >= 2 ** 24:
        raise ValueError(f"too many workgroups: F * ceil(P / 32) = {F} * {-(-P // DONOR_TILE)} must stay below 2**24, pass the frames in batches")
    thr, sc, k = _criteria(r_thr, angle, scale)
    g_h = None
    if group is not None:
        g_h = _lib.host(group).reshape(-1)
        if g_h.size != N or not np.issubdtype(g_h.dtype, np.integer) or g_h.min() < 0 or g_h.max() > 127:
            raise ValueError(f"group must be {N} integers in 0 .. 127 (0: in neither subunit)")
        g_h = g_h.astype(np.int8)
    cap = _capacity(capacity, max(4096, 2 * F * (P + A)))
    model = _model_of(model, x)
    h = model.handle
    side = _lib.Side(x, model._gpu)
    xd, dd, ad = side.put(x, np.float32), side.put(dh_h, np.int32), side.put(acc_h, np.int32)
    gd = None if g_h is None else side.put(g_h, np.int8)
    offsets = side.empty((F + 1,), np.int64)
    lib = _lib.load()

    def call(cap, trip, d, sz):
        _lib.check(lib.pesto_frame_hbonds(h, F, N, P, A, side.ptr(xd), side.ptr(dd), side.ptr(ad), side.ptr(gd), thr, sc, k, cap, side.ptr(offsets),
                                          side.ptr(trip), side.ptr(d), sz.ctypes.data, side.kind, side.stream), lib.pesto_hbonds_last_error)
    trip, d, _ = _sized(call, side, min(cap, MAX_LIST), 3, np.float32)
    return offsets, trip, d


def baker_hubbard(xyz, dh, acc, freq=0.1, r_thr=2.5, angle=120.0, scale=10.0, model=None, return_counts=False):
    """triplets int32 [k, 3]: md.baker_hubbard(traj, freq, periodic=False) on index tables - the candidate triplets bonded in more than
    ``freq`` of the frames (float(n) / float(F) > freq, strict), in candidate order; with return_counts also counts int32 [k], the number
    of frames n of each. freq must be finite and not negative (freq = 0: bonded in at least one frame). A workgroup keeps the counts of
    its 32 donor pairs x 64 acceptors in registers over the frames: no [P, A] array on either side."""
    x, F, N, P, A, dh_h, acc_h = _tables(xyz, dh, acc)
    fq = float(freq)
    if not (np.isfinite(fq) and fq >= 0):
        raise ValueError(f"freq must be finite and not negative, got {freq!r}")
    thr, sc, k = _criteria(r_thr, angle, scale)
    model = _model_of(model, x)
    h = model.handle
    side = _lib.Side(x, model._gpu)
    xd, dd, ad = side.put(x, np.float32), side.put(dh_h, np.int32), side.put(acc_h, np.int32)
    lib = _lib.load()

    def call(cap, trip, n, sz):
        _lib.check(lib.pesto_hbond_occupancy(h, F, N, P, A, side.ptr(xd), side.ptr(dd), side.ptr(ad), thr, sc, k, fq, cap, side.ptr(trip),
                                             side.ptr(n), sz.ctypes.data, side.kind, side.stream), lib.pesto_hbonds_last_error)
    trip, n, _ = _sized(call, side, min(max(4096, 4 * (P + A)), MAX_LIST), 3, np.int32)
    return (trip, n) if return_counts else trip


def hydrogen_bonds(xyz, dh, acc, ids_R, ids_L, r_thr=2.5, angle=120.0, scale=10.0, model=None):
    """(nhb float64 [F], list of int32 [k_f, 3]): the reference's hydrogen_bonds(sub_R, sub_L, traj) on index arrays - per frame the bonds
    between the two subunits ids_R and ids_L (atom indices or masks; what ``align`` returns; disjoint): the rows with the donor in L and
    the acceptor in R first, then donor in R and acceptor in L, each in list order. One group-filtered launch sequence over all frames;
    the regrouping is made on the host from the offsets (the lists are copied to the host for it; with ROCm inputs the rows come back as
    ROCm tensors). When a frame has no bond with a donor in L (or in R) at all, the reference takes that side's rows from an earlier frame
    (a stale variable; NameError in the first frame): here such a frame simply has none."""
    x = _frames(xyz, "xyz")
    N = int(x.shape[1])
    sR, nR = _selection(ids_R, N, "ids_R")
    sL, nL = _selection(ids_L, N, "ids_L")
    if sR is None or sL is None or nR < 1 or nL < 1:
        raise ValueError("ids_R and ids_L: give the atom indices of the two subunits (at least one each)")
    group = np.zeros(N, np.int8)
    group[sR] = 1
    if np.any(group[sL]):
        raise ValueError("ids_R and ids_L must not share an atom")
    group[sL] = 2
    offsets, trip, _ = frame_hbonds(x, dh, acc, r_thr, angle, scale, group, model)
    off, t = _lib.host(offsets), _lib.host(trip)
    nhb = np.diff(off).astype(np.float64)
    rows = []
    for f in range(off.size - 1):
        tf = t[off[f]:off[f + 1]]
        tf = np.concatenate([tf[group[tf[:, 0]] == 2], tf[group[tf[:, 0]] == 1]])
        if _lib.is_torch(trip):
            import torch
            tf = torch.from_numpy(np.ascontiguousarray(tf)).to(trip.device)
        rows.append(tf)
    return nhb, rows


def unwrap_pbc(xyz, unitcell_lengths, mol, masses=None, elements=None, model=None, return_images=False):
    """float32 [F, N, 3]: the reference's unwrap_pbc(traj) on arrays - every molecule but the first shifted, frame by frame, to the
    periodic image whose centre of mass is nearest to molecule 0's (the definition is in the module docstring); the input is not
    modified. mol int [N]: the molecule row of every atom (the reference's chains), dense 0 .. M - 1, every row with an atom; they need
    not be contiguous. masses float64 [N], positive and finite, or elements [N] (atomic_masses); exactly one of the two. With
    return_images also image int32 [F, M], the chosen image k of every (frame, molecule). The molecule permutation is built on the host
    (a ROCm ``mol`` is copied there: N integers)."""
    x = _xyz(getattr(xyz, "xyz", xyz), "xyz")
    F, N = int(x.shape[0]), int(x.shape[1])
    if F > MAX_FRAMES:
        raise ValueError(f"at most 2**23 frames, got {F}")
    if tuple(unitcell_lengths.shape if hasattr(unitcell_lengths, "shape") else np.shape(unitcell_lengths)) != (F, 3):
        raise ValueError(f"unitcell_lengths must be [{F}, 3]")
    perm, off, M = _residue_order(mol, N, "mol")
    if F * M >= 2 ** 31:
        raise ValueError(f"F * M = {F} * {M} must stay below 2**31, pass the frames in batches")
    if (masses is None) == (elements is None):
        raise ValueError("give exactly one of masses and elements")
    if masses is None:
        ms = atomic_masses(elements)
    else:
        ms = np.asarray(_lib.host(masses), np.float64).reshape(-1)
    if ms.size != N or not np.all(np.isfinite(ms) & (ms > 0)):
        raise ValueError(f"masses must be {N} positive finite numbers")
    model = _model_of(model, x)
    h = model.handle
    side = _lib.Side(x, model._gpu)
    xd, ld = side.put(x, np.float32), side.put(unitcell_lengths, np.float32)
    pd, md = side.put(perm, np.int32), side.put(ms, np.float64)
    out, image = side.empty((F, N, 3), np.float32), side.empty((F, M), np.int32)
    off = np.ascontiguousarray(off, np.int32)
    lib = _lib.load()
    _lib.check(lib.pesto_unwrap_pbc(h, F, N, M, side.ptr(xd), side.ptr(ld), side.ptr(pd), off.ctypes.data, side.ptr(md), side.ptr(out),
                                    side.ptr(image), side.kind, side.stream), lib.pesto_hbonds_last_error)
    return (out, image) if return_images else out
