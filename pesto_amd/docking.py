"""Docking metrics and frame contacts on the GPU: how a complex holds together over an MD run.

The reference (md_analysis/mdtraj_utils/trajectory_utils.py) answers this with Python loops over the frames: ``contacts`` builds a dense
[Na, Nb] torch matrix per frame and copies three arrays to the host per frame, ``atoms_to_residue_contacts`` loops per frame and residue
pair, ``interface_residues_within`` builds an [N, residues] matrix, ``irmsd`` and ``interface_rigid_docking`` run batched NumPy SVDs around a
transformed copy of the whole trajectory. Here every function is one launch sequence over all frames (pesto_docking.hip):
    frame_contacts / contacts            the atom pairs closer than r_thr in every frame, with their distances
    frame_residue_contacts               their distinct residue pairs per frame with the minimum distance
    interface_atoms                      the atoms of every residue within r_thr of the other subunit in the reference frame
    irmsd                                CA-RMSD of that interface after superposition on it (the second CAPRI measure, next to fnat)
    interface_rigid_docking              translation and rotation vector of the ligand against its bound pose
Chain alignment (the reference's ``align``) stays with mdtraj: callers pass index arrays. Coordinates are float32 [F, N, 3] arrays, or
[N, 3] where a single frame is meant. The lead argument decides where a call runs (_lib.Side): ROCm tensors stay on the device (device
pointers, torch's current stream, ROCm tensors out); NumPy arrays are staged and NumPy arrays come back. ``model`` lends its device handle;
without one a weightless handle is used. Arguments are checked before any launch (ValueError). There is no CPU or PyTorch fallback.

Definition. ``scale`` multiplies distances before the comparison (mdtraj keeps nanometres and the reference multiplies by 10: the default);
scale and r_thr are rounded to float32 and
    d = fl32(sqrt_rn((dx*dx + dy*dy) + dz*dz)) * fl32(scale)       every operation rounded as written, the root correctly rounded
A contact has d < r_thr; the interface has d <= r_thr, as interface_residues_within has it; a NaN distance passes neither. The lists, the
residue pairs, d, dmin and the interface equal this definition exactly (the reference's own d differs from it by one float32 unit in
about 0.6 % of the entries: torch's CPU sqrt is not correctly rounded). irmsd, t and r are evaluated in double from the float32 inputs
and rounded once; the reference's float32 results deviate from a float64 restatement by e_ref (tests/golden/make_docking_golden.py) and
the tests allow max(4 e_ref, 4 eps32 max|value|). Every output is bit-identical from call to call and between host and device inputs.
"""
import numpy as np

from . import _lib
from .trajectory import F32_MAX, _model_of, _residue_order, _selection, _xyz

MAX_FRAMES = 2 ** 23            # PESTO_DOCKING_MAX_FRAMES
MAX_MAP_WORDS = 2 ** 28         # PESTO_DOCKING_MAX_MAP_WORDS: F * ceil(Ra * Rb / 32) of frame_residue_contacts
MAX_LIST = 2 ** 30 - 1          # entries of one list


def _cutoff(r_thr, scale):
    thr, sc = float(r_thr), float(scale)
    if not (np.isfinite(thr) and abs(thr) <= F32_MAX) or not (0 < sc <= F32_MAX and np.float32(sc) > 0):
        raise ValueError(f"r_thr must be finite and scale positive and finite, got {r_thr!r}, {scale!r}")
    return thr, sc


def _frames(x, name):
    """[F, N, 3] of a coordinate argument; a single frame [N, 3] becomes [1, N, 3]"""
    a = getattr(x, "xyz", x)
    if not (_lib.is_torch(a) or isinstance(a, np.ndarray)):
        a = np.asarray(a, np.float32)
    return _xyz(a[None] if len(a.shape) == 2 else a, name)


def _sized(call, side, cap, width, dtype):
    """The capacity protocol of a list-valued entry point: call(cap, rows, values, sizes) until the count fits. Returns (rows, values, K)."""
    for _ in range(2):
        rows, vals, sz = side.empty((cap, width), np.int32), side.empty((cap,), dtype), np.zeros(1, np.int64)
        call(cap, rows, vals, sz)
        K = int(sz[0])
        if K <= cap:
            return rows[:K], vals[:K], K
        if K > MAX_LIST:
            raise ValueError(f"{K} list entries: at most 2**30 - 1 per call, pass the frames in batches")
        cap = K
    raise RuntimeError("the list capacity did not converge")


def frame_contacts(xyz_a, xyz_b, r_thr=5.0, scale=10.0, model=None, capacity=None):
    """(offsets int64 [F + 1], pairs int32 [K, 2], d float32 [K]): frame f owns the rows offsets[f]:offsets[f + 1], exactly the pairs
    (i, j) of atom i of xyz_a [F, Na, 3] and atom j of xyz_b [F, Nb, 3] with d < r_thr, i ascending, then j ascending (torch.where's
    order), with their d. A NaN distance is in no list. The [Na, Nb] matrix is never stored. capacity: the rows to allocate for the first
    attempt (default: 2 F (Na + Nb), at least 4096); the call is repeated once with the exact count if it was too small."""
    a, b = _frames(xyz_a, "xyz_a"), _frames(xyz_b, "xyz_b")
    F, Na, Nb = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
    if int(b.shape[0]) != F:
        raise ValueError(f"the two sides have {F} and {int(b.shape[0])} frames")
    if F > MAX_FRAMES:
        raise ValueError(f"at most 2**23 frames, got {F}")
    if Na * Nb >= 2 ** 31:
        raise ValueError(f"too many atom pairs per frame: Na * Nb = {Na} * {Nb} must stay below 2**31")
    if F * -(-Na // 32) >= 2 ** 24:
        raise ValueError(f"too many workgroups: F * ceil(Na / 32) = {F} * {-(-Na // 32)} must stay below 2**24, pass the frames in batches")
    thr, sc = _cutoff(r_thr, scale)
    cap = max(4096, 2 * F * (Na + Nb)) if capacity is None else int(capacity)
    if not 1 <= cap <= MAX_LIST:
        raise ValueError(f"capacity must be in 1 .. 2**30 - 1, got {capacity!r}")
    model = _model_of(model, a)
    h = model.handle
    side = _lib.Side(a, model._gpu)
    xa, xb = side.put(a, np.float32), side.put(b, np.float32)
    offsets = side.empty((F + 1,), np.int64)
    lib = _lib.load()

    def call(cap, pairs, d, sz):
        _lib.check(lib.pesto_frame_contacts(h, F, Na, Nb, side.ptr(xa), side.ptr(xb), thr, sc, cap, side.ptr(offsets), side.ptr(pairs), side.ptr(d),
                                            sz.ctypes.data, side.kind, side.stream), lib.pesto_docking_last_error)
    pairs, d, _ = _sized(call, side, min(cap, MAX_LIST), 2, np.float32)
    return offsets, pairs, d


def contacts(xyz_a, xyz_b, ids_a=None, ids_b=None, r_thr=5.0, scale=10.0, model=None):
    """The reference's contacts(sub_a, sub_b, traj, r_thr) on already selected coordinates: a list with one [d float32 [k], ids int32
    [k, 2]] per frame, ids[:, 0] / ids[:, 1] mapped through ids_a [Na] / ids_b [Nb] (the atoms' indices in the trajectory; None: the rows
    of xyz_a / xyz_b themselves). The per-frame views are made on the host from the offsets (one copy of F + 1 integers)."""
    a, b = _frames(xyz_a, "xyz_a"), _frames(xyz_b, "xyz_b")
    maps = []
    for ids, n, name in ((ids_a, int(a.shape[1]), "ids_a"), (ids_b, int(b.shape[1]), "ids_b")):
        if ids is not None:
            v = _lib.host(ids).reshape(-1)
            if v.size != n or not np.issubdtype(v.dtype, np.integer) or (v.size and (v.min() < 0 or v.max() >= 2 ** 31)):
                raise ValueError(f"{name} must be {n} non-negative int32 atom indices")
            ids = v.astype(np.int32)
        maps.append(ids)
    offsets, pairs, d = frame_contacts(a, b, r_thr, scale, model)
    if maps[0] is not None or maps[1] is not None:
        if _lib.is_torch(pairs):
            import torch
            cols = [pairs[:, c] if m is None else torch.from_numpy(m).to(pairs.device)[pairs[:, c].long()] for c, m in enumerate(maps)]
            pairs = torch.stack(cols, 1)
        else:
            pairs = np.stack([pairs[:, c] if m is None else m[pairs[:, c]] for c, m in enumerate(maps)], 1)
    off = _lib.host(offsets)
    return [[d[off[f]:off[f + 1]], pairs[off[f]:off[f + 1]]] for f in range(off.size - 1)]


def _residue_rows(res, n_atoms, name):
    """(res int32 [n_atoms], R): dense residue rows 0 .. R - 1, every row with an atom (trajectory._residue_order's checks)"""
    _, _, R = _residue_order(res, n_atoms, name)
    return _lib.host(res).reshape(-1).astype(np.int32), R


def frame_residue_contacts(xyz_a, xyz_b=None, res_a=None, res_b=None, r_thr=5.0, scale=10.0, model=None):
    """(offsets int64 [F + 1], rpairs int32 [U, 2], dmin float32 [U]): per frame the distinct (res_a[i], res_b[j]) over that frame's
    contacts in lexicographic order (np.unique(axis=0)), each with the minimum d - the reference's atoms_to_residue_contacts for every
    frame. res_a [Na], res_b [Nb]: the residue row of each atom, dense 0 .. Ra - 1 / 0 .. Rb - 1 (every row with an atom; they need not
    be contiguous). Instead of the coordinates, the output of frame_contacts can be passed as the first argument (xyz_b None; r_thr and
    scale are then not used), so the search runs once. F * ceil(Ra * Rb / 32) <= MAX_MAP_WORDS."""
    if res_a is None or res_b is None:
        raise ValueError("res_a and res_b: give the residue row of every atom of the two sides")
    ra_h, rb_h = _lib.host(res_a).reshape(-1), _lib.host(res_b).reshape(-1)
    if xyz_b is None:
        if not (isinstance(xyz_a, (tuple, list)) and len(xyz_a) == 3):
            raise ValueError("without xyz_b the first argument must be the (offsets, pairs, d) of frame_contacts")
        offsets, pairs, d = xyz_a
        F, K = int(offsets.shape[0]) - 1, int(pairs.shape[0])
        if F < 1 or len(offsets.shape) != 1 or tuple(pairs.shape) != (K, 2) or tuple(d.shape) != (K,):
            raise ValueError(f"offsets [F + 1], pairs [K, 2] and d [K] expected, got {list(offsets.shape)}, {list(pairs.shape)}, {list(d.shape)}")
        Na, Nb = int(ra_h.size), int(rb_h.size)
    else:
        a, b = _frames(xyz_a, "xyz_a"), _frames(xyz_b, "xyz_b")
        F, Na, Nb = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
        _cutoff(r_thr, scale)
    if Na < 1 or Nb < 1:
        raise ValueError("res_a and res_b must not be empty")
    ra, Ra = _residue_rows(ra_h, Na, "res_a")
    rb, Rb = _residue_rows(rb_h, Nb, "res_b")
    if F > MAX_FRAMES:
        raise ValueError(f"at most 2**23 frames, got {F}")
    if F * -(-Ra * Rb // 32) > MAX_MAP_WORDS:
        raise ValueError(f"residue map too large: F * ceil(Ra * Rb / 32) = {F} * {-(-Ra * Rb // 32)} must stay within 2**28, pass the frames in batches")
    if xyz_b is not None:
        offsets, pairs, d = frame_contacts(a, b, r_thr, scale, model)
        K = int(pairs.shape[0])
    if K > MAX_LIST:
        raise ValueError(f"{K} contacts: at most 2**30 - 1 per call")
    model = _model_of(model, offsets)
    h = model.handle
    side = _lib.Side(offsets, model._gpu)
    od, pd, dd = side.put(offsets, np.int64), side.put(pairs, np.int32), side.put(d, np.float32)
    rad, rbd = side.put(ra, np.int32), side.put(rb, np.int32)
    roff = side.empty((F + 1,), np.int64)
    lib = _lib.load()

    def call(cap, rpairs, dmin, sz):
        _lib.check(lib.pesto_frame_residue_contacts(h, F, Na, Nb, K, side.ptr(od), side.ptr(pd), side.ptr(dd), side.ptr(rad), side.ptr(rbd), Ra, Rb,
                                                    cap, side.ptr(roff), side.ptr(rpairs), side.ptr(dmin), sz.ctypes.data, side.kind, side.stream),
                   lib.pesto_docking_last_error)
    rpairs, dmin, _ = _sized(call, side, max(1, K), 2, np.float32)      # (no more residue pairs than contacts)
    return roff, rpairs, dmin


def _interface(xyz0, ids_a, ids_b, res_of_atom, r_thr, scale, model):
    """(flags uint8 [2, N] on the call's side, N, model)"""
    x = _frames(xyz0, "xyz0")
    N = int(x.shape[1])
    if N >= 2 ** 30:
        raise ValueError(f"at most 2**30 - 1 atoms, got {N}")
    sa, na = _selection(ids_a, N, "ids_a")
    sb, nb = _selection(ids_b, N, "ids_b")
    if sa is None or sb is None or na < 1 or nb < 1:
        raise ValueError("ids_a and ids_b: give the atom indices of the two subunits (at least one each)")
    r = _lib.host(res_of_atom).reshape(-1)
    if r.size != N or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"res_of_atom must be {N} integer residue rows, got {r.dtype} [{r.size}]")
    if r.min() < 0 or r.max() >= N:
        raise ValueError(f"res_of_atom: rows must lie in 0 .. {N - 1}")
    thr, sc = _cutoff(r_thr, scale)
    R = int(r.max()) + 1
    model = _model_of(model, x)
    h = model.handle
    side = _lib.Side(x, model._gpu)
    x0 = side.put(x[0], np.float32)
    ia, ib, rd = side.put(sa, np.int32), side.put(sb, np.int32), side.put(r.astype(np.int32), np.int32)
    flags = side.empty((2, N), np.uint8)
    lib = _lib.load()
    _lib.check(lib.pesto_interface_atoms(h, N, side.ptr(x0), na, side.ptr(ia), nb, side.ptr(ib), side.ptr(rd), R, thr, sc, side.ptr(flags), side.kind,
                                         side.stream), lib.pesto_docking_last_error)
    return flags, N, model


def interface_atoms(xyz0, ids_a, ids_b, res_of_atom, r_thr=10.0, scale=10.0, model=None):
    """(ids_ira, ids_irb), both ascending int64: the reference's interface_residues_within on index arrays. xyz0 [N, 3], or frame 0 of
    [F, N, 3]; ids_a / ids_b: the atom indices of the two subunits (what ``align`` returns); res_of_atom [N]: the residue row of every
    atom. ids_ira holds every atom of the whole topology (not only of ids_a) whose residue contains an atom of ids_a with d <= r_thr
    to some atom of ids_b; ids_irb likewise for ids_b. (<= here, < in contacts: the reference's own choice.) The per-atom flags are made
    on the device; the index lists are their non-zero positions (one synchronisation for the sizes)."""
    flags, _, _ = _interface(xyz0, ids_a, ids_b, res_of_atom, r_thr, scale, model)
    if _lib.is_torch(flags):
        return flags[0].nonzero().reshape(-1), flags[1].nonzero().reshape(-1)
    return np.nonzero(flags[0])[0].astype(np.int64), np.nonzero(flags[1])[0].astype(np.int64)


def _interface_lists(xyz_ref, ids_a, ids_b, res_of_atom, r_thr, scale, model):
    """the two interface index lists as host int32 arrays (N flags copied to the host), and N"""
    flags, N, model = _interface(xyz_ref, ids_a, ids_b, res_of_atom, r_thr, scale, model)
    f = _lib.host(flags)
    return np.nonzero(f[0])[0].astype(np.int32), np.nonzero(f[1])[0].astype(np.int32), N, model


def irmsd(xyz_ref, xyz, ids_a, ids_b, res_of_atom, ca, r_thr=10.0, scale=10.0, model=None):
    """float32 [F]: the reference's irmsd - the interface is interface_atoms of frame 0 of xyz_ref, the selection its atoms (both sides)
    with ``ca`` [N] true, ascending, and the result trajectory.rmsd(xyz_ref, xyz, sel, sel, scale) bit for bit: superposition on the
    interface's CA atoms, then their RMSD times scale - with one difference: a frame whose selected atoms equal the reference's bit for
    bit is fitted by the identity itself and gives exactly 0, where trajectory.rmsd returns the rounding residue of its rotation (some
    1e-15). That takes the fit of the rigid-docking kernel (pesto_interface_rmsd) instead of a call of trajectory.rmsd. xyz_ref has one
    frame or one per frame of xyz. Fewer than 3 selected atoms: ValueError."""
    y, x = _frames(xyz_ref, "xyz_ref"), _frames(xyz, "xyz")
    if int(y.shape[0]) not in (1, int(x.shape[0])):
        raise ValueError(f"xyz_ref must have 1 or {int(x.shape[0])} frames, got {int(y.shape[0])}")
    if int(x.shape[0]) > MAX_FRAMES:
        raise ValueError(f"at most 2**23 frames, got {int(x.shape[0])}")
    mask = _lib.host(ca).reshape(-1)
    if mask.size != int(y.shape[1]) or int(x.shape[1]) != mask.size:
        raise ValueError(f"xyz_ref, xyz and ca must agree in the number of atoms, got {int(y.shape[1])}, {int(x.shape[1])} and {mask.size}")
    ira, irb, _, model = _interface_lists(y, ids_a, ids_b, res_of_atom, r_thr, scale, model)
    both = np.union1d(ira, irb)
    sel = both[mask[both] != 0]
    if sel.size < 3:
        raise ValueError(f"the interface holds {sel.size} CA atoms: a superposition needs at least 3")
    F, Fr, N = int(x.shape[0]), int(y.shape[0]), int(x.shape[1])
    h = model.handle
    side = _lib.Side(x, model._gpu)
    xd, yd, sd = side.put(x, np.float32), side.put(y, np.float32), side.put(sel.astype(np.int32), np.int32)
    out = side.empty((F,), np.float32)
    lib = _lib.load()
    _lib.check(lib.pesto_interface_rmsd(h, F, Fr, N, side.ptr(yd), side.ptr(xd), sel.size, side.ptr(sd), float(scale), side.ptr(out), side.kind,
                                        side.stream), lib.pesto_docking_last_error)
    return out


def interface_rigid_docking(xyz_ref, xyz, ids_R, ids_L, res_of_atom, r_thr=10.0, scale=10.0, model=None):
    """(t float32 [F, 3], r float32 [F, 3]): the reference's interface_rigid_docking(sub_R, sub_L, traj_ref, traj) on index arrays.
    The interfaces are interface_atoms of frame 0 of xyz_ref for the receptor ids_R and the ligand ids_L; xyz_ref has 1 or F frames.
    Per frame, in double from the float32 inputs:
        1  the frame is superposed onto the reference on the receptor's interface atoms (the fit of trajectory.superpose, including its
           treatment of degenerate selections);
        2  the transformed ligand interface atoms - only they - are fitted onto the reference's: t_cm, R2, t_ref2;
        3  t = t_ref2 - t_cm, in the coordinates' unit;
        4  r = the rotation vector of R2 as scipy's Rotation.from_matrix(R2).as_rotvec() reads it: unit quaternion with w >= 0,
           angle = 2 atan2(|v|, w) in [0, pi], r = angle v / |v|, 0 for the identity.
    The reference first recentres traj_ref on its receptor interface; that shift moves t_ref2 and, through step 1, t_cm alike, cancels in
    t and is not part of this definition. Near angle = pi the sign of the axis is decided by rounding in any implementation: r and -r
    describe the same rotation there. A selection that equals the reference's bit for bit is fitted by the identity itself, so a frame
    that is the reference gives t = 0 and r = 0 exactly. Fewer than 3 interface atoms on either side: ValueError."""
    y, x = _frames(xyz_ref, "xyz_ref"), _frames(xyz, "xyz")
    Fr, F, N = int(y.shape[0]), int(x.shape[0]), int(x.shape[1])
    if F > MAX_FRAMES:
        raise ValueError(f"at most 2**23 frames, got {F}")
    if Fr not in (1, F):
        raise ValueError(f"xyz_ref must have 1 or {F} frames, got {Fr}")
    if int(y.shape[1]) != N:
        raise ValueError(f"xyz_ref has {int(y.shape[1])} atoms and xyz {N}")
    sR, sL, _, model = _interface_lists(y, ids_R, ids_L, res_of_atom, r_thr, scale, model)
    if sR.size < 3 or sL.size < 3:
        raise ValueError(f"the interface holds {sR.size} receptor and {sL.size} ligand atoms: a superposition needs at least 3 of each")
    h = model.handle
    side = _lib.Side(x, model._gpu)
    xd, yd = side.put(x, np.float32), side.put(y, np.float32)
    rd, ld = side.put(sR, np.int32), side.put(sL, np.int32)
    t, r = side.empty((F, 3), np.float32), side.empty((F, 3), np.float32)
    lib = _lib.load()
    _lib.check(lib.pesto_rigid_docking(h, F, Fr, N, side.ptr(yd), side.ptr(xd), sR.size, side.ptr(rd), sL.size, side.ptr(ld), side.ptr(t), side.ptr(r),
                                       side.kind, side.stream), lib.pesto_docking_last_error)
    return t, r
