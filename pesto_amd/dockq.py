"""DockQ scoring of docking decoys on the GPU: how well each of F poses of a complex reproduces the bound one.

The package had the three CAPRI measures in pieces: ``trajectory.fnat`` through an all-pairs [F, Ra, Rb] residue map of every frame,
``docking.irmsd``, and no ligand RMSD, for which a pose is fitted on the receptor and measured on the ligand. Here one launch
(k_dockq, pesto_dockq.hip) reads every decoy once and gives all of them, the DockQ score (Basu and Wallner 2016) and the CAPRI class:
    dockq                the five measures of every decoy: fnat, preserved, irmsd, lrmsd, dockq, capri (and n_native)
    native_pairs         the residue pairs in contact in the bound complex
    lrmsd                the ligand RMSD alone
    fit_rmsd             the RMSD of one selection after a superposition on another (the general form of lrmsd)
    capri_class          the class cascade on given arrays (host NumPy)
Conventions are those of docking.py: xyz_ref is the bound complex [N, 3] or [1, N, 3], xyz the decoys float32 [F, N, 3] in the same atom
order; ids_R / ids_L are the receptor's and the ligand's atom indices (the caller decides which is which and whether hydrogens are in),
res_of_atom [N] the residue row of every atom, bb [N] true on backbone atoms (N, CA, C, O for DockQ proper; a CA mask reproduces the
reference's irmsd). The lead argument decides where a call runs (_lib.Side): NumPy in, NumPy out; ROCm tensors in, ROCm tensors out on
torch's current stream. ``model`` lends its device handle. There is no CPU or PyTorch fallback. Arguments are checked on the host before
the scoring launch (ValueError); the two checks that need the bound complex's contacts (no native pair, an interface under three
backbone atoms) follow the set-up launches that find them.

Definition. d, < and <= are docking.py's: scale and the thresholds are rounded to float32, d = fl32(sqrt_rn((dx*dx + dy*dy) + dz*dz)) *
fl32(scale), and a NaN distance passes no test.
    native pairs   the residue pairs (r, s), r a residue of an atom of ids_R and s of ids_L, with some atom pair d < r_contact in
                   xyz_ref, ascending by (r, s); P of them (P = 0: ValueError). Made once per call by docking.frame_residue_contacts on
                   the one reference frame.
    preserved[f]   int32: the native pairs with an atom pair d < r_contact in decoy f - by construction
                   trajectory.native_contacts(residue_contact_maps(ref), residue_contact_maps(xyz)) over the full sides
    fnat[f]        float32(double(preserved[f]) / double(P))
    irmsd[f]       docking.irmsd(xyz_ref, xyz, ids_R, ids_L, res_of_atom, ca=bb, r_thr=r_interface, scale=scale), bit for bit: the same
                   sums in the same order, exactly 0 for a selection that equals the reference's bitwise; under 3 atoms: ValueError
    lrmsd[f]       fit set S_R = ids_R with bb, ascending (at least 3 atoms), measure set S_L = ids_L with bb (at least 1). The decoy is
                   fitted onto the reference on S_R, in double from the float32 inputs, by the first fit of interface_rigid_docking with
                   its identity short cut; lrmsd = float32(sqrt(sum over S_L of |x' - y|^2 / |S_L|) * scale). A decoy that is the
                   reference gives exactly 0. For the RMSDs scale is used as given (a double), as docking.irmsd uses it.
    dockq[f]       float32((fnat + 1 / (1 + (irmsd / 1.5)^2) + 1 / (1 + (lrmsd / 8.5)^2)) / 3) in double from the three float32 values,
                   every operation rounded as written
    capri[f]       uint8, the highest class whose condition holds, the fnat conditions tested on the integers:
                   3 (high)        2 preserved >= P      and (lrmsd <= 1  or irmsd <= 1)
                   2 (medium)      10 preserved >= 3 P   and (lrmsd <= 5  or irmsd <= 2)
                   1 (acceptable)  10 preserved >= P     and (lrmsd <= 10 or irmsd <= 4)
                   0               otherwise
Every output is bit-identical from call to call and between host and device inputs. (DockQ scores ONE receptor-ligand pair; the
interface score of a whole assembly, over all its chain pairs and with its chain mapping, is qsscore.py's QS-score.)

Limits: F <= 2**23, N < 2**30 (docking.py's); P <= MAX_PAIRS = 2**24 native pairs, each with fewer than 2**31 atom pairs; the
selections hold distinct atoms, so at most N each; the set-up goes through frame_contacts at one frame, so |ids_R| * |ids_L| < 2**31.
Every excess raises ValueError before any launch of its step.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from .docking import MAX_FRAMES, _cutoff, _frames, _interface_lists, frame_residue_contacts
from .trajectory import _model_of, _residue_order, _selection

MAX_PAIRS = 2 ** 24             # PESTO_DOCKQ_MAX_PAIRS

DockQ = namedtuple("DockQ", "fnat preserved n_native irmsd lrmsd dockq capri")


def _reference(xyz_ref):
    """the one reference frame as [1, N, 3], and N"""
    y = _frames(xyz_ref, "xyz_ref")
    if int(y.shape[0]) != 1:
        raise ValueError(f"xyz_ref must be the one bound complex, [N, 3] or [1, N, 3], got {int(y.shape[0])} frames")
    N = int(y.shape[1])
    if N >= 2 ** 30:
        raise ValueError(f"at most 2**30 - 1 atoms, got {N}")
    return y, N


def _decoys(xyz, N):
    x = _frames(xyz, "xyz")
    if int(x.shape[1]) != N:
        raise ValueError(f"xyz_ref has {N} atoms and xyz {int(x.shape[1])}")
    if int(x.shape[0]) > MAX_FRAMES:
        raise ValueError(f"at most 2**23 frames, got {int(x.shape[0])}")
    return x


def _subunits(ids_R, ids_L, N):
    """the two subunits' distinct atom indices, ascending int32"""
    out = []
    for ids, name in ((ids_R, "ids_R"), (ids_L, "ids_L")):
        s, n = _selection(ids, N, name)
        if s is None or n < 1:
            raise ValueError(f"{name}: give the atom indices of the subunit (at least one)")
        out.append(np.unique(s))
    return out


def _rows(res_of_atom, N):
    r = _lib.host(res_of_atom).reshape(-1)
    if r.size != N or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"res_of_atom must be {N} integer residue rows, got {r.dtype} [{r.size}]")
    if r.min() < 0 or r.max() >= N:
        raise ValueError(f"res_of_atom: rows must lie in 0 .. {N - 1}")
    return r.astype(np.int64)


def _mask(bb, N):
    m = _lib.host(bb).reshape(-1)
    if m.size != N or not (m.dtype == np.bool_ or np.issubdtype(m.dtype, np.integer)):
        raise ValueError(f"bb must be a mask of {N} atoms, got {m.dtype} [{m.size}]")
    return m != 0


def _backbone(sR, sL, mask):
    """S_R and S_L: the backbone atoms of the two subunits"""
    SR, SL = sR[mask[sR]], sL[mask[sL]]
    if SR.size < 3:
        raise ValueError(f"the receptor holds {SR.size} backbone atoms: a superposition needs at least 3")
    if SL.size < 1:
        raise ValueError("the ligand holds no backbone atom to measure")
    return SR, SL


def _take(y, idx):
    """the atoms idx of y [1, N, 3] on y's side, contiguous"""
    if _lib.is_torch(y):
        import torch
        return y.index_select(1, torch.from_numpy(idx.astype(np.int64)).to(y.device)).contiguous()
    return np.ascontiguousarray(y[:, idx])


def _native_rows(y, sR, sL, dense_R, dense_L, thr, sc, model):
    """host int32 [P, 2]: the residue pairs in contact in the reference frame, as dense rows of each side, ascending (one frame through
    frame_contacts and frame_residue_contacts: the set-up of a call)"""
    _, rpairs, _ = frame_residue_contacts(_take(y, sR), _take(y, sL), dense_R, dense_L, thr, sc, model)
    return _lib.host(rpairs).reshape(-1, 2)


def _native(y, sR, sL, rows, thr, sc, model):
    """(pairs int32 [P, 2] in res_of_atom's rows, ranges int32 [P, 4], perm int32 [|sR| + |sL|]): the native pairs and, for the kernel,
    the two subunits' atoms sorted by residue (trajectory._residue_order) with every pair's two ranges of that permutation"""
    uR, dR = np.unique(rows[sR], return_inverse=True)
    uL, dL = np.unique(rows[sL], return_inverse=True)
    dR, dL = dR.reshape(-1).astype(np.int32), dL.reshape(-1).astype(np.int32)
    rp = _native_rows(y, sR, sL, dR, dL, thr, sc, model)
    P = int(rp.shape[0])
    if P == 0:
        raise ValueError("no native pair: no atom of ids_R lies within r_contact of an atom of ids_L in xyz_ref")
    if P > MAX_PAIRS:
        raise ValueError(f"{P} native pairs: at most 2**24 per call")
    pR, oR, _ = _residue_order(dR, sR.size, "res_of_atom")
    pL, oL, _ = _residue_order(dL, sL.size, "res_of_atom")
    oR, oL = oR.astype(np.int64), oL.astype(np.int64) + sR.size
    ranges = np.stack([oR[rp[:, 0]], oR[rp[:, 0] + 1], oL[rp[:, 1]], oL[rp[:, 1] + 1]], 1)
    if ((ranges[:, 1] - ranges[:, 0]) * (ranges[:, 3] - ranges[:, 2])).max() >= 2 ** 31:
        raise ValueError("a native pair has 2**31 atom pairs or more")
    pairs = np.stack([uR[rp[:, 0]], uL[rp[:, 1]]], 1).astype(np.int32)
    return pairs, ranges.astype(np.int32), np.concatenate([sR[pR], sL[pL]]).astype(np.int32)


def native_pairs(xyz_ref, ids_R, ids_L, res_of_atom, r_contact=5.0, scale=10.0, model=None):
    """int32 [P, 2]: the residue pairs (r, s) of res_of_atom's rows, r of the receptor ids_R and s of the ligand ids_L, with some atom
    pair d < r_contact in the bound complex xyz_ref, ascending by (r, s). No pair: ValueError."""
    y, N = _reference(xyz_ref)
    sR, sL = _subunits(ids_R, ids_L, N)
    rows = _rows(res_of_atom, N)
    thr, sc = _cutoff(r_contact, scale)
    pairs = _native(y, sR, sL, rows, thr, sc, model)[0]
    if _lib.is_torch(y) and y.is_cuda:
        import torch
        return torch.from_numpy(pairs).to(y.device)
    return pairs


def capri_class(preserved, n_native, irmsd, lrmsd):
    """uint8 [F] on the host: the CAPRI cascade of dockq() on given arrays - preserved integer counts out of n_native pairs, irmsd and
    lrmsd as float32. The fnat conditions are tested on the integers."""
    k = _lib.host(preserved).astype(np.int64)
    P = int(n_native)
    if P < 1 or np.any(k < 0) or np.any(k > P):
        raise ValueError(f"0 <= preserved <= n_native and n_native >= 1 expected, got n_native = {n_native!r}")
    ir, lr = _lib.host(irmsd).astype(np.float32), _lib.host(lrmsd).astype(np.float32)
    one, two, four, five, ten = (np.float32(v) for v in (1, 2, 4, 5, 10))
    with np.errstate(invalid="ignore"):
        high = (2 * k >= P) & ((lr <= one) | (ir <= one))
        medium = (10 * k >= 3 * P) & ((lr <= five) | (ir <= two))
        acceptable = (10 * k >= P) & ((lr <= ten) | (ir <= four))
    return np.where(high, 3, np.where(medium, 2, np.where(acceptable, 1, 0))).astype(np.uint8)


def dockq(xyz_ref, xyz, ids_R, ids_L, res_of_atom, bb, r_contact=5.0, r_interface=10.0, scale=10.0, model=None):
    """DockQ(fnat float32 [F], preserved int32 [F], n_native int, irmsd float32 [F], lrmsd float32 [F], dockq float32 [F], capri uint8
    [F]) of the F decoys xyz against the bound complex xyz_ref: see the module's definition. The native pairs, the interface and the
    atoms' order by residue are set up once per call (three small launches on the reference frame and host index arithmetic); the decoys
    are then read once, by one launch."""
    y, N = _reference(xyz_ref)
    x = _decoys(xyz, N)
    sR, sL = _subunits(ids_R, ids_L, N)
    rows = _rows(res_of_atom, N)
    mask = _mask(bb, N)
    thr, sc = _cutoff(r_contact, scale)
    _cutoff(r_interface, scale)
    SR, SL = _backbone(sR, sL, mask)
    pairs, ranges, perm = _native(y, sR, sL, rows, thr, sc, model)
    ira, irb, _, model = _interface_lists(y, sR, sL, rows, r_interface, scale, model)
    both = np.union1d(ira, irb)
    SI = both[mask[both]]
    if SI.size < 3:
        raise ValueError(f"the interface holds {SI.size} backbone atoms: a superposition needs at least 3")
    F, P = int(x.shape[0]), int(pairs.shape[0])
    model = _model_of(model, x)
    h = model.handle
    side = _lib.Side(x, model._gpu)
    xd, yd = side.put(x, np.float32), side.put(y, np.float32)
    rg, pm, si, sr, sl = (side.put(v.astype(np.int32), np.int32) for v in (ranges, perm, SI, SR, SL))
    fn, kept, ir, lr, dq = (side.empty((F,), t) for t in (np.float32, np.int32, np.float32, np.float32, np.float32))
    cls = side.empty((F,), np.uint8)
    lib = _lib.load()
    _lib.check(lib.pesto_dockq(h, F, N, side.ptr(yd), side.ptr(xd), P, side.ptr(rg), perm.size, side.ptr(pm), SI.size, side.ptr(si), SR.size,
                               side.ptr(sr), SL.size, side.ptr(sl), thr, sc, side.ptr(fn), side.ptr(kept), side.ptr(ir), side.ptr(lr), side.ptr(dq),
                               side.ptr(cls), side.kind, side.stream), lib.pesto_dockq_last_error)
    return DockQ(fn, kept, P, ir, lr, dq, cls)


def fit_rmsd(xyz_ref, xyz, sel_fit, sel_measure, scale=10.0, model=None):
    """float32 [F]: every frame of xyz superposed onto xyz_ref (1 or F frames) on the atoms sel_fit (indices or a mask, at least 3), then
    sqrt(mean over the atoms sel_measure (at least 1) of the squared deviation) * scale - different atoms for fit and measure, which
    trajectory.rmsd does not offer. Evaluated in double from the float32 inputs and rounded once; a frame whose fit atoms equal the
    reference's bit for bit is fitted by the identity itself."""
    y, x = _frames(xyz_ref, "xyz_ref"), _frames(xyz, "xyz")
    Fr, F, N = int(y.shape[0]), int(x.shape[0]), int(x.shape[1])
    if F > MAX_FRAMES:
        raise ValueError(f"at most 2**23 frames, got {F}")
    if Fr not in (1, F):
        raise ValueError(f"xyz_ref must have 1 or {F} frames, got {Fr}")
    if int(y.shape[1]) != N:
        raise ValueError(f"xyz_ref has {int(y.shape[1])} atoms and xyz {N}")
    if N >= 2 ** 30:
        raise ValueError(f"at most 2**30 - 1 atoms, got {N}")
    sf, nf = _selection(sel_fit, N, "sel_fit")
    sm, nm = _selection(sel_measure, N, "sel_measure")
    if sf is None or sm is None:
        raise ValueError("sel_fit and sel_measure: give the atoms to fit on and the atoms to measure")
    if nf < 3 or nf > N:
        raise ValueError(f"a superposition needs 3 to {N} atoms, got {nf}")
    if nm < 1 or nm > N:
        raise ValueError(f"1 to {N} atoms to measure, got {nm}")
    sc = float(scale)
    if not (np.isfinite(sc) and sc > 0):
        raise ValueError(f"scale must be positive and finite, got {scale!r}")
    model = _model_of(model, x)
    h = model.handle
    side = _lib.Side(x, model._gpu)
    xd, yd = side.put(x, np.float32), side.put(y, np.float32)
    fd, md = side.put(sf, np.int32), side.put(sm, np.int32)
    out = side.empty((F,), np.float32)
    lib = _lib.load()
    _lib.check(lib.pesto_fit_rmsd(h, F, Fr, N, side.ptr(yd), side.ptr(xd), nf, side.ptr(fd), nm, side.ptr(md), sc, side.ptr(out), side.kind,
                                  side.stream), lib.pesto_dockq_last_error)
    return out


def lrmsd(xyz_ref, xyz, ids_R, ids_L, bb, scale=10.0, model=None):
    """float32 [F]: the ligand RMSD of dockq() alone - fit_rmsd on the backbone atoms of the receptor ids_R, measured on the backbone
    atoms of the ligand ids_L - bit for bit."""
    y, N = _reference(xyz_ref)
    x = _decoys(xyz, N)
    sR, sL = _subunits(ids_R, ids_L, N)
    SR, SL = _backbone(sR, sL, _mask(bb, N))
    return fit_rmsd(y, x, SR, SL, scale, model)
