"""lDDT model-quality scoring on the GPU (Mariani et al. 2013): how well every residue of a model, or of every frame of an MD run, keeps
the distances the reference structure has around it - without any superposition.

The package compared a structure with its reference after a fit (trajectory.rmsd, docking.irmsd, dockq.lrmsd), through contacts (fnat,
dockq) and by clustering frames on RMSD; this is the per-residue measure that CASP, CAMEO and CAPRI report and that AlphaFold's pLDDT
(carried through patches and structure_io as the b-factor column) predicts. Its result is an [F, R] array, the shape forward_frames and
postprocess give for interface probabilities (pesto_lddt.hip):
    lddt                 Lddt(score [F], residue [F, R], preserved [F, R, T], total [R], n_pairs) of F frames against one reference
    reference_pairs      the reference's pair list (offsets, j, d_ref), to be passed back as pairs= so later calls skip the set-up
    ilddt                lddt over the pairs between different chains (mode="inter"): the interface score that goes with DockQ
    lddt_ca              lddt over the CA atoms
    structure_lddt       two structures or two PDB paths, atoms matched on the host by (chain, residue number, atom name)
Conventions are those of docking.py: xyz_ref is [N, 3] or [1, N, 3], xyz float32 [F, N, 3] in the same atom order, res_of_atom [N] the
residue row of every atom (dense rows 0 .. R - 1; a residue's atoms need not be adjacent), scale multiplies distances before every
comparison (mdtraj keeps nanometres: the default 10 gives angstroms). The lead argument decides where a call runs (_lib.Side): NumPy in,
NumPy out; ROCm tensors in, ROCm tensors out on torch's current stream. ``model`` lends its device handle. There is no CPU or PyTorch
fallback. Arguments are checked on the host before any launch (ValueError); the indices are checked again by a kernel whose verdict is
read before anything else is launched, so a refused call writes nothing.

Definition. The distance is d(a, b) = fl32(sqrt_rn((dx*dx + dy*dy) + dz*dz)) * fl32(scale): dist2 of pesto_geom.h, the correctly rounded
root, no contraction. A NaN distance passes no test.
    reference pairs  the ordered pairs (i, j), i != j, that meet all of: both atoms are selected (sel, default all);
                     res_of_atom[i] != res_of_atom[j]; d_ref(i, j) < fl32(r_incl), r_incl defaulting to 15 A; for mode="inter"
                     chain_of_atom[i] != chain_of_atom[j]; for mode="intra" the chains are equal; mode="all" has no chain test and needs
                     no chain_of_atom. An atom with a non-finite reference coordinate has no pairs. K is their number.
    total[r]         int32: the number of pairs with i in residue r. Every unordered pair is counted once for each of its two residues.
    preserved[f,r,k] int32: the number of those pairs with fabsf(d_f(i, j) - d_ref(i, j)) < fl32(thresholds[k]). The subtraction is
                     rounded once in float32. An atom that is missing in frame f has NaN coordinates there and preserves nothing.
    thresholds       1 to 8 ascending positive values, default (0.5, 1, 2, 4). T is their number.
    residue[f,r]     float32(double(sum_k preserved[f, r, k]) / double(T * total[r])). It is NaN where total[r] == 0.
    score[f]         the same quotient over the int64 sums over the residues. It is NaN when K == 0.
Both tests are strict. This is our definition; no equality with OpenStructure's lddt is claimed. Not reproduced: the stereochemistry
filter, the renaming of symmetric side-chain atoms (ASP OD1/OD2 and the like), a sequence separation, periodic images. (The contact-based
interface score of an assembly, QS-score with ICS, which is reported next to lDDT: qsscore.py.)
Every output is bit-identical from call to call, and between host and device inputs.

Ragged batch. sizes= (atom counts, as in sasa.py) lays B structures back to back in xyz_ref and xyz, one model each: an AlphaFold model
set against its experimental structures in one call. res_of_atom then numbers the residues of the whole batch, structure after
structure; pairs never cross structures; score and n_pairs have one entry per structure; a structure without any pair scores NaN.

Limits: F <= 2**23, N < 2**30, K <= MAX_ENTRIES = 2**30, T <= 8. Every excess raises ValueError before the launch of its step.
"""
import os
from collections import namedtuple

import numpy as np

from . import _lib
from .docking import _cutoff, _frames
from .dockq import _decoys, _reference
from .trajectory import _model_of, _residue_order, _selection

MAX_FRAMES = 2 ** 23            # PESTO_LDDT_MAX_FRAMES
MAX_ENTRIES = 2 ** 30           # PESTO_LDDT_MAX_ENTRIES
MAX_THRESHOLDS = 8              # PESTO_LDDT_MAX_THRESHOLDS
MODES = {"all": 0, "inter": 1, "intra": 2}

Lddt = namedtuple("Lddt", "score residue preserved total n_pairs")


def _thresholds(thresholds):
    t = np.asarray(_lib.host(thresholds), np.float64).reshape(-1)
    if not 1 <= t.size <= MAX_THRESHOLDS:
        raise ValueError(f"1 to {MAX_THRESHOLDS} thresholds, got {t.size}")
    with np.errstate(over="ignore"):
        t32 = t.astype(np.float32)
    if not np.all(np.isfinite(t32)) or not np.all(t32 > 0) or not np.all(t32[1:] > t32[:-1]):
        raise ValueError(f"thresholds must be positive, finite and ascending in float32, got {t.tolist()}")
    return np.ascontiguousarray(t32)


def _topology(N, res_of_atom, chain_of_atom, mode, sel, sizes):
    """the host side of a call's index arrays: dict of res int32 [N], perm, roff, R, chain int32 [N] or None, mask uint8 [N] or None,
    mode code, offs / rso int32 [B + 1] (the atoms and the residue rows of every structure), B"""
    if mode not in MODES:
        raise ValueError(f"mode must be 'all', 'inter' or 'intra', got {mode!r}")
    perm, roff, R = _residue_order(res_of_atom, N, "res_of_atom")
    res = _lib.host(res_of_atom).reshape(-1).astype(np.int32)
    chain = None
    if chain_of_atom is not None:
        c = _lib.host(chain_of_atom).reshape(-1)
        if c.size != N or not np.issubdtype(c.dtype, np.integer) or (c.size and (c.min() < -2 ** 31 or c.max() >= 2 ** 31)):
            raise ValueError(f"chain_of_atom must be {N} int32 chain numbers, got {c.dtype} [{c.size}]")
        chain = c.astype(np.int32)
    elif mode != "all":
        raise ValueError(f"mode={mode!r} needs chain_of_atom")
    mask = None
    if sel is not None:
        s, _ = _selection(sel, N, "sel")
        mask = np.zeros(N, np.uint8)
        mask[s] = 1
    sizes = [N] if sizes is None else [int(v) for v in np.asarray(_lib.host(sizes)).reshape(-1)]
    if not sizes or min(sizes) < 1 or sum(sizes) != N:
        raise ValueError(f"sizes must be positive atom counts that add up to {N}, got {sizes if len(sizes) <= 8 else sizes[:8] + ['...']}")
    offs = _lib.offsets(sizes)
    B = len(sizes)
    s_atom = np.searchsorted(offs, np.arange(N), "right") - 1
    s_res = s_atom[perm[roff[:-1]]]
    if np.any(s_atom != s_res[res]) or np.any(np.diff(s_res) < 0):
        raise ValueError("res_of_atom: with sizes, the residue rows must be numbered structure after structure, none shared")
    rso = np.searchsorted(s_res, np.arange(B + 1), "left").astype(np.int32)
    return dict(res=res, perm=perm, roff=roff, R=R, chain=chain, mask=mask, mode=MODES[mode], offs=offs, rso=rso, B=B)


def _radius(r_incl, scale):
    thr, sc = _cutoff(r_incl, scale)
    with np.errstate(over="ignore", divide="ignore"):
        q = np.float32(thr) / np.float32(sc)
    if not thr > 0 or not (np.isfinite(q) and q > 0):
        raise ValueError(f"r_incl must be positive (and r_incl / scale a float32), got {r_incl!r}, {scale!r}")
    return thr, sc


def _list(pairs, N):
    """(offsets, j, d, K) of a pairs= argument, shapes checked (the values are checked on the device)"""
    if not (isinstance(pairs, (tuple, list)) and len(pairs) == 3):
        raise ValueError("pairs must be the (offsets, j, d_ref) of reference_pairs")
    off, j, d = pairs
    K = int(j.shape[0]) if len(j.shape) == 1 else -1
    if tuple(off.shape) != (N + 1,) or K < 0 or tuple(d.shape) != (K,):
        raise ValueError(f"pairs must be offsets [{N + 1}], j [K] and d_ref [K], got {list(off.shape)}, {list(j.shape)}, {list(d.shape)}")
    if K > MAX_ENTRIES:
        raise ValueError(f"{K} reference pairs: at most 2**30 per call")
    return off, j, d, K


def _count_and_fill(side, h, N, tp, yd, thr, sc):
    """the two calls of the list: the count (K), then the fill into arrays of K entries. (offsets, j, d, K) on the call's side, rows in
    the order of the fill pass."""
    lib = _lib.load()
    rd, cd, md = side.put(tp["res"], np.int32), (None if tp["chain"] is None else side.put(tp["chain"], np.int32)), \
        (None if tp["mask"] is None else side.put(tp["mask"], np.uint8))
    off = side.empty((N + 1,), np.int64)
    n = np.zeros(1, np.int64)

    def call(cap, j, d):
        _lib.check(lib.pesto_lddt_pairs(h, N, tp["B"], tp["offs"].ctypes.data, side.ptr(yd), side.ptr(rd), side.ptr(cd), side.ptr(md), tp["mode"], thr, sc,
                                        cap, side.ptr(off), side.ptr(j), side.ptr(d), n.ctypes.data_as(_lib.ctypes.POINTER(_lib.ctypes.c_int64)),
                                        side.kind, side.stream), lib.pesto_lddt_last_error)
    try:
        call(0, None, None)
    except _lib.PestoError as e:
        if int(n[0]) > MAX_ENTRIES:
            raise ValueError(f"{int(n[0])} reference pairs: at most 2**30 per call") from e
        raise
    K = int(n[0])
    j, d = side.empty((K,), np.int32), side.empty((K,), np.float32)
    if K:
        call(K, j, d)
    return off, j, d, K


def reference_pairs(xyz_ref, res_of_atom, chain_of_atom=None, mode="all", sel=None, r_incl=15.0, scale=10.0, sizes=None, model=None):
    """(offsets int64 [N + 1], j int32 [K], d_ref float32 [K]): the reference pairs of the module's definition in the caller's atom
    numbering - row i = offsets[i]:offsets[i + 1] holds atom i's partners j, ascending, with d_ref(i, j). The rows are sorted on the way
    out (the list the kernels make is in the cell grid's order). Pass the result as lddt(pairs=...) to skip the set-up."""
    y, N = _reference(xyz_ref)
    tp = _topology(N, res_of_atom, chain_of_atom, mode, sel, sizes)
    thr, sc = _radius(r_incl, scale)
    model = _model_of(model, y)
    side = _lib.Side(y, model._gpu)
    off, j, d, K = _count_and_fill(side, model.handle, N, tp, side.put(y, np.float32), thr, sc)
    if K:
        if side.device is None:
            order = np.lexsort((j, np.repeat(np.arange(N), np.diff(off))))
        else:
            import torch
            rows = torch.repeat_interleave(torch.arange(N, device=side.device), off[1:] - off[:-1])
            order = torch.argsort(rows * N + j.long())
        j, d = j[order], d[order]
    return side.result(off), side.result(j), side.result(d)


def lddt(xyz_ref, xyz, res_of_atom, chain_of_atom=None, mode="all", sel=None, thresholds=(0.5, 1, 2, 4), r_incl=15.0, scale=10.0, sizes=None,
         pairs=None, model=None):
    """Lddt(score float32 [F], residue float32 [F, R], preserved int32 [F, R, T], total int32 [R], n_pairs int) of the F frames xyz
    against xyz_ref: see the module's definition. With sizes= (B structures back to back, one frame) score is float32 [B] and n_pairs
    int64 [B]. pairs=: the result of reference_pairs for the same atoms (chain_of_atom, mode, sel and r_incl are then not used, and xyz_ref
    only for its shape), so the call is the scoring launch alone."""
    y, N = _reference(xyz_ref)
    x = _decoys(xyz, N)
    F = int(x.shape[0])
    if sizes is not None and F != 1:
        raise ValueError(f"with sizes, xyz holds one model of every structure: [N, 3] or [1, N, 3], got {F} frames")
    t32 = _thresholds(thresholds)
    T = int(t32.size)
    given = pairs is not None
    tp = _topology(N, res_of_atom, None if given else chain_of_atom, "all" if given else mode, None if given else sel, sizes)
    thr, sc = _radius(r_incl, scale)
    R, B = tp["R"], tp["B"]
    if F * R * T > 2 ** 36:
        raise ValueError(f"F * R * T = {F} * {R} * {T} counts do not fit one call: pass the frames in batches")
    off = j = d = None
    K = 0
    if given:
        off, j, d, K = _list(pairs, N)
    model = _model_of(model, x)
    h = model.handle
    side = _lib.Side(x, model._gpu)
    xd = side.put(x, np.float32)
    yd = None if given else side.put(y, np.float32)
    rd, pd, od = side.put(tp["res"], np.int32), side.put(tp["perm"], np.int32), side.put(tp["roff"], np.int32)
    cd = None if tp["chain"] is None else side.put(tp["chain"], np.int32)
    md = None if tp["mask"] is None else side.put(tp["mask"], np.uint8)
    if given:
        off, j, d = side.put(off, np.int64), side.put(j, np.int32), side.put(d, np.float32)
    score, residue = side.empty((F, B), np.float32), side.empty((F, R), np.float32)
    preserved, total = side.empty((F, R, T), np.int32), side.empty((R,), np.int32)
    n_pairs = np.zeros(B, np.int64)
    lib = _lib.load()
    try:
        _lib.check(lib.pesto_lddt(h, F, N, B, tp["offs"].ctypes.data, tp["rso"].ctypes.data, side.ptr(yd), side.ptr(xd), R, side.ptr(rd), side.ptr(pd),
                                  side.ptr(od), side.ptr(cd), side.ptr(md), tp["mode"], T, t32.ctypes.data, thr, sc, K, side.ptr(off), side.ptr(j),
                                  side.ptr(d), side.ptr(score), side.ptr(residue), side.ptr(preserved), side.ptr(total), n_pairs.ctypes.data,
                                  side.kind, side.stream), lib.pesto_lddt_last_error)
    except _lib.PestoError as e:
        if int(n_pairs[0]) > MAX_ENTRIES:               # (the refusal after the count pass leaves K there)
            raise ValueError(f"{int(n_pairs[0])} reference pairs: at most 2**30 per call; lower r_incl, or select fewer atoms") from e
        raise
    score, residue, preserved, total = (side.result(v) for v in (score, residue, preserved, total))
    if sizes is None:
        return Lddt(score.reshape(F), residue, preserved, total, int(n_pairs[0]))
    return Lddt(score.reshape(B), residue, preserved, total, n_pairs)


def ilddt(xyz_ref, xyz, res_of_atom, chain_of_atom, **kw):
    """lddt over the pairs between different chains (mode="inter"): every residue's share of preserved inter-chain distances, NaN away
    from the interface."""
    return lddt(xyz_ref, xyz, res_of_atom, chain_of_atom, mode="inter", **kw)


def lddt_ca(xyz_ref, xyz, res_of_atom, ca, **kw):
    """lddt with sel set to the CA mask ``ca`` [N] (or the CA atoms' indices)."""
    if "sel" in kw:
        raise ValueError("lddt_ca selects the CA atoms itself: pass ca, not sel")
    return lddt(xyz_ref, xyz, res_of_atom, sel=ca, **kw)


# ------------------------------------------------------------------ two structures
def _structure_dict(item):
    """the structure dict (with 'chain_name') of a path, a Structure, a dict or a dict of subunits. A path is read by structure_io and
    loses water and hydrogens as the package's cleaning drops them (resname HOH / DOD, element H / D; of alternate locations the first) -
    but it KEEPS the file's residue numbers and insertion codes: structure_io's clean step renumbers the residues 1, 2, 3, ... in
    the order met, which would pair residue k of one file with residue k of the other whatever their numbers."""
    from .structure_io import Structure
    if isinstance(item, (str, bytes, os.PathLike)):
        d = Structure.read_pdb(os.fspath(item)).to_dict()
        keep = ~(np.isin(d["resname"], ("HOH", "DOD")) | np.isin(d["element"], ("H", "D")))
        return {k: v[keep] for k, v in d.items()}
    if isinstance(item, Structure):
        return item.to_dict()
    if not isinstance(item, dict) or not item:
        raise ValueError("a structure is a path, a Structure, a dict with 'xyz', 'name' and 'resid', or a dict of such subunits")
    if "xyz" in item and not isinstance(item["xyz"], dict):
        parts = [dict(item)]
        if "chain_name" not in item:
            parts[0]["chain_name"] = np.full(np.asarray(item["xyz"]).reshape(-1, 3).shape[0], "")
    else:
        parts = [dict(su, chain_name=np.full(np.asarray(su["xyz"]).reshape(-1, 3).shape[0], str(cn))) for cn, su in item.items()]
    for p in parts:
        if not all(k in p for k in ("xyz", "name", "resid")):
            raise ValueError("a structure needs 'xyz', 'name' and 'resid'")
    keys = ["xyz", "name", "resid", "chain_name"] + [k for k in ("resname", "icode") if all(k in p for p in parts)]
    return {k: np.concatenate([np.asarray(p[k]).reshape((-1, 3) if k == "xyz" else (-1,)) for p in parts]) for k in keys}


def match_atoms(reference, predicted):
    """The host-side matching of structure_lddt. Both arguments as structure_lddt takes them. Residues are matched by the numbers the
    two structures carry: a path keeps its file's numbering, while a Structure or a dict is taken as it is - one that went through
    structure_io's preprocess() has been renumbered 1, 2, 3, ... and matches another only if both hold the same residues.
    Returns (xyz_ref float32 [N, 3], xyz float32 [1, N, 3], res_of_atom int32 [N], chain_of_atom int32 [N], table): the reference's
    atoms in its own order; the model's atom with the same (chain, residue number, insertion code where both have one, atom name) under
    each, NaN where the model lacks it (of duplicates the first counts); model atoms that the reference lacks are dropped. table: dict
    of chain_name, resid (and resname, icode) of the R residue rows, in the reference's order of first appearance."""
    return _matched(reference, predicted)[:5]


def _matched(reference, predicted):
    """match_atoms' five results and the reference atoms' names"""
    a, b = _structure_dict(reference), _structure_dict(predicted)
    icode = "icode" in a and "icode" in b

    def keys(s):
        cols = [np.asarray(s["chain_name"]).astype(str), np.asarray(s["resid"]).astype(np.int64).astype(str), np.asarray(s["name"]).astype(str)]
        if icode:
            cols.insert(2, np.asarray(s["icode"]).astype(str))
        return list(zip(*cols))
    ka, kb = keys(a), keys(b)
    N = len(ka)
    if N < 1:
        raise ValueError("the reference has no atoms")
    where = {}
    for n, k in enumerate(kb):
        where.setdefault(k, n)
    src = np.array([where.get(k, -1) for k in ka], np.int64)
    xb = np.asarray(b["xyz"], np.float32).reshape(-1, 3)
    x = np.full((1, N, 3), np.nan, np.float32)
    x[0, src >= 0] = xb[src[src >= 0]]
    rows, first, res = {}, [], np.zeros(N, np.int32)
    for n, k in enumerate(ka):
        if k[:-1] not in rows:
            rows[k[:-1]] = len(rows)
            first.append(n)
        res[n] = rows[k[:-1]]
    first = np.array(first, np.int64)
    chains = {}
    chain = np.array([chains.setdefault(k[0], len(chains)) for k in ka], np.int32)
    table = {"chain_name": np.asarray(a["chain_name"]).astype(str)[first], "resid": np.asarray(a["resid"]).astype(np.int64)[first]}
    if "resname" in a:
        table["resname"] = np.asarray(a["resname"]).astype(str)[first]
    if icode:
        table["icode"] = np.asarray(a["icode"]).astype(str)[first]
    return np.ascontiguousarray(np.asarray(a["xyz"], np.float32).reshape(-1, 3)), x, res, chain, table, np.asarray(a["name"]).astype(str)


def structure_lddt(reference, predicted, mode="all", ca_only=False, thresholds=(0.5, 1, 2, 4), r_incl=15.0, model=None):
    """(Lddt, table): lDDT of the structure ``predicted`` against ``reference``. Each is a PDB path (read by structure_io, water and
    hydrogens dropped, the file's residue numbers kept), a structure_io.Structure, a structure dict or a dict of subunits, in angstroms
    (scale 1). Atoms are matched on the host (match_atoms) by chain, residue number, insertion code and atom name: reference atoms that
    the model lacks enter as NaN and preserve nothing, model atoms that the reference lacks are dropped. ca_only: score the CA atoms
    alone. ``table`` names the R residue rows of the reference (chain_name, resid, resname, icode), in the order of residue[0]; a row
    without any pair (total 0) is NaN there. ``model`` lends a device handle."""
    y, x, res, chain, table, names = _matched(reference, predicted)
    sel = None
    if ca_only:
        sel = names == "CA"
    return lddt(y, x, res, chain, mode, sel, thresholds, r_incl, 1.0, model=model), table
