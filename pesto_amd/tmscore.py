"""TM-score and GDT scoring of models and frames on the GPU (Zhang and Skolnick 2004; Zemla 2003): how much of a model, or of every frame
of an MD run, superposes onto the reference, maximised over superpositions.

The package compared a structure with its reference after ONE fit (trajectory.rmsd, docking.irmsd, dockq.lrmsd, dockq.fit_rmsd), through
contacts (fnat, dockq) and without any fit (lddt). A model with one domain displaced gets a large RMSD and a low score under that one
global fit; the global fold measures that CASP, CAMEO and the AlphaFold literature report next to lDDT search over superpositions and
report the best one (pesto_tmscore.hip):
    tm_score             TMScore(tm, gdt_ts, gdt_ha, counts, rmsd, seed, rotation, translation) of F frames against one reference
    gdt                  GDT(gdt_ts, gdt_ha, counts) alone
    tm_ca                tm_score over the CA atoms
    structure_tmscore    two structures or two PDB paths, atoms matched on the host as structure_lddt matches them
    seed_windows         the (start, length) of every seed number, to read ``seed`` by; default_d0: the d0 formula
This is for a GIVEN residue correspondence: model and reference share the atom order, and ``sel`` names the L atoms scored, normally the
CA atoms, IN SEQUENCE ORDER (indices in that order, or a mask). Conventions are those of docking.py: xyz_ref is [N, 3] or [1, N, 3], xyz
float32 [F, N, 3], scale multiplies distances (mdtraj keeps nanometres: the default 10 gives angstroms). The lead argument decides where a
call runs (_lib.Side): NumPy in, NumPy out; ROCm tensors in, ROCm tensors out on torch's current stream. ``model`` lends its device handle.
There is no CPU or PyTorch fallback. Arguments are checked on the host before any launch (ValueError); sel is checked again by a kernel
whose verdict is read before anything is written.

Definition. Everything is in double from the float32 inputs. Under a fit, x' the model moved by it, d_i = sqrt(|x'_i - y_i|^2) * scale.
    d0            max(0.5, 1.24 * cbrt(max(L_norm - 15, 0)) - 1.8); L_norm defaults to L; norm_len= and d0= override them
    d_search      min(8, max(4.5, d0))
    TM(fit)       (sum_i 1 / (1 + (d_i / d0)^2)) / L_norm
    count_c(fit)  the number of i with d_i < c, for the GDT cut-offs c = 0.5, 1, 2, 4, 8
    seeds         windows of the sequence: the lengths n_k = L >> k for k = 0 .. 5 while n_k > 4, then one last length min(L, 4); the
                  starts 0, step, 2 step, ... <= L - n, plus L - n if that was not hit (step >= 1, default 1). Seeds are numbered in
                  that order: length first, then start.
    one search    S = the window; up to n_iter (20) times: fit the model onto the reference on S (the fit of pesto_fit.h; point sets
                  that are equal bit for bit are fitted by the identity itself); compute every d_i - this fit is *visited*; with d_cut =
                  d_search form S' = {i: d_i < d_cut}, and while |S'| < min(3, L) raise d_cut by 0.5 and form S' again; stop if S' == S,
                  else S = S'. (A fit that needs more than MAX_RAISE = 4096 raises, 2048 A, ends its seed: no structure does.)
    tm[f]         float32, rounded once: the maximum of TM(fit) over all visited fits of all seeds
    seed[f]       int32: the lowest seed number that attains tm[f]
    rotation[f], translation[f]   float64 [3, 3] and [3]: that seed's (first) best fit x' = (x - m) R + m_ref, stored as R and
                  t = m_ref - m R, so x' = x @ R + t in the input's unit
    counts[f, c]  int32: the maximum of count_c over all visited fits
    gdt_ts[f]     float32(double(c1 + c2 + c4 + c8) / double(4 L)); gdt_ha[f] likewise over (0.5, 1, 2, 4)
    rmsd[f]       dockq.fit_rmsd(xyz_ref, xyz, sel, sel), bit for bit (the same kernel): the RMSD after the ONE global fit
A frame with a non-finite selected coordinate gets NaN scores (and fit), zero counts and seed -1; a non-finite selected reference
coordinate raises ValueError. This is our definition; no bitwise equality with Zhang's TMscore program is claimed (it shares d0, the
window seeds and the iterated refit, not the program's schedule of cut-offs). Every output is bit-identical from call to call, between host
and device inputs, and between a frame scored alone and in a batch.

Ragged batch. sizes= (atom counts, as in lddt.py) lays B structures back to back in xyz_ref and xyz, one model each; sel is grouped by
structure; L, d0 and the seeds are per structure (norm_len= and d0= take one value or B), and every output has one entry per structure.

Not built: MaxSub, mass weighting. (The correspondence is given here; structalign.py searches for it and has the pairwise TM matrix;
chainmap.py finds the chain permutation of an oligomer and puts the model's chains in the reference's order first.)

Limits: 3 <= L <= MAX_LENGTH = 4096 per structure, F <= 2**23, N < 2**30, n_iter <= 1024. Every excess raises ValueError.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from .dockq import _decoys, _reference
from .trajectory import _model_of, _selection

MAX_FRAMES = 2 ** 23            # PESTO_TMSCORE_MAX_FRAMES
MAX_LENGTH = 4096               # PESTO_TMSCORE_MAX_LENGTH
MAX_ITER = 1024                 # PESTO_TMSCORE_MAX_ITER
MAX_RAISE = 4096                # PESTO_TMSCORE_MAX_RAISE
GDT_CUTOFFS = (0.5, 1.0, 2.0, 4.0, 8.0)

TMScore = namedtuple("TMScore", "tm gdt_ts gdt_ha counts rmsd seed rotation translation")
GDT = namedtuple("GDT", "gdt_ts gdt_ha counts")


def default_d0(norm_len):
    """float64: max(0.5, 1.24 * cbrt(max(L_norm - 15, 0)) - 1.8)"""
    n = np.asarray(norm_len, np.float64)
    return np.maximum(0.5, 1.24 * np.cbrt(np.maximum(n - 15.0, 0.0)) - 1.8)


def seed_windows(L, step=1):
    """int64 [n_seeds, 2]: (start, length) of every seed of a structure of L atoms, in the order of their numbers"""
    L, step = int(L), int(step)
    if L < 3 or step < 1:
        raise ValueError(f"L >= 3 and step >= 1 expected, got {L}, {step}")
    lengths = []
    for k in range(6):
        if (L >> k) <= 4:
            break
        lengths.append(L >> k)
    lengths.append(min(L, 4))
    out = []
    for n in lengths:
        starts = list(range(0, L - n + 1, step))
        if starts[-1] != L - n:
            starts.append(L - n)
        out += [(s, n) for s in starts]
    return np.array(out, np.int64)


def _per_structure(value, B, name, default):
    """float64 [B] of an argument that is one value or one per structure (None: default); positive and finite"""
    if value is None:
        return np.ascontiguousarray(default, np.float64)
    v = np.asarray(_lib.host(value), np.float64).reshape(-1)
    if v.size == 1:
        v = np.repeat(v, B)
    if v.size != B or not np.all(np.isfinite(v)) or not np.all(v > 0):
        raise ValueError(f"{name} must be positive and finite, one value or one per structure ({B}), got {value!r}")
    return np.ascontiguousarray(v)


def _layout(sel, N, sizes):
    """(sel int32 [n], offsets int32 [B + 1] into it, B) of the atoms scored, grouped by structure"""
    s, _ = _selection(sel, N, "sel")
    if s is None:
        s = np.arange(N, dtype=np.int32)
    sizes = [N] if sizes is None else [int(v) for v in np.asarray(_lib.host(sizes)).reshape(-1)]
    if not sizes or min(sizes) < 1 or sum(sizes) != N:
        raise ValueError(f"sizes must be positive atom counts that add up to {N}, got {sizes if len(sizes) <= 8 else sizes[:8] + ['...']}")
    B = len(sizes)
    offs = _lib.offsets(sizes)
    which = np.searchsorted(offs, s, "right") - 1
    if np.any(np.diff(which) < 0):
        raise ValueError("sel: with sizes, the atoms must be grouped structure after structure")
    so = np.searchsorted(which, np.arange(B + 1), "left").astype(np.int32)
    L = np.diff(so)
    if L.min() < 3 or L.max() > MAX_LENGTH:
        b = int(np.argmax((L < 3) | (L > MAX_LENGTH)))
        raise ValueError(f"sel must name 3 to {MAX_LENGTH} atoms of every structure, got {int(L[b])}" + (f" in structure {b}" if B > 1 else ""))
    return np.ascontiguousarray(s, np.int32), so, B


def tm_score(xyz_ref, xyz, sel=None, *, sizes=None, norm_len=None, d0=None, step=1, n_iter=20, scale=10.0, model=None):
    """TMScore(tm float32 [F], gdt_ts float32 [F], gdt_ha float32 [F], counts int32 [F, 5], rmsd float32 [F], seed int32 [F], rotation
    float64 [F, 3, 3], translation float64 [F, 3]) of the F frames xyz against xyz_ref on the atoms sel (in sequence order; default all):
    see the module's definition. With sizes= (B structures back to back, one model each) every output has B entries."""
    y, N = _reference(xyz_ref)
    x = _decoys(xyz, N)
    F = int(x.shape[0])
    if sizes is not None and F != 1:
        raise ValueError(f"with sizes, xyz holds one model of every structure: [N, 3] or [1, N, 3], got {F} frames")
    s, so, B = _layout(sel, N, sizes)
    ln = _per_structure(norm_len, B, "norm_len", np.diff(so))
    dz = _per_structure(d0, B, "d0", default_d0(ln))
    if isinstance(step, bool) or isinstance(n_iter, bool) or step != int(step) or n_iter != int(n_iter) or not 1 <= step < 2 ** 31 or not 1 <= n_iter <= MAX_ITER:
        raise ValueError(f"step >= 1 and 1 <= n_iter <= {MAX_ITER} (integers) expected, got {step!r}, {n_iter!r}")
    sc = float(scale)
    if not (np.isfinite(sc) and sc > 0):
        raise ValueError(f"scale must be positive and finite, got {scale!r}")
    if _lib.is_torch(y):
        import torch
        finite = bool(torch.isfinite(y[0][torch.from_numpy(s.astype(np.int64)).to(y.device)]).all())
    else:
        finite = bool(np.isfinite(y[0][s]).all())
    if not finite:
        raise ValueError("xyz_ref: a selected atom of the reference has a non-finite coordinate")
    model = _model_of(model, x)
    h = model.handle
    side = _lib.Side(x, model._gpu)
    xd, yd, sd = side.put(x, np.float32), side.put(y, np.float32), side.put(s, np.int32)
    U = B if sizes is not None else F
    tm, ts, ha, rmsd = (side.empty((U,), np.float32) for _ in range(4))
    counts, seed = side.empty((U, 5), np.int32), side.empty((U,), np.int32)
    rot, tr = side.empty((U, 3, 3), np.float64), side.empty((U, 3), np.float64)
    lib = _lib.load()
    _lib.check(lib.pesto_tmscore(h, F, N, B, so.ctypes.data, side.ptr(sd), side.ptr(yd), side.ptr(xd), ln.ctypes.data, dz.ctypes.data, int(step),
                                 int(n_iter), sc, side.ptr(tm), side.ptr(ts), side.ptr(ha), side.ptr(counts), side.ptr(rmsd), side.ptr(seed),
                                 side.ptr(rot), side.ptr(tr), side.kind, side.stream), lib.pesto_tmscore_last_error)
    return TMScore(*(side.result(v) for v in (tm, ts, ha, counts, rmsd, seed, rot, tr)))


def gdt(xyz_ref, xyz, sel=None, **kw):
    """GDT(gdt_ts float32 [F], gdt_ha float32 [F], counts int32 [F, 5]): the two GDT scores of tm_score and the counts under
    (0.5, 1, 2, 4, 8) A they are made of."""
    out = tm_score(xyz_ref, xyz, sel, **kw)
    return GDT(out.gdt_ts, out.gdt_ha, out.counts)


def tm_ca(xyz_ref, xyz, names, **kw):
    """tm_score over the CA atoms: names [N] holds the atom names (the atoms must be in sequence order)."""
    if "sel" in kw:
        raise ValueError("tm_ca selects the CA atoms itself: pass names, not sel")
    n = np.asarray(_lib.host(names)).reshape(-1).astype(str)
    return tm_score(xyz_ref, xyz, np.char.strip(n) == "CA", **kw)


def structure_tmscore(reference, predicted, model=None, **kw):
    """(TMScore, table): the CA TM-score and GDT of the structure ``predicted`` against ``reference``. Each is a PDB path, a
    structure_io.Structure, a structure dict or a dict of subunits, in angstroms (scale 1), matched on the host by lddt.match_atoms'
    matcher: chain, residue number, insertion code and atom name. Scored are the reference's CA atoms that the model has too, in the
    reference's order, and the scores are normalised by the number of the reference's CA atoms (as TMscore normalises by the native's
    length) unless norm_len= says otherwise; GDT counts over the matched atoms. ``table``: chain_name and resid of the scored residues,
    and n_ref."""
    from .lddt import _matched
    if "sel" in kw or "sizes" in kw or "scale" in kw:
        raise ValueError("structure_tmscore selects the matched CA atoms itself, in angstroms: sel, sizes and scale are not taken")
    y, x, res, _, table, names = _matched(reference, predicted)
    ca = np.char.strip(names) == "CA"
    sel = np.nonzero(ca & np.isfinite(x[0]).all(1))[0]
    kw.setdefault("norm_len", int(ca.sum()) if ca.any() else None)
    if sel.size < 3:
        raise ValueError(f"the two structures share {sel.size} CA atoms: a superposition needs at least 3")
    out = tm_score(y, x, sel, scale=1.0, model=model, **kw)
    rows = res[sel]
    return out, {"chain_name": table["chain_name"][rows], "resid": table["resid"][rows], "n_ref": int(ca.sum())}
