"""Interface patches on the GPU: spatially connected residues predicted to be an interface of one class, or of two classes at once.

The reference's interfaceome pipeline (interfaceome/cluster_interfaces.py, cluster_multi_interfaces.py, used again by
selecting_alphafold_models.ipynb) builds, per protein and per class (or class pair), a dense NumPy distance matrix over the selected
residues' CA atoms and grows each connected component with Python sets (follow_rabbits). Here one launch (pesto_interface_patches) does it
for a whole batch of structures and all selections:
    interface_patches_batch / interface_patches   the reference's output: {label: [[rows], ...]} (pairs=True) or [[[rows], ...]] * 5
    patch_labels                                  the raw per-row outputs (device tensors stay on the device)
    residue_ca                                    CA coordinates per residue row, in Structure.encode's numbering
    save_patches                                  clustered_interfaces.json / clustered_multi_interfaces.json in the reference's layout
Definition, for a selection (i, j), i <= j (cluster_interfaces uses (i, i), cluster_multi_interfaces every pair):
    node r      afs[r] > afs_thr & has_ca[r] & p[r,i] > p_thr & p[r,j] > p_thr      (float32, strict; NaN never passes; no afs: no test)
    edge (a,b)  NumPy's float32 sqrt((dx*dx + dy*dy) + dz*dz) < d_thr
    patches     connected components, in the order of their smallest member (follow_rabbits' order); members ascending
Members are residue rows of p (the model's output rows); a residue without a CA atom is never a node.
"""
import json
import os

import numpy as np

from . import _lib

LABELS = ["protein", "dna/rna", "ion", "ligand", "lipid"]       # interfaceome/cluster_multi_interfaces.py:38
AFS_THR, P_THR, D_THR = 70.0, 0.5, 10.0                         # main() of both scripts
SMALL_MAX = 4096        # PESTO_PATCHES_SMALL_MAX: structures of more rows take the large-structure path (node-pair tiles over many workgroups)
MAX_SEL = 1024
FORCE_LARGE = 1         # PESTO_PATCHES_FORCE_LARGE


def selections(n_labels=len(LABELS), pairs=True):
    """The reference's loop order: (i, i) for i < n (pairs=False), or (i, j) for i = 0..n-1, j = i..n-1 (pairs=True)."""
    if pairs:
        return [(i, j) for i in range(n_labels) for j in range(i, n_labels)]
    return [(i, i) for i in range(n_labels)]


def selection_keys(labels=LABELS, pairs=True):
    """cluster_multi_interfaces' keys: labels[i] for i == j, else 'labels[i]+labels[j]'."""
    return [labels[i] if i == j else f"{labels[i]}+{labels[j]}" for i, j in selections(len(labels), pairs)]


def _validate(ps, xyzs, afss, has_ca, n_sel, d_thr):
    if not isinstance(ps, (list, tuple)) or not ps:
        raise ValueError("ps must be a non-empty list of [R_s, C] probability tables")
    if len(xyzs) != len(ps) or (afss is not None and len(afss) != len(ps)) or (has_ca is not None and len(has_ca) != len(ps)):
        raise ValueError("ps, xyzs, afss and has_ca must be lists of the same length")
    d = float(d_thr)
    if not (0 < d <= float(np.finfo(np.float32).max)) or not np.float32(d) > 0:      # (checked in double first: no float32 overflow)
        raise ValueError(f"d_thr must be a positive finite distance, got {d_thr!r}")
    if not 1 <= n_sel <= MAX_SEL:
        raise ValueError(f"1 to {MAX_SEL} selections, got {n_sel}")
    C = None
    sizes = []
    for s, p in enumerate(ps):
        shp = tuple(p.shape)
        if len(shp) != 2 or shp[0] < 1 or shp[1] < 1:
            raise ValueError(f"structure {s}: p must be [R >= 1, C], got {shp}")
        if C is None:
            C = shp[1]
        elif shp[1] != C:
            raise ValueError(f"structure {s}: p has {shp[1]} classes, the first structure {C}")
        if tuple(xyzs[s].shape) != (shp[0], 3):
            raise ValueError(f"structure {s}: xyz must be [{shp[0]}, 3], got {tuple(xyzs[s].shape)}")
        if afss is not None and afss[s] is not None and tuple(afss[s].shape) != (shp[0],):
            raise ValueError(f"structure {s}: afs must be [{shp[0]}], got {tuple(afss[s].shape)}")
        if has_ca is not None and has_ca[s] is not None and tuple(has_ca[s].shape) != (shp[0],):
            raise ValueError(f"structure {s}: has_ca must be [{shp[0]}], got {tuple(has_ca[s].shape)}")
        sizes.append(shp[0])
    if afss is not None and any(a is None for a in afss) and not all(a is None for a in afss):
        raise ValueError("afss: give a confidence array for every structure or for none")
    return C, sizes


def patch_labels(model, ps, xyzs, afss=None, has_ca=None, sel=None, afs_thr=AFS_THR, p_thr=P_THR, d_thr=D_THR, force_large=False):
    """pesto_interface_patches on a batch: returns (patch_of [n_sel, R] int32, n_patches [S, n_sel] int32, patch_size [n_sel, R] int32,
    patch_mean [n_sel, R, 2] float32, offsets [S + 1] numpy) with R the rows of all structures (structure s: rows offsets[s]:offsets[s+1]).
    patch_of: the patch number within (structure, selection), -1 off the nodes; size and mean (of p[:, i], p[:, j]) at each patch's
    smallest member row. sel: [(i, j)] (default: every pair of the classes). ps[0] decides where the call runs: ROCm tensors run on the
    device buffers (device pointers, torch's current stream; the other arrays are copied to its GPU where needed; the results are ROCm
    tensors); numpy arrays / CPU tensors are staged (numpy results)."""
    n_class = int(ps[0].shape[1]) if ps and len(ps[0].shape) == 2 else 0
    sel = selections(n_class, True) if sel is None else [tuple(int(v) for v in ij) for ij in sel]
    C, sizes = _validate(ps, xyzs, afss, has_ca, len(sel), d_thr)
    for i, j in sel:
        if not 0 <= i <= j < C:
            raise ValueError(f"selection ({i}, {j}): need 0 <= i <= j < {C}")
    if afss is not None and afss[0] is None:
        afss = None
    if has_ca is not None and any(h is None for h in has_ca):
        if not all(h is None for h in has_ca):
            has_ca = [np.ones(n, np.uint8) if h is None else h for h, n in zip(has_ca, sizes)]
        else:
            has_ca = None
    offs = _lib.offsets(sizes)
    R, S, K = int(offs[-1]), len(ps), len(sel)
    if R * max(C, K) >= 2 ** 31:
        raise ValueError(f"too many rows ({R}) for {C} classes and {K} selections")
    sel_a = np.ascontiguousarray(np.asarray(sel, np.int32).reshape(K, 2))
    h = model.handle
    side = _lib.Side(ps[0], model._gpu)
    p = side.cat(ps, np.float32)
    x = side.cat(xyzs, np.float32)
    a = side.cat(afss, np.float32) if afss is not None else None
    c = side.cat([q != 0 for q in has_ca], np.uint8) if has_ca is not None else None
    po, psz = side.empty((K, R), np.int32), side.empty((K, R), np.int32)
    npch = side.empty((S, K), np.int32)
    pm = side.empty((K, R, 2), np.float32)
    lib = _lib.load()
    _lib.check(lib.pesto_interface_patches(h, S, offs.ctypes.data, C, side.ptr(x), side.ptr(p), side.ptr(a), side.ptr(c), K, sel_a.ctypes.data,
                                           float(afs_thr), float(p_thr), float(d_thr), side.ptr(po), side.ptr(npch), side.ptr(psz),
                                           side.ptr(pm), FORCE_LARGE if force_large else 0, side.kind, side.stream),
               lib.pesto_patches_last_error)
    return po, npch, psz, pm, offs


def _lists(patch_of, n_patches, patch_size, patch_mean, offs, with_stats):
    """per structure, per selection: [[rows ascending], ...] in patch order (and (sizes [n], means [n, 2]))"""
    out, stats = [], []
    for s in range(offs.size - 1):
        r0, r1 = int(offs[s]), int(offs[s + 1])
        per, per_st = [], []
        for k in range(patch_of.shape[0]):
            lab = patch_of[k, r0:r1]
            npk = int(n_patches[s, k])
            rows = np.nonzero(lab >= 0)[0]
            order = np.argsort(lab[rows], kind="stable")
            members = rows[order]
            cuts = np.cumsum(np.bincount(lab[rows], minlength=npk))[:-1]
            per.append([m.tolist() for m in np.split(members, cuts)] if npk else [])
            if with_stats:
                first = members[np.r_[0, cuts]] if npk else np.zeros(0, np.int64)       # each patch's smallest member, in patch order
                per_st.append((patch_size[k, r0 + first].astype(np.int32), patch_mean[k, r0 + first].astype(np.float32)))
        out.append(per)
        stats.append(per_st)
    return out, stats


def interface_patches_batch(model, ps, xyzs, afss=None, has_ca=None, pairs=True, afs_thr=AFS_THR, p_thr=P_THR, d_thr=D_THR, labels=LABELS,
                            return_stats=False, force_large=False):
    """Interface patches of a list of structures in ONE launch. ps [R_s, C >= len(labels)] probabilities, xyzs [R_s, 3] CA coordinates,
    afss [R_s] confidences (AlphaFold pLDDT) or None, has_ca [R_s] (0: no CA, never a node) or None. Per structure: pairs=True ->
    {key: [[rows], ...]} with cluster_multi_interfaces' 15 keys in its order; pairs=False -> cluster_interfaces' list of 5 lists.
    return_stats: also, in the same layout, (sizes int32 [n_patches], means float32 [n_patches, 2]) with the mean of p[:, i] and p[:, j].
    ROCm tensors stay on the device; only the per-row labels come back to the host to build the lists."""
    sel = selections(len(labels), pairs)
    if ps and len(ps[0].shape) == 2 and int(ps[0].shape[1]) < len(labels):
        raise ValueError(f"p has {int(ps[0].shape[1])} classes, {len(labels)} labels need at least as many")
    po, npch, psz, pm, offs = patch_labels(model, ps, xyzs, afss, has_ca, sel, afs_thr, p_thr, d_thr, force_large)
    po, npch, psz, pm = (_lib.host(v) for v in (po, npch, psz, pm))
    lists, stats = _lists(po, npch, psz, pm, offs, return_stats)
    if pairs:
        keys = selection_keys(labels, True)
        lists = [dict(zip(keys, per)) for per in lists]
        stats = [dict(zip(keys, per)) for per in stats]
    return (lists, stats) if return_stats else lists


def _default_model(device=0):
    """A weightless handle: the entry point needs only a device and a stream."""
    from .evaluate import _scoring_model
    return _scoring_model(device)


def interface_patches(p, xyz, afs=None, has_ca=None, model=None, pairs=True, afs_thr=AFS_THR, p_thr=P_THR, d_thr=D_THR, labels=LABELS,
                      return_stats=False, force_large=False):
    """interface_patches_batch for ONE structure (the reference's cluster_interfaces(entry, ...) with pairs=False, cluster_multi_interfaces
    with pairs=True). Without a model the call runs on a weightless handle of p's GPU (GPU 0 for host arrays)."""
    if model is None:
        model = _default_model(p.device.index if _lib.is_torch(p) and p.is_cuda else 0)
    r = interface_patches_batch(model, [p], [xyz], None if afs is None else [afs], None if has_ca is None else [has_ca], pairs, afs_thr,
                                p_thr, d_thr, labels, return_stats, force_large)
    return (r[0][0], r[1][0]) if return_stats else r[0]


def residue_ca(structure):
    """(xyz float32 [R, 3], has_ca uint8 [R], ca_atom int64 [R]) per residue row in Structure.encode's numbering (the model's output
    rows): the coordinates of the residue's first atom named CA of element C (0 and has_ca = 0, ca_atom = -1 where there is none, e.g.
    nucleotides, ions - a calcium ion's atom is also named CA - and ligands). ``structure``: a Structure (as it stands, e.g. preprocessed)
    or the reference's structure dict."""
    from .structure_io import Structure
    s = structure if isinstance(structure, Structure) else Structure.from_dict(structure)
    X, _, roa, R = s.encode(30)
    d = s.to_dict()
    is_ca = (d["name"] == "CA") & (np.char.upper(d["element"].astype(str)) == "C")
    ca_atom = np.full(R, -1, np.int64)
    idx = np.nonzero(is_ca)[0]
    res, first = np.unique(roa[idx], return_index=True)     # the first CA (lowest atom index) of each residue that has one
    ca_atom[res] = idx[first]
    has = ca_atom >= 0
    xyz = np.zeros((R, 3), np.float32)
    xyz[has] = X[ca_atom[has]]
    return xyz, has.astype(np.uint8), ca_atom


def save_patches(path, patches):
    """Write {key: patches} (key: the reference's uniprot id or any name) as JSON in the reference's layout: the pairs=True form gives
    clustered_multi_interfaces.json ({key: {label: [[ids]]}}), the pairs=False form clustered_interfaces.json ({key: [[[ids]]]})."""
    def plain(v):
        if isinstance(v, dict):
            return {str(k): plain(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        return int(v)
    path = os.fspath(path)
    tmp = path + ".tmp"
    with open(tmp, "w") as f:
        json.dump({str(k): plain(v) for k, v in patches.items()}, f)
    os.replace(tmp, path)
    return path
