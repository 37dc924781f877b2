"""Evaluation on the GPU: interface labels of biological assemblies and the reference's binary-classification scores.

The reference measures a prediction in three steps: the true interface of every chain from its assembly (processing/build_dataset.py:176-240,
extract_all_contacts / locate_contacts in src/data_encoding.py:116-176, contacts_types build_dataset.py:38-51, load_interface_labels
in model/save/i_v4_1_2021-09-07_11-21/data_handler.py:9-23 with the classes of config_data, config.py:14-21), the model on the chain alone,
and bc_scoring (src/scoring.py:77-96) - dense torch distance matrices per pair of subunits and sklearn's AUC on the host. Here:
    interface_labels / interface_labels_batch   {subunit: bool [R_s, C]}   (pesto_interface_labels: k_contact_labels, a cell-grid search)
    bc_scoring / bc_scores_batch                [8, C] / [S, 8, C]         (pesto_bc_scores: k_bc_scores, exact counts and pairwise AUC)
    benchmark_assemblies                        PDB assemblies in, per-subunit scores out
The host only turns resnames into per-atom class masks. Label definition, for a subunit s0 of an assembly after the reference's preprocessing:
    y[s0][r, c] = resname(r) in l_types and some atom of r is closer than r_thr (float32 torch.norm) to an atom b of another subunit
                  with resname(b) in r_types[c]
"""
import numpy as np

from . import _lib
from .structure_io import ALL, PestoIOError, Structure

# the residue-name categories of the reference (src/data_encoding.py:31-43) and the interface classes of config_data (config.py:14-21)
CATEG_TO_RESNAMES = {
    "protein": ["GLU", "LEU", "ALA", "ASP", "SER", "VAL", "GLY", "THR", "ARG", "PHE", "TYR", "ILE", "PRO", "ASN", "LYS", "GLN", "HIS",
                "TRP", "MET", "CYS"],
    "rna": ["A", "U", "G", "C"],
    "dna": ["DA", "DT", "DG", "DC"],
    "ion": ["MG", "ZN", "CL", "CA", "NA", "MN", "K", "IOD", "CD", "CU", "FE", "NI", "SR", "BR", "CO", "HG"],
    "ligand": ["SO4", "NAG", "PO4", "EDO", "ACT", "MAN", "HEM", "FMT", "BMA", "ADP", "FAD", "NAD", "NO3", "GLC", "ATP", "NAP", "BGC",
               "GDP", "FUC", "FES", "FMN", "GAL", "GTP", "PLP", "MLI", "ANP", "H4B", "AMP", "NDP", "SAH", "OXY"],
    "lipid": ["PLM", "CLR", "CDL", "RET"],
}
L_TYPES = CATEG_TO_RESNAMES["protein"]
R_TYPES = [CATEG_TO_RESNAMES["protein"], CATEG_TO_RESNAMES["dna"] + CATEG_TO_RESNAMES["rna"], CATEG_TO_RESNAMES["ion"],
           CATEG_TO_RESNAMES["ligand"], CATEG_TO_RESNAMES["lipid"]]
R_THR = 5.0
BC_SCORE_NAMES = ["acc", "ppv", "npv", "tpr", "tnr", "mcc", "auc", "std"]      # src/scoring.py:7
MAX_CLASSES = 32


_scoring_models = {}


def _scoring_model(device=0):
    """A handle for the entry points that need only a device, a stream and a workspace (bc_scoring without a model)."""
    if device not in _scoring_models:
        from .config import CONFIGS
        from .model import Model
        from .weights import blob_size
        m = Model(CONFIGS["i_v4_0"])
        m.load_blob(np.zeros(blob_size(m.config), np.float32))
        _scoring_models[device] = m.to(device)
    return _scoring_models[device]


# ------------------------------------------------------------------ labels
def resname_masks(resnames, l_types=L_TYPES, r_types=R_TYPES):
    """(receptor uint8 [N], partner_mask uint32 [N]) of per-atom resnames: receptor = resname in l_types, bit c = resname in r_types[c]."""
    if not 1 <= len(r_types) <= MAX_CLASSES:
        raise ValueError(f"1 to {MAX_CLASSES} interface classes, got {len(r_types)}")
    rn = np.asarray(resnames).astype(str)
    receptor = np.isin(rn, np.asarray(list(l_types), dtype=str)).astype(np.uint8)
    mask = np.zeros(rn.shape, np.uint32)
    for c, types in enumerate(r_types):
        mask |= np.isin(rn, np.asarray(list(types), dtype=str)).astype(np.uint32) << np.uint32(c)
    return receptor, mask


def contact_labels(model, X, subunit, residue, receptor, partner_mask, sizes, n_res, r_thr=R_THR):
    """pesto_interface_labels on a batch of assemblies (``sizes`` atoms each, concatenated): (labels uint32 [n_res], ties uint8 [N]).
    X decides where the call runs (pesto_amd._lib.Side): a ROCm X runs on the GPU buffers as they are (device pointers, torch's current
    stream; the other arrays are copied to its GPU where needed; labels: the int32 of the uint32 bits); numpy / CPU tensors are staged."""
    h = model.handle
    offs = _lib.offsets(sizes)
    n = int(offs[-1])
    side = _lib.Side(X, model._gpu)
    X = side.put(X, np.float32, (n, 3), "X")
    su = side.put(subunit, np.int32, (n,), "subunit")
    rs = side.put(residue, np.int32, (n,), "residue")
    rc = side.put(receptor, np.uint8, (n,), "receptor")
    pm = side.put(partner_mask, np.uint32, (n,), "partner_mask")
    labels = side.empty((int(n_res),), np.uint32)
    ties = side.empty((n,), np.uint8)
    lib = _lib.load()
    _lib.check(lib.pesto_interface_labels(h, n, len(offs) - 1, offs.ctypes.data, side.ptr(X), side.ptr(su), side.ptr(rs), side.ptr(rc),
                                          side.ptr(pm), int(n_res), float(r_thr), side.ptr(labels), side.ptr(ties), side.kind, side.stream),
               lib.pesto_eval_last_error)
    return labels, ties


def _subunits_of(item):
    if isinstance(item, Structure):
        return item.subunits()
    if isinstance(item, dict) and "xyz" in item and not isinstance(item["xyz"], dict):
        return Structure.from_dict(item).preprocess(ALL).subunits()     # one assembly as the reference's structure dict
    return item


def interface_labels_batch(model, assemblies, r_thr=R_THR, l_types=L_TYPES, r_types=R_TYPES, on_device=False, return_ties=False):
    """interface_labels for a list of assemblies in ONE launch -> [{subunit: bool [R_s, C]}]. An assembly is a preprocessed Structure
    (its subunits() are the subunits), the reference's {name: subunit dict} (xyz, resname, resid) or a raw structure dict (preprocessed here).
    on_device: the per-atom arrays go to the GPU as ROCm tensors first (the device-pointer path). return_ties: also
    [{subunit: bool [R_s]}], the residues with a partner atom at exactly r_thr (float32)."""
    subs = [_subunits_of(a) for a in assemblies]
    X, su, rs, rn, sizes, rows = [], [], [], [], [], []
    n_sub, r_base = 0, 0
    for sd in subs:
        n_a = 0
        for name, s in sd.items():
            xyz = np.asarray(s["xyz"], np.float32).reshape(-1, 3)
            _, res = np.unique(np.asarray(s["resid"]), return_inverse=True)      # encode_structure's residue columns (src/data_encoding.py:73)
            R = int(res.max()) + 1 if res.size else 0
            X.append(xyz); su.append(np.full(xyz.shape[0], n_sub, np.int32)); rs.append(res.astype(np.int32) + r_base)
            rn.append(np.asarray(s["resname"]))
            rows.append((name, r_base, R))
            n_sub += 1; r_base += R; n_a += xyz.shape[0]
        sizes.append(n_a)
    if r_base == 0:
        raise ValueError("no atoms")
    keep = [i for i, n in enumerate(sizes) if n > 0]            # (an assembly without atoms has no subunits)
    receptor, pmask = resname_masks(np.concatenate(rn), l_types, r_types)
    args = [np.concatenate(X), np.concatenate(su), np.concatenate(rs), receptor, pmask]
    if on_device:
        import torch
        dev = torch.device("cuda", model._gpu)
        args = [torch.from_numpy(np.ascontiguousarray(a if a.dtype != np.uint32 else a.view(np.int32))).to(dev) for a in args]
    labels, ties = contact_labels(model, *args, [sizes[i] for i in keep], r_base, r_thr)
    labels, ties = _lib.host(labels).view(np.uint32), _lib.host(ties)
    bits = (labels[:, None] >> np.arange(len(r_types), dtype=np.uint32)[None, :]) & 1
    res_all = np.concatenate(rs)
    tie_res = np.zeros(r_base, bool)
    tie_res[res_all[ties != 0]] = True
    out, out_t, k = [], [], 0
    for sd in subs:
        d, dt = {}, {}
        for _ in sd:
            name, r0, R = rows[k]
            d[name] = bits[r0:r0 + R].astype(bool)
            dt[name] = tie_res[r0:r0 + R]
            k += 1
        out.append(d)
        out_t.append(dt)
    return (out, out_t) if return_ties else out


def interface_labels(model, structure_or_subunits, r_thr=R_THR, l_types=L_TYPES, r_types=R_TYPES):
    """{subunit name: bool [R_s, C]}: the interface labels of every subunit of ONE assembly (see the module docstring)."""
    return interface_labels_batch(model, [structure_or_subunits], r_thr, l_types, r_types)[0]


# ------------------------------------------------------------------ scores
def bc_scores_batch(model, ys, ps):
    """[S, 8, C] float32: bc_scoring of every (y [R_s, C], p [R_s, C]) pair in one launch (rows in BC_SCORE_NAMES order). ps[0] decides
    where the call runs: ROCm tensors stay on the GPU (the other arrays are copied there where needed; result: a ROCm tensor); numpy / CPU
    tensors are staged (result: numpy, or a CPU tensor for CPU tensors)."""
    if len(ys) != len(ps) or not ys:
        raise ValueError("ys and ps must be non-empty lists of the same length")
    h = model.handle
    shp = [tuple(p.shape) if len(p.shape) == 2 else (int(p.shape[0]), 1) for p in ps]
    C = shp[0][1]
    for y, s in zip(ys, shp):
        if s[1] != C or s[0] < 1 or int(y.shape[0]) != s[0] or (int(y.shape[1]) if len(y.shape) == 2 else 1) != C:
            raise ValueError("every y / p pair must be [R_s >= 1, C] with one C")
    offs = _lib.offsets([s[0] for s in shp])
    S = len(ps)
    side = _lib.Side(ps[0], model._gpu)
    p = side.cat([q.reshape(s) for q, s in zip(ps, shp)], np.float32)
    y = side.cat([t.reshape(s) != 0 for t, s in zip(ys, shp)], np.uint8)
    out = side.empty((S, 8, C), np.float32)
    lib = _lib.load()
    _lib.check(lib.pesto_bc_scores(h, S, offs.ctypes.data, C, side.ptr(y), side.ptr(p), side.ptr(out), side.kind, side.stream),
               lib.pesto_eval_last_error)
    return side.result(out)


def bc_scoring(y, p, model=None):
    """src/scoring.py:77-96: y [R, C] (0/1), p [R, C] probabilities -> [8, C] (acc, ppv, npv, tpr, tnr, mcc, auc, std). Without a model the
    call runs on a weightless handle of the tensors' GPU (GPU 0 for host arrays)."""
    if model is None:
        model = _scoring_model(p.device.index if _lib.is_torch(p) and p.is_cuda else 0)
    return bc_scores_batch(model, [y], [p])[0]


# ------------------------------------------------------------------ benchmark
def benchmark_assemblies(model, pdb_filepaths, r_thr=R_THR, l_types=L_TYPES, r_types=R_TYPES, min_num_res=0, max_atoms=24576, on_error=print):
    """Score ``model`` on the interfaces of biological assemblies: for every readable file, read + preprocess(ALL), label all subunits
    on the GPU, keep every subunit with at least one positive label (and at least ``min_num_res`` residues) - the reference's
    select_by_interface_types selection (src/dataset.py:36-47) - forward each kept subunit ALONE (encode_features(s0)[0] features,
    its own GPU k-NN, independent structures several per launch), p = sigmoid(z), scores on the GPU.
    Returns (records, summary): records = [{"file", "subunit", "residues", "scores" [8, C], "y" bool [R, C], "p" [R, C]}] and
    summary = {metric: nan-median over the records [C]}. Files that cannot be read go to ``on_error`` and are skipped."""
    import torch
    n_out = model.config["dm"]["N2"]
    if n_out != len(r_types):
        raise ValueError(f"the model predicts {n_out} classes, r_types has {len(r_types)}")
    n0 = model.config["em"]["N0"]
    dev = torch.device("cuda", model._gpu)
    files, structs = [], []
    for path in pdb_filepaths:
        try:
            structs.append(Structure.read_pdb(path).preprocess(ALL))
            files.append(path)
        except (PestoIOError, OSError) as e:
            if on_error:
                on_error(f"error with {path}: {e}")
    if not structs:
        return [], {k: np.full(n_out, np.nan, np.float32) for k in BC_SCORE_NAMES}
    subs = [s.subunits() for s in structs]
    labels = interface_labels_batch(model, subs, r_thr, l_types, r_types)
    chosen = []                                                       # (file, name, subunit dict, y)
    for path, sd, lab in zip(files, subs, labels):
        for name, s in sd.items():
            y = lab[name]
            if y.any() and y.shape[0] >= min_num_res:
                chosen.append((path, name, s, y))
    records = []
    group, atoms = [], 0

    def flush(group):
        if not group:
            return
        enc = [Structure.from_dict(s).encode(n0) for _, _, s, _ in group]
        sizes = [e[0].shape[0] for e in enc]
        r_off = np.cumsum([0] + [e[3] for e in enc])
        X = torch.from_numpy(np.concatenate([e[0] for e in enc])).to(dev)
        q = torch.from_numpy(np.concatenate([e[1] for e in enc])).to(dev)
        roa = torch.from_numpy(np.concatenate([e[2] + r_off[i] for i, e in enumerate(enc)]).astype(np.int32)).to(dev)
        ids = model.knn_collate(X, sizes)
        z = model.forward_segments(X, ids, q, roa, int(r_off[-1]), sizes=sizes)
        p, _ = model.postprocess(z)
        ps = [p[r_off[i]:r_off[i + 1]] for i in range(len(group))]
        for (_, _, _, y), e in zip(group, enc):
            if y.shape[0] != e[3]:
                raise RuntimeError("residue numbering of the labels and the encoding disagree")
        sc = bc_scores_batch(model, [torch.from_numpy(g[3]).to(dev) for g in group], ps).cpu().numpy()
        pn = p.cpu().numpy()
        for i, (path, name, _, y) in enumerate(group):
            records.append({"file": path, "subunit": name, "residues": int(y.shape[0]), "scores": sc[i], "y": y,
                            "p": pn[r_off[i]:r_off[i + 1]]})

    for item in chosen:
        n = np.asarray(item[2]["xyz"]).shape[0]
        if group and atoms + n > max_atoms:
            flush(group)
            group, atoms = [], 0
        group.append(item)
        atoms += n
    flush(group)
    model.synchronize()
    if records:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)          # (all-NaN columns: NaN median)
            med = np.nanmedian(np.stack([r["scores"] for r in records]), axis=0)
    else:
        med = np.full((8, n_out), np.nan, np.float32)
    return records, {k: med[i] for i, k in enumerate(BC_SCORE_NAMES)}
