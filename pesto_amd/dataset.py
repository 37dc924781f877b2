"""The contacts training dataset on the GPU: the reference's processing/build_dataset.py without gemmi, h5py or dense maps.

The reference builds ``contacts_rr5A_64nn_8192.h5`` (the input of training, model/main.py, and of the benchmark notebooks) with one dense
torch distance matrix per pair of subunits (extract_all_contacts, src/data_encoding.py:116-167), a dense N x N topology per subunit and a
dense [R0, R1, 79, 79] bool map per pair (contacts_types, build_dataset.py:41-60). Here:
    extract_all_contacts(_batch)   {cid_i: {cid_j: {'ids', 'd'}}}     pesto_contacts: a cell-grid search, pairs in the reference's order
    pack_dataset_items             (structures_data, contacts_data)  typed keys and T from the same call; topology from knn_collate
    build_dataset                  the reference's HDF5 layout       host threads read / preprocess, a thread writes while the GPU works
    ContactsDataset                data_handler.Dataset without h5py (the same attributes, selection and items)
The reference's selection helpers (src/dataset.py: select_by_sid, select_by_max_ba, select_by_interface_types) work on a ContactsDataset
unchanged; they are restated here for convenience.
"""
import gzip
import os
import queue
import re
import threading
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from .structure_io import ALL, CLEAN, FILTER_NON_ATOMIC, REMOVE_DUPLICATES, SPLIT, TAG_HETATM, PestoIOError, Structure

# processing/build_dataset.py:15-37 (config_dataset) and the encodings of src/data_encoding.py:6-46 (config_encoding)
MOLECULE_IDS = np.array([
    'GLU', 'LEU', 'ALA', 'ASP', 'SER', 'VAL', 'GLY', 'THR', 'ARG', 'PHE', 'TYR', 'ILE', 'PRO', 'ASN', 'LYS', 'GLN', 'HIS', 'TRP', 'MET',
    'CYS', 'A', 'U', 'G', 'C', 'DA', 'DT', 'DG', 'DC', 'MG', 'ZN', 'CL', 'CA', 'NA', 'MN', 'K', 'IOD', 'CD', 'CU', 'FE', 'NI', 'SR', 'BR',
    'CO', 'HG', 'SO4', 'NAG', 'PO4', 'EDO', 'ACT', 'MAN', 'HEM', 'FMT', 'BMA', 'ADP', 'FAD', 'NAD', 'NO3', 'GLC', 'ATP', 'NAP', 'BGC',
    'GDP', 'FUC', 'FES', 'FMN', 'GAL', 'GTP', 'PLP', 'MLI', 'ANP', 'H4B', 'AMP', 'NDP', 'SAH', 'OXY', 'PLM', 'CLR', 'CDL', 'RET'])
STD_ELEMENTS = np.array(['C', 'O', 'N', 'S', 'P', 'Se', 'Mg', 'Cl', 'Zn', 'Fe', 'Ca', 'Na', 'F', 'Mn', 'I', 'K', 'Br', 'Cu', 'Cd', 'Ni',
                         'Co', 'Sr', 'Hg', 'W', 'As', 'B', 'Mo', 'Ba', 'Pt'])
STD_RESNAMES = np.array(['LEU', 'GLU', 'ARG', 'LYS', 'VAL', 'ILE', 'PHE', 'ASP', 'TYR', 'ALA', 'THR', 'SER', 'GLN', 'ASN', 'PRO', 'GLY',
                         'HIS', 'TRP', 'MET', 'CYS', 'G', 'A', 'C', 'U', 'DG', 'DA', 'DT', 'DC'])
STD_NAMES = np.array(['CA', 'N', 'C', 'O', 'CB', 'CG', 'CD2', 'CD1', 'CG1', 'CG2', 'CD', 'OE1', 'OE2', 'OG', 'OG1', 'OD1', 'OD2', 'CE',
                      'NZ', 'NE', 'CZ', 'NH2', 'NH1', 'ND2', 'CE2', 'CE1', 'NE2', 'OH', 'ND1', 'SD', 'SG', 'NE1', 'CE3', 'CZ3', 'CZ2', 'CH2',
                      'P', "C3'", "C4'", "O3'", "C5'", "O5'", "O4'", "C1'", "C2'", "O2'", "OP1", "OP2", 'N9', 'N2', 'O6', 'N7', 'C8', 'N1',
                      'N3', 'C2', 'C4', 'C6', 'C5', 'N6', 'N4', 'O2', 'O4'])
R_THR = 5.0
MAX_NUM_ATOMS = 8192
MAX_NUM_NN = 64
KEY_RE = re.compile(r'.*/([a-z0-9]*)\.pdb([0-9]*)\.gz')        # build_dataset.py:207
_Q_SPLIT = ((0, 30), (30, 59), (59, 123))                       # qe | qr | qn columns of the native encoder's n0 = 123 one-hot


def default_key_of(path):
    """(pdbid, bid) from the reference's file name pattern (``.../1abc.pdb1.gz``); ValueError for any other name."""
    m = KEY_RE.match(os.fspath(path))
    if m is None:
        raise ValueError(f"{path}: file name does not match {KEY_RE.pattern}")
    return m[1], m[2]


# ------------------------------------------------------------------ the library call
def _subunit_rows(subunits, mids):
    """Per subunit of one assembly: (name, xyz f32 [n,3], residue column int32 [n], type int32 [n] (-1: resname not in mids), R)."""
    index = {str(m): i for i, m in enumerate(mids)}
    rows = []
    for name, s in subunits.items():
        xyz = np.asarray(s["xyz"], np.float32).reshape(-1, 3)
        _, res = np.unique(np.asarray(s["resid"]), return_inverse=True)        # encode_structure's M columns (src/data_encoding.py:72)
        res = res.astype(np.int32).reshape(-1)
        rn = np.asarray(s["resname"]).astype(str).reshape(-1)
        typ = np.array([index.get(r, -1) for r in rn], np.int32)
        rows.append((name, xyz, res, typ, int(res.max()) + 1 if res.size else 0))
    return rows


def _subunits_of(item):
    if isinstance(item, Structure):
        return item.subunits()
    if isinstance(item, dict) and "xyz" in item and not isinstance(item["xyz"], dict):
        return Structure.from_dict(item).preprocess(ALL).subunits()     # one assembly as the reference's structure dict
    return item


def _contacts_call(model, assemblies, r_thr, mids, on_device):
    """pesto_contacts on a batch: assemblies = [[(name, xyz, res, typ, R), ...]]. Returns (out, meta): out holds the library's arrays
    (sliced to their sizes; on the device for on_device), meta the per-assembly subunit names and atom starts."""
    X, su, rs, ty, sizes, meta = [], [], [], [], [], []
    n_sub, base = 0, 0
    for rows in assemblies:
        names, starts = [], []
        n_a = 0
        for name, xyz, res, typ, _ in rows:
            if xyz.shape[0] == 0:
                continue
            X.append(xyz); su.append(np.full(xyz.shape[0], n_sub, np.int32)); rs.append(res); ty.append(typ)
            names.append(name); starts.append(base + n_a)
            n_sub += 1; n_a += xyz.shape[0]
        meta.append((names, starts, n_sub - len(names)))
        sizes.append(n_a)
        base += n_a
    keep = [i for i, n in enumerate(sizes) if n > 0]
    if not keep:
        return None, meta
    if n_sub > 0xffff:
        raise ValueError(f"{n_sub} subunits in one call: at most 65535")
    args = [np.concatenate(X), np.concatenate(su), np.concatenate(rs), np.concatenate(ty)]
    h = model.handle
    offs = _lib.offsets([sizes[i] for i in keep])
    n = int(offs[-1])
    if on_device:
        import torch
        args[0] = torch.from_numpy(args[0]).to(torch.device("cuda", model._gpu))
    side = _lib.Side(args[0], model._gpu)
    Xs = side.put(args[0], np.float32, (n, 3), "X")
    sub = side.put(args[1], np.int32, (n,), "subunit")
    res = side.put(args[2], np.int32, (n,), "residue")
    typ = side.put(args[3], np.int32, (n,), "type")
    nt = len(mids)
    cap, capg = max(4096, 16 * n), max(64, 4 * n_sub)
    lib = _lib.load()
    for _ in range(3):
        pairs, d = side.empty((cap, 2), np.int32), side.empty((cap,), np.float32)
        groups = side.empty((capg, 4), np.int32)
        keys, rkeys = side.empty((cap, 4), np.int16), side.empty((cap, 4), np.int16)
        T, ties = side.empty((capg, nt, nt), np.uint8), side.empty((n,), np.uint8)
        sz = np.zeros(3, np.int64)
        _lib.check(lib.pesto_contacts(h, n, len(offs) - 1, offs.ctypes.data, n_sub, side.ptr(Xs), side.ptr(sub), side.ptr(res), side.ptr(typ),
                                      nt, float(r_thr), cap, capg, side.ptr(pairs), side.ptr(d), side.ptr(groups), side.ptr(keys),
                                      side.ptr(rkeys), side.ptr(T), side.ptr(ties), sz.ctypes.data, side.kind, side.stream),
                   lib.pesto_contacts_last_error)
        K, G, U = (int(v) for v in sz)
        if K <= cap and 0 <= G <= capg:
            break
        cap, capg = max(cap, K), max(capg, G if G > 0 else min(K, capg * 4))
    else:
        raise RuntimeError("pesto_contacts: the capacities did not converge")
    out = dict(pairs=pairs[:K], d=d[:K], groups=_lib.host(groups[:G]), keys=keys[:U], rkeys=rkeys[:U], T=T[:G], ties=ties, K=K, G=G, U=U)
    return out, meta


def _group_ranges(out):
    """Per group (i, j, p0, p1, k0, k1): batch subunit ids, its rows of pairs and of keys."""
    g = out["groups"]
    p0 = g[:, 2].astype(np.int64)
    p1 = np.append(p0[1:], out["K"])
    k1 = np.cumsum(g[:, 3].astype(np.int64))
    k0 = k1 - g[:, 3]
    return [(int(g[x, 0]), int(g[x, 1]), int(p0[x]), int(p1[x]), int(k0[x]), int(k1[x])) for x in range(g.shape[0])]


def _contact_dicts(out, meta):
    """The reference's nested dicts per assembly, in its insertion order (the pair loop i < j)."""
    pairs, d = out["pairs"], out["d"]
    torch_side = _lib.is_torch(pairs)
    if torch_side:
        import torch
    sub_of, name_of = {}, {}
    for a, (names, starts, first) in enumerate(meta):
        for k, (nm, st) in enumerate(zip(names, starts)):
            sub_of[first + k] = (a, st)
            name_of[first + k] = nm
    res = [{} for _ in meta]
    for i, j, p0, p1, _, _ in _group_ranges(out):
        a, si = sub_of[i]
        _, sj = sub_of[j]
        ab = pairs[p0:p1]
        if torch_side:
            ids_i, ids_j = ab[:, 0].long() - si, ab[:, 1].long() - sj
            fwd, rev = torch.stack([ids_i, ids_j], 1), torch.stack([ids_j, ids_i], 1)
        else:
            ids_i, ids_j = ab[:, 0].astype(np.int64) - si, ab[:, 1].astype(np.int64) - sj
            fwd, rev = np.stack([ids_i, ids_j], 1), np.stack([ids_j, ids_i], 1)
        dij = d[p0:p1]
        ci, cj = name_of[i], name_of[j]
        res[a].setdefault(ci, {})[cj] = {"ids": fwd, "d": dij}
        res[a].setdefault(cj, {})[ci] = {"ids": rev, "d": dij}
    return res


def extract_all_contacts_batch(model, assemblies, r_thr=R_THR, on_device=False):
    """extract_all_contacts for a list of assemblies in ONE launch -> [{cid_i: {cid_j: {'ids': int64 [K,2], 'd': float32 [K]}}}], the
    reference's keys, insertion order, contact order (ids_i, then ids_j ascending) and float32 distances (torch.norm's rounding), both
    directions sharing 'd'. An assembly is a preprocessed Structure, the reference's {name: subunit dict} or a raw structure dict
    (preprocessed here). on_device: the arrays are ROCm tensors of the model's GPU (the device-pointer path), else numpy."""
    rows = [[(nm, xyz, np.zeros_like(res), np.full_like(typ, -1), R) for nm, xyz, res, typ, R in _subunit_rows(_subunits_of(a), MOLECULE_IDS)]
            for a in assemblies]                            # (residues and types play no part in the contacts themselves)
    out, meta = _contacts_call(model, rows, r_thr, MOLECULE_IDS, on_device)
    return [{} for _ in meta] if out is None else _contact_dicts(out, meta)


def extract_all_contacts(model, subunits, r_thr=R_THR, on_device=False):
    """src/data_encoding.py:147-167 for ONE assembly ({name: subunit dict}, Structure or raw structure dict): see extract_all_contacts_batch."""
    return extract_all_contacts_batch(model, [subunits], r_thr, on_device)[0]


# ------------------------------------------------------------------ packing
def _check_uint16(name, n_atoms, n_res):
    if n_atoms > 0xffff or n_res > 0xffff:
        raise ValueError(f"subunit {name}: {n_atoms} atoms / {n_res} residues do not fit the dataset's uint16 indices (at most 65535)")
    if n_res > 8192:
        raise ValueError(f"subunit {name}: {n_res} residues; the typed contact keys hold at most 8192 per subunit")


def _check_rows(rows):
    for name, xyz, _, _, R in rows:
        _check_uint16(name, xyz.shape[0], R)


def _structure_items(model, subs, max_num_nn):
    """{name: (data, attrs)} of pack_structure_data (build_dataset.py:63-74) for [(name, subunit dict)]: X, the native encoder's qe / qr /
    qn and M as torch.where index pairs, ids_topk [N, min(max_num_nn, N)] from knn_collate (local, 0-based)."""
    enc = []
    for name, s in subs:
        X, q, roa, R = Structure.from_dict(s).encode(123)
        _check_uint16(name, X.shape[0], R)
        enc.append((name, X, q, roa, R))
    if not enc:
        return {}
    sizes = [e[1].shape[0] for e in enc]
    ids = _lib.host(model.knn_collate(np.concatenate([e[1] for e in enc]), sizes, max(1, min(64, max_num_nn))))
    out, base = {}, 0
    for (name, X, q, roa, R), n in zip(enc, sizes):
        k = min(max_num_nn, n)
        topk = ids[base:base + n, :k] - 1 - base
        base += n
        rows = np.arange(n, dtype=np.uint16)
        data = {"X": X, "ids_topk": topk.astype(np.uint16)}
        attrs = {}
        for fn, (c0, c1) in zip(("qe", "qr", "qn"), _Q_SPLIT):
            data[fn] = np.stack([rows, np.argmax(q[:, c0:c1], axis=1).astype(np.uint16)], axis=1)
            attrs[fn + "_shape"] = (n, c1 - c0)
        data["M"] = np.stack([rows, roa.astype(np.uint16)], axis=1)
        attrs["M_shape"] = (n, int(R))
        out[name] = ({k_: data[k_] for k_ in ("X", "ids_topk", "qe", "qr", "qn", "M")},
                     {k_: attrs[k_] for k_ in ("qe_shape", "qr_shape", "qn_shape", "M_shape")})
    return out


def _typed_items(out, meta, rows_of, nt):
    """Per assembly {(cid0, cid1): ((Y, attrs), (Y reversed, attrs))} for every pair with typed contacts (pack_contacts_data)."""
    name_of, r_of = {}, {}
    for a, (names, _, first) in enumerate(meta):
        for k, nm in enumerate(names):
            name_of[first + k] = (a, nm)
            r_of[first + k] = rows_of[a][nm]
    keys, rkeys, T = _lib.host(out["keys"]).view(np.uint16), _lib.host(out["rkeys"]).view(np.uint16), _lib.host(out["T"]).astype(bool)
    res = [{} for _ in meta]
    for g, (i, j, _, _, k0, k1) in enumerate(_group_ranges(out)):
        if k1 == k0:
            continue
        a, ci = name_of[i]
        _, cj = name_of[j]
        Ri, Rj = r_of[i], r_of[j]
        res[a][(ci, cj)] = (({"Y": keys[k0:k1]}, {"Y_shape": (Ri, Rj, nt, nt), "ctype": T[g]}),
                            ({"Y": rkeys[k0:k1]}, {"Y_shape": (Rj, Ri, nt, nt), "ctype": np.ascontiguousarray(T[g].T)}))
    return res


def _pack(contacts, typed, structures):
    """pack_dataset_items' dicts (build_dataset.py:85-140) in its insertion order, from contacts (the nested dict) and the typed items."""
    structures_data, contacts_data = {}, {}
    for cid0 in contacts:
        structures_data[cid0] = structures[cid0]
        contacts_data.setdefault(cid0, {})
        for cid1 in contacts[cid0]:
            contacts_data.setdefault(cid1, {})
            if cid1 not in contacts_data[cid0]:
                item = typed.get((cid0, cid1))
                rev = False
                if item is None and (cid1, cid0) in typed:
                    item, rev = typed[(cid1, cid0)], True
                if item is not None:
                    f, r = (item[1], item[0]) if rev else item
                    contacts_data[cid0][cid1] = f
                    contacts_data[cid1][cid0] = r
    return structures_data, contacts_data


def pack_dataset_items(model, subunits, contacts, molecule_ids=MOLECULE_IDS, max_num_nn=MAX_NUM_NN, r_thr=R_THR):
    """processing/build_dataset.py:85-140 -> (structures_data, contacts_data), numpy arrays and attrs in the reference's dict order.
    ``contacts`` is extract_all_contacts(model, subunits, r_thr) (its keys and order decide what is packed); the typed keys and T come
    from the same GPU search run with ``molecule_ids`` as the types. A subunit of more than 65535 atoms or residues is refused (ValueError)."""
    subunits = _subunits_of(subunits)
    mids = np.asarray(molecule_ids).astype(str)
    rows = _subunit_rows(subunits, mids)
    _check_rows([r for r in rows if r[0] in contacts])
    out, meta = _contacts_call(model, [rows], r_thr, mids, False)
    typed = _typed_items(out, meta, [{r[0]: r[4] for r in rows}], len(mids))[0] if out is not None else {}
    structures = _structure_items(model, [(c, subunits[c]) for c in contacts], max_num_nn)
    return _pack(contacts, typed, structures)


# ------------------------------------------------------------------ the build
def _metadata_rows(key, structures_data, contacts_data):
    """store_dataset_items' metadata rows (build_dataset.py:143-173): (key, size, ckey, ctype) per typed contact group."""
    out = []
    for cid0 in contacts_data:
        k = f"{key}/{cid0}"
        for cid1 in contacts_data[cid0]:
            size = (np.max(structures_data[cid0][0]["M"], axis=0) + 1).astype(int)
            out.append((k, size, f"{k}/{cid1}", contacts_data[cid0][cid1][1]["ctype"]))
    return out


def _write_items(hf, key, structures_data, contacts_data, compression):
    for cid0 in contacts_data:
        k = f"{key}/{cid0}"
        g = f"data/structures/{k}"
        hf.create_group(g)
        data, attrs = structures_data[cid0]
        for name, arr in data.items():
            hf.create_dataset(f"{g}/{name}", arr, compression)
        hf.set_attrs(g, attrs)
        for cid1 in contacts_data[cid0]:
            gc = f"data/contacts/{k}/{cid1}"
            hf.create_group(gc)
            data, attrs = contacts_data[cid0][cid1]
            for name, arr in data.items():
                hf.create_dataset(f"{gc}/{name}", arr, compression)
            hf.set_attrs(gc, attrs)


def _read_assembly(path, key_of, max_num_atoms):
    """Host side of one file: ('ok', key, subunits) or (reason, key or error, None); reason in unreadable / size / monomer / error."""
    try:
        pdbid, bid = key_of(path)
    except Exception as e:            # noqa: BLE001 - a bad name goes to on_error, it does not stop the build
        return "error", f"{path}: {e}", None
    try:
        if os.fspath(path).endswith(".gz"):                # the reference's inputs are gzipped (gemmi reads them as they are)
            with gzip.open(path, "rb") as f:
                s = Structure.parse_pdb(f.read())
        else:
            s = Structure.read_pdb(path)
    except (PestoIOError, OSError, EOFError, zlib.error) as e:
        return "unreadable", f"{path}: {e}", None
    if len(s) >= max_num_atoms:
        return "size", path, None
    s.preprocess(CLEAN | TAG_HETATM | SPLIT | FILTER_NON_ATOMIC)
    if len(np.unique(s._text(4))) < 2:
        return "monomer", path, None
    s.preprocess(REMOVE_DUPLICATES)
    key = f"{pdbid.upper()[1:3]}/{pdbid.upper()}/{bid}"
    return "ok", key, s.subunits()


def build_dataset(model, pdb_filepaths, dataset_filepath, r_thr=R_THR, max_num_atoms=MAX_NUM_ATOMS, max_num_nn=MAX_NUM_NN,
                  molecule_ids=MOLECULE_IDS, workers=8, key_of=None, compression=None, on_error=print, batch_atoms=65536):
    """Write the reference's contacts dataset (processing/build_dataset.py:176-254) for ``pdb_filepaths`` to ``dataset_filepath``.

    Per file, in input order (the reference's DataLoader shuffles; here the order is deterministic): skip unreadable files, assemblies of
    >= max_num_atoms atoms as read, then clean -> tag hetatm -> split -> filter non-atomic, skip fewer than 2 subunits, remove duplicates,
    skip assemblies without contacts. Host threads read and preprocess, several assemblies share one GPU launch (contacts, typed keys,
    k-NN), and a writer thread stores each batch while the GPU works on the next. ``key_of(path) -> (pdbid, bid)`` defaults to the
    reference's file name pattern; a path it rejects goes to ``on_error``. The layout is the reference's: data/structures/{key},
    data/contacts/{key}/{cid1}, metadata/{std_elements, std_resnames, std_names, mids, keys, sizes, ckeys, ctypes}.
    compression: None (unfiltered, the default) or "gzip" (deflate, when the HDF5 C library has it). The reference writes h5py's "lzf"
    filter, a plugin libhdf5 does not ship; h5py reads either form. A subunit of more than 65535 atoms or residues (possible only with a
    larger max_num_atoms) is refused with ValueError: the reference's uint16 indices would wrap silently.
    Returns a summary: {'read', 'skipped': {reason: n}, 'structures', 'contacts'}."""
    from .h5store import H5Store
    if compression not in (None, "gzip"):
        raise ValueError(f"compression must be None or 'gzip' (deflate), got {compression!r}")
    key_of = key_of or default_key_of
    mids = np.asarray(molecule_ids).astype(str)
    summary = {"read": 0, "skipped": {"unreadable": 0, "size": 0, "monomer": 0, "no_contacts": 0, "error": 0}, "structures": 0, "contacts": 0}
    metadata = []
    hf = H5Store(dataset_filepath, "w")
    q = queue.Queue(maxsize=2)
    failure = []

    def writer():
        while True:
            item = q.get()
            if item is None:
                return
            if failure:
                continue
            try:
                for key, sd, cd in item:
                    _write_items(hf, key, sd, cd, compression)
            except Exception as e:    # noqa: BLE001 - re-raised by the main thread
                failure.append(e)

    wt = threading.Thread(target=writer, daemon=True)
    try:
        hf.create_dataset("metadata/std_elements", STD_ELEMENTS.astype(np.bytes_))
        hf.create_dataset("metadata/std_resnames", STD_RESNAMES.astype(np.bytes_))
        hf.create_dataset("metadata/std_names", STD_NAMES.astype(np.bytes_))
        hf.create_dataset("metadata/mids", mids.astype(np.bytes_))
        wt.start()
        batch, atoms = [], 0

        def flush(batch):
            if not batch:
                return
            rows = [_subunit_rows(subs, mids) for _, subs in batch]
            for rw in rows:
                _check_rows(rw)
            out, meta = _contacts_call(model, rows, r_thr, mids, False)
            if out is None:
                contacts, typed = [{} for _ in batch], [{} for _ in batch]
            else:
                contacts = _contact_dicts(out, meta)
                typed = _typed_items(out, meta, [{r[0]: r[4] for r in rw} for rw in rows], len(mids))
            todo = [(b, c, t) for b, c, t in zip(batch, contacts, typed) if c]
            summary["skipped"]["no_contacts"] += len(batch) - len(todo)
            structures = _structure_items(model, [((x, c0), subs[c0]) for x, ((_, subs), c, _) in enumerate(todo) for c0 in c], max_num_nn)
            items = []
            for x, ((key, _), c, t) in enumerate(todo):
                sd, cd = _pack(c, t, {c0: structures[(x, c0)] for c0 in c})
                items.append((key, sd, cd))
                metadata.extend(_metadata_rows(key, sd, cd))
                summary["structures"] += len(sd)
                summary["contacts"] += sum(len(v) for v in cd.values())
            if failure:
                raise failure[0]
            q.put(items)

        with ThreadPoolExecutor(max_workers=max(1, int(workers))) as ex:
            for status, key, subs in ex.map(lambda p: _read_assembly(p, key_of, max_num_atoms), list(pdb_filepaths)):
                if status != "ok":
                    summary["skipped"][status] += 1
                    if status in ("unreadable", "error") and on_error:
                        on_error(f"error with {key}")
                    if status == "error":
                        continue
                    summary["read"] += status != "unreadable"
                    continue
                summary["read"] += 1
                n = sum(np.asarray(s["xyz"]).shape[0] for s in subs.values())
                if batch and atoms + n > batch_atoms:
                    flush(batch)
                    batch, atoms = [], 0
                batch.append((key, subs))
                atoms += n
            flush(batch)
        q.put(None)
        wt.join()
        if failure:
            raise failure[0]
        hf.create_dataset("metadata/keys", np.array([m[0] for m in metadata]).astype(np.bytes_))
        hf.create_dataset("metadata/sizes", np.array([m[1] for m in metadata]).reshape(-1, 2).astype(np.int64))
        hf.create_dataset("metadata/ckeys", np.array([m[2] for m in metadata]).astype(np.bytes_))
        ct = np.array([m[3] for m in metadata]).reshape(-1, len(mids), len(mids))
        hf.create_dataset("metadata/ctypes", np.stack(np.where(ct), axis=1).astype(np.uint32))
    finally:
        if wt.is_alive():
            q.put(None)
            wt.join()
        hf.close()
    return summary


# ------------------------------------------------------------------ reading
def load_sparse_mask(hf, group, k):
    """src/dataset.py:50-59 on an H5Store group: the dense float32 [shape] mask of the index pairs ``k``."""
    import torch as pt
    shape = tuple(int(v) for v in hf.attrs(group)[k + "_shape"])
    M = pt.zeros(shape, dtype=pt.float)
    ids = pt.from_numpy(hf.read(f"{group}/{k}").astype(np.int64))
    M.scatter_(1, ids[:, 1:], 1.0)
    return M


def load_interface_labels(hf, group, t0, t1_l):
    """model/save/i_v4_1_2021-09-07_11-21/data_handler.py:9-23 on an H5Store contacts group (the same torch operations)."""
    import torch as pt
    shape = tuple(int(v) for v in hf.attrs(group)["Y_shape"])
    ids = pt.from_numpy(hf.read(f"{group}/Y").astype(np.int64))
    y_ctc_r = pt.any((ids[:, 2].view(-1, 1) == t0), dim=1).view(-1, 1)
    y_ctc_l = pt.stack([pt.any((ids[:, 3].view(-1, 1) == t1), dim=1) for t1 in t1_l], dim=1)
    y_ctc = (y_ctc_r & y_ctc_l)
    y = pt.zeros((shape[0], len(t1_l)), dtype=pt.bool)
    y[ids[:, 0], pt.where(y_ctc)[1]] = True
    return y


class ContactsDataset:
    """data_handler.Dataset (model/save/i_v4_1_2021-09-07_11-21/data_handler.py:39-126) over the H5Store binding: the same attributes
    (keys, sizes, ckeys, ctypes, std_elements, std_resnames, std_names, mids, m), update_mask / set_types / get_largest, and items
    (X, ids_topk, q, M, y) - load_sparse_mask + load_interface_labels OR-ed over the item's ckeys."""

    def __init__(self, dataset_filepath, features_flags=(True, False, False)):
        from .h5store import H5Store
        import torch as pt
        self.dataset_filepath = dataset_filepath
        self.ftrs = [fn for fn, ff in zip(['qe', 'qr', 'qn'], features_flags) if ff]
        with H5Store(dataset_filepath) as hf:
            self.keys = hf.read("metadata/keys").astype(np.dtype('U'))
            self.sizes = hf.read("metadata/sizes")
            self.ckeys = hf.read("metadata/ckeys").astype(np.dtype('U'))
            self.ctypes = hf.read("metadata/ctypes")
            self.std_elements = hf.read("metadata/std_elements").astype(np.dtype('U'))
            self.std_resnames = hf.read("metadata/std_resnames").astype(np.dtype('U'))
            self.std_names = hf.read("metadata/std_names").astype(np.dtype('U'))
            self.mids = hf.read("metadata/mids").astype(np.dtype('U'))
        self.m = np.ones(len(self.keys), dtype=bool)
        self._update_selection()
        self.t0 = pt.arange(self.mids.shape[0])
        self.t1_l = [pt.arange(self.mids.shape[0])]

    def _update_selection(self):
        self.ckeys_map = {}
        for key, ckey in zip(self.keys[self.m], self.ckeys[self.m]):
            self.ckeys_map.setdefault(key, []).append(ckey)
        self.ukeys = list(self.ckeys_map)

    def update_mask(self, m):
        self.m &= m
        self._update_selection()

    def set_types(self, l_types, r_types_l):
        import torch as pt
        self.t0 = pt.from_numpy(np.where(np.isin(self.mids, l_types))[0])
        self.t1_l = [pt.from_numpy(np.where(np.isin(self.mids, r_types))[0]) for r_types in r_types_l]

    def get_largest(self):
        i = np.argmax(self.sizes[:, 0] * self.m.astype(int))
        k = np.where(np.isin(self.ukeys, self.keys[i]))[0][0]
        return self[k]

    def __len__(self):
        return len(self.ukeys)

    def __getitem__(self, k):
        from .h5store import H5Store
        import torch as pt
        key = self.ukeys[k]
        with H5Store(self.dataset_filepath) as hf:
            g = "data/structures/" + key
            X = pt.from_numpy(hf.read(g + "/X").astype(np.float32))
            M = load_sparse_mask(hf, g, "M")
            ids_topk = pt.from_numpy(hf.read(g + "/ids_topk").astype(np.int64))
            q = pt.cat([load_sparse_mask(hf, g, fn) for fn in self.ftrs], dim=1)
            y = pt.zeros((M.shape[1], len(self.t1_l)), dtype=pt.bool)
            for ckey in self.ckeys_map[key]:
                y |= load_interface_labels(hf, "data/contacts/" + ckey, self.t0, self.t1_l)
        return X, ids_topk, q, M, y.float()


# ------------------------------------------------------------------ selections (src/dataset.py:8-47)
def select_by_sid(dataset, sids_sel):
    sids = np.array(['_'.join([s.split(':')[0] for s in key.split('/')[1::2]]) for key in dataset.keys])
    return np.isin(sids, sids_sel)


def select_by_max_ba(dataset, max_ba):
    aids = np.array([int(key.split('/')[2]) for key in dataset.keys])
    return aids <= max_ba


def select_by_interface_types(dataset, l_types, r_types):
    t0 = np.where(np.isin(dataset.mids, l_types))[0]
    t1 = np.where(np.isin(dataset.mids, r_types))[0]
    cm = (np.isin(dataset.ctypes[:, 1], t0) & np.isin(dataset.ctypes[:, 2], t1))
    return np.isin(np.arange(dataset.keys.shape[0]), dataset.ctypes[cm, 0])
