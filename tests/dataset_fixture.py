"""Readers of the dataset-build fixture (tests/golden/dataset_<case>.npz, written by tests/golden/make_dataset_golden.py) and the NumPy
restatement of the reference's contact definitions that the tests pin it to."""
import gzip
import os

import numpy as np

from conftest import GOLDEN

PDB_CASES = ["1H9D", "1OL5", "1ZNS", "6O1T", "3IVK", "7KHT"]
SYNTH_CASES = ["tie", "ions", "two_resnames", "many", "untyped", "monomer", "dups"]
CASES = PDB_CASES + SYNTH_CASES


def load(case):
    return np.load(os.path.join(GOLDEN, f"dataset_{case}.npz"))


def unpack(g, prefix):
    """{name: array} of make_dataset_golden.pack()."""
    out = {}
    for name, dt, shp, off in zip(g[f"{prefix}_names"], g[f"{prefix}_dtypes"], g[f"{prefix}_shapes"], g[f"{prefix}_offsets"]):
        dt = np.dtype(str(dt))
        shape = tuple(int(v) for v in str(shp).split(",") if v)
        n = int(np.prod(shape)) if shape else 1
        out[str(name)] = g[f"{prefix}_blob_{dt.name}"][int(off):int(off) + n].reshape(shape)
    return out


def attrs(g):
    """{group path: {attr: value}} of the recorded tree."""
    out = {}
    for k, v in unpack(g, "attr").items():
        path, a = k.rsplit("|", 1)
        out.setdefault(path, {})[a] = v
    return out


def contacts(g):
    """[(cid_i, cid_j, ids int64 [K,2], d float32 [K])] in the recorded dict's insertion order."""
    out, o = [], 0
    for (ci, cj), n in zip(g["contact_pairs"].astype(str).reshape(-1, 2), g["contact_counts"]):
        out.append((ci, cj, g["contact_ids"][o:o + n], g["contact_d"][o:o + n]))
        o += int(n)
    return out


def structure_of(case):
    """The case's structure as a native Structure, as read (before preprocessing)."""
    from pesto_amd.structure_io import Structure
    if case in PDB_CASES:
        return Structure.parse_pdb(gzip.open(os.path.join(GOLDEN, "pdb", f"{case}.pdb1.gz"), "rb").read())
    g = load(case)
    d = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    return Structure.from_dict(d)


def subunits_of(case):
    """The reference's subunits of the case after the build's preprocessing (None for a monomer)."""
    from pesto_amd.structure_io import ALL
    s = structure_of(case).preprocess(ALL)
    sub = s.subunits()
    return sub if len(sub) >= 2 else None


def np_contacts(subunits, r_thr=5.0):
    """extract_all_contacts restated: torch.norm's float32 distance (topology._norm_xyz), D < r_thr, torch.where's row-major order."""
    from pesto_amd.topology import _norm_xyz
    names = list(subunits)
    out = []
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            Xi = np.asarray(subunits[names[i]]["xyz"], np.float32)
            Xj = np.asarray(subunits[names[j]]["xyz"], np.float32)
            D = _norm_xyz(Xi[:, None, :] - Xj[None, :, :]).astype(np.float32)
            a, b = np.where(D < np.float32(r_thr))
            if a.size:
                out.append((names[i], names[j], np.stack([a, b], 1).astype(np.int64), D[a, b]))
    return out


def np_typed_keys(s0, s1, ids, mids):
    """contacts_types + pack_contacts_data restated: Y[r0, r1] = H[k] for the contacts k in order (torch's index_put_ on the CPU: the last
    contact of a residue pair decides its slab, which holds (t0, t1) when both atoms are typed and nothing otherwise), then torch.where
    -> sorted (r0, r1, t0, t1) rows, and T."""
    index = {m: t for t, m in enumerate(np.asarray(mids).astype(str))}
    t0 = np.array([index.get(r, -1) for r in np.asarray(s0["resname"]).astype(str)])[ids[:, 0]]
    t1 = np.array([index.get(r, -1) for r in np.asarray(s1["resname"]).astype(str)])[ids[:, 1]]
    r0 = np.unique(s0["resid"], return_inverse=True)[1].reshape(-1)[ids[:, 0]]
    r1 = np.unique(s1["resid"], return_inverse=True)[1].reshape(-1)[ids[:, 1]]
    last = {}
    for k in range(ids.shape[0]):
        last[(int(r0[k]), int(r1[k]))] = (int(t0[k]), int(t1[k]))
    rows = sorted((a, b, x, y) for (a, b), (x, y) in last.items() if x >= 0 and y >= 0)
    Y = np.array(rows, np.uint16).reshape(-1, 4)
    T = np.zeros((len(index), len(index)), bool)
    T[Y[:, 2], Y[:, 3]] = True
    return Y, T
