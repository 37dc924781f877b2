#!/usr/bin/env python3
"""Generate the dataset-build goldens (tests/golden/dataset_<case>.npz) by IMPORTING the reference's own functions from /root/reference
(build container only; nothing under tests/ reads the reference at run time).

Per case, the loop body of processing/build_dataset.py:196-245 on one assembly read with pesto_amd's native reader (as make_eval_golden.py
does): the size check, clean_structure -> tag_hetatm_chains -> split_by_chain -> filter_non_atomic_subunits, the monomer check,
remove_duplicate_tagged_subunits, extract_all_contacts (src/data_encoding.py:147-167), pack_dataset_items and store_dataset_items
(build_dataset.py:85-173) into a RECORDING fake h5py file that keeps every group path, dataset (with its dtype) and attribute, followed by
the metadata datasets of build_dataset.py:246-254. The items of data_handler.Dataset (model/save/i_v4_1_2021-09-07_11-21/data_handler.py:
100-126) are recorded through the same fake groups: the reference's load_sparse_mask and load_interface_labels read them, since h5py is
absent. ids_topk of the PDB cases is not stored (too large): the tests check it against pesto_amd.topology.extract_topology.

Cases: the three tests/golden/pdb/*.pdb1.gz, 6O1T (two models), 3IVK (RNA) and 7KHT (lipids) from the reference's examples (gzipped into
tests/golden/pdb/), and synthetic assemblies: a pair at exactly r_thr in float32, one-atom ion subunits, a residue whose atoms carry two
resnames, a few hundred subunits, contacts that are all untyped, a monomer and duplicate ligand copies.

Usage:  python tests/golden/make_dataset_golden.py
"""
import gzip
import os
import sys

import numpy as np
import torch as pt

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_eval_golden import import_reference  # noqa: E402

PDB_CASES = ["1H9D", "1OL5", "1ZNS", "6O1T", "3IVK", "7KHT"]


class _Attrs(dict):
    def __init__(self, rec, path):
        super().__init__()
        self.rec, self.path = rec, path

    def __setitem__(self, k, v):
        # what h5py stores: a torch.Size / tuple as an int64 array, numpy arrays as they are
        a = np.asarray(tuple(v), np.int64) if isinstance(v, (tuple, pt.Size)) else np.asarray(v)
        super().__setitem__(k, a)
        self.rec["attrs"].setdefault(self.path, {})[k] = a


class _Group:
    def __init__(self, rec, path):
        self.rec, self.path = rec, path
        self.attrs = _Attrs(rec, path)

    def create_dataset(self, key, data, compression=None):
        self.rec["datasets"][f"{self.path}/{key}"] = np.asarray(data)

    def __getitem__(self, k):
        return self.rec["datasets"][f"{self.path}/{k}"]


class _File:
    def __init__(self):
        self.rec = {"groups": [], "datasets": {}, "attrs": {}}
        self.groups = {}

    def create_group(self, path):
        self.rec["groups"].append(path)
        g = _Group(self.rec, path)
        self.groups[path] = g
        return g

    def __setitem__(self, key, value):
        self.rec["datasets"][key] = np.asarray(value)


def pack(out, prefix, items):
    """Many small arrays as one flat array per dtype: {prefix}_names, _dtypes, _shapes (str), _offsets and {prefix}_blob_<dtype>."""
    out[f"{prefix}_names"] = np.array([k for k, _ in items] or [""])[:len(items)]
    out[f"{prefix}_dtypes"] = np.array([v.dtype.str for _, v in items] or [""])[:len(items)]
    out[f"{prefix}_shapes"] = np.array([",".join(map(str, v.shape)) for _, v in items] or [""])[:len(items)]
    offs, blobs = [], {}
    for _, v in items:
        b = blobs.setdefault(v.dtype.str, [])
        offs.append(sum(x.size for x in b))
        b.append(v.ravel())
    out[f"{prefix}_offsets"] = np.array(offs, np.int64)
    for dt, b in blobs.items():
        out[f"{prefix}_blob_{np.dtype(dt).name}"] = np.concatenate(b)


def structure(chains):
    """A raw structure dict from [(chain, het, [(resid, resname, [(name, element, xyz)])])]."""
    d = {k: [] for k in ("xyz", "name", "element", "resname", "resid", "het_flag", "chain_name", "icode")}
    for chain, het, residues in chains:
        for resid, resname, atoms in residues:
            for name, element, xyz in atoms:
                d["xyz"].append(xyz); d["name"].append(name); d["element"].append(element); d["resname"].append(resname)
                d["resid"].append(resid); d["het_flag"].append("H" if het else "A"); d["chain_name"].append(chain); d["icode"].append("")
    out = {k: np.array(v) for k, v in d.items()}
    out["xyz"] = out["xyz"].astype(np.float32).reshape(-1, 3)
    out["resid"] = out["resid"].astype(np.int32)
    return out


def _ala(x, y, z):
    return [("N", "N", (x, y, z)), ("CA", "C", (x + 1.2, y, z)), ("C", "C", (x + 2.0, y + 1.0, z)), ("O", "O", (x + 2.0, y + 2.2, z))]


def synthetic_cases():
    rng = np.random.default_rng(7)
    cases = {}
    # exactly r_thr in float32: (0,0,0) / (3,4,0) at 5.0 is no contact; the second pair (0,10,0) / (0,14.9,0) is
    cases["tie"] = structure([("A", False, [(1, "ALA", [("CA", "C", (0, 0, 0)), ("CB", "C", (0, 10, 0))])]),
                              ("B", False, [(1, "GLY", [("CA", "C", (3, 4, 0)), ("C", "C", (0, 14.9, 0))])])])
    # one-atom ion subunits around a protein chain (tag_hetatm_chains makes each its own subunit)
    prot = [(r + 1, "ALA", _ala(4.0 * r, 0, 0)) for r in range(6)]
    ions = [(100 + k, ["ZN", "MG", "NA", "CL"][k % 4], [(["ZN", "MG", "NA", "CL"][k % 4], ["Zn", "Mg", "Na", "Cl"][k % 4], (4.0 * k + 1, 3.0, 0.5))])
            for k in range(5)]
    cases["ions"] = structure([("A", False, prot), ("A", True, ions)])
    # a residue whose atoms carry two resnames (per-atom types: more than one (t0, t1) per residue pair)
    cases["two_resnames"] = structure([("A", False, [(1, "ALA", _ala(0, 0, 0)[:2]), (1, "GLY", _ala(0, 0, 0)[2:]), (2, "SER", _ala(4, 0, 0))]),
                                       ("B", False, [(1, "LEU", _ala(0, 3.5, 0)), (2, "LEU", _ala(4, 3.5, 0))])])
    # a few hundred subunits: 3-atom chains on a jittered grid, 3.8 A apart
    chains = []
    k = 0
    for ix in range(7):
        for iy in range(7):
            for iz in range(7):
                c = np.array([3.8 * ix, 3.8 * iy, 3.8 * iz]) + rng.normal(0, 0.3, 3)
                name = f"{chr(65 + k % 26)}{k // 26}"
                chains.append((name, False, [(1, ["GLY", "ALA", "XYZ"][k % 3], [("N", "N", tuple(c)), ("CA", "C", tuple(c + [1.4, 0, 0])),
                                                                              ("C", "C", tuple(c + [1.4, 1.4, 0]))])]))
                k += 1
    cases["many"] = structure(chains)
    # contacts, none of them typed (resnames outside molecule_ids)
    cases["untyped"] = structure([("A", False, [(1, "XAA", _ala(0, 0, 0)), (2, "XAA", _ala(4, 0, 0))]),
                                  ("B", False, [(1, "XBB", _ala(0, 3.0, 0))])])
    # a monomer (skipped)
    cases["monomer"] = structure([("A", False, [(r + 1, "ALA", _ala(4.0 * r, 0, 0)) for r in range(4)])])
    # duplicate ligand copies: two identical SO4 on the same spot (the second is removed), one elsewhere
    so4 = [("S", "S", (2.0, 2.0, 2.0)), ("O1", "O", (3.4, 2.0, 2.0)), ("O2", "O", (2.0, 3.4, 2.0)), ("O3", "O", (2.0, 2.0, 3.4))]
    so4b = [(n, e, (x + 6, y, z)) for n, e, (x, y, z) in so4]
    cases["dups"] = structure([("A", False, [(r + 1, "ALA", _ala(4.0 * r, 0, 0)) for r in range(4)]),
                               ("A", True, [(201, "SO4", so4), (202, "SO4", so4), (203, "SO4", so4b)])])
    return cases


def main():
    import_reference()
    from src.structure import (clean_structure, tag_hetatm_chains, split_by_chain, filter_non_atomic_subunits,
                               remove_duplicate_tagged_subunits)
    from src.data_encoding import extract_all_contacts
    from src.dataset import load_sparse_mask
    from build_dataset import config_dataset, pack_dataset_items, store_dataset_items
    from data_handler import load_interface_labels
    from pesto_amd.structure_io import Structure
    cfg = config_dataset
    mids = cfg["molecule_ids"]
    inputs = {}
    for name in PDB_CASES:
        st = Structure.parse_pdb(gzip.open(os.path.join(HERE, "pdb", f"{name}.pdb1.gz"), "rb").read()).to_dict()
        st["resid"] = st["resid"].astype(np.int32)
        inputs[name] = (st, name.lower(), "1", None)
    for name, st in synthetic_cases().items():
        inputs[name] = (st, f"9{name[:3]}", "1", st)
    for name, (structure_, pdbid, bid, raw) in inputs.items():
        hf = _File()
        out = {"case": np.array(name), "pdbid": np.array(pdbid), "bid": np.array(bid), "skipped": np.array("")}
        if raw is not None:
            for k, v in raw.items():
                out["in_" + k] = v
        metadata_l = []
        contacts = {}
        # build_dataset.py:210-241
        if structure_["xyz"].shape[0] >= cfg["max_num_atoms"]:
            out["skipped"] = np.array("size")
        else:
            s = clean_structure(structure_)
            s = tag_hetatm_chains(s)
            subunits = split_by_chain(s)
            subunits = filter_non_atomic_subunits(subunits)
            if len(subunits) < 2:
                out["skipped"] = np.array("monomer")
            else:
                subunits = remove_duplicate_tagged_subunits(subunits)
                contacts = extract_all_contacts(subunits, cfg["r_thr"])
                if len(contacts) == 0:
                    out["skipped"] = np.array("no_contacts")
                else:
                    sd, cd = pack_dataset_items(subunits, contacts, mids, cfg["max_num_nn"])
                    metadata_l.extend(store_dataset_items(hf, pdbid, bid, sd, cd))
                out["subunits"] = np.array(list(subunits))
        # the contact dict, in its insertion order
        order = [(ci, cj) for ci in contacts for cj in contacts[ci]]
        out["contact_pairs"] = np.array(order).reshape(-1, 2)
        out["contact_counts"] = np.array([contacts[ci][cj]["ids"].shape[0] for ci, cj in order], np.int64)
        out["contact_ids"] = np.concatenate([contacts[ci][cj]["ids"].numpy() for ci, cj in order]).reshape(-1, 2) if order else np.zeros((0, 2), np.int64)
        out["contact_d"] = np.concatenate([contacts[ci][cj]["d"].numpy() for ci, cj in order]) if order else np.zeros(0, np.float32)
        # build_dataset.py:246-254 (for this case alone)
        if metadata_l:
            hf["metadata/keys"] = np.array([m["key"] for m in metadata_l]).astype(np.bytes_)
            hf["metadata/sizes"] = np.array([m["size"] for m in metadata_l])
            hf["metadata/ckeys"] = np.array([m["ckey"] for m in metadata_l]).astype(np.bytes_)
            hf["metadata/ctypes"] = np.stack(np.where(np.array([m["ctype"] for m in metadata_l])), axis=1).astype(np.uint32)
        rec = hf.rec
        out["groups"] = np.array(rec["groups"])
        big = raw is None
        ds_names = [k for k in rec["datasets"] if not (big and k.endswith("/ids_topk"))]
        out["dataset_names"] = np.array(sorted(rec["datasets"]))
        out["dataset_dtypes"] = np.array([rec["datasets"][k].dtype.str for k in sorted(rec["datasets"])])
        out["dataset_shapes"] = np.array([str(rec["datasets"][k].shape) for k in sorted(rec["datasets"])])
        pack(out, "ds", [(k, rec["datasets"][k]) for k in sorted(ds_names)])
        pack(out, "attr", [(f"{path}|{a}", v) for path, attrs in rec["attrs"].items() for a, v in attrs.items()])
        # data_handler.Dataset items with the default types (every molecule id on both sides)
        if metadata_l:
            keys = [m["key"] for m in metadata_l]
            ckeys_map = {}
            for key, ckey in zip(keys, [m["ckey"] for m in metadata_l]):
                ckeys_map.setdefault(key, []).append(ckey)
            t0 = pt.arange(mids.shape[0])
            t1_l = [pt.arange(mids.shape[0])]
            for k, key in enumerate(ckeys_map):
                g = hf.groups["data/structures/" + key]
                M = load_sparse_mask(g, "M")
                q = pt.cat([load_sparse_mask(g, "qe")], dim=1)
                y = pt.zeros((M.shape[1], len(t1_l)), dtype=pt.bool)
                for ckey in ckeys_map[key]:
                    y |= load_interface_labels(hf.groups["data/contacts/" + ckey], t0, t1_l)
                out[f"item|{k}|key"] = np.array(key)
                out[f"item|{k}|M_sum"] = M.sum(0).numpy()
                out[f"item|{k}|q_argmax"] = q.argmax(1).numpy()
                out[f"item|{k}|y"] = y.float().numpy()
        path = os.path.join(HERE, f"dataset_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{name}: skipped={out['skipped']} groups={len(rec['groups'])} datasets={len(rec['datasets'])} "
              f"contacts={int(out['contact_counts'].sum())} -> {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
