#!/usr/bin/env python
"""Generate the surface golden (tests/golden/surface.npz) from the reference checkout's MaSIF-site benchmark data (build container only,
on the CPU; nothing under tests/ needs the reference at run time).

    python tests/golden/make_surface_golden.py /path/to/reference

It reads masif-site_benchmark/: ground_truth/*.ply (meshes with the per-vertex interface flag), masif_pred/*.ply (MaSIF's per-vertex
scores), sppider_pred/, psiver_pred/psiver_pdbs/ and intpred_pred/intpred_pdbs/ (PDB files with the prediction in the b-factor),
testing_transient.txt (the benchmark's chains) and the STORED OUTPUTS of masif_sppider_Intpred_comp.ipynb (the printed ROC AUCs, parsed
from the notebook's JSON; none of its code is read). Everything computed here is the NumPy restatement of tests/test_surface_fixture.py.

Stored:
  chains                                   the three whole chains kept (small ones: 4,100 - 4,900 vertices)
  <chain>_vertices / faces / iface / masif the ground-truth mesh, its interface flags, MaSIF's scores on the same vertices
  <chain>_<pred>_xyz / atom_residue / ca_index / bfactor    the atoms of the predictor's file
  <chain>_<tag>_out_*                      the restatement's outputs for tag in sppider, psiver, intpred, masif: nearest, distance,
                                           area_fixed, the residue table, the scored list, vertex_score and the two AUCs
  table_<pred>_names / ours / printed      for every chain of the predictor's set: the restatement's (per-point, per-residue) ROC AUC and the
                                           pair the notebook printed; table_<pred>_printed_medians; table_worst [3, 2] and median_worst
                                           [3, 2]: the largest differences, which tests/test_surface_fixture.py takes as its bound
An array that equals one stored before (two predictors' files with the same atoms, the areas of one mesh under four predictions) is stored
as the string "=<the earlier key>"; faces are stored as uint16. T.fetch and T.stored_chain undo both.
For the tables the nearest atom comes from a k-d tree in float64 that proposes eight candidates per vertex, among which the float32 key
of the definition decides; the script asserts that no other atom can win and that this equals the brute force on the stored chains."""
import json
import os
import re
import sys

import numpy as np
from scipy.spatial import cKDTree

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_surface_fixture as T  # noqa: E402
from pesto_amd import surface as S  # noqa: E402

DIRS = {"sppider": "sppider_pred", "psiver": os.path.join("psiver_pred", "psiver_pdbs"), "intpred": os.path.join("intpred_pred", "intpred_pdbs")}


def nearest_tree(vertices, xyz):
    """nearest_one through a k-d tree: (index, distance); asserts that the candidates hold the winner"""
    k = min(8, xyz.shape[0])
    assert np.isfinite(vertices).all() and np.isfinite(xyz).all()
    d, idx = cKDTree(xyz.astype(np.float64)).query(vertices.astype(np.float64), k=k)
    d, idx = d.reshape(-1, k), idx.reshape(-1, k)
    keys = T.keys_from_diff(xyz[idx] - vertices[:, None, :])
    best = keys.min(axis=1)
    if k < xyz.shape[0]:
        assert np.all(d[:, -1] ** 2 * (1 - 1e-4) > best.astype(np.float64)), "a ninth atom could win"
    index = np.where(keys == best[:, None], idx, np.iinfo(np.int64).max).min(axis=1).astype(np.int32)
    return index, np.sqrt(best)


def chain_fast(mesh, atoms, p_atom, p_res, valid):
    """(per-point, per-residue) ROC AUC of one chain: T.chain_def with nearest_tree"""
    V, N, R = mesh["vertices"].shape[0], atoms["xyz"].shape[0], atoms["n_residues"]
    vo, ao, fo, ro = (np.array([0, n], np.int32) for n in (V, N, mesh["faces"].shape[0], R))
    nearest, _ = nearest_tree(mesh["vertices"], atoms["xyz"])
    area = T.areas_def(mesh["vertices"], mesh["faces"], vo, fo)
    iface = mesh["attributes"]["iface"]
    t = T.residues_def(nearest, atoms["atom_residue"], area, iface, None, vo, ao, ro)
    _, _, y, p = T.scored_def(t["n_vertices"], t["label"], p_res, valid, ro)
    return T.auc_def(iface != 0, T.gather_def(nearest, p_atom)), T.auc_def(y, p)


def printed(nb_path):
    """{pred: ({chain: (per point, per residue)}, (median per point, median per residue))} from the notebook's stored stdout"""
    nb = json.load(open(nb_path))
    out = {}
    for cell in nb["cells"]:
        text = "".join("".join(o.get("text", [])) for o in cell.get("outputs", []) if o.get("output_type") == "stream" and o.get("name") == "stdout")
        rows = re.findall(r"Per residue ROC AUC: ([0-9.]+)\n(\S+) Per point ROC AUC (\S+) : ([0-9.]+)", text)
        if not rows:
            continue
        preds = {p for p, d in DIRS.items() if any(r[1].rstrip("/") == d.replace(os.sep, "/") for r in rows)}
        if len(preds) != 1:
            continue                                                # (the cell of a directory that is not in the checkout)
        med_pt = re.search(r"Median ROC AUC per protein : ([0-9.]+)", text)
        med_res = re.search(r"Median ROC AUC per residue per protein: ([0-9.]+)", text)
        out[preds.pop()] = ({r[2]: (float(r[3]), float(r[0])) for r in rows}, (float(med_pt.group(1)), float(med_res.group(1))))
    return out


def aliased(out):
    """out with every array that equals an earlier one (type, shape and bytes) replaced by the string "=<the earlier key>" (T.fetch);
    the tables are left as they are"""
    seen, res = {}, {}
    for key, a in out.items():
        a = np.asarray(a)
        sig = (a.dtype.str, a.shape, a.tobytes())
        if a.size > 16 and sig in seen and not key.startswith("table_"):
            res[key] = np.array("=" + seen[sig])
        else:
            seen.setdefault(sig, key)
            res[key] = a
    return res


def main():
    ref = os.path.join(sys.argv[1], "masif-site_benchmark")
    transient = {line[:4] for line in open(os.path.join(ref, "testing_transient.txt"))}
    prints = printed(os.path.join(ref, "masif_sppider_Intpred_comp.ipynb"))
    assert set(prints) == set(T.PREDICTORS)
    out = {"chains": np.array(T.CHAINS, "S")}
    meshes = {}

    def mesh_of(name):
        if name not in meshes:
            meshes[name] = S.read_ply(os.path.join(ref, "ground_truth", name + ".ply"))
        return meshes[name]

    # ---- the tables over every chain of the three sets
    worst, med_worst = np.zeros((3, 2)), np.zeros((3, 2))
    for i, pred in enumerate(T.PREDICTORS):
        table, med = prints[pred]
        names = sorted(f[:-4] for f in os.listdir(os.path.join(ref, DIRS[pred])) if f.endswith(".pdb") and f[:4] in transient)
        assert sorted(table) == names, (pred, sorted(set(table) ^ set(names)))
        ours = []
        for name in names:
            atoms = S.structure_atoms(os.path.join(ref, DIRS[pred], name + ".pdb"))
            ours.append(chain_fast(mesh_of(name), atoms, *T.ca_prediction_def(atoms["bfactor"], atoms["ca_index"])))
        ours, pr = np.array(ours, np.float64), np.array([table[n] for n in names], np.float64)
        worst[i], med_worst[i] = np.abs(ours - pr).max(axis=0), np.abs(np.median(ours, axis=0) - np.array(med))
        out.update({f"table_{pred}_names": np.array(names, "S"), f"table_{pred}_ours": ours, f"table_{pred}_printed": pr,
                    f"table_{pred}_printed_medians": np.array(med, np.float64)})
        print(f"{pred}: {len(names)} chains, largest difference per point {worst[i, 0]:.4f} per residue {worst[i, 1]:.4f}; medians "
              f"{np.median(ours, axis=0)} printed {med}")
    out.update(table_worst=worst, median_worst=med_worst)

    # ---- the three whole chains
    for name in T.CHAINS:
        mesh, masif = mesh_of(name), S.read_ply(os.path.join(ref, "masif_pred", name + ".ply"))
        assert mesh["faces"].max() < 65536 and np.array_equal(masif["vertices"], mesh["vertices"]) and np.array_equal(masif["faces"], mesh["faces"])
        out.update({f"{name}_vertices": mesh["vertices"], f"{name}_faces": mesh["faces"].astype(np.uint16), f"{name}_iface": (mesh["attributes"]["iface"] != 0).astype(np.uint8),
                    f"{name}_masif": masif["attributes"]["iface"]})
        for pred in T.PREDICTORS:
            a = S.structure_atoms(os.path.join(ref, DIRS[pred], name + ".pdb"))
            out.update({f"{name}_{pred}_{k}": a[k] for k in ("xyz", "atom_residue", "ca_index", "bfactor")})
    path = os.path.join(OUT, "surface.npz")
    np.savez_compressed(path, **aliased(out))                                         # (T.stored_runs reads the inputs from the file)
    for name in T.CHAINS:
        for tag, kw in T.stored_runs(name):
            d = T.chain_def(**kw)
            tree = nearest_tree(kw["vertices"], kw["xyz"])
            assert np.array_equal(tree[0], d["nearest"]) and T.same(tree[1], d["distance"]), (name, tag)
            pre = f"{name}_{tag}_out_"
            out.update({pre + k: d[k] for k in T.RECORDED})
            out.update({pre + "table_" + k: d["table"][k] for k in T.TABLE if d["table"][k] is not None})
            out[pre + "auc"] = np.array([d["point_auc"], d["residue_auc"]], np.float64)
            if tag in T.PREDICTORS:
                row = list(out[f"table_{tag}_names"].astype(str)).index(name)
                assert np.array_equal(out[f"table_{tag}_ours"][row], out[pre + "auc"]), (name, tag)
            print(f"{name} {tag}: V {kw['vertices'].shape[0]} N {kw['xyz'].shape[0]} R {kw['n_res']} scored {d['y'].size} "
                  f"positives {int(d['y'].sum())} AUC per point {d['point_auc']:.4f} per residue {d['residue_auc']:.4f}")
    np.savez_compressed(path, **aliased(out))
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= T.MAX_BYTES


if __name__ == "__main__":
    main()
