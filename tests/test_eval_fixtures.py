"""CPU checks of the evaluation fixtures (tests/golden/make_eval_golden.py) and of the host side of pesto_amd.evaluate: the fixtures load,
the host's resname tables are the reference's, and the stored reference labels satisfy the label definition recomputed by brute force."""
import numpy as np
import pytest
import torch

from conftest import golden
from pesto_amd import evaluate


def _labels():
    return golden("eval_labels")


def test_fixtures_load():
    g = _labels()
    n = g["X"].shape[0]
    assert g["atom_offsets"][0] == 0 and g["atom_offsets"][-1] == n and g["names"].size == 16
    assert g["atom_sub"].shape == g["atom_res"].shape == g["atom_resname"].shape == (n,)
    assert g["res_offsets"][-1] == g["labels"].shape[0] and g["labels"].shape[1] == 5 and g["labels"].dtype == bool
    assert g["sub_names"].size == g["sub_assembly"].size == g["res_offsets"].size - 1
    assert float(g["r_thr"]) == evaluate.R_THR
    for k in range(g["sub_names"].size):            # residue rows of every subunit: 0 .. R_s - 1, all present
        res = g["atom_res"][g["atom_sub"] == k]
        assert np.array_equal(np.unique(res), np.arange(g["res_offsets"][k + 1] - g["res_offsets"][k]))
    s = golden("eval_scores")
    for case in s["cases"].astype(str):
        y, p, off, sc = (s[f"{case}_{k}"] for k in ("y", "p", "offsets", "scores"))
        assert y.shape == p.shape and off[-1] == y.shape[0] and sc.shape == (off.size - 1, 8, y.shape[1])
        assert np.all(np.diff(off) >= 1) and set(np.unique(y)) <= {0, 1}


def test_host_tables_are_the_references():
    g = _labels()
    categ = {c: list(g["categ_" + c].astype(str)) for c in g["categ_names"].astype(str)}
    assert categ == evaluate.CATEG_TO_RESNAMES
    assert evaluate.L_TYPES == categ["protein"]
    assert evaluate.R_TYPES == [categ["protein"], categ["dna"] + categ["rna"], categ["ion"], categ["ligand"], categ["lipid"]]
    mids = set(g["molecule_ids"].astype(str))
    assert all(set(t) <= mids for t in evaluate.R_TYPES) and set(evaluate.L_TYPES) <= mids
    table = g["resname_table"].astype(str)
    rec, mask = evaluate.resname_masks(table)
    for i, rn in enumerate(table):
        assert rec[i] == (rn in categ["protein"])
        assert mask[i] == sum(1 << c for c, t in enumerate(evaluate.R_TYPES) if rn in t)
    with pytest.raises(ValueError):
        evaluate.resname_masks(table, r_types=[["ALA"]] * 33)
    rec, mask = evaluate.resname_masks(table, r_types=[[c] for c in categ["protein"]])      # config.py:22, one class per amino acid
    assert mask.max() < (1 << 20) and np.all((mask != 0) == rec.astype(bool))


def _assembly(g, a):
    a0, a1 = g["atom_offsets"][a], g["atom_offsets"][a + 1]
    return (g["X"][a0:a1], g["atom_sub"][a0:a1].astype(np.int64), g["atom_res"][a0:a1],
            g["resname_table"].astype(str)[g["atom_resname"][a0:a1]])


@pytest.mark.parametrize("name", ["1ZNS", "1H9D", "7KHT", "6O1T", "1OL5", "2VGO"])
def test_fixture_labels_match_definition(name):
    """The stored labels of an assembly = the issue's definition, recomputed with the reference's distance (torch.norm over xyz, CPU)."""
    g = _labels()
    a = list(g["names"].astype(str)).index(name)
    X, sub, res, rn = _assembly(g, a)
    rec, mask = evaluate.resname_masks(rn)
    Xt = torch.from_numpy(X)
    for k in np.unique(sub):
        me = sub == k
        y = np.zeros((int(res[me].max()) + 1, 5), bool)
        for j in np.unique(sub):
            if j == k:
                continue
            ot = (sub == j) & (mask != 0)
            if not ot.any():
                continue
            D = torch.norm(Xt[me].unsqueeze(1) - Xt[ot].unsqueeze(0), dim=2).numpy()
            ia, ib = np.where(D < 5.0)
            ok = rec[me][ia] != 0
            for c in range(5):
                hit = ok & ((mask[ot][ib] >> c) & 1 != 0)
                y[res[me][ia[hit]], c] = True
        r0, r1 = g["res_offsets"][k], g["res_offsets"][k + 1]
        assert np.array_equal(y, g["labels"][r0:r1]), (name, g["sub_names"][k])
