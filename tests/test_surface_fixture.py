"""The definitions of pesto_amd.surface restated in NumPy, pinned to the reference's notebook (CPU; no GPU needed).

tests/golden/surface.npz (tests/golden/make_surface_golden.py) holds three whole chains of the reference's MaSIF-site benchmark with the
restatement's outputs, and for every chain of the three predictor sets the restatement's per-point and per-residue ROC AUC next to the
pair the notebook printed. This module
    - recomputes the three stored chains from the stored inputs and requires equality,
    - compares the two tables within the bound the maker recorded (the restatement's worst case, which comes from FLANN being
      approximate, plus 0.005 for the print's two decimals) and the medians likewise,
    - round-trips a stored mesh through write_ply / read_ply bit for bit,
    - checks the argument checks of surface.py that need no GPU.
tests/test_surface.py imports the restatement functions for the GPU tests."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
from pesto_amd.topology import _fma_round_f32
from test_ranking_fixture import curve_def

VTILE, ATILE, SLAB = 256, 256, 512          # pesto_surface.hip: SF_VTILE, SF_ATILE, PESTO_SURFACE_SLAB (surface.VERTEX_TILE, ATOM_TILE, SLAB)
FIXED = 2.0 ** 40
CHAINS = ("3O5T_A", "4XL5_C", "2V9T_B")
PREDICTORS = ("sppider", "psiver", "intpred")
ALPHA = 1e-2
PRINT_ROUNDING = 0.005
MAX_BYTES = 1_000_000


# ------------------------------------------------------------------ the definitions (NumPy)
def keys_from_diff(r):
    """float32 [...]: fma(rz, rz, fma(ry, ry, rx * rx)) of float32 differences r [..., 3], every step rounded once"""
    assert r.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        rx, ry, rz = (r[..., c].astype(np.float64) for c in range(3))
        k = (rx * rx).astype(np.float32)
        k = _fma_round_f32(ry * ry, k.astype(np.float64))
        return _fma_round_f32(rz * rz, k.astype(np.float64))


def keys_def(vertices, xyz):
    """float32 [V, N]: the keys of every (vertex, atom) pair, from the float32 differences atom - vertex"""
    with np.errstate(over="ignore", invalid="ignore"):
        return keys_from_diff(xyz[None, :, :].astype(np.float32) - vertices[:, None, :].astype(np.float32))


_NEAREST = {}


def nearest_one(vertices, xyz, chunk=256):
    """(index int32 [V], distance float32 [V], key float32 [V]) of one structure: the smallest finite key, the lowest index among equal
    keys; -1 / NaN without a finite key. Computed once per (vertices, xyz) and kept. With finite coordinates of ordinary size the fused
    chain is evaluated only where it can matter: the plain float32 sum of squares differs from it by a few units in the last place, so
    only atoms within 1e-5 (relative) of the plain minimum can hold the smallest key."""
    memo = (vertices.shape, xyz.shape, hash(vertices.tobytes()), hash(xyz.tobytes()))
    if memo in _NEAREST:
        return _NEAREST[memo]
    V = vertices.shape[0]
    index, key = np.full(V, -1, np.int32), np.full(V, np.nan, np.float32)
    with np.errstate(invalid="ignore"):
        plain = bool(np.isfinite(vertices).all() and np.isfinite(xyz).all() and max(np.abs(vertices).max(), np.abs(xyz).max()) < 1e15)
    for v0 in range(0, V, chunk):
        if plain:
            r = xyz[None, :, :].astype(np.float32) - vertices[v0:v0 + chunk, None, :].astype(np.float32)
            approx = (r * r).sum(axis=-1)
            rows, cols = np.nonzero(approx <= approx.min(axis=1, keepdims=True) * np.float32(1 + 1e-5) + np.float32(1e-30))
            k = keys_from_diff(r[rows, cols])
            order = np.lexsort((cols, k, rows))                    # per vertex: by key, then by index
            first = order[np.r_[True, rows[order][1:] != rows[order][:-1]]]
            index[v0 + rows[first]], key[v0 + rows[first]] = cols[first], k[first]
            continue
        k = keys_def(vertices[v0:v0 + chunk], xyz)
        k = np.where(np.isfinite(k), k, np.float32(np.inf))
        j = np.argmin(k, axis=1)                                   # (the first of equal minima)
        best = k[np.arange(k.shape[0]), j]
        ok = np.isfinite(best)
        index[v0:v0 + chunk] = np.where(ok, j, -1)
        key[v0:v0 + chunk] = np.where(ok, best, np.float32(np.nan))
    with np.errstate(invalid="ignore"):
        _NEAREST[memo] = index, np.sqrt(key), key
    return _NEAREST[memo]


def nearest_def(vertices, xyz, v_offsets, a_offsets):
    """(index, distance) over a batch, the index in batch order"""
    idx, dist = [], []
    for s in range(len(v_offsets) - 1):
        i, d, _ = nearest_one(vertices[v_offsets[s]:v_offsets[s + 1]], xyz[a_offsets[s]:a_offsets[s + 1]])
        idx.append(np.where(i >= 0, i + a_offsets[s], -1).astype(np.int32))
        dist.append(d)
    return np.concatenate(idx), np.concatenate(dist)


def face_thirds_def(vertices, faces):
    """int64 [F]: llrint(area / 3 * 2^40) of every face of one structure, the area in float64 without contraction"""
    p = vertices.astype(np.float64)
    u, w = p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]]
    cx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    cy = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    cz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    return np.rint(area / 3.0 * FIXED).astype(np.int64)


def areas_def(vertices, faces, v_offsets, f_offsets):
    """int64 [V]: the fixed-point vertex areas of a batch (faces local to their structure)"""
    out = np.zeros(vertices.shape[0], np.int64)
    for s in range(len(v_offsets) - 1):
        f = faces[f_offsets[s]:f_offsets[s + 1]].astype(np.int64)
        q = face_thirds_def(vertices[v_offsets[s]:v_offsets[s + 1]], f)
        for c in range(3):
            np.add.at(out, v_offsets[s] + f[:, c], q)
    return out


def residues_def(nearest, atom_residue, area_fixed, iface, score, v_offsets, a_offsets, r_offsets):
    """the residue table of a batch: n_vertices, area_fixed, iface_area_fixed, area, iface_area, label, max_score (None without score)"""
    R = int(r_offsets[-1])
    struct_of_atom = np.repeat(np.arange(len(a_offsets) - 1), np.diff(a_offsets))
    res_of_atom = np.asarray(r_offsets)[struct_of_atom] + atom_residue
    has = nearest >= 0
    r = res_of_atom[nearest[has]]
    n, a, ia = np.zeros(R, np.int32), np.zeros(R, np.int64), np.zeros(R, np.int64)
    np.add.at(n, r, 1)
    np.add.at(a, r, area_fixed[has])
    on = iface[has] != 0
    np.add.at(ia, r[on], area_fixed[has][on])
    af, iaf = a.astype(np.float64) / FIXED, ia.astype(np.float64) / FIXED
    with np.errstate(invalid="ignore", divide="ignore"):
        label = ((iaf > 5.0) & (iaf / af > 0.04)).astype(np.uint8)
    mx = None
    if score is not None:
        mx = np.full(R, -np.inf, np.float32)
        np.maximum.at(mx, r, score[has].astype(np.float32))
        mx = np.where(mx == 0, np.float32(0), mx)                  # -0.0 is +0.0
        mx = np.where(n > 0, mx, np.float32(np.nan)).astype(np.float32)
    return {"n_vertices": n, "area_fixed": a, "iface_area_fixed": ia, "area": af, "iface_area": iaf, "label": label, "max_score": mx}


def gather_def(nearest, p_atom):
    return np.where(nearest >= 0, p_atom[np.maximum(nearest, 0)], np.float32(np.nan)).astype(np.float32)


def scored_def(n_vertices, label, p_res, valid, r_offsets):
    """(offsets int32 [S + 1], residue int32 [K], y uint8 [K], p float32 [K])"""
    keep = (n_vertices > 0) & (np.ones(n_vertices.size, bool) if valid is None else np.asarray(valid) != 0)
    counts = [int(keep[r_offsets[s]:r_offsets[s + 1]].sum()) for s in range(len(r_offsets) - 1)]
    rows = np.nonzero(keep)[0].astype(np.int32)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), rows, (label[rows] != 0).astype(np.uint8), p_res[rows].astype(np.float32)


def auc_def(y, p):
    """ranking's roc_auc of one column: the integer u2 = sum (fps[k] - fps[k-1]) (tps[k] + tps[k-1]) over 2 P N, NaN unless both labels occur"""
    _, tps, fps = curve_def(np.asarray(y), np.asarray(p, np.float32))
    P, N = int(tps[-1]), int(fps[-1])
    if not (P and N):
        return np.nan
    t0, f0 = np.r_[0, tps[:-1]], np.r_[0, fps[:-1]]
    u2 = int(((fps - f0) * (tps + t0)).sum())
    return float(u2) / (2.0 * float(P) * float(N))


def ca_prediction_def(bfactor, ca_index, alpha=ALPHA):
    """(p_atom, p_res, valid): the notebook's reading of a predictor's file - b-factor times alpha, a residue's from its CA, valid with a
    CA whose b-factor is not negative"""
    has = ca_index >= 0
    b = np.where(has, bfactor[np.where(has, ca_index, 0)], np.float32(-1)).astype(np.float32)
    a = np.float32(alpha)
    return (bfactor.astype(np.float32) * a).astype(np.float32), (b * a).astype(np.float32), has & (b >= 0)


def chain_def(vertices, faces, iface, xyz, atom_residue, n_res, p_atom=None, p_res=None, valid=None, vertex_score=None):
    """everything the driver computes for ONE structure, as a dict; predictions per residue (p_atom, p_res, valid) or per vertex"""
    vo, ao, fo, ro = (np.array([0, n], np.int32) for n in (vertices.shape[0], xyz.shape[0], faces.shape[0], n_res))
    nearest, distance = nearest_def(vertices, xyz, vo, ao)
    area = areas_def(vertices, faces, vo, fo)
    t = residues_def(nearest, atom_residue, area, iface, vertex_score, vo, ao, ro)
    if vertex_score is None:
        pv = gather_def(nearest, p_atom)
    else:
        pv, p_res, valid = vertex_score, t["max_score"], None
    off, res, y, p = scored_def(t["n_vertices"], t["label"], p_res, valid, ro)
    return {"nearest": nearest, "distance": distance, "area_fixed": area, "table": t, "vertex_score": pv, "residue": res, "y": y, "p": p,
            "point_auc": auc_def(iface != 0, pv), "residue_auc": auc_def(y, p)}


# ------------------------------------------------------------------ the fixture
def fetch(g, key):
    """g[key], through the fixture's aliases: an array equal to one stored before is stored as the string "=<that key>"""
    a = g[key]
    return g[str(a)[1:]] if a.ndim == 0 and a.dtype.kind == "U" and str(a).startswith("=") else a


def stored_chain(g, name):
    """the inputs of one stored chain: mesh (faces are stored as uint16), ground truth, MaSIF's scores, and per predictor the atoms of its
    file with their b-factors"""
    d = {k: fetch(g, f"{name}_{k}") for k in ("vertices", "iface", "masif")}
    d["faces"] = fetch(g, f"{name}_faces").astype(np.int32)
    for pred in PREDICTORS:
        d[pred] = {k: fetch(g, f"{name}_{pred}_{k}") for k in ("xyz", "atom_residue", "ca_index", "bfactor")}
    return d


def stored_runs(name):
    """[(tag, kwargs of chain_def)] of one stored chain: the three predictors and MaSIF's max path (on SPPIDER's atoms, as the notebook)"""
    g = golden("surface")
    c = stored_chain(g, name)
    runs = []
    for pred in PREDICTORS:
        a = c[pred]
        p_atom, p_res, valid = ca_prediction_def(a["bfactor"], a["ca_index"])
        runs.append((pred, dict(vertices=c["vertices"], faces=c["faces"], iface=c["iface"], xyz=a["xyz"], atom_residue=a["atom_residue"],
                                n_res=a["ca_index"].size, p_atom=p_atom, p_res=p_res, valid=valid)))
    a = c["sppider"]
    runs.append(("masif", dict(vertices=c["vertices"], faces=c["faces"], iface=c["iface"], xyz=a["xyz"], atom_residue=a["atom_residue"],
                               n_res=a["ca_index"].size, vertex_score=c["masif"])))
    return runs


RECORDED = ("nearest", "distance", "area_fixed", "vertex_score", "residue", "y", "p")
TABLE = ("n_vertices", "area_fixed", "iface_area_fixed", "label", "max_score")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_against_fixture(g, name, tag, out):
    """the arrays of one run equal what the fixture holds for it (the AUCs to the bit)"""
    pre = f"{name}_{tag}_out_"
    for k in RECORDED:
        assert same(out[k], fetch(g, pre + k)), (name, tag, k)
    for k in TABLE:
        if out["table"][k] is not None:
            assert same(out["table"][k], fetch(g, pre + "table_" + k)), (name, tag, k)
    assert same(np.array([out["point_auc"], out["residue_auc"]], np.float64), g[pre + "auc"]), (name, tag)


def test_fixture_is_small_and_holds_what_the_issue_lists():
    path = os.path.join(ROOT, "tests", "golden", "surface.npz")
    assert os.path.getsize(path) <= MAX_BYTES
    g = golden("surface")
    assert tuple(g["chains"].astype(str)) == CHAINS
    for name in CHAINS:
        c = stored_chain(g, name)
        V = c["vertices"].shape[0]
        assert 4000 <= V <= 5000 and c["faces"].dtype == np.int32 and c["iface"].shape == (V,) and c["masif"].shape == (V,)
        assert 0 < int((c["iface"] != 0).sum()) < V
    for pred, n in zip(PREDICTORS, (51, 51, 50)):
        assert g[f"table_{pred}_names"].size == n and g[f"table_{pred}_ours"].shape == (n, 2) and g[f"table_{pred}_printed"].shape == (n, 2)


@pytest.mark.parametrize("name", CHAINS)
def test_restatement_reproduces_the_stored_chains(name):
    g = golden("surface")
    for tag, kw in stored_runs(name):
        check_against_fixture(g, name, tag, chain_def(**kw))


def test_restatement_agrees_with_the_notebooks_prints():
    """Per chain |ours - printed| <= the maker's recorded worst case + 0.005 (the print has two decimals); the worst case itself is a
    property of the reference's approximate neighbour search and is recorded by the maker, not chosen here. The medians likewise."""
    g = golden("surface")
    worst = g["table_worst"]                                       # [3 predictors, 2]: per point, per residue
    for i, pred in enumerate(PREDICTORS):
        ours, printed = g[f"table_{pred}_ours"], g[f"table_{pred}_printed"]
        diff = np.abs(ours - printed).max(axis=0)
        print(pred, "largest per-chain difference per point / per residue", diff, "recorded", worst[i])
        assert np.array_equal(diff, worst[i])                      # the recorded worst case is the tables' own
        assert np.all(np.abs(ours - printed) <= worst[i] + PRINT_ROUNDING)
        med, med_printed, med_worst = np.median(ours, axis=0), g[f"table_{pred}_printed_medians"], g["median_worst"][i]
        print(pred, "medians", med, "printed", med_printed)
        assert np.array_equal(np.abs(med - med_printed), med_worst)
        assert np.all(np.abs(med - med_printed) <= med_worst + PRINT_ROUNDING)
    # the bounds stay what an exact neighbour against an approximate one can explain: a few hundredths per chain, thousandths in the median
    assert worst[:, 0].max() < 0.02 and worst[:, 1].max() < 0.05 and g["median_worst"].max() < 0.005


def test_stored_auc_rows_are_the_table_rows():
    g = golden("surface")
    for pred in PREDICTORS:
        names = list(g[f"table_{pred}_names"].astype(str))
        for name in CHAINS:
            if name in names:
                assert np.array_equal(g[f"table_{pred}_ours"][names.index(name)], g[f"{name}_{pred}_out_auc"])


def test_ply_round_trip_is_bit_for_bit(tmp_path):
    from pesto_amd import surface as S
    c = stored_chain(golden("surface"), CHAINS[0])
    attrs = {"iface": c["iface"].astype(np.float32), "masif": c["masif"], "tiny": np.linspace(-1e-30, 3e12, c["masif"].size).astype(np.float32)}
    path = tmp_path / "mesh.ply"
    S.write_ply(path, c["vertices"], c["faces"], attrs)
    m = S.read_ply(path)
    assert same(m["vertices"], c["vertices"]) and same(m["faces"], c["faces"]) and list(m["attributes"]) == list(attrs)
    assert all(same(m["attributes"][k], attrs[k]) for k in attrs)
    S.write_ply(path, c["vertices"][:3], np.zeros((0, 3), np.int32))
    m = S.read_ply(path)
    assert m["faces"].shape == (0, 3) and same(m["vertices"], c["vertices"][:3]) and m["attributes"] == {}


def test_read_ply_reads_the_dialect_and_refuses_the_rest(tmp_path):
    from pesto_amd import surface as S
    head = "ply\nformat ascii 1.0\ncomment Generated by PyMesh\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nproperty float iface\n"
    body = "0 0 0 1\n1 0 0 0\n0 1.5 0 -0\n"
    p = tmp_path / "a.ply"
    p.write_text(head + "element face 1\nproperty list uchar int vertex_indices\nend_header\n" + body + "3 0 1 2\n")
    m = S.read_ply(p)
    assert m["vertices"].dtype == np.float32 and np.array_equal(m["vertices"], [[0, 0, 0], [1, 0, 0], [0, 1.5, 0]])
    assert np.array_equal(m["faces"], [[0, 1, 2]]) and m["faces"].dtype == np.int32
    assert same(m["attributes"]["iface"], np.array([1, 0, -0.0], np.float32))
    p.write_text(head + "element face 1\nproperty list uchar int vertex_indices\nend_header\n" + body + "4 0 1 2 0\n")
    with pytest.raises(ValueError, match="triangle"):
        S.read_ply(p)
    p.write_text(head.replace("ascii", "binary_little_endian") + "element face 0\nproperty list uchar int vertex_indices\nend_header\n")
    with pytest.raises(ValueError, match="binary"):
        S.read_ply(p)
    p.write_text(head.replace("property float iface", "property uchar iface") + "end_header\n" + body)
    with pytest.raises(ValueError, match="float"):
        S.read_ply(p)
    p.write_text(head + "element face 1\nproperty list uchar int vertex_indices\nend_header\n" + body + "3 0 1 3\n")
    with pytest.raises(ValueError, match="index"):
        S.read_ply(p)
    p.write_text("solid\n")
    with pytest.raises(ValueError, match="PLY"):
        S.read_ply(p)
    with pytest.raises(ValueError):
        S.write_ply(p, np.zeros((3, 3), np.float32), np.array([[0, 1, 2, 0]]))


def test_structure_atoms_reads_residues_and_ca(tmp_path):
    from pesto_amd import surface as S
    rows = [("N", "ALA", "A", 1, " ", 10.0), ("CA", "ALA", "A", 1, " ", 11.0), ("N", "GLY", "A", 2, " ", 20.0), ("N", "GLY", "A", 2, "A", 30.0),
            ("CA", "GLY", "A", 2, "A", -1.0), ("CA", "SER", "B", 2, " ", 41.0), ("O", "SER", "B", 2, " ", 42.0)]
    lines = [f"ATOM  {i + 1:5d}  {n:<3s} {rn} {ch}{ri:4d}{ic}   {float(i):8.3f}{0.0:8.3f}{0.0:8.3f}  1.00{b:6.2f}           {n[0]}  " for i, (n, rn, ch, ri, ic, b) in enumerate(rows)]
    p = tmp_path / "x.pdb"
    p.write_text("\n".join(lines) + "\nTER\nEND\n")
    a = S.structure_atoms(str(p))
    assert np.array_equal(a["atom_residue"], [0, 0, 1, 2, 2, 3, 3]) and a["n_residues"] == 4 and a["atom_residue"].dtype == np.int32
    assert np.array_equal(a["ca_index"], [1, -1, 4, 5]) and np.array_equal(a["bfactor"], np.float32([10, 11, 20, 30, -1, 41, 42]))
    assert np.array_equal(a["xyz"][:, 0], np.arange(7, dtype=np.float32))
    p_atom, p_res, valid = S.ca_prediction(a)
    want = ca_prediction_def(a["bfactor"], a["ca_index"])
    assert same(p_atom, want[0]) and same(p_res, want[1]) and np.array_equal(valid, want[2]) and np.array_equal(valid, [True, False, False, True])


def test_bad_arguments_raise_before_any_launch():
    from pesto_amd import surface as S
    v, x = np.zeros((5, 3), np.float32), np.zeros((4, 3), np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    near, ar, area, iface = np.zeros(5, np.int32), np.zeros(4, np.int32), np.zeros(5, np.int64), np.zeros(5, np.uint8)
    bad = [
        lambda: S.nearest_atoms(v.astype(np.float64), x),
        lambda: S.nearest_atoms(v[:, :2], x),
        lambda: S.nearest_atoms(v[:0], x),
        lambda: S.nearest_atoms(v, x, [0, 2, 5], [0, 4]),                      # two structures against one
        lambda: S.nearest_atoms(v, x, [0, 2, 2, 5], [0, 1, 2, 4]),             # an empty structure
        lambda: S.nearest_atoms(v, x, [0, 3, 4], [0, 2, 4]),                   # v_offsets does not end at V
        lambda: S.nearest_atoms(v, x, slab=100),
        lambda: S.vertex_areas(v, f.astype(np.int64)),
        lambda: S.vertex_areas(v, f[:, :2]),
        lambda: S.vertex_areas(v, f, [0, 2, 5], [0, 2, 1]),                    # f_offsets runs backwards
        lambda: S.residue_surface(near, ar, area.astype(np.float64), iface),
        lambda: S.residue_surface(near, ar, area[:4], iface),
        lambda: S.residue_surface(near, ar, area, iface[:4]),
        lambda: S.residue_surface(near, ar, area, iface, np.zeros(5, np.float64)),
        lambda: S.residue_surface(near, ar, area, iface, v_offsets=[0, 2, 5], a_offsets=[0, 2, 4]),      # a batch without r_offsets
        lambda: S.vertex_scores(near, np.zeros(4, np.float64)),
        lambda: S.vertex_scores(near.astype(np.int64), np.zeros(4, np.float32)),
        lambda: S.scored_residues({"n_vertices": near, "label": iface, "r_offsets": np.array([0, 5], np.int32)}, np.zeros(4, np.float32)),
        lambda: S.benchmark_surfaces([]),
        lambda: S.benchmark_surfaces([{"vertices": v}], "mean"),
        lambda: S.benchmark_surfaces([{"vertices": v, "faces": f, "iface": iface, "xyz": x, "atom_residue": ar}]),      # no prediction
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} did not raise")


def test_new_symbols_are_declared_exported_and_bound():
    import pesto_amd
    from pesto_amd import _lib
    from pesto_amd import surface as S
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    new = ["pesto_surface_last_error", "pesto_surface_nearest", "pesto_surface_areas", "pesto_surface_residues", "pesto_surface_vertex_scores",
           "pesto_surface_scored"]
    lib = _lib.load()
    for name in new:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert lib.pesto_surface_last_error.restype is not None
    for const, value in (("VERTEX_TILE", S.VERTEX_TILE), ("ATOM_TILE", S.ATOM_TILE), ("SLAB", S.SLAB)):
        assert int(re.search(rf"PESTO_SURFACE_{const} = (\d+)", hdr).group(1)) == value
    assert (S.VERTEX_TILE, S.ATOM_TILE, S.SLAB) == (VTILE, ATILE, SLAB) and S.FIXED_ONE == FIXED
    assert pesto_amd.surface is S and pesto_amd.benchmark_surfaces is S.benchmark_surfaces and "surface" in pesto_amd.__all__
    # the C checks that run before the handle is looked at
    o = np.array([0, 1], np.int32)
    z = np.zeros(8, np.float32)
    assert lib.pesto_surface_nearest(None, 1, o.ctypes.data, o.ctypes.data, z.ctypes.data, z.ctypes.data, 100, z.ctypes.data, z.ctypes.data, 0, None) == -1
    assert b"slab" in lib.pesto_surface_last_error()
    assert lib.pesto_surface_nearest(None, 1, o.ctypes.data, o.ctypes.data, z.ctypes.data, z.ctypes.data, 0, z.ctypes.data, z.ctypes.data, 0, None) != 0
    assert b"handle" in lib.pesto_surface_last_error().lower()      # valid arguments reach the handle check
