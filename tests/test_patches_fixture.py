"""CPU checks of the interface-patch fixture (tests/golden/make_patch_golden.py) and of the host side of pesto_amd.patches: the reference's
recorded patches equal a NumPy restatement of the definition, bad arguments raise ValueError before any launch, the b-factor column
survives the native reader and preprocessing, residue_ca and save_patches."""
import gzip
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

LABELS = ["protein", "dna/rna", "ion", "ligand", "lipid"]
SEL = [(i, j) for i in range(5) for j in range(i, 5)]


def case_inputs(g, case):
    xyz = g[f"{case}_xyz"] if f"{case}_xyz" in g.files else (g[f"{case}_xyz256"].astype(np.float64) / 256).astype(np.float32)
    afs = g[f"{case}_afs"] if f"{case}_afs" in g.files else None
    return g[f"{case}_offsets"], xyz, g[f"{case}_p"], afs, g[f"{case}_has_ca"]


def recorded(g, case, t, form="multi"):
    """[structure][selection][patch] -> ascending member rows, as the reference produced them"""
    npatch, lens, mem = (g[f"{case}_t{t}_{form}_{k}"] for k in ("npatch", "len", "members"))
    out, pi, mi = [], 0, 0
    for s in range(npatch.shape[0]):
        per = []
        for k in range(npatch.shape[1]):
            pl = []
            for _ in range(npatch[s, k]):
                pl.append(mem[mi:mi + lens[pi]].tolist())
                mi += lens[pi]
                pi += 1
            per.append(pl)
        out.append(per)
    return out


def definition(xyz, p, afs, has_ca, sel, thr):
    """The definition restated: float32 node test, NumPy's float32 distance matrix, components ordered by their smallest member."""
    afs_thr, p_thr, d_thr = (np.float32(v) for v in thr)
    i, j = sel
    m = (p[:, i] > p_thr) & (p[:, j] > p_thr) & (has_ca != 0)
    if afs is not None:
        m &= afs > afs_thr
    ids = np.nonzero(m)[0]
    x = xyz[ids]
    par = list(range(len(ids)))

    def find(a):
        while par[a] != a:
            par[a] = par[par[a]]
            a = par[a]
        return a
    for c0 in range(0, len(ids), 512):
        D = np.sqrt(np.sum(np.square(x[None] - x[c0:c0 + 512, None]), axis=2))
        for a, b in np.argwhere(D < d_thr):
            ra, rb = find(c0 + int(a)), find(int(b))
            if ra != rb:
                par[max(ra, rb)] = min(ra, rb)
    comp = {}
    for a in range(len(ids)):
        comp.setdefault(find(a), []).append(int(ids[a]))
    return [comp[r] for r in sorted(comp)]


@pytest.mark.parametrize("case", ["synth", "examples", "pdbs53", "big"])
def test_fixture_is_the_definition(case):
    g = golden("patches")
    offs, xyz, p, afs, has = case_inputs(g, case)
    t = 0
    while f"{case}_t{t}_thr" in g.files:
        thr = tuple(g[f"{case}_t{t}_thr"])
        ref = recorded(g, case, t)
        single = recorded(g, case, t, "single")
        assert len(ref) == offs.size - 1
        for s in range(offs.size - 1):
            r0, r1 = offs[s], offs[s + 1]
            for k, ij in enumerate(SEL):
                want = definition(xyz[r0:r1], p[r0:r1], None if afs is None else afs[r0:r1], has[r0:r1], ij, thr)
                assert ref[s][k] == want, (case, t, s, ij)
            assert single[s] == [ref[s][SEL.index((i, i))] for i in range(5)]
        t += 1
    assert t >= 1


def test_fixture_covers_the_edges():
    g = golden("patches")
    assert set(g["cases"].astype(str)) == {"pdbs53", "examples", "synth", "big"}
    big = recorded(g, "big", 0)[0]
    assert [len(pl) for pl in big[0]] == [20000] and all(pl == [] for pl in big[1:])
    assert g["big_offsets"][-1] > 4096
    synth = recorded(g, "synth", 0)
    assert synth[1][0] == [[0]]                                       # R = 1
    assert all(pl == [] for pl in synth[2])                           # nothing selected
    # the planted pairs: (0,0,0)-(6,8,0) and (0,0,0)-(10,0,0) are exactly d_thr apart: no edge; one ulp inside joins them
    pairs = synth[0][0]
    joined = {m[0] // 2 for m in pairs if len(m) == 2}
    assert 0 not in joined and 3 not in joined and 4 in joined and 5 not in joined
    assert g["examples_has_ca"].min() == 0 and np.any(g["examples_p"] == np.float32(0.5))
    assert np.isnan(g["synth_afs"]).any() and len(g["pdbs53_offsets"]) == 54


def test_arguments_raise_before_any_launch():
    from pesto_amd.patches import interface_patches_batch, patch_labels
    m = object()                # no handle: the checks must come first
    p, x = np.full((4, 5), 0.9, np.float32), np.zeros((4, 3), np.float32)
    for d in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="d_thr"):
            interface_patches_batch(m, [p], [x], d_thr=d)
    with pytest.raises(ValueError):
        interface_patches_batch(m, [], [])
    with pytest.raises(ValueError):
        interface_patches_batch(m, [p], [x[:3]])
    with pytest.raises(ValueError):
        interface_patches_batch(m, [p, p[:, :4]], [x, x])
    with pytest.raises(ValueError):
        interface_patches_batch(m, [p[:0]], [x[:0]])
    with pytest.raises(ValueError):
        interface_patches_batch(m, [p], [x], afss=[np.zeros(3, np.float32)])
    with pytest.raises(ValueError):
        interface_patches_batch(m, [p], [x], has_ca=[np.ones(5, np.uint8)])
    with pytest.raises(ValueError):
        interface_patches_batch(m, [p[:, :3]], [x])                   # fewer classes than labels
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                  # a float32 overflow warning must not come first
        for d in (1e39, 1e300, -1e300):
            with pytest.raises(ValueError, match="d_thr"):
                interface_patches_batch(m, [p], [x], d_thr=d)
    for bad in ([(1, 0)], [(0, 5)], [(-1, 0)]):
        with pytest.raises(ValueError, match="selection"):
            patch_labels(m, [p], [x], sel=bad)


def _pdb_lines(path):
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rt") as f:
        return [l.rstrip("\n") for l in f if l.startswith(("ATOM", "HETATM"))]


@pytest.mark.parametrize("name", sorted(os.listdir(os.path.join(GOLDEN, "pdb"))))
def test_bfactor_is_the_file_column(name, tmp_path):
    from pesto_amd.structure_io import Structure
    lines = _pdb_lines(os.path.join(GOLDEN, "pdb", name))
    path = str(tmp_path / name.replace(".gz", ""))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    col = {(l[21], l[22:27], l[12:16].strip(), round(float(l[30:38]), 3), round(float(l[38:46]), 3), round(float(l[46:54]), 3)):
           float(l[60:66]) for l in lines}
    for prep in (False, True):
        s = Structure.read_pdb(path)
        if prep:
            s.preprocess()
        bf = s.bfactor()
        d = s.to_dict()
        assert bf.dtype == np.float32 and bf.shape == (len(s),) and "bfactor" not in d
        by_xyz = {}
        for k, v in col.items():
            by_xyz.setdefault((k[2],) + k[3:], set()).add(np.float32(v))
        for i in range(len(s)):
            key = (d["name"][i],) + tuple(round(float(v), 3) for v in d["xyz"][i])
            assert bf[i] in by_xyz[key], (name, i)


def test_bfactor_of_a_dict_structure_is_zero():
    from pesto_amd.structure_io import Structure
    d = {"xyz": np.zeros((2, 3), np.float32), "name": np.array(["N", "CA"]), "element": np.array(["N", "C"]), "resname": np.array(["ALA", "ALA"]),
         "resid": np.array([1, 1]), "het_flag": np.array(["A", "A"]), "chain_name": np.array(["A", "A"])}
    assert np.array_equal(Structure.from_dict(d).bfactor(), np.zeros(2, np.float32))


def test_residue_ca():
    from pesto_amd.patches import residue_ca
    from pesto_amd.structure_io import Structure
    s = Structure.parse_pdb("\n".join(_pdb_lines(os.path.join(GOLDEN, "pdb", "1ZNS.pdb1.gz")))).preprocess()
    X, _, roa, R = s.encode(30)
    xyz, has, ca = residue_ca(s)
    d = s.to_dict()
    assert xyz.shape == (R, 3) and has.shape == (R,) and ca.shape == (R,)
    assert np.all(roa[ca[has != 0]] == np.nonzero(has)[0])
    assert np.all(d["name"][ca[has != 0]] == "CA") and np.array_equal(xyz[has != 0], X[ca[has != 0]])
    prot = np.isin(d["resname"], ["ALA", "GLY", "LYS", "GLU", "LEU", "SER"])
    assert np.all(has[np.unique(roa[prot])] == 1)
    ions = np.unique(roa[d["resname"] == "ZN"])
    assert ions.size and np.all(has[ions] == 0) and np.all(ca[ions] == -1)
    assert residue_ca(s.to_dict())[0].shape == (R, 3)
    # a residue with two atoms named CA: the first one is its CA
    d = {"xyz": np.arange(9, dtype=np.float32).reshape(3, 3), "name": np.array(["N", "CA", "CA"]), "element": np.array(["N", "C", "C"]),
         "resname": np.array(["ALA"] * 3), "resid": np.array([1, 1, 1]), "het_flag": np.array(["A"] * 3), "chain_name": np.array(["A"] * 3)}
    xyz1, has1, ca1 = residue_ca(d)
    assert ca1.tolist() == [1] and has1.tolist() == [1] and xyz1.tolist() == [[3.0, 4.0, 5.0]]


def test_save_patches_layout(tmp_path):
    from pesto_amd.patches import save_patches, selection_keys
    multi = {k: [[np.int64(3), 4], [7]] if k == "protein" else [] for k in selection_keys()}
    single = [[[1, 2]], [], [], [], []]
    save_patches(tmp_path / "m.json", {"P12345": multi})
    save_patches(tmp_path / "s.json", {"P12345": single})
    m = json.load(open(tmp_path / "m.json"))
    assert list(m["P12345"]) == selection_keys() and m["P12345"]["protein"] == [[3, 4], [7]]
    assert json.load(open(tmp_path / "s.json")) == {"P12345": single}
    assert selection_keys()[:6] == ["protein", "protein+dna/rna", "protein+ion", "protein+ligand", "protein+lipid", "dna/rna"]
    assert selection_keys(pairs=False) == LABELS
