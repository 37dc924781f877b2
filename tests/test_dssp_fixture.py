"""CPU checks of the DSSP fixture (tests/golden/make_dssp_golden.py -> dssp.npz) and of the host side of pesto_amd.dssp: the golden loads
and its planted known answers hold; backbone_table on the reader's dicts equals the stored tables; every argument error is a ValueError
raised without the library; the simplified mapping; save_dssp / load_dssp round-trip; the header and ABI_SYMBOLS name the two new symbols."""
import gzip
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden

BLANK, H, B, E, G, I, T, S, NA = range(9)
FULL = np.array([" ", "H", "B", "E", "G", "I", "T", "S", "NA"])


def case(g, name):
    """(X [F, n, 3], (table, proline, chain), sizes, codes [F, R], partners [F, R, 4], e_m [F, R, 4])"""
    return (g[f"{name}_X"], (g[f"{name}_table"], g[f"{name}_pro"], g[f"{name}_chain"]), g[f"{name}_sizes"].tolist(), g[f"{name}_codes"],
            g[f"{name}_partners"], g[f"{name}_em"])


def planted_names(g):
    return [str(n) for n in g["planted_names"]]


def text(codes):
    return "".join(FULL[c] if c != NA else "?" for c in codes)


def batch_dicts(g):
    from pesto_amd.structure_io import Structure
    return [Structure.parse_pdb(gzip.open(os.path.join(GOLDEN, "pdb", str(n) + ".gz"), "rb").read()).to_dict() for n in g["batch_names"]]


def test_golden_loads_and_its_planted_answers_hold():
    g = golden("dssp")
    names = planted_names(g)
    assert {"helix", "helix310", "helix_proline", "helix_stretched", "helix_missing_O", "helix_nan", "helix_R1", "helix_R2", "helix_R4",
            "helix_R5", "helix_R6", "one_between", "ca_9_0", "ca_8_5", "hairpin_1OL5", "meander_1OL5", "pair_antiparallel", "pair_parallel",
            "crop6O1T_127", "crop6O1T_128", "crop6O1T_129", "crop6O1T_255", "crop6O1T_256", "crop6O1T_257"} <= set(names)
    for name in names + ["batch", "frames"]:
        X, (table, pro, chain), sizes, codes, partners, em = case(g, "planted_" + name if name in names else name)
        R = table.shape[0]
        assert X.dtype == np.float32 and X.ndim == 3 and codes.dtype == np.uint8 and codes.shape == (X.shape[0], R)
        assert partners.shape == em.shape == (X.shape[0], R, 4) and sum(sizes) == R and table.max() < X.shape[1]
        assert ((partners >= 0) == (em < 0)).all() and em.min() >= -9900 and codes.max() <= NA
        assert ((codes == NA) == (table < 0).any(1)[None]).all()
        # best first, and a partner is a residue of the same structure
        assert (em[..., 0] <= em[..., 1]).all() and (em[..., 2] <= em[..., 3]).all()
        assert (partners < np.repeat(sizes, sizes)[None, :, None]).all()
    assert text(case(g, "planted_helix")[3][0]) == " " + "H" * 10 + " "
    assert case(g, "planted_helix")[4][0][4:, 0].tolist() == list(range(8))            # the i + 4 -> i bonds
    assert text(case(g, "planted_helix310")[3][0]) == " " + "G" * 10 + " "
    assert case(g, "planted_helix_proline")[4][0][6, :2].tolist() == [-1, -1]
    assert text(case(g, "planted_helix_stretched")[3][0]) == " HHHH  HHHH "
    assert case(g, "planted_helix_missing_O")[3][0][5] == NA
    assert [text(case(g, f"planted_helix_R{n}")[3][0]) for n in (1, 2, 4, 5, 6)] == [" ", "  ", "    ", " TTT ", " HHHH "]
    assert text(case(g, "planted_one_between")[3][0]) == " " + "H" * 10 + "   " + "H" * 10 + " "
    X9, X85 = case(g, "planted_ca_9_0")[0][0], case(g, "planted_ca_8_5")[0][0]
    assert X9[9].tolist() == [9.0, 0.0, 0.0] and X9[5].tolist() == [0.0, 0.0, 0.0] and X85[9].tolist() == [8.5, 0.0, 0.0]
    assert (case(g, "planted_ca_9_0")[4] == -1).all()                                   # exactly 9.0 is not < 9.0
    assert case(g, "planted_ca_8_5")[4][0][1, 0] == 2 and case(g, "planted_ca_8_5")[5][0][1, 0] == -2867
    m = text(case(g, "planted_meander_1OL5")[3][0])
    assert m[2:27] == "EEEEEEEEEETTEEEEEEEETTT  " and m[27:31] == "EEEE"                  # the turn behind the hairpin is not E
    assert text(case(g, "planted_hairpin_1OL5")[3][0])[2:22] == "EEEEEEEEEETTEEEEEEEE"
    assert (case(g, "planted_pair_antiparallel")[3] == E).sum() >= 6 and (case(g, "planted_pair_parallel")[3] == E).sum() >= 4
    assert g["scale10_ok"].size >= 1 and g["scale10_X"].shape == g["batch_X"].shape[1:]
    assert g["agreement_simplified"].shape == (5,) and g["frames_X"].shape[0] == 8
    every = np.concatenate([g["batch_codes"].ravel(), g["frames_codes"].ravel()])
    assert set(np.unique(every).tolist()) >= {BLANK, H, B, E, G, T, S, NA}


def test_backbone_table_on_the_readers_dicts():
    from pesto_amd.dssp import backbone_table
    g = golden("dssp")
    dicts = batch_dicts(g)
    start, atoms = 0, 0
    for name, d in zip(g["batch_names"], dicts):
        table, pro, chain, R = backbone_table(d)
        tag = str(name)[:4]
        assert table.dtype == np.int32 and pro.dtype == np.uint8 and chain.dtype == np.int32 and R == table.shape[0]
        assert np.array_equal(table, g[f"batch_full_{tag}_table"]) and np.array_equal(pro, g[f"batch_full_{tag}_pro"])
        assert np.array_equal(chain, g[f"batch_full_{tag}_chain"])
        # the golden's batch keeps the residues with a backbone atom, as backbone-only coordinates
        keep = (table >= 0).any(1)
        n = int(keep.sum())
        tb = g["batch_table"][start:start + n]
        assert np.array_equal(tb >= 0, table[keep] >= 0)
        assert np.array_equal(g["batch_X"][0][tb[tb >= 0]], d["xyz"][table[keep][table[keep] >= 0]])
        assert np.array_equal(g["batch_pro"][start:start + n], pro[keep]) and np.array_equal(g["batch_chain"][start:start + n], chain[keep])
        start += n
    assert start == g["batch_table"].shape[0] and np.unique(g["batch_full_1H9D_chain"]).size >= 2
    # a dict of subunits is concatenated in order; every subunit's chains are numbered on
    d = dicts[1]
    half = int(np.nonzero(d["chain_name"] != d["chain_name"][0])[0][0])
    subs = {"a": {k: v[:half] for k, v in d.items()}, "b": {k: v[half:] for k, v in d.items()}}
    t1, p1, c1, R1 = backbone_table(subs)
    t0, p0, c0, R0 = backbone_table(d)
    assert R1 == R0 and np.array_equal(t1, t0) and np.array_equal(p1, p0) and np.array_equal(c1, c0)
    # the first atom of a name counts; a residue changes with the name, the number, the insertion code or the chain
    toy = dict(name=np.array(["N", "CA", "C", "O", "CA", "N", "CA", "C", "N", "CA", "C", "O"]),
               resname=np.array(["ALA"] * 5 + ["PRO"] * 3 + ["GLY"] * 4), resid=np.array([1] * 5 + [2] * 3 + [2] * 4),
               chain_name=np.array(["B"] * 8 + ["A"] * 4))
    t, p, c, R = backbone_table(toy)
    assert R == 3 and t.tolist() == [[0, 1, 2, 3], [5, 6, 7, -1], [8, 9, 10, 11]] and p.tolist() == [0, 1, 0] and c.tolist() == [0, 0, 1]


def test_simplified_mapping():
    from pesto_amd.dssp import CODES, SIMPLIFIED, letters
    assert CODES.tolist() == FULL.tolist()
    assert dict(zip(CODES.tolist(), SIMPLIFIED.tolist())) == {"H": "H", "G": "H", "I": "H", "B": "E", "E": "E", "T": "C", "S": "C", " ": "C",
                                                                "NA": "NA"}
    c = np.arange(9, dtype=np.uint8)[None]
    assert letters(c, simplified=False).tolist() == [FULL.tolist()] and letters(c).dtype == np.dtype("<U2")
    assert letters(c).tolist() == [["C", "H", "E", "E", "H", "H", "C", "C", "NA"]]
    with pytest.raises(ValueError):
        letters(np.array([9]))
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    for k, name in enumerate(("BLANK", "H", "B", "E", "G", "I", "T", "S", "NA")):
        assert int(re.search(rf"PESTO_DSSP_{name} = (\d+)", hdr).group(1)) == k
    from pesto_amd import dssp
    assert int(re.search(r"PESTO_DSSP_MAX_RESIDUES = (\d+)", hdr).group(1)) == dssp.MAX_RESIDUES


def test_arguments_raise_before_the_library_is_loaded(monkeypatch):
    from pesto_amd import _lib
    from pesto_amd import dssp as DS

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    m = object()                # no handle either
    x = np.zeros((2, 12, 3), np.float32)
    t = np.arange(12, dtype=np.int32).reshape(3, 4)
    for bad in (np.zeros((12, 2), np.float32), np.zeros((2, 12, 4), np.float32), np.zeros(3, np.float32), np.zeros((0, 3), np.float32),
                np.zeros((1, 2, 12, 3), np.float32)):
        with pytest.raises(ValueError, match="xyz"):
            DS.compute_dssp(bad, t, model=m)
    for table in (t.reshape(4, 3), t.astype(np.float32), t[:0], t + 1, t - 2, (t, np.zeros(2, np.uint8), np.zeros(3, np.int32)),
                  (t, np.zeros(3, np.uint8), np.zeros(4, np.int32)), (t, np.zeros(3, np.uint8), np.zeros(3, np.float32)),
                  (t, np.zeros(3, np.uint8), np.zeros(3, np.int32), 4)):
        with pytest.raises(ValueError):
            DS.compute_dssp(x, table, model=m)
    for kw in (dict(sizes=[2, 2]), dict(sizes=[3, 0]), dict(sizes=[4, -1]), dict(sizes=[]), dict(scale=np.nan), dict(scale=np.inf)):
        with pytest.raises(ValueError):
            DS.compute_dssp(x, t, model=m, **kw)
        with pytest.raises(ValueError):
            DS.kabsch_sander(x, t, model=m, **kw)
    wide = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2 ** 20, 2 ** 11, 3), (0, 0, 0))          # the shape alone decides
    with pytest.raises(ValueError, match="too large"):
        DS.compute_dssp(wide, t, model=m)
    long = np.lib.stride_tricks.as_strided(np.zeros(1, np.int32), (DS.MAX_RESIDUES + 1, 4), (0, 0))
    with pytest.raises(ValueError, match="residues"):
        DS.compute_dssp(x, long, model=m)
    for bad in ({}, {"xyz": np.zeros((2, 3), np.float32)}, {"name": np.array(["N"]), "resname": np.array(["ALA", "ALA"]), "resid": np.array([1])},
                {"name": np.array(["N"]), "resname": np.array(["ALA"]), "resid": np.array([1]), "chain_name": np.array(["A", "B"])}):
        with pytest.raises(ValueError):
            DS.backbone_table(bad)
        with pytest.raises(ValueError):
            DS.structure_dssp(bad, model=m)
    with pytest.raises(ValueError, match="xyz"):
        DS.structure_dssp({"name": np.array(["N", "CA"]), "resname": np.array(["ALA"] * 2), "resid": np.array([1, 1])}, model=m)
    assert DS.structure_dssp([], model=m) == []


def test_save_dssp_round_trips(tmp_path):
    from pesto_amd import h5store
    from pesto_amd.dssp import letters, load_dssp, save_dssp
    if not h5store.available():
        pytest.skip("no HDF5 C library on this machine")
    g = golden("dssp")
    full = letters(g["batch_codes"], simplified=False)              # [1, R], as md.compute_dssp gives it
    res = {"AF-P12345-F1": full, "AF-Q9/x": g["planted_helix_codes"][0], "s": letters(g["planted_helix_missing_O_codes"][0])}
    path = save_dssp(str(tmp_path / "ss.h5"), res)
    assert not os.path.exists(path + ".tmp")
    with h5store.H5Store(path) as hf:
        raw = hf.read("AF-P12345-F1")                               # the reference's layout: the ravelled letters as byte strings
        assert raw.dtype.kind == "S" and raw.shape == (full.size,) and raw.tolist() == full.ravel().astype(bytes).tolist()
        assert [k.decode() for k in hf.read("metadata/keys")] == list(res)
    back = load_dssp(path)
    assert list(back) == list(res) and np.array_equal(back["AF-P12345-F1"], full.ravel())
    assert "".join(back["AF-Q9/x"]) == " " + "H" * 10 + " " and back["s"].tolist()[4:7] == ["C", "NA", "C"]
    assert load_dssp(save_dssp(str(tmp_path / "empty.h5"), {})) == {}


def test_header_and_binding_name_the_new_symbols():
    from pesto_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    declared = set(re.findall(r"\b(pesto_[a-z_]+)\s*\(", hdr))
    assert declared == set(_lib.ABI_SYMBOLS) and {"pesto_dssp", "pesto_dssp_last_error"} <= declared
    assert "interfaceome/secondary_structures.py:27-31" in hdr
    lib = _lib.load()
    assert hasattr(lib, "pesto_dssp") and hasattr(lib, "pesto_dssp_last_error")


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """pesto_dssp checks what needs no device data first: PESTO_ERR_INVALID with a message, whatever the handle (none here)."""
    from pesto_amd import _lib
    lib = _lib.load()
    X = np.zeros((2, 12, 3), np.float32)
    t, pro, chain = np.arange(12, dtype=np.int32).reshape(3, 4), np.zeros(3, np.uint8), np.zeros(3, np.int32)
    codes, offs = np.zeros((2, 3), np.uint8), np.array([0, 1, 3], np.int32)

    def call(F=2, N=12, scale=1.0, R=3, ns=2, offsets=offs, table=t, out=codes):
        return lib.pesto_dssp(None, F, N, X.ctypes.data, scale, R, ns, offsets.ctypes.data, table.ctypes.data, pro.ctypes.data, chain.ctypes.data,
                              None if out is None else out.ctypes.data, None, None, _lib.PTR_HOST, None)
    long = np.array([0, 70000], np.int32)
    for kw in (dict(F=0), dict(N=0), dict(F=2 ** 20, N=2 ** 11), dict(R=0), dict(F=2 ** 30), dict(ns=0), dict(offsets=np.array([0, 1, 2], np.int32)),
               dict(offsets=np.array([0, 2, 2, 3], np.int32), ns=3), dict(offsets=np.array([1, 2, 3], np.int32)), dict(scale=np.nan),
               dict(out=None), dict(table=t + 1), dict(table=t - 2),
               dict(F=1, R=70000, ns=1, offsets=long, table=np.zeros((70000, 4), np.int32))):
        assert call(**kw) == -1 and lib.pesto_dssp_last_error(), kw
    assert call() != 0 and b"handle" in lib.pesto_dssp_last_error().lower()      # valid arguments reach the handle check
