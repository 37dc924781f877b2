"""CPU checks of the dataset build: the fixture pinned to a NumPy restatement of the reference's definitions, the HDF5 types the layout
needs, ContactsDataset on a file written from the fixture, and argument errors."""
import numpy as np
import pytest

import dataset_fixture as fx
from pesto_amd import dataset, h5store
from pesto_amd.topology import extract_topology


@pytest.mark.parametrize("case", fx.CASES)
def test_fixture_contacts_match_numpy_restatement(case):
    g = fx.load(case)
    sub = fx.subunits_of(case)
    if sub is None:
        assert str(g["skipped"]) == "monomer"
        return
    want = fx.np_contacts(sub)
    got = fx.contacts(g)
    order = {}
    for ci, cj, _, _ in want:                     # the reference's insertion order: the pair loop i < j, both directions
        order.setdefault(ci, []).append(cj)
        order.setdefault(cj, []).append(ci)
    assert [(a, b) for a, b, _, _ in got] == [(a, b) for a in order for b in order[a]]
    fwd = {(ci, cj): (ids, d) for ci, cj, ids, d in got}
    assert len(got) == 2 * len(want)
    for ci, cj, ids, d in want:
        gi, gd = fwd[(ci, cj)]
        np.testing.assert_array_equal(gi, ids)
        assert gd.view(np.int32).tolist() == d.view(np.int32).tolist()
        ri, rd = fwd[(cj, ci)]
        np.testing.assert_array_equal(ri, ids[:, ::-1])
        np.testing.assert_array_equal(rd, d)


@pytest.mark.parametrize("case", fx.CASES)
def test_fixture_typed_keys_match_numpy_restatement(case):
    g = fx.load(case)
    sub = fx.subunits_of(case)
    if sub is None or not len(g["ds_names"]):
        return
    ds, at = fx.unpack(g, "ds"), fx.attrs(g)
    key = f"{str(g['pdbid']).upper()[1:3]}/{str(g['pdbid']).upper()}/{g['bid']}"
    mids = dataset.MOLECULE_IDS
    n = 0
    for ci, cj, ids, _ in fx.np_contacts(sub):
        Y, T = fx.np_typed_keys(sub[ci], sub[cj], ids, mids)
        path = f"data/contacts/{key}/{ci}/{cj}"
        if not Y.shape[0]:
            assert path + "/Y" not in ds
            continue
        np.testing.assert_array_equal(ds[path + "/Y"], Y)
        np.testing.assert_array_equal(at[path]["ctype"], T)
        Yr = ds[f"data/contacts/{key}/{cj}/{ci}/Y"]
        np.testing.assert_array_equal(Yr, np.unique(Y[:, [1, 0, 3, 2]], axis=0))          # torch.where of Y.permute(1, 0, 3, 2)
        np.testing.assert_array_equal(at[f"data/contacts/{key}/{cj}/{ci}"]["ctype"], T.T)
        n += 2
    assert n == sum(1 for k in ds if k.startswith("data/contacts/"))


def _write_fixture(path, cases):
    """The recorded trees of ``cases`` in one HDF5 file (metadata concatenated in case order), through the new H5Store types."""
    meta = {"keys": [], "sizes": [], "ckeys": [], "ctypes": []}
    n_rows = 0
    with h5store.H5Store(path, "w") as hf:
        hf.create_dataset("metadata/std_elements", dataset.STD_ELEMENTS.astype(np.bytes_))
        hf.create_dataset("metadata/std_resnames", dataset.STD_RESNAMES.astype(np.bytes_))
        hf.create_dataset("metadata/std_names", dataset.STD_NAMES.astype(np.bytes_))
        hf.create_dataset("metadata/mids", dataset.MOLECULE_IDS.astype(np.bytes_))
        for case in cases:
            g = fx.load(case)
            ds, at = fx.unpack(g, "ds"), fx.attrs(g)
            for grp in g["groups"]:
                hf.create_group(str(grp))
            for k, v in ds.items():
                if not k.startswith("metadata/"):
                    hf.create_dataset(k, v)
                if k.endswith("/X") and k[:-2] + "/ids_topk" not in ds:        # (not stored for the PDB cases)
                    hf.create_dataset(k[:-2] + "/ids_topk", extract_topology(v, 64).astype(np.uint16))
            for p, a in at.items():
                hf.set_attrs(p, a)
            if "metadata/keys" in ds:
                meta["keys"].append(ds["metadata/keys"]); meta["sizes"].append(ds["metadata/sizes"]); meta["ckeys"].append(ds["metadata/ckeys"])
                ct = ds["metadata/ctypes"].copy()
                ct[:, 0] += n_rows
                meta["ctypes"].append(ct)
                n_rows += ds["metadata/keys"].shape[0]
        w = max(a.dtype.itemsize for a in meta["keys"])
        hf.create_dataset("metadata/keys", np.concatenate([a.astype(f"S{w}") for a in meta["keys"]]))
        hf.create_dataset("metadata/sizes", np.concatenate(meta["sizes"]))
        w = max(a.dtype.itemsize for a in meta["ckeys"])
        hf.create_dataset("metadata/ckeys", np.concatenate([a.astype(f"S{w}") for a in meta["ckeys"]]))
        hf.create_dataset("metadata/ctypes", np.concatenate(meta["ctypes"]))


def check_items(ds_obj, cases):
    """ContactsDataset items against the recorded data_handler.Dataset items of ``cases`` (in order)."""
    rec = []
    for case in cases:
        g = fx.load(case)
        k = 0
        while f"item|{k}|key" in g.files:
            rec.append((str(g[f"item|{k}|key"]), g[f"item|{k}|M_sum"], g[f"item|{k}|q_argmax"], g[f"item|{k}|y"],
                        fx.unpack(g, "ds")["data/structures/" + str(g[f"item|{k}|key"]) + "/X"]))
            k += 1
    assert list(ds_obj.ukeys) == [r[0] for r in rec]
    for k, (key, M_sum, q_arg, y, X) in enumerate(rec):
        Xg, ids, q, M, yg = ds_obj[k]
        np.testing.assert_array_equal(Xg.numpy(), X)
        np.testing.assert_array_equal(M.sum(0).numpy(), M_sum)
        np.testing.assert_array_equal(q.argmax(1).numpy(), q_arg)
        assert ids.dtype.is_floating_point is False and ids.shape[0] == X.shape[0]
        np.testing.assert_array_equal(yg.numpy(), y)


def test_contacts_dataset_reads_fixture_tree(tmp_path):
    pytest.importorskip("torch")
    try:
        h5store.load()
    except h5store.H5Unavailable:
        pytest.skip("no HDF5 C library")
    cases = ["tie", "ions", "two_resnames", "dups", "1ZNS"]
    path = str(tmp_path / "c.h5")
    _write_fixture(path, cases)
    d = dataset.ContactsDataset(path)
    assert d.mids.tolist() == dataset.MOLECULE_IDS.tolist() and d.std_names.tolist() == dataset.STD_NAMES.tolist()
    check_items(d, cases)
    # the reference's selections work on it
    m = dataset.select_by_interface_types(d, ["ALA", "GLY"], ["ZN"])
    assert m.dtype == bool and m.shape == d.keys.shape and m.any()
    d.update_mask(dataset.select_by_max_ba(d, 1) & m)
    assert 0 < len(d) < len(d.keys)
    assert dataset.select_by_sid(d, ["AB_CD"]).shape == d.keys.shape


def test_h5store_layout_types_round_trip(tmp_path):
    try:
        h5store.load()
    except h5store.H5Unavailable:
        pytest.skip("no HDF5 C library")
    path = str(tmp_path / "t.h5")
    T = np.zeros((79, 79), bool)
    T[3, 5] = T[0, 78] = True
    with h5store.H5Store(path, "w") as hf:
        hf.create_dataset("metadata/mids", dataset.MOLECULE_IDS.astype(np.bytes_))
        hf.create_group("data/structures/AB/1ABC/1/A:0")
        hf.create_dataset("data/structures/AB/1ABC/1/A:0/M", np.arange(20, dtype=np.uint16).reshape(10, 2), compression="gzip")
        hf.set_attrs("data/structures/AB/1ABC/1/A:0", {"M_shape": (10, 4), "ctype": T})
        hf.create_dataset("flags", np.array([True, False, True]), attrs={"n": (3,)})
        hf["plain"] = np.arange(4, dtype=np.float32)
    with h5store.H5Store(path) as hf:
        m = hf.read("metadata/mids")
        assert m.dtype.kind == "S" and m.astype(str).tolist() == dataset.MOLECULE_IDS.tolist()
        np.testing.assert_array_equal(hf.read("data/structures/AB/1ABC/1/A:0/M"), np.arange(20).reshape(10, 2))
        a = hf.attrs("data/structures/AB/1ABC/1/A:0")
        assert a["M_shape"].dtype == np.int64 and a["M_shape"].tolist() == [10, 4]
        assert a["ctype"].dtype == bool and np.array_equal(a["ctype"], T)
        assert hf.read("flags").tolist() == [True, False, True] and hf.attrs("flags")["n"].tolist() == [3]
        np.testing.assert_array_equal(hf["plain"], np.arange(4, dtype=np.float32))
        assert hf.keys() == sorted(["metadata/mids", "data/structures/AB/1ABC/1/A:0/M", "flags", "plain"])
        with pytest.raises(KeyError):
            hf.attrs("nope")


def test_key_of_and_argument_errors(tmp_path):
    assert dataset.default_key_of("/data/all_biounits/ab/1abc.pdb2.gz") == ("1abc", "2")
    with pytest.raises(ValueError):
        dataset.default_key_of("tests/golden/pdb/1H9D.pdb1.gz")           # upper case: not the reference's pattern
    try:
        h5store.load()
    except h5store.H5Unavailable:
        pytest.skip("no HDF5 C library")
    errors = []
    summary = dataset.build_dataset(None, ["x/1H9D.pdb1.gz", "y/README"], str(tmp_path / "e.h5"), on_error=errors.append)
    assert len(errors) == 2 and summary["skipped"]["error"] == 2 and summary["read"] == 0 and summary["contacts"] == 0
    with pytest.raises(ValueError):
        dataset.build_dataset(None, [], str(tmp_path / "f.h5"), compression="lzf")
    big = {"xyz": np.zeros((70000, 3), np.float32), "name": np.array(["CA"] * 70000), "element": np.array(["C"] * 70000),
           "resname": np.array(["ALA"] * 70000), "resid": np.arange(70000), "het_flag": np.array(["A"] * 70000)}
    with pytest.raises(ValueError, match="uint16"):
        dataset._structure_items(None, [("A:0", big)], 64)
