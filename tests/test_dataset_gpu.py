"""GPU checks of the dataset build (pesto_contacts): contact dicts bit-exact against the reference's recorded output through host and
device pointers and batch vs one assembly per call, typed keys / T / metadata exact, the whole build_dataset tree read back equal to
the recorded tree, ContactsDataset items equal to the reference's, a large synthetic assembly against the NumPy restatement, and the
uint16 refusal."""
import os
import re

import numpy as np
import pytest

import dataset_fixture as fx
from conftest import GOLDEN, weights
from pesto_amd import dataset, h5store
from pesto_amd.topology import _norm_xyz, extract_topology

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    import torch
    from pesto_amd import Model
    from pesto_amd.config import CONFIGS
    assert torch.cuda.is_available()
    m = Model(CONFIGS["i_v4_0"]).to("cuda:0")
    m.load_state_dict(weights("i_v4_0"))
    return m


def _assert_contacts(got, g):
    ref = fx.contacts(g)
    assert [(a, b) for a in got for b in got[a]] == [(a, b) for a, b, _, _ in ref]
    for ci, cj, ids, d in ref:
        gi, gd = dataset._lib.host(got[ci][cj]["ids"]), dataset._lib.host(got[ci][cj]["d"])
        assert gi.dtype == np.int64 and gd.dtype == np.float32
        np.testing.assert_array_equal(gi, ids)
        assert gd.view(np.int32).tolist() == d.view(np.int32).tolist()


@pytest.mark.parametrize("on_device", [False, True])
def test_contacts_bit_exact_single_and_batch(model, on_device):
    subs = {c: fx.subunits_of(c) for c in fx.CASES}
    cases = [c for c in fx.CASES if subs[c] is not None]
    batch = dataset.extract_all_contacts_batch(model, [subs[c] for c in cases], on_device=on_device)
    for c, got in zip(cases, batch):
        _assert_contacts(got, fx.load(c))
        one = dataset.extract_all_contacts(model, subs[c], on_device=on_device)
        if on_device:
            for a in got:
                for b in got[a]:
                    assert got[a][b]["ids"].is_cuda and got[a][b]["d"].is_cuda
        _assert_contacts(one, fx.load(c))


def _ids_topk_equal(ids, ref, X):
    """exact, or the same float32 keys where the reference's keys tie: key = d, plus max(D) over the structure for d < 1e-2
    (src/data_encoding.py:87-99; self and coincident atoms go last, and tie with the structure's farthest pair when N <= 64)"""
    if np.array_equal(ids, ref):
        return True
    if ids.shape != ref.shape:
        return False
    dmax = max(float(_norm_xyz(X[i:i + 256, None, :] - X[None, :, :]).astype(np.float32).max()) for i in range(0, X.shape[0], 256))

    def key(t):
        d = _norm_xyz(X[t.astype(np.int64)] - X[:, None, :]).astype(np.float32)
        return np.where(d < 1e-2, d + np.float32(dmax), d)
    return np.array_equal(key(ids), key(ref))


@pytest.mark.parametrize("case", [c for c in fx.CASES if c != "monomer"])
def test_pack_dataset_items_match_recorded_tree(model, case):
    g = fx.load(case)
    sub = fx.subunits_of(case)
    contacts = dataset.extract_all_contacts(model, sub)
    sd, cd = dataset.pack_dataset_items(model, sub, contacts)
    ds, at = fx.unpack(g, "ds"), fx.attrs(g)
    key = f"{str(g['pdbid']).upper()[1:3]}/{str(g['pdbid']).upper()}/{g['bid']}"
    want_groups = [str(p) for p in g["groups"]]
    got_groups = []
    for c0 in cd:
        got_groups.append(f"data/structures/{key}/{c0}")
        got_groups += [f"data/contacts/{key}/{c0}/{c1}" for c1 in cd[c0]]
    assert got_groups == want_groups
    assert sorted(sd) == sorted(cd)      # (structures_data follows contacts; contacts_data the partner-side inserts)
    for c0, (data, attrs) in sd.items():
        p = f"data/structures/{key}/{c0}"
        for k, v in data.items():
            if k == "ids_topk":
                ref = ds.get(p + "/ids_topk")
                if ref is None:
                    ref = extract_topology(data["X"], 64)
                assert v.dtype == np.uint16 and _ids_topk_equal(v, ref, data["X"]), (p, k)
            else:
                assert v.dtype == ds[f"{p}/{k}"].dtype, (p, k)
                np.testing.assert_array_equal(v, ds[f"{p}/{k}"], err_msg=f"{p}/{k}")
        assert sorted(attrs) == sorted(at[p])
        for k, v in attrs.items():
            np.testing.assert_array_equal(np.asarray(v, np.int64), at[p][k])
    for c0 in cd:
        for c1, (data, attrs) in cd[c0].items():
            p = f"data/contacts/{key}/{c0}/{c1}"
            assert data["Y"].dtype == np.uint16
            np.testing.assert_array_equal(data["Y"], ds[p + "/Y"], err_msg=p)
            np.testing.assert_array_equal(np.asarray(attrs["Y_shape"], np.int64), at[p]["Y_shape"])
            assert attrs["ctype"].dtype == bool
            np.testing.assert_array_equal(attrs["ctype"], at[p]["ctype"])


def _pdb_key(path):
    m = re.match(r".*/([A-Za-z0-9]*)\.pdb([0-9]*)\.gz", path)
    return m[1].lower(), m[2]


@pytest.mark.parametrize("compression", [None, "gzip"])
def test_build_dataset_tree_and_items(model, tmp_path, compression):
    try:
        h5store.load()
    except h5store.H5Unavailable:
        pytest.skip("no HDF5 C library")
    paths = [os.path.join(GOLDEN, "pdb", f"{c}.pdb1.gz") for c in fx.PDB_CASES] + [os.path.join(GOLDEN, "pdb", "missing.pdb1.gz")]
    out = str(tmp_path / "contacts.h5")
    errors = []
    summary = dataset.build_dataset(model, paths, out, key_of=_pdb_key, compression=compression, on_error=errors.append, workers=3,
                                    batch_atoms=12000)
    assert summary["read"] == 6 and summary["skipped"]["unreadable"] == 1 and len(errors) == 1
    want_groups, want_meta = [], {"keys": [], "sizes": [], "ckeys": [], "ctypes": []}
    n_rows = 0
    with h5store.H5Store(out) as hf:
        names = set(hf.keys())
        for c in fx.PDB_CASES:
            g = fx.load(c)
            ds, at = fx.unpack(g, "ds"), fx.attrs(g)
            want_groups += [str(p) for p in g["groups"]]
            for k, v in ds.items():
                if k.startswith("metadata/"):
                    continue
                r = hf.read(k)
                assert r.dtype == v.dtype, k
                np.testing.assert_array_equal(r, v, err_msg=k)
            for p in g["groups"]:
                p = str(p)
                if p.startswith("data/structures/"):
                    X = hf.read(p + "/X")
                    assert _ids_topk_equal(hf.read(p + "/ids_topk"), extract_topology(X, 64), X), p
                got = hf.attrs(p)
                assert sorted(got) == sorted(at[p]), p
                for k, v in at[p].items():
                    assert got[k].dtype == v.dtype, (p, k)
                    np.testing.assert_array_equal(got[k], v)
            for k in ("keys", "sizes", "ckeys"):
                want_meta[k].append(ds["metadata/" + k])
            ct = ds["metadata/ctypes"].copy()
            ct[:, 0] += n_rows
            want_meta["ctypes"].append(ct)
            n_rows += ds["metadata/keys"].shape[0]
        n_ds = sum(len([k for k in fx.unpack(fx.load(c), "ds") if not k.startswith("metadata/")]) for c in fx.PDB_CASES)
        n_topk = sum(1 for p in want_groups if p.startswith("data/structures/"))
        assert len([k for k in names if not k.startswith("metadata/")]) == n_ds + n_topk
        assert summary["structures"] == n_topk and summary["contacts"] == len(want_groups) - n_topk
        for k in ("keys", "ckeys"):
            assert hf.read("metadata/" + k).astype(str).tolist() == np.concatenate(want_meta[k]).astype(str).tolist()
        s = hf.read("metadata/sizes")
        assert s.dtype == np.int64
        np.testing.assert_array_equal(s, np.concatenate(want_meta["sizes"]))
        c = hf.read("metadata/ctypes")
        assert c.dtype == np.uint32
        np.testing.assert_array_equal(c, np.concatenate(want_meta["ctypes"]))
        for k, v in (("mids", dataset.MOLECULE_IDS), ("std_elements", dataset.STD_ELEMENTS), ("std_resnames", dataset.STD_RESNAMES),
                     ("std_names", dataset.STD_NAMES)):
            r = hf.read("metadata/" + k)
            assert r.dtype.kind == "S" and r.astype(str).tolist() == v.tolist()
    from test_dataset_fixture import check_items
    check_items(dataset.ContactsDataset(out), fx.PDB_CASES)


def test_large_synthetic_against_numpy(model):
    rng = np.random.default_rng(3)
    subs = {}
    for k in range(50):
        n = 160
        c = rng.uniform(0, 40, 3)
        xyz = (c + rng.normal(0, 4.0, (n, 3))).astype(np.float32)
        subs[f"S{k:02d}"] = {"xyz": xyz, "resid": np.repeat(np.arange(n // 8), 8),
                             "resname": np.array([["ALA", "GLY", "ZN", "XYZ"][(k + r) % 4] for r in np.repeat(np.arange(n // 8), 8)])}
    want = fx.np_contacts(subs)
    got = dataset.extract_all_contacts(model, subs)
    assert sum(len(v) for v in got.values()) == 2 * len(want)
    for ci, cj, ids, d in want:
        np.testing.assert_array_equal(dataset._lib.host(got[ci][cj]["ids"]), ids)
        assert dataset._lib.host(got[ci][cj]["d"]).view(np.int32).tolist() == d.view(np.int32).tolist()
    rows = dataset._subunit_rows(subs, dataset.MOLECULE_IDS)
    out, meta = dataset._contacts_call(model, [rows], 5.0, dataset.MOLECULE_IDS, False)
    typed = dataset._typed_items(out, meta, [{r[0]: r[4] for r in rows}], len(dataset.MOLECULE_IDS))[0]
    n = 0
    for ci, cj, ids, _ in want:
        Y, T = fx.np_typed_keys(subs[ci], subs[cj], ids, dataset.MOLECULE_IDS)
        if not Y.shape[0]:
            assert (ci, cj) not in typed
            continue
        (f, fa), (r, ra) = typed[(ci, cj)]
        np.testing.assert_array_equal(f["Y"], Y)
        np.testing.assert_array_equal(fa["ctype"], T)
        np.testing.assert_array_equal(r["Y"], np.unique(Y[:, [1, 0, 3, 2]], axis=0))
        n += 1
    assert n == len(typed) > 0


def test_uint16_refusal(model):
    n = 70000
    xyz = np.stack([np.arange(n) * 0.9, np.zeros(n), np.zeros(n)], 1).astype(np.float32)
    subs = {"A:0": {"xyz": xyz, "name": np.array(["CA"] * n), "element": np.array(["C"] * n), "resname": np.array(["ALA"] * n),
                    "resid": np.arange(n) // 10, "het_flag": np.array(["A"] * n)},
            "B:0": {"xyz": xyz[:4] + np.float32([0, 3, 0]), "name": np.array(["CA"] * 4), "element": np.array(["C"] * 4),
                    "resname": np.array(["GLY"] * 4), "resid": np.arange(4), "het_flag": np.array(["A"] * 4)}}
    contacts = dataset.extract_all_contacts(model, subs)
    assert "A:0" in contacts and "B:0" in contacts["A:0"]
    with pytest.raises(ValueError, match="uint16"):
        dataset.pack_dataset_items(model, subs, contacts)
