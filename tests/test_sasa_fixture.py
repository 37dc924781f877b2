"""CPU checks of the SASA fixture (tests/golden/make_sasa_golden.py -> sasa.npz) and of the host side of pesto_amd.sasa: this file's own
brute-force restatement of the definition (every j, no pruning) reproduces the golden on the planted cases and on a 300-atom crop of the
MD case; an isolated atom has 4 pi R^2 and two overlapping spheres the analytic cap; the sphere points, the radius table and every
ValueError of shrake_rupley (raised without the library); save_sasa round-trips through h5store."""
import gzip
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

PROBE = np.float32(1.4)


def definition_counts(X, R, S, sizes=None):
    """int [N] for one frame, straight from the definition: every j != i of the structure with finite data, float32 operations"""
    X, R, S = np.asarray(X, np.float32), np.asarray(R, np.float32), np.asarray(S, np.float32)
    out = np.full(X.shape[0], S.shape[0], np.int64)
    start = 0
    with np.errstate(all="ignore"):
        for n in ([X.shape[0]] if sizes is None else sizes):
            x, r = X[start:start + n], R[start:start + n]
            ok = np.isfinite(x).all(1) & np.isfinite(r)
            rr = r * r
            for i in range(n):
                t = x[i] + r[i] * S
                buried = np.zeros(S.shape[0], bool)
                for j in range(n):
                    if j == i or not ok[j]:
                        continue
                    d = t - x[j]
                    buried |= ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < rr[j]
                out[start + i] = S.shape[0] - int(buried.sum())
            start += n
    return out


def areas_of(counts, R, P):
    """float32: ((c0 * count) * R) * R evaluated in double and rounded once"""
    R = np.asarray(R, np.float32).astype(np.float64)
    return (((4.0 * np.pi / P) * np.asarray(counts).astype(np.float64)) * R * R).astype(np.float32)


def areas64(counts, R, P):
    R = np.asarray(R, np.float32).astype(np.float64)
    return ((4.0 * np.pi / P) * np.asarray(counts).astype(np.float64)) * R * R


def group_sums(counts, R, P, rows):
    """float32 [F, G]: the double areas added in atom order (np.add.at adds one element after the other), rounded once"""
    a = areas64(counts, R, P)
    out = np.zeros((a.shape[0], int(rows.max()) + 1))
    for f in range(a.shape[0]):
        np.add.at(out[f], rows.astype(np.int64), a[f])
    return out.astype(np.float32)


def planted_case(g, name):
    return (g[f"planted_{name}_X"], g[f"planted_{name}_R"], int(g[f"planted_{name}_P"]), g[f"planted_{name}_sizes"].tolist(),
            g[f"planted_{name}_counts"].astype(np.int64))


def planted_names(g):
    return [str(n) for n in g["planted_names"]]


def batch_structures(g):
    """[(name, xyz, element)] of the batch case, read with the project's reader"""
    from pesto_amd.structure_io import Structure
    out = []
    for name in g["batch_names"]:
        d = Structure.parse_pdb(gzip.open(os.path.join(GOLDEN, "pdb", str(name) + ".gz"), "rb").read()).to_dict()
        out.append((str(name), d["xyz"], d["element"]))
    return out


def test_restatement_reproduces_the_planted_cases():
    from pesto_amd.sasa import sphere_points
    g = golden("sasa")
    names = planted_names(g)
    assert {"two_spheres", "touching", "q_equals_r2", "coincident", "nonfinite", "single", "one_in_batch", "crop_P1", "crop_P64", "crop_P960",
            "crop_P1000"} <= set(names)
    for name in names:
        X, R, P, sizes, want = planted_case(g, name)
        assert np.array_equal(definition_counts(X, R, sphere_points(P), sizes), want), name
    assert planted_case(g, "two_spheres")[4].tolist() == [712, 712]
    t = planted_case(g, "touching")
    assert t[0][1, 0] < t[0][3, 0] < t[0][5, 0] and t[0][3, 0] == t[1][0] + t[1][1]          # one float32 step either side of R_i + R_j
    q = planted_case(g, "q_equals_r2")
    assert q[2] == 1 and q[4].tolist()[0] == 1 and q[4].tolist()[2] == 0                      # q == R_j^2 is not buried; one step more is
    n = planted_case(g, "nonfinite")
    assert n[4][1] == 960 and n[4][3] == 960 and n[4][5] == 960 and 0 < n[4][0] < 960
    assert planted_case(g, "single")[4].tolist() == [960] and planted_case(g, "one_in_batch")[4][20] == 960


def test_restatement_reproduces_a_crop_of_md():
    g, f = golden("sasa"), golden("frames_md_1JTG_uL")
    X, R = f["X_frames"][0], g["md_R"]
    assert g["md_counts"].shape == (29, 2030) and g["md_counts"].dtype == np.uint16
    # the 300 atoms nearest to atom 1000 with everything that can reach them: atoms within 2 max R + 0.1 of the crop
    order = np.argsort(((X - X[1000]) ** 2).sum(1))
    crop = order[:300]
    d = np.sqrt(((X[:, None, :].astype(np.float64) - X[crop][None].astype(np.float64)) ** 2).sum(-1)).min(1)
    shell = np.nonzero(d < 2.0 * float(R.max()) + 0.1)[0]
    pos = {int(a): k for k, a in enumerate(shell)}
    got = definition_counts(X[shell], R[shell], g["points960"])
    assert np.array_equal(got[[pos[int(a)] for a in crop]], g["md_counts"][0][crop])
    total = float(areas64(g["md_counts"][0], R, 960).sum())
    assert abs(total - 11779.0) < 1.0 and abs((g["md_counts"][0] == 0).mean() - 0.42) < 0.01


def test_analytic_values():
    from pesto_amd.sasa import sphere_points
    R = np.float32(3.2)
    assert areas_of([960], [R], 960)[0] == np.float32(4.0 * np.pi * float(R) * float(R))
    for P in (64, 960, 1000):
        S = sphere_points(P)
        for Rv, dist in ((3.1, 3.0), (2.0, 1.0), (3.0, 5.0)):
            c = definition_counts(np.array([[0, 0, 0], [0, dist, 0]], np.float32), [Rv, Rv], S)
            assert abs(c[0] - P * (1.0 + dist / (2.0 * Rv)) / 2.0) <= 1.0 and c[0] == c[1], (P, Rv, dist, c)


def test_sphere_points():
    from pesto_amd.sasa import MAX_POINTS, sphere_points
    g = golden("sasa")
    assert np.array_equal(sphere_points(), g["points960"]) and sphere_points().dtype == np.float32
    for n in (1, 64, 960, 1000, MAX_POINTS):
        S = sphere_points(n)
        assert S.shape == (n, 3) and np.abs(np.linalg.norm(S.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
        assert np.abs(np.diff(S[:, 1].astype(np.float64)) - 2.0 / n).max() <= 1e-6 if n > 1 else S.tolist() == [[1.0, 0.0, 0.0]]
    for bad in (0, -3, MAX_POINTS + 1):
        with pytest.raises(ValueError, match="n_sphere_points"):
            sphere_points(bad)


def test_atomic_radii():
    from pesto_amd.dataset import STD_ELEMENTS
    from pesto_amd.sasa import VDW_RADII, atomic_radii
    want = {"H": 1.20, "C": 1.70, "N": 1.55, "O": 1.52, "F": 1.47, "P": 1.80, "S": 1.80}
    r = atomic_radii(list(want))
    assert r.dtype == np.float32 and np.array_equal(r, np.array(list(want.values()), np.float32))
    assert np.array_equal(atomic_radii(["c", "ZN", " Se"]), np.array([1.70, VDW_RADII["Zn"], VDW_RADII["Se"]], np.float32))
    every = atomic_radii(np.arange(len(STD_ELEMENTS)))                           # the whole vocabulary has an entry
    assert every.shape == (29,) and np.array_equal(every, atomic_radii(STD_ELEMENTS)) and every.min() >= 1.0 and every.max() <= 3.1
    assert np.array_equal(atomic_radii(["C", "O"], unit="nm"), (np.array([1.70, 1.52]) * 0.1).astype(np.float32))
    g, f = golden("sasa"), golden("frames_md_1JTG_uL")
    assert np.array_equal(atomic_radii(f["q_idx"][:, 0]) + PROBE, g["md_R"])
    assert np.array_equal(np.concatenate([atomic_radii(e) + PROBE for _, _, e in batch_structures(g)]), g["batch_R"])
    for bad in (["Xx"], ["C", "D"], [29], [-1], np.array([0, 30])):
        with pytest.raises(ValueError, match="radii="):
            atomic_radii(bad)
    with pytest.raises(ValueError, match="unit"):
        atomic_radii(["C"], unit="pm")


def test_arguments_raise_before_the_library_is_loaded(monkeypatch):
    from pesto_amd import _lib
    from pesto_amd import sasa as SA

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    m = object()                # no handle either
    x = np.zeros((2, 5, 3), np.float32)
    el = ["C", "N", "O", "S", "C"]
    for kw in (dict(), dict(radii=np.ones(4)), dict(elements=el[:4]), dict(elements=el + ["C"]), dict(elements=["C", "N", "O", "S", "Xx"]),
               dict(elements=el, probe_radius=np.nan), dict(elements=el, probe_radius=-1.0), dict(elements=el, n_sphere_points=0),
               dict(elements=el, n_sphere_points=SA.MAX_POINTS + 1), dict(elements=el, mode="chain"), dict(elements=el, mode="residue"),
               dict(elements=el, mode="residue", residue=[0, 0, 1, 1]), dict(elements=el, mode="residue", residue=[0, 0, 2, 2, 3]),
               dict(elements=el, mode="residue", residue=[0.0, 0.0, 1.0, 1.0, 2.0]), dict(elements=el, sizes=[2, 2]),
               dict(elements=el, sizes=[5, 0]), dict(elements=el, sizes=[6, -1]), dict(elements=el, sizes=[])):
        with pytest.raises(ValueError):
            SA.shrake_rupley(x, model=m, **kw)
    for bad in (np.zeros((5, 2), np.float32), np.zeros((2, 5, 4), np.float32), np.zeros(3, np.float32), np.zeros((0, 3), np.float32),
                np.zeros((1, 2, 5, 3), np.float32)):
        with pytest.raises(ValueError, match="xyz"):
            SA.shrake_rupley(bad, radii=np.ones(5), model=m)
    wide = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2 ** 16, 2 ** 15, 3), (0, 0, 0))       # the shape alone decides
    with pytest.raises(ValueError, match="too large"):
        SA.shrake_rupley(wide, radii=np.lib.stride_tricks.as_strided(np.ones(1, np.float32), (2 ** 15,), (0,)), model=m)
    with pytest.raises(ValueError, match="trajectory"):
        SA.sasa(x[0], elements=el, model=m)
    with pytest.raises(ValueError, match="subunit"):
        SA.buried_area(x, np.ones(5), [0, 0, 1, 1], model=m)
    with pytest.raises(ValueError, match="subunit"):
        SA.buried_area(x, np.ones(5), [0.0, 0.0, 1.0, 1.0, 1.0], model=m)
    with pytest.raises(ValueError):
        SA.structure_sasa({"xyz": np.zeros((2, 3), np.float32)}, model=m)
    with pytest.raises(ValueError, match="radii="):
        SA.structure_sasa({"xyz": np.zeros((2, 3), np.float32), "element": np.array(["C", "Qq"])}, model=m)


def test_save_sasa_round_trips(tmp_path):
    from pesto_amd import h5store
    from pesto_amd.sasa import load_sasa, save_sasa
    if not h5store.available():
        pytest.skip("no HDF5 C library on this machine")
    rng = np.random.default_rng(3)
    res = {"AF-P12345-F1": rng.uniform(0, 1.5, 211).astype(np.float32), "AF-Q9/x": np.array([0.0, 0.25, 1e-7], np.float32)[None]}
    path = save_sasa(str(tmp_path / "sasa.h5"), res)
    assert not os.path.exists(path + ".tmp")
    with h5store.H5Store(path) as hf:
        raw = hf.read("AF-P12345-F1")                                           # the reference's layout: the values as byte strings
        assert raw.dtype.kind == "S" and raw.shape == (211,) and raw.tolist() == res["AF-P12345-F1"].astype(bytes).tolist()
        assert [k.decode() for k in hf.read("metadata/keys")] == list(res)
    back = load_sasa(path)
    assert list(back) == list(res) and all(np.array_equal(back[k], np.ravel(res[k])) for k in res)
    assert load_sasa(save_sasa(str(tmp_path / "empty.h5"), {})) == {}


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """pesto_sasa checks what needs no device data first: PESTO_ERR_INVALID with a message, whatever the handle (none here)."""
    from pesto_amd import _lib
    lib = _lib.load()
    X, R, S = np.zeros((2, 5, 3), np.float32), np.ones(5, np.float32), np.zeros((4, 3), np.float32)
    counts, offs = np.zeros((2, 5), np.int32), np.array([0, 2, 5], np.int32)

    def call(F=2, N=5, ns=2, offsets=offs, P=4, c0=np.pi, out=counts, groups=0, gout=None):
        return lib.pesto_sasa(None, F, N, ns, offsets.ctypes.data, X.ctypes.data, R.ctypes.data, P, S.ctypes.data, c0,
                              None if out is None else out.ctypes.data, None, groups, None, None, None if gout is None else gout.ctypes.data,
                              _lib.PTR_HOST, None)
    for kw in (dict(P=0), dict(P=8193), dict(F=0), dict(N=0), dict(F=2 ** 20, N=2 ** 11), dict(ns=0), dict(offsets=np.array([0, 2, 4], np.int32)),
               dict(offsets=np.array([0, 2, 2, 5], np.int32), ns=3), dict(offsets=np.array([1, 2, 5], np.int32)), dict(c0=np.nan), dict(out=None),
               dict(groups=0, gout=np.zeros((2, 1), np.float32))):
        assert call(**kw) == -1 and lib.pesto_sasa_last_error(), kw
    assert call() != 0 and b"handle" in lib.pesto_sasa_last_error().lower()      # valid arguments reach the handle check
