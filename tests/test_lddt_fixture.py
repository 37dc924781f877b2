"""CPU checks of the definitions behind pesto_amd.lddt and of its host side: the NumPy statements of the reference pairs (pairs_def) and
of the counts and quotients (lddt_def), built on dist_def of the docking fixture, are pinned by hand-worked lattice cases with exact ties
and by the recorded ``iface`` system of tests/golden/docking.npz; bad arguments raise ValueError without a GPU, the header's new symbols
are exported and bound, and the host-side atom matching of structure_lddt does what it says. The definitions are the yardsticks of the
GPU tests (tests/test_lddt.py), which also draws its seeded systems from here."""
import functools
import gzip
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden
from test_docking_fixture import dist_def, system

DEFAULT_T = (0.5, 1, 2, 4)


# ------------------------------------------------------------------ the definitions (NumPy)
def _struct_of(N, sizes):
    offs = np.concatenate([[0], np.cumsum([N] if sizes is None else list(sizes))])
    return np.searchsorted(offs, np.arange(N), "right") - 1


def _mask(sel, N):
    if sel is None:
        return np.ones(N, bool)
    s = np.asarray(sel)
    if s.dtype == np.bool_:
        return s.copy()
    m = np.zeros(N, bool)
    m[s] = True
    return m


def pairs_def(xyz_ref, roa, chain=None, mode="all", sel=None, r_incl=15.0, scale=10.0, sizes=None):
    """(offsets int64 [N + 1], j int32 [K], d_ref float32 [K]): the ordered reference pairs, rows ascending by atom i, j ascending"""
    y = np.asarray(xyz_ref, np.float32).reshape(-1, 3)
    N = y.shape[0]
    roa = np.asarray(roa)
    with np.errstate(invalid="ignore"):                         # (an infinite coordinate: inf - inf)
        D = dist_def(y[None], y[None], scale)[0]
        ok = D < np.float32(r_incl)
    ok &= roa[:, None] != roa[None, :]
    ok &= ~np.eye(N, dtype=bool)
    m = _mask(sel, N)
    ok &= m[:, None] & m[None, :]
    if mode == "inter":
        ok &= np.asarray(chain)[:, None] != np.asarray(chain)[None, :]
    elif mode == "intra":
        ok &= np.asarray(chain)[:, None] == np.asarray(chain)[None, :]
    else:
        assert mode == "all"
    s = _struct_of(N, sizes)
    ok &= s[:, None] == s[None, :]
    i, j = np.nonzero(ok)
    offsets = np.zeros(N + 1, np.int64)
    offsets[1:] = np.cumsum(ok.sum(1))
    return offsets, j.astype(np.int32), D[i, j]


def lddt_def(xyz_ref, xyz, roa, chain=None, mode="all", sel=None, thresholds=DEFAULT_T, r_incl=15.0, scale=10.0, sizes=None, pairs=None):
    """dict of score float32 [F] ([B] with sizes), residue float32 [F, R], preserved int32 [F, R, T], total int32 [R], n_pairs (int, or
    int64 [B] with sizes): the module's definition, frame by frame on dist_def"""
    y = np.asarray(xyz_ref, np.float32).reshape(-1, 3)
    x = np.asarray(xyz, np.float32)
    x = x[None] if x.ndim == 2 else x
    roa = np.asarray(roa)
    N, F, R, T = y.shape[0], x.shape[0], int(roa.max()) + 1, len(thresholds)
    off, j, d = pairs_def(y, roa, chain, mode, sel, r_incl, scale, sizes) if pairs is None else pairs
    i = np.repeat(np.arange(N), np.diff(off))
    total = np.bincount(roa[i], minlength=R).astype(np.int32)
    preserved = np.zeros((F, R, T), np.int32)
    for f in range(F):
        with np.errstate(invalid="ignore"):
            df = dist_def(x[f:f + 1], x[f:f + 1], scale)[0][i, j]
            gap = np.abs(df - d)                                    # float32 - float32: rounded once
            for k, t in enumerate(thresholds):
                preserved[f, :, k] = np.bincount(roa[i][gap < np.float32(t)], minlength=R)
    kept = preserved.sum(2, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        residue = (kept.astype(np.float64) / (T * total.astype(np.int64)).astype(np.float64)[None]).astype(np.float32)
        s_res = np.zeros(R, np.int64)
        s_res[roa] = _struct_of(N, sizes)
        B = 1 if sizes is None else len(sizes)
        score = np.zeros((F, B), np.float32)
        n_pairs = np.zeros(B, np.int64)
        for b in range(B):
            rows = s_res == b
            score[:, b] = (kept[:, rows].sum(1).astype(np.float64) / np.float64(T * int(total[rows].sum(dtype=np.int64)))).astype(np.float32)
            n_pairs[b] = int(total[rows].sum(dtype=np.int64))
    if sizes is None:
        return dict(score=score[:, 0], residue=residue, preserved=preserved, total=total, n_pairs=int(n_pairs[0]))
    return dict(score=score[0], residue=residue, preserved=preserved, total=total, n_pairs=n_pairs)


# ------------------------------------------------------------------ hand-worked cases (integer coordinates, scale 1)
def lattice():
    """Five atoms in four residues and two chains; frame 0 is the reference, frame 1 moves atom 2 from (3, 0, 0) to (4, 0, 0), frame 2
    lacks atom 2 (NaN).
        atom 0 (0, 0, 0)     residue 0  chain 0
        atom 1 (9, 12, 0)    residue 1  chain 0     d(0, 1) = 15 exactly: excluded by the strict test
        atom 2 (3, 0, 0)     residue 2  chain 1     d(0, 2) = 3, and 4 in frame 1: |4 - 3| = 1 is not < 1 and is < 2
        atom 3 (0, 4, 0)     residue 0  chain 0     d(0, 3) = 4 inside the radius, but the same residue: excluded
        atom 4 (100, 0, 0)   residue 3  chain 1     isolated: total 0, NaN
    reference pairs (unordered): {0, 2} d 3; {1, 2} d sqrt(180) = 13.42; {2, 3} d 5; {1, 3} d sqrt(145) = 12.04. K = 8 ordered.
    frame 1: {0, 2} 4, gap 1; {1, 2} 13, gap 0.42; {2, 3} sqrt(32) = 5.66, gap 0.66; {1, 3} unchanged."""
    ref = np.array([[0, 0, 0], [9, 12, 0], [3, 0, 0], [0, 4, 0], [100, 0, 0]], np.float32)
    xyz = np.stack([ref, ref, ref])
    xyz[1, 2] = (4, 0, 0)
    xyz[2, 2] = np.nan
    return dict(ref=ref, xyz=xyz, roa=np.array([0, 1, 2, 0, 3]), chain=np.array([0, 0, 1, 0, 1]), scale=1.0)


LATTICE_ALL = dict(
    offsets=[0, 1, 3, 6, 8, 8], j=[2, 2, 3, 0, 1, 3, 1, 2], n_pairs=8, total=[3, 2, 3, 0],
    preserved=[[[3, 3, 3, 3], [2, 2, 2, 2], [3, 3, 3, 3], [0, 0, 0, 0]],
               [[1, 2, 3, 3], [2, 2, 2, 2], [1, 2, 3, 3], [0, 0, 0, 0]],
               [[1, 1, 1, 1], [1, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0]]],
    residue=[[1, 1, 1, np.nan], [0.75, 1, 0.75, np.nan], [1 / 3, 0.5, 0, np.nan]], score=[1, 26 / 32, 8 / 32])
LATTICE_INTER = dict(n_pairs=6, total=[2, 1, 3, 0], j=[2, 2, 0, 1, 3, 2])        # {0, 2}, {1, 2}, {2, 3}
LATTICE_INTRA = dict(n_pairs=2, total=[1, 1, 0, 0], j=[3, 1])                    # {1, 3}


def test_lattice_all_by_hand():
    s = lattice()
    off, j, d = pairs_def(s["ref"], s["roa"], scale=1.0)
    assert off.tolist() == LATTICE_ALL["offsets"] and j.tolist() == LATTICE_ALL["j"]
    assert d[0] == 3 and d[2] == np.sqrt(np.float32(145)) and d[5] == 5
    assert dist_def(s["ref"][None, :1], s["ref"][None, 1:2], 1.0)[0, 0, 0] == 15.0          # the tie at the radius: exactly 15, out
    assert dist_def(s["ref"][None, :1], s["ref"][None, 3:4], 1.0)[0, 0, 0] == 4.0           # same residue, inside the radius: out
    got = lddt_def(s["ref"], s["xyz"], s["roa"], scale=1.0)
    assert got["n_pairs"] == 8 and got["total"].tolist() == LATTICE_ALL["total"]
    assert got["preserved"].tolist() == LATTICE_ALL["preserved"]
    assert np.array_equal(got["residue"], np.array(LATTICE_ALL["residue"], np.float32), equal_nan=True)
    assert np.array_equal(got["score"], np.array(LATTICE_ALL["score"], np.float32))
    # the tie at a threshold: d_ref = 3, d_f = 4 is not preserved at 1 and is at 2
    assert got["preserved"][1, 2].tolist() == [1, 2, 3, 3] and got["preserved"][1, 0, 1] == 2
    # a radius just above the tie takes the pair in
    assert pairs_def(s["ref"], s["roa"], r_incl=np.nextafter(np.float32(15), np.float32(16)), scale=1.0)[0][-1] == 10


def test_lattice_two_chains_by_hand():
    s = lattice()
    for mode, want in (("inter", LATTICE_INTER), ("intra", LATTICE_INTRA)):
        off, j, _ = pairs_def(s["ref"], s["roa"], s["chain"], mode, scale=1.0)
        got = lddt_def(s["ref"], s["xyz"], s["roa"], s["chain"], mode, scale=1.0)
        assert got["n_pairs"] == want["n_pairs"] == off[-1] and got["total"].tolist() == want["total"] and j.tolist() == want["j"]
    inter = lddt_def(s["ref"], s["xyz"], s["roa"], s["chain"], "inter", scale=1.0)
    assert inter["preserved"][1].tolist() == [[0, 1, 2, 2], [1, 1, 1, 1], [1, 2, 3, 3], [0, 0, 0, 0]]
    assert np.array_equal(inter["score"], np.array([1, 18 / 24, 0], np.float32))           # frame 2: every inter pair holds atom 2
    intra = lddt_def(s["ref"], s["xyz"], s["roa"], s["chain"], "intra", scale=1.0)
    assert np.array_equal(intra["score"], np.array([1, 1, 1], np.float32)) and np.isnan(intra["residue"][:, 2:]).all()


def test_selection_batch_and_missing_reference_atoms():
    s = lattice()
    got = lddt_def(s["ref"], s["xyz"], s["roa"], sel=[0, 1, 3, 4], scale=1.0)              # without atom 2: {1, 3} alone
    assert got["n_pairs"] == 2 and got["total"].tolist() == [1, 1, 0, 0] and np.array_equal(got["score"], np.ones(3, np.float32))
    ref = s["ref"].copy()
    ref[2, 1] = np.nan                                                                      # a reference atom without coordinates
    got = lddt_def(ref, s["xyz"], s["roa"], scale=1.0)
    assert got["n_pairs"] == 2 and got["total"].tolist() == [1, 1, 0, 0]
    # two structures back to back: atoms 0 .. 2 and 3 .. 4 (residues 0, 1, 2 | 3, 4); the pairs {2, 3} and {1, 3} cross and vanish
    roa = np.array([0, 1, 2, 3, 4])
    got = lddt_def(s["ref"], s["xyz"][1], roa, scale=1.0, sizes=[3, 2])
    assert got["n_pairs"].tolist() == [4, 0] and got["total"].tolist() == [1, 1, 2, 0, 0]
    assert got["score"][0] == np.float32(12 / 16) and np.isnan(got["score"][1])
    nan_frame = np.full((1, 5, 3), np.nan, np.float32)
    got = lddt_def(s["ref"], nan_frame, s["roa"], scale=1.0)                               # a frame without any atom scores 0, not NaN
    assert got["score"][0] == 0 and got["preserved"].sum() == 0 and np.isnan(got["residue"][0, 3])


# ------------------------------------------------------------------ the recorded system
@functools.lru_cache(maxsize=None)
def iface():
    """the recorded interface of the docking fixture as an lDDT input: xyz [32, 1408, 3] nm, roa, chain (0 on ids_a, 1 on ids_b), ca"""
    s = system(golden("docking"), "iface")
    chain = np.full(s["roa"].size, 2, np.int64)
    chain[s["ids_a"]], chain[s["ids_b"]] = 0, 1
    return dict(xyz=s["xyz"], roa=s["roa"], chain=chain, ca=s["ca"])


@functools.lru_cache(maxsize=None)
def iface_def(mode="all", ca=False):
    s = iface()
    return lddt_def(s["xyz"][0], s["xyz"], s["roa"], s["chain"], mode, s["ca"] if ca else None)


def test_recorded_interface():
    s = iface()
    assert s["xyz"].shape == (32, 1408, 3) and int(s["roa"].max()) + 1 == 178 and set(s["chain"].tolist()) == {0, 1}
    off, j, d = pairs_def(s["xyz"][0], s["roa"])
    n = np.diff(off)
    assert off[-1] == 505876 and n.min() == 63 and n.max() == 688
    assert pairs_def(s["xyz"][0], s["roa"], s["chain"], "inter")[0][-1] == 145372
    got = iface_def()
    assert got["n_pairs"] == 505876 and got["score"][0] == 1.0 and np.all(got["residue"][0] == 1.0)
    assert 0.685 <= got["score"].min() < 0.695
    assert iface_def("inter")["n_pairs"] == 145372


# ------------------------------------------------------------------ seeded systems of the GPU sweep
def hub_system(seed, ks=(0, 1, 63, 64, 65, 129, 255, 256, 257), F=2, sat_res=70):
    """Far-apart hubs, hub h with ks[h] satellites within 7 A of it (so within 15 A of each other) in residues of at most sat_res atoms
    that belong to no other hub; every hub a residue of one atom. The hub's row has ks[h] entries. Chains alternate over the satellites.
    Angstroms, scale 1. Frame 0 is the reference; the others add noise of 0.6 A, so gaps fall on both sides of every threshold."""
    rng = np.random.default_rng(seed)
    pos, roa, chain, r = [], [], [], 0
    for h, k in enumerate(ks):
        c = np.array([200.0 * h, 50.0 * (h % 3), 0.0])
        pos.append(c); roa.append(r); chain.append(0)
        r += 1
        v = rng.normal(size=(k, 3))
        v = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(1.0, 7.0, (k, 1))
        for a in range(k):
            pos.append(c + v[a]); roa.append(r + a // sat_res); chain.append(a % 2)
        r += -(-k // sat_res)
    ref = np.array(pos, np.float32)
    xyz = np.stack([ref] + [ref + rng.normal(0, 0.6, ref.shape).astype(np.float32) for _ in range(F - 1)])
    return dict(ref=ref, xyz=xyz, roa=np.array(roa), chain=np.array(chain), scale=1.0)


def random_system(seed, N, R, F, box=22.0, nan_atoms=0):
    """N atoms uniform in a box of `box` A, rows 0 .. R - 1 dealt at random (a residue's atoms are not adjacent; every row has an atom),
    two chains by residue, F frames: the reference, then copies with noise between 0.2 and 1.5 A; nan_atoms atoms of the last frame
    missing."""
    rng = np.random.default_rng(seed)
    ref = rng.uniform(0, box, (N, 3)).astype(np.float32)
    roa = np.concatenate([np.arange(R), rng.integers(0, R, N - R)])
    rng.shuffle(roa)
    chain = (roa % 2).astype(np.int64)
    xyz = np.stack([ref] + [ref + rng.normal(0, rng.uniform(0.2, 1.5), ref.shape).astype(np.float32) for _ in range(F - 1)])
    if nan_atoms:
        xyz[-1, rng.choice(N, nan_atoms, replace=False)] = np.nan
    return dict(ref=ref, xyz=xyz, roa=roa, chain=chain, scale=1.0)


def test_hub_rows_have_the_prescribed_lengths():
    s = hub_system(1)
    n = np.diff(pairs_def(s["ref"], s["roa"], scale=1.0)[0])
    assert {0, 1, 63, 64, 65, 129, 255, 256, 257} <= set(n.tolist())     # the wave's 64 lanes and its four chunks in flight
    cnt = np.bincount(s["roa"])
    assert cnt.min() == 1 and cnt.max() == 70
    got = lddt_def(s["ref"], s["xyz"], s["roa"], scale=1.0)
    assert got["score"][0] == 1.0 and 0 < got["score"][1] < 1 and np.isnan(got["residue"][:, 0]).all()         # hub 0 is alone


# ------------------------------------------------------------------ the host side of pesto_amd.lddt
def test_arguments_raise_before_any_launch():
    from pesto_amd import lddt as L
    m = object()                # no handle: the checks must come first
    y, x = np.zeros((5, 3), np.float32), np.zeros((4, 5, 3), np.float32)
    roa, chain = np.array([0, 0, 1, 1, 2]), np.array([0, 0, 0, 1, 1])
    bad = (dict(xyz=x[:, :4]), dict(xyz=x[:, :, :2]), dict(xyz_ref=np.zeros((2, 5, 3), np.float32)), dict(res_of_atom=roa[:4]),
           dict(res_of_atom=roa * 1.0), dict(res_of_atom=-roa), dict(res_of_atom=np.array([0, 0, 1, 1, 3])), dict(thresholds=(1, 0.5)),
           dict(thresholds=(1, 1)), dict(thresholds=()), dict(thresholds=tuple(range(1, 10))), dict(thresholds=(0, 1)), dict(thresholds=(1, np.nan)),
           dict(mode="inter"), dict(mode="intra"), dict(mode="both"), dict(chain_of_atom=chain[:4], mode="inter"), dict(chain_of_atom=chain * 0.5),
           dict(sel=[0, 5]), dict(sel=np.ones(4, bool)), dict(sel=np.zeros(5)), dict(r_incl=0.0), dict(r_incl=np.nan), dict(r_incl=-1.0),
           dict(scale=0.0), dict(scale=np.inf), dict(sizes=[2, 2], xyz=x[:1]), dict(sizes=[5, 0], xyz=x[:1]), dict(sizes=[1, 4], xyz=x[:1]),
           dict(pairs=(np.zeros(6, np.int64),)), dict(pairs=(np.zeros(5, np.int64), np.zeros(2, np.int32), np.zeros(2, np.float32))),
           dict(pairs=(np.zeros(6, np.int64), np.zeros(2, np.int32), np.zeros(3, np.float32))))
    for kw in bad:
        args = dict(xyz_ref=y, xyz=x, res_of_atom=roa, model=m)
        args.update(kw)
        with pytest.raises(ValueError):
            L.lddt(**args)
    with pytest.raises(ValueError, match="one model"):           # sizes that add up, but several frames
        L.lddt(y, x, np.array([0, 0, 1, 2, 2]), sizes=[3, 2], model=m)
    with pytest.raises(ValueError, match="structure after structure"):          # residue 1 spans the two structures
        L.lddt(y, x[:1], np.array([0, 1, 1, 1, 2]), sizes=[3, 2], model=m)
    long = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2 ** 23 + 1, 5, 3), (0, 0, 0))
    with pytest.raises(ValueError, match="frames"):
        L.lddt(y, long, roa, model=m)
    for kw in (dict(res_of_atom=roa[:4]), dict(mode="inter"), dict(sel=[7]), dict(r_incl=np.inf), dict(sizes=[1, 1]), dict(xyz_ref=x)):
        args = dict(xyz_ref=y, res_of_atom=roa, model=m)
        args.update(kw)
        with pytest.raises(ValueError):
            L.reference_pairs(**args)
    with pytest.raises(ValueError):
        L.ilddt(y, x, roa, None, model=m)
    with pytest.raises(ValueError):
        L.lddt_ca(y, x, roa, np.ones(5, bool), sel=[0], model=m)


def test_new_symbols_are_declared_exported_and_bound():
    from pesto_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    new = ["pesto_lddt_last_error", "pesto_lddt_pairs", "pesto_lddt"]
    lib = _lib.load()
    for name in new:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.pesto_lddt_last_error.restype is not None
    assert int(re.search(r"PESTO_LDDT_MAX_FRAMES = 1 << (\d+)", hdr).group(1)) == 23
    assert int(re.search(r"PESTO_LDDT_MAX_ENTRIES = 1 << (\d+)", hdr).group(1)) == 30
    assert int(re.search(r"PESTO_LDDT_MAX_THRESHOLDS = (\d+)", hdr).group(1)) == 8
    import pesto_amd
    from pesto_amd import lddt
    assert lddt.MAX_FRAMES == 2 ** 23 and lddt.MAX_ENTRIES == 2 ** 30 and lddt.MAX_THRESHOLDS == 8
    assert pesto_amd.ilddt is lddt.ilddt and pesto_amd.reference_pairs is lddt.reference_pairs and pesto_amd.structure_lddt is lddt.structure_lddt
    assert pesto_amd.lddt_ca is lddt.lddt_ca and lddt.Lddt._fields == ("score", "residue", "preserved", "total", "n_pairs")
    src = open(os.path.join(ROOT, "pesto_amd", "csrc", "pesto_lddt.hip")).read()
    assert "asm" not in src and "atomicAdd" not in src                  # plain C++: no inline assembly, no sums through atomics


# ------------------------------------------------------------------ structure_lddt's atom matching
def perturbed_1thf(seed=3):
    """(reference dict, model dict, removed residue key, swapped atom rows): 1thf_D cleaned by structure_io, and a copy with noise of
    0.5 A, residue 10 of the list removed, two atoms of another residue exchanged in the file order and one atom that the reference lacks"""
    from pesto_amd.structure_io import Structure
    with gzip.open(os.path.join(GOLDEN, "pdb", "1thf_D.pdb.gz"), "rt") as f:
        ref = Structure.parse_pdb(f.read()).preprocess().to_dict()
    rng = np.random.default_rng(seed)
    keys = list(dict.fromkeys(zip(ref["chain_name"].tolist(), ref["resid"].tolist())))
    gone = keys[10]
    keep = ~((ref["chain_name"] == gone[0]) & (ref["resid"] == gone[1]))
    order = np.nonzero(keep)[0]
    a = int(np.nonzero((ref["resid"][order] == keys[20][1]) & (ref["chain_name"][order] == keys[20][0]))[0][0])
    order[[a, a + 1]] = order[[a + 1, a]]
    model = {k: np.asarray(v)[order] for k, v in ref.items()}
    model["xyz"] = (model["xyz"] + rng.normal(0, 0.5, model["xyz"].shape)).astype(np.float32)
    extra = {k: np.asarray(v)[:1].copy() for k, v in model.items()}
    extra["name"][:] = "XX"
    model = {k: np.concatenate([model[k], extra[k]]) for k in model}
    return ref, model, gone, (int(order[a]), int(order[a + 1]))


def test_structure_matching_on_1thf():
    from pesto_amd.lddt import match_atoms
    ref, model, gone, (p, q) = perturbed_1thf()
    y, x, res, chain, table = match_atoms(ref, model)
    N = ref["xyz"].shape[0]
    assert y.shape == (N, 3) and x.shape == (1, N, 3) and np.array_equal(y, ref["xyz"])
    missing = (ref["chain_name"] == gone[0]) & (ref["resid"] == gone[1])
    assert missing.sum() > 3 and np.array_equal(np.isnan(x[0]).any(1), missing)            # the removed residue, and nothing else, is NaN
    assert np.abs(x[0, ~missing] - y[~missing]).max() < 4.0 and np.abs(x[0, ~missing] - y[~missing]).max() > 0.5
    back = {tuple(np.round(v, 3)) for v in model["xyz"][:-1].tolist()}                      # every model atom but the extra one is placed
    assert {tuple(np.round(v, 3)) for v in x[0, ~missing].tolist()} == back
    row = {k: n for n, k in enumerate(zip(model["chain_name"].tolist(), model["resid"].tolist(), model["name"].tolist()))}
    for n in (p, q, 0, N - 1):                                                              # the exchanged atoms sit under their own names
        assert np.array_equal(x[0, n], model["xyz"][row[(ref["chain_name"][n], int(ref["resid"][n]), ref["name"][n])]])
    R = len(table["resid"])
    assert res.min() == 0 and res.max() == R - 1 and np.all(np.diff(res) >= 0) and R == len(set(zip(ref["chain_name"].tolist(), ref["resid"].tolist())))
    assert np.array_equal(table["resid"][res], ref["resid"]) and np.array_equal(table["chain_name"][res], ref["chain_name"])
    assert len(set(chain.tolist())) == len(set(ref["chain_name"].tolist()))
    with pytest.raises(ValueError):
        match_atoms({}, model)


def _pdb_without(text, resnum):
    """the PDB text without the ATOM / HETATM records of residue number resnum (columns 23-26)"""
    return "".join(ln for ln in text.splitlines(True) if not (ln[:6] in ("ATOM  ", "HETATM") and int(ln[22:26]) == resnum))


def test_two_files_match_on_their_own_residue_numbers(tmp_path):
    """Two PDB paths whose residue sets differ: the files' residue numbers decide, not the residues' ordinals. The same coordinates on
    both sides, so every atom that both files hold must sit under itself, and only the missing residue may be NaN."""
    from pesto_amd.lddt import match_atoms
    from pesto_amd.structure_io import Structure
    with gzip.open(os.path.join(GOLDEN, "pdb", "1thf_D.pdb.gz"), "rt") as f:
        text = f.read()
    raw = Structure.parse_pdb(text).to_dict()
    heavy = ~(np.isin(raw["resname"], ("HOH", "DOD")) | np.isin(raw["element"], ("H", "D")))
    numbers = list(dict.fromkeys(raw["resid"][heavy].tolist()))
    gone = int(numbers[2])                                          # the third residue of the file: everything behind it would shift
    full, cut = str(tmp_path / "full.pdb"), str(tmp_path / "cut.pdb")
    open(full, "w").write(text)
    open(cut, "w").write(_pdb_without(text, gone))
    # (a) the model lacks a residue
    y, x, res, chain, table = match_atoms(full, cut)
    assert np.array_equal(y, raw["xyz"][heavy]) and x.shape == (1, y.shape[0], 3)
    missing = raw["resid"][heavy] == gone
    assert 3 < missing.sum() < 30 and np.array_equal(np.isnan(x[0]).any(1), missing)
    assert np.array_equal(x[0, ~missing], y[~missing])              # every atom of both files under itself
    assert np.array_equal(table["resid"], np.array(numbers)) and np.array_equal(table["resid"][res], raw["resid"][heavy])       # the file's numbers
    assert len(table["resid"]) == len(numbers) and table["resname"][res].tolist() == raw["resname"][heavy].tolist()
    # (b) the reference lacks one: its atoms all match, the model's extra residue is dropped
    y2, x2, res2, _, table2 = match_atoms(cut, full)
    assert np.array_equal(y2, y[~missing]) and np.array_equal(x2[0], y2) and not np.isnan(x2).any()
    assert np.array_equal(table2["resid"], np.array([n for n in numbers if n != gone])) and int(res2.max()) + 1 == len(numbers) - 1
    # a file against itself
    y3, x3, res3, _, _ = match_atoms(full, full)
    assert np.array_equal(x3[0], y3) and np.array_equal(res3, res)
