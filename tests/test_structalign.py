"""GPU tests of pesto_amd.structalign (pesto_structalign.hip) against the NumPy definition of test_structalign_fixture.py, through host
arrays and ROCm tensors. The sweep pairs keep the two decision margins (asserted by the fixture), so every integer - map, n_aligned,
n_ident, dp_score, the history's scores and counts, and with them which rounds ran - is compared by equality; tm_r, tm_a and tm_b within
one float32 unit of the definition's; the chosen (unit, round) by the definition's tm64 within 1e-12, and the outputs are the
definition's for that choice; the transform by orthonormality within 1e-12 and by the tm it reproduces in NumPy. tm_a, tm_b and rmsd
equal a hand call of tmscore.tm_score on the gathered pairs bit for bit."""
import gzip
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_docking_fixture import ulp_apart
from test_sequences_fixture import pdb_path
from test_structalign_fixture import (BLOCKS, LONGEST, SWEEP, chosen_def, disagreeing_pair, planted_deletion, structalign_def, sweep_def,
                                      sweep_pair)
from test_tmscore_fixture import d0_def, domain16

pytestmark = pytest.mark.gpu

FIELDS = ("map", "n_aligned", "n_ident", "dp_score", "unit", "round", "tm_a", "tm_b", "rotation", "translation", "rmsd", "history")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same_bits(a, b):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(host(b))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run(chains, pairs=None, on_device=False, **kw):
    from pesto_amd import structalign as SA
    coords = np.concatenate(chains)
    return SA.align_structures(dev(coords) if on_device else coords, [c.shape[0] for c in chains], pairs, **kw)


def pair_of(out, p):
    """the outputs of pair p on the host, as a dict"""
    o = {k: host(getattr(out, k)) for k in FIELDS}
    lo, hi = int(out.map_offsets[p]), int(out.map_offsets[p + 1])
    return {k: (v[lo:hi] if k == "map" else v[p]) for k, v in o.items()}


def check(got, want, a, b, scale=10.0, codes=None, tag=""):
    """every assertion of the sweep on one pair's outputs"""
    m, n = a.shape[0], b.shape[0]
    h, hw = got["history"], want["history"]
    assert h.shape == hw.shape, tag
    print(f"{tag}: winner {got['unit']}, {got['round']} (definition {want['unit']}, {want['round']}), tm {got['tm_a']:.6f} / {got['tm_b']:.6f}, "
          f"n_aligned {got['n_aligned']}, rounds run {np.isfinite(h[:, :, 0]).sum(1).tolist()}")
    assert np.array_equal(np.isnan(h), np.isnan(hw)), (tag, "the rounds that ran")
    assert np.array_equal(np.nan_to_num(h[..., 1:], nan=-7), np.nan_to_num(hw[..., 1:], nan=-7)), (tag, "dp_score and n_aligned of every round")
    ran = np.isfinite(hw[..., 0])
    assert ulp_apart(h[..., 0][ran].astype(np.float32), hw[..., 0][ran].astype(np.float32)) <= 1, tag
    u, r = int(got["unit"]), int(got["round"])
    assert u >= 0 and ran[u, r], tag
    assert np.nanmax(want["tm64"]) - want["tm64"][u, r] <= 1e-12, (tag, "the chosen unit and round attain the maximum")
    ca, cb = (None, None) if codes is None else codes
    w = chosen_def(a, b, want, u, r, codes_a=ca, codes_b=cb, scale=scale)
    assert np.array_equal(got["map"], w["map"]) and got["map"].dtype == np.int32, tag
    for k in ("n_aligned", "n_ident", "dp_score"):
        assert int(got[k]) == w[k], (tag, k)
    assert ulp_apart(np.array([got["tm_a"], got["tm_b"]], np.float32), np.array([w["tm_a"], w["tm_b"]], np.float32)) <= 1, tag
    R, t = got["rotation"], got["translation"]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1) <= 1e-12, tag
    hit = np.nonzero(got["map"] >= 0)[0]
    X, Y = a[hit].astype(np.float64), b[got["map"][hit]].astype(np.float64)
    lnorm = min(m, n)
    D = np.sqrt(((X @ R + t - Y) ** 2).sum(-1)) * scale
    again = np.float32((1.0 / (1.0 + (D / d0_def(lnorm)) ** 2)).sum() / lnorm)
    assert ulp_apart(np.array([got["tm_a"] if m <= n else got["tm_b"]], np.float32), np.array([again], np.float32)) <= 1, tag


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", SWEEP + [BLOCKS], ids=lambda c: "m%d-n%d" % c[:2])
def test_seeded_sweep(case, on_device):
    a, b = sweep_pair(*case[:3])
    out = run([a, b], [[0, 1]], on_device, frag_starts=case[3])
    for k in FIELDS:
        v = getattr(out, k)
        assert v.is_cuda if on_device else isinstance(v, np.ndarray), k
    check(pair_of(out, 0), sweep_def(*case), a, b, tag="m%d-n%d" % case[:2])


def by_hand(a, b, amap, scale, on_device=False):
    """(tm_a, tm_b, rmsd) of tmscore.tm_score called by hand on the gathered pairs"""
    from pesto_amd import tmscore as T
    hit = np.nonzero(amap >= 0)[0]
    place = dev if on_device else np.ascontiguousarray
    X, Y = place(a[hit][None]), place(b[amap[hit]])
    m, n = a.shape[0], b.shape[0]
    ta = T.tm_score(Y, X, norm_len=m, d0=T.default_d0(m), step=1, scale=scale)
    tb = T.tm_score(Y, X, norm_len=n, d0=T.default_d0(n), step=1, scale=scale)
    return ta, tb


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_scores_are_a_hand_call_of_tm_score(on_device):
    chains = [sweep_pair(65, 63, 0)[0], sweep_pair(65, 63, 0)[1], sweep_pair(30, 36, 1)[0], sweep_pair(30, 36, 1)[1], sweep_pair(129, 127, 0)[0]]
    pairs = [[0, 1], [2, 3], [1, 4], [3, 0], [4, 4]]
    out = run(chains, pairs, on_device)
    for p, (i, j) in enumerate(pairs):
        got = pair_of(out, p)
        ta, tb = by_hand(chains[i], chains[j], got["map"], 10.0, on_device)
        assert same_bits(np.float32(got["tm_a"]), host(ta.tm)[0]) and same_bits(np.float32(got["tm_b"]), host(tb.tm)[0]), p
        assert same_bits(np.float32(got["rmsd"]), host(ta.rmsd)[0]), p
        short = ta if chains[i].shape[0] <= chains[j].shape[0] else tb
        assert same_bits(got["rotation"], host(short.rotation)[0]) and same_bits(got["translation"], host(short.translation)[0]), p
    assert pair_of(out, 4)["tm_a"] == 1.0 and pair_of(out, 4)["rmsd"] == 0.0


def test_hand_worked_cases_on_the_device():
    a, _ = sweep_pair(64, 64, 0)
    out = run([a, a], [[0, 1]], True, codes=dev(np.tile(np.arange(64) % 20, 2).astype(np.uint8)))
    got = pair_of(out, 0)
    assert got["map"].tolist() == list(range(64)) and got["tm_a"] == 1.0 and got["tm_b"] == 1.0 and (got["unit"], got["round"]) == (0, 0)
    assert got["n_ident"] == 64 and np.array_equal(got["rotation"], np.eye(3)) and np.array_equal(got["translation"], np.zeros(3))
    ref, x, _ = domain16()
    got = pair_of(run([x[0], ref], [[0, 1]], True, scale=1.0), 0)
    assert got["map"].tolist() == list(range(16)) and got["tm_a"] == np.float32((8 + 8 / 40001) / 16) and got["tm_a"] == got["tm_b"]
    a, b, planted = planted_deletion()
    got = pair_of(run([a, b], [[0, 1]], True, scale=1.0), 0)
    want = structalign_def(a, b, scale=1.0)
    assert np.array_equal(got["map"], want["map"]) and (got["unit"], got["round"]) == (want["unit"], want["round"])
    far = np.array([r for r in range(a.shape[0]) if min(abs(r - 7), abs(r - 8)) >= 3])
    assert np.array_equal(got["map"][far], planted[far]) and np.array_equal(got["map"], planted)
    assert got["tm_a"] == 1.0 and got["n_aligned"] == 20 >= b.shape[0] - 4 - 6
    a, b = disagreeing_pair()
    got = pair_of(run([a, b], [[0, 1]], True), 0)
    assert (got["unit"], got["round"]) == (2, 0)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_a_nan_chain_and_its_neighbours(on_device):
    a, b = sweep_pair(9, 8, 0)
    bad = a.copy()
    bad[4, 2] = np.nan
    out = run([a, b, bad], [[0, 1], [2, 1], [0, 2], [0, 1]], on_device)
    good = pair_of(out, 0)
    assert all(same_bits(good[k], pair_of(out, 3)[k]) for k in FIELDS)
    for p in (1, 2):
        got = pair_of(out, p)
        assert np.isnan(got["tm_a"]) and np.isnan(got["tm_b"]) and got["unit"] == -1 and got["round"] == -1 and (got["map"] == -1).all()
        assert np.isnan(got["rotation"]).all() and np.isnan(got["translation"]).all() and np.isnan(got["rmsd"]) and np.isnan(got["history"]).all()
        assert got["n_aligned"] == 0 and got["n_ident"] == 0 and got["dp_score"] == 0
    check(good, sweep_def(9, 8, 0, 16), a, b, tag="next to a NaN chain")


def test_the_same_bits_alone_in_a_list_on_either_side_and_again():
    a, b = sweep_pair(65, 63, 0)
    alone = pair_of(run([a, b], [[0, 1]]), 0)
    others = [sweep_pair(m, n, 0) for m, n in ((8, 8), (9, 8), (4, 9), (63, 65))]
    chains = [a, b] + [c for pr in others for c in pr]
    pairs = [[2 + 2 * (k % 4), 3 + 2 * (k % 4)] for k in range(65)]
    pairs[37] = [0, 1]
    for on_device in (False, True, True):
        out = run(chains, pairs, on_device)
        got = pair_of(out, 37)
        assert all(same_bits(got[k], alone[k]) for k in FIELDS), [k for k in FIELDS if not same_bits(got[k], alone[k])]
        assert all(same_bits(pair_of(out, 0)[k], pair_of(out, 64)[k]) for k in FIELDS)


def test_all_pairs_is_the_explicit_list():
    chains = [sweep_pair(8, 8, 0)[0], sweep_pair(9, 8, 0)[0], sweep_pair(4, 9, 0)[1], sweep_pair(30, 36, 1)[0]]
    every = run(chains, None, True)
    listed = run(chains, [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]], True)
    assert all(same_bits(getattr(every, k), getattr(listed, k)) for k in FIELDS) and np.array_equal(every.map_offsets, listed.map_offsets)


def test_an_initial_map_from_the_sequence_alignment():
    from pesto_amd import sequences as sq
    a, b = sweep_pair(65, 63, 0)
    rng = np.random.RandomState(4)
    sb = rng.randint(0, 20, 70).astype(np.uint8)
    sa = np.concatenate([sb[:30], sb[35:]]).copy()              # the copy lost five residues ...
    sa[rng.randint(0, 65, 6)] = 20                              # ... and six of the others are unknown
    sb = sb[:63]
    init = host(sq.align_maps([sa, sb], [[0, 1]], mode="overlap").map)
    assert init.size == 65 and (init >= 0).sum() >= 50
    out = run([a, b], [[0, 1]], True, init=[init], codes=np.concatenate([sa, sb]))
    got = pair_of(out, 0)
    want = structalign_def(a, b, codes_a=sa, codes_b=sb, init=init)
    assert got["history"].shape == (6, 20, 3) and np.isfinite(got["history"][4, 0]).all() and got["history"][4, 0, 2] == (init >= 0).sum()
    check(got, want, a, b, codes=(sa, sb), tag="init")
    plain = pair_of(run([a, b], [[0, 1]], True), 0)
    assert same_bits(plain["history"], got["history"][:4])       # the caller's map adds units, it changes none


def test_structure_align_on_a_renumbered_file(tmp_path):
    from pesto_amd import sequences as sq, structalign as SA
    a, b = pdb_path(tmp_path, "6I9F.pdb"), pdb_path(tmp_path, "6I9F_i0.pdb")
    out, chains, match = SA.structure_align(a, b)
    assert len(chains) == 1 and out.map.tolist() == list(range(155)) and out.n_aligned[0] == 155 and out.n_ident[0] == 155
    assert out.tm_a[0] == 1.0 and out.tm_b[0] == 1.0 and out.rmsd[0] == 0.0
    want = sq.match_atoms(a, b)
    for g, w in zip(match[:4], want[:4]):
        assert np.array_equal(g, w, equal_nan=True)
    assert all(np.array_equal(match[4][k], want[4][k]) for k in want[4])


def test_the_two_halves_of_a_barrel():
    """1thf_D is a (beta alpha)8 barrel grown by duplication; its two halves are aligned by structure (TM recorded in DESIGN.md)"""
    from pesto_amd import structalign as SA
    path = os.path.join(GOLDEN, "pdb", "1thf_D.pdb.gz")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "1thf_D.pdb")
        with gzip.open(path, "rb") as fi, open(p, "wb") as fo:
            fo.write(fi.read())
        (_, xyz, codes, _), = SA.ca_traces(p)
    h = xyz.shape[0] // 2
    a, b = np.ascontiguousarray(xyz[:h]), np.ascontiguousarray(xyz[h:])
    out = run([a, b], [[0, 1]], True, scale=1.0, frag_starts=4, codes=codes)
    got = pair_of(out, 0)
    want = structalign_def(a, b, codes_a=codes[:h], codes_b=codes[h:], scale=1.0, frag_starts=4)
    print(f"1thf_D halves ({h} and {xyz.shape[0] - h} residues): tm {got['tm_a']:.4f} / {got['tm_b']:.4f}, n_aligned {got['n_aligned']}, "
          f"n_ident {got['n_ident']}, rmsd {got['rmsd']:.2f} A, winner {got['unit']}, {got['round']}; margins {want['qmargin']:.3g}, "
          f"{min(want['margin'], want.get('final_margin', np.inf)):.3g}")
    check(got, want, a, b, scale=1.0, codes=(codes[:h], codes[h:]), tag="1thf_D halves")


def test_tm_matrix_feeds_the_clustering():
    from pesto_amd import clustering as C, structalign as SA
    base, _ = sweep_pair(64, 64, 0)
    other, _ = sweep_pair(63, 65, 0)
    rng = np.random.default_rng(2)
    chains = [base, (base + 0.005 * rng.normal(size=base.shape)).astype(np.float32), base[3:60].copy(), other, (other + 0.005 * rng.normal(size=other.shape)).astype(np.float32)]
    T = SA.tm_matrix(chains)
    out = run(chains)
    assert T.shape == (5, 5) and T.dtype == np.float32 and (np.diag(T) == 1).all()
    iu = np.triu_indices(5, 1)
    assert same_bits(T[iu], out.tm_b) and same_bits(T.T[iu], out.tm_a)
    D = (1 - np.minimum(T, T.T)).astype(np.float32)
    labels, centers, sizes = C.gromos_clusters(D, 0.5)
    assert host(labels)[0] == host(labels)[1] == host(labels)[2] and host(labels)[3] == host(labels)[4] != host(labels)[0]
    assert same_bits(host(SA.tm_matrix([dev(c) for c in chains])), T)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_a_refused_call_writes_nothing(on_device):
    from pesto_amd import _lib
    from pesto_amd.patches import _default_model
    a, b = sweep_pair(9, 8, 0)
    model, lib = _default_model(0), _lib.load()
    place = dev if on_device else (lambda v: np.ascontiguousarray(v))
    kinds = ((np.int32, 9), (np.int32, 1), (np.int32, 1), (np.int32, 1), (np.int32, 1), (np.int32, 1), (np.float32, 2), (np.float64, 9), (np.float64, 3),
             (np.float32, 1), (np.float64, 4 * 20 * 3))
    d0 = np.array([[d0_def(8), d0_def(9), d0_def(8)]])

    def call(chains, pairs, **kw):
        xyz = place(np.concatenate(chains))
        side = _lib.Side(xyz, model._gpu)
        offs = _lib.offsets([c.shape[0] for c in chains])
        pr = np.asarray(pairs, np.int32)
        outs = [place(np.full(w, 7, dt)) for dt, w in kinds]
        k = dict(go=0.6, rounds=20, frag=16, scale=10.0)
        k.update(kw)
        rc = lib.pesto_structalign(model.handle, len(chains), offs.ctypes.data, side.ptr(xyz), None, 1, pr.ctypes.data, None, d0.ctypes.data, k["go"],
                                   k["rounds"], k["frag"], k["scale"], *(side.ptr(o) for o in outs), side.kind, side.stream)
        return rc, [host(o) for o in outs]

    rc, good = call([a, b], [[0, 1]])
    assert rc == 0 and (good[6] != 7).all() and good[6][0] > 0 and (good[0] >= 0).sum() == good[1][0] >= 3
    for chains, pairs, kw in (([a, b[:2]], [[0, 1]], {}), ([a, b], [[0, 2]], {}), ([a, b], [[-1, 1]], {}), ([a, b], [[0, 1]], dict(rounds=65)),
                              ([a, b], [[0, 1]], dict(frag=1)), ([a, b], [[0, 1]], dict(go=1.5)), ([a, b], [[0, 1]], dict(scale=0.0))):
        rc, outs = call(chains, pairs, **kw)
        assert rc == -1 and lib.pesto_structalign_last_error(), (pairs, kw)
        assert all((o == 7).all() for o in outs), (pairs, kw)
    assert b"residues" in (call([a, b[:2]], [[0, 1]]), lib.pesto_structalign_last_error())[1]
    rc, again = call([a, b], [[0, 1]])
    assert rc == 0 and all(same_bits(x, y) for x, y in zip(again, good))


def test_the_longest_chain():
    m, n, seed, frag = LONGEST
    a, b = sweep_pair(m, n, seed)
    out = run([a, b], [[0, 1]], True, rounds=1, frag_starts=frag)
    want = sweep_def(m, n, seed, frag, 1)
    assert want["qmargin"] >= 1e-8
    check(pair_of(out, 0), want, a, b, tag="4096 x 64")


def test_new_symbols_are_exported():
    from pesto_amd import _lib
    lib = _lib.load()
    for name in ("pesto_structalign_last_error", "pesto_structalign"):
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert lib.pesto_structalign_last_error.restype is not None
