"""CPU checks of the sweep generators (tests/analysis_sweep.py): every listed case builds and its definitions evaluate quickly; lattice
cases have exact float32 squared distances and thresholds / bin edges that are attained and never missed by one float32 unit; the rough
cell-grid cases keep the pairs within 1e-3 of r_thr to 1 % of their contacts; the superposition cases leave the rotation undetermined
exactly where they were built to; the case lists cover every edge set; every case has non-trivial output."""
import time

import numpy as np
import pytest

import analysis_sweep as S
from test_hbonds_fixture import bonded_def
from test_sasa_fixture import definition_counts
from test_trajectory_fixture import dist

ALL = S.all_cases()
IDS = [f"{entry}:{S.case_id(case)}" for entry, case in ALL]
GROUPS = dict(trajectory=("counts", "loglik", "maps", "centroids"), hbonds=("hbonds", "unwrap"), docking=("docking",), sasa=("sasa",),
              cellgrid=("cellgrid",))


def exact_squares(xa, xb):
    """every float32 squared distance of the two clouds equals the float64 one"""
    with np.errstate(invalid="ignore"):
        d32 = xa[:, None, :] - xb[None, :, :]
        s32 = (d32[..., 0] * d32[..., 0] + d32[..., 1] * d32[..., 1]) + d32[..., 2] * d32[..., 2]
        d64 = xa.astype(np.float64)[:, None, :] - xb.astype(np.float64)[None, :, :]
        s64 = (d64 * d64).sum(-1)
    ok = np.isfinite(s64)
    return s32.dtype == np.float32 and np.array_equal(s32[ok].astype(np.float64), s64[ok]) and (s64[ok] < 2.0 ** 14).all()


def on_lattice(*arrays, span=32):
    for a in arrays:
        v = a[np.isfinite(a)].astype(np.float64)
        if not (np.array_equal(v * 16, np.round(v * 16)) and (np.abs(v) < span).all()):
            return False
    return True


def attained_never_grazed(d, thr):
    """some finite float32 d equals thr and none lies one float32 unit beside it"""
    d = d[np.isfinite(d) & (d > 0)]
    gap = S.ulps_apart(d, np.full(d.shape, thr, np.float32))
    return bool((gap == 0).any()) and not bool((gap == 1).any())


@pytest.mark.parametrize("entry,case", ALL, ids=IDS)
def test_case_builds_quickly_and_has_output(entry, case):
    t0 = time.perf_counter()
    c = S.BUILDERS[entry](case)                       # (not the cached build: the time of the definitions is what is measured)
    took = time.perf_counter() - t0
    print(f"{entry} {S.case_id(case)}: attempt {c['attempt']}, {took:.3f} s")
    assert took < 1.0 * (1 + c["attempt"]), (case, took)
    family, seed, shape = case
    kind, flags = S.parse(family)
    if entry == "counts":
        assert c["counts"].sum() > 0 and c["counts"].shape == (shape[0], shape[1] or shape[0], shape[3])
    elif entry == "loglik":
        assert np.isfinite(c["L"]).all() and c["L"].max() > 0 and np.isfinite(c["KL"]).all() and np.abs(c["KL"]).max() > 0
    elif entry == "maps":
        assert c["maps"][0].sum() > 0 and c["native"].max() > 0
    elif entry == "centroids":
        assert np.isfinite(c["want"]).any()
    elif entry == "hbonds":
        P, A, F = shape
        assert c["off"][-1] > 0 and c["occ_n"].size > 0
        if P * A >= 2:                                  # a frame or donor pair without a bond, and a frame with several
            assert (c["per_pair"] == 0).any() and (np.diff(c["off"]) >= 2).any()
        if F >= 2:
            assert np.diff(c["off"])[-1] == 0
        if c["group"] is not None:
            assert 0 < c["goff"][-1] and c["nhb"].sum() == c["goff"][-1]
        assert np.isin(c["dh"][:, 0], c["acc"]).any() or A < 4          # acceptors that are donors too
        if c["freq"] > 0:                               # the occupancy threshold is attained and excluded by the strict comparison
            assert (c["occ_n"] > c["freq"] * F).all() and c["occ_n"].size < occupancy_size(c, 0.0)
    elif entry == "unwrap":
        M = len(shape[0])
        assert c["image"].shape == (shape[1], M) and not c["image"][:, 0].any()
        assert M == 1 or "tie" in flags or c["image"].any()
        ties = c["gap"] <= 1e-6
        assert ties.any() == ("tie" in flags)
    elif entry == "docking":
        Na, Nb, F, _ = shape
        assert c["off"][-1] > 0 and c["roff"][-1] > 0 and c["ira"].size > 0 and c["irb"].size > 0
        if Na * Nb >= 2:
            assert (c["per_atom"] == 0).any() and (np.diff(c["off"]) >= 2).any()
        if F >= 2:
            assert np.diff(c["off"])[-1] == 0
    elif entry == "sasa":
        assert (c["counts"] < c["P"]).any() and (c["counts"] > 0).any()
    elif entry == "cellgrid":
        assert c["pairs"].shape[0] > 0 and c["labelled"].any()
    else:
        assert np.isfinite(c["rmsd64"]).all()
    if "nan" in flags or "inf" in flags:
        arrays = [v for k, v in c.items() if k in ("x0", "x1", "xa", "xb", "x", "xyz", "X") and v is not None]
        arrays += [a for a, _ in c.get("asm", [])]
        bad = sum(int((np.isnan(a) if "nan" in flags else np.isinf(a)).sum()) for a in arrays)
        assert bad >= 1 and bad <= 2 + (entry == "unwrap"), (case, bad)          # (docking's xb sits in xyz too; unwrap: an atom and a box length)


def occupancy_size(c, freq):
    from test_hbonds_fixture import occupancy_def
    return occupancy_def(c["xyz"], c["dh"], c["acc"], freq, c["r_thr"], c["angle"], c["scale"])[1].size


@pytest.mark.parametrize("entry,case", [(e, c) for e, c in ALL if S.parse(c[0])[0] == "lattice" and e not in ("centroids", "superpose")],
                         ids=[i for i, (e, c) in zip(IDS, ALL) if S.parse(c[0])[0] == "lattice" and e not in ("centroids", "superpose")])
def test_lattice_cases_are_exact_and_sit_on_their_thresholds(entry, case):
    c = S.build(entry, case)
    if entry in ("counts", "loglik"):
        x0, x1 = c["x0"], c["x0"] if c["x1"] is None else c["x1"]
        assert on_lattice(x0, x1) and all(exact_squares(a, b) for a, b in zip(x0, x1))
        d = dist(x0, x1)
        d = d[np.isfinite(d)]
        att = np.unique(d).astype(np.float64)
        real = np.array([e for e in c["bins"] if e not in c["synthetic"]])
        hit = np.isin(real, att)
        assert hit.sum() == min(real.size, att.size) and hit[:hit.sum()].all(), case
        for e in real[hit]:
            assert not (S.ulps_apart(d, np.full(d.shape, e, np.float32)) == 1).any(), (case, e)
        if c["synthetic"]:                              # [e, e+) holds exactly d == e; the bin behind it nothing
            k = int(np.nonzero(c["bins"] == c["synthetic"][0])[0][0])
            cnt = c["counts"] if entry == "counts" else None
            assert c["bins"][k + 1] == c["synthetic"][1] and (d.astype(np.float64) == c["bins"][k - 1]).any()
            if cnt is not None:
                assert cnt[..., k - 1].sum() == (d.astype(np.float64) == c["bins"][k - 1]).sum() and cnt[..., k].sum() == 0
    elif entry in ("maps", "docking"):
        assert c["scale"] == 1.0 and on_lattice(c["xa"], c["xb"]) and all(exact_squares(a, b) for a, b in zip(c["xa"], c["xb"]))
        d = dist(c["xa"], c["xb"])
        if entry == "maps" and d.size == 1:             # the single pair is a contact one lattice step inside
            assert d.max() < 5.0
        else:
            assert attained_never_grazed(d, c["r_thr"]), case
    elif entry == "hbonds":
        assert c["scale"] == 1.0 and on_lattice(c["xyz"])
        H, A = c["xyz"][:, c["dh"][:, 1]], c["xyz"][:, c["acc"]]
        assert all(exact_squares(a, b) for a, b in zip(H, A))
        assert attained_never_grazed(dist(H, A), c["r_thr"])
        # a triplet on the threshold that passes the angle test: in for <=, out for <
        wider = float(np.nextafter(np.float32(c["r_thr"]), np.float32(9)))
        n_tie = sum(int(bonded_def(x, c["dh"], c["acc"], wider, c["angle"], 1.0)[0].sum() - bonded_def(x, c["dh"], c["acc"], c["r_thr"], c["angle"], 1.0)[0].sum())
                    for x in c["xyz"][:1])
        assert n_tie >= 1, case
    elif entry == "unwrap":
        # (no float32 distance here: the centres of mass are single divisions of exact sums, so the images are decided exactly)
        assert on_lattice(c["xyz"], c["box"], span=128) and np.array_equal(c["masses"], np.round(c["masses"]))
    elif entry == "sasa":
        assert on_lattice(c["X"]) and np.array_equal(c["R"] * 16, np.round(c["R"] * 16))
        start = 0
        for n in c["sizes"]:
            assert all(exact_squares(x[start:start + n], x[start:start + n]) for x in c["X"])
            start += n
    elif entry == "cellgrid":
        for xyz, n0 in c["asm"]:
            assert on_lattice(xyz) and exact_squares(xyz[:n0], xyz[n0:])
        D = np.concatenate([S.chain_dist(xyz[:n0], xyz[n0:]).reshape(-1) for xyz, n0 in c["asm"]])
        assert attained_never_grazed(D, S.R_THR) and c["ties"].any()
        assert np.array_equal(c["pairs"], c["pairs64"])                          # the float32 chain and the float64 brute force agree throughout


@pytest.mark.parametrize("entry,case", [(e, c) for e, c in ALL if c[0] == "graze"], ids=[i for i, (e, c) in zip(IDS, ALL) if c[0] == "graze"])
def test_graze_cases_hold_a_pair_whose_squared_distance_is_inside_and_whose_distance_is_not(entry, case):
    """exactly one pair of frame 0 has float32 s one unit below r_thr^2 and d = sqrt(s) * 1 == r_thr: the definition (d < r_thr) leaves
    it out, a comparison of s with r_thr^2, or s <= s* with the host's threshold s*, would take it"""
    c = S.build(entry, case)
    if entry == "hbonds":
        a, b = c["xyz"][0][c["dh"][:, 1]], c["xyz"][0][c["acc"]]
    else:
        a, b = c["xa"][0], c["xb"][0]
    d32 = a[:, None, :] - b[None, :, :]
    s = (d32[..., 0] * d32[..., 0] + d32[..., 1] * d32[..., 1]) + d32[..., 2] * d32[..., 2]
    thr = np.float32(c["r_thr"])
    graze = (np.sqrt(s) == thr) & (s < thr * thr)
    assert c["scale"] == 1.0 and graze.sum() == 1 and s[graze][0] == np.nextafter(thr * thr, np.float32(0)), (case, int(graze.sum()))
    i, j = (int(v[0]) for v in np.nonzero(graze))
    if entry == "hbonds":                               # the angle test passes: the distance alone keeps the triplet out
        wider = float(np.nextafter(thr, np.float32(9)))
        assert bonded_def(c["xyz"][0], c["dh"], c["acc"], wider, c["angle"], 1.0)[0][i, j] and not bonded_def(c["xyz"][0], c["dh"], c["acc"], c["r_thr"], c["angle"], 1.0)[0][i, j]
        assert not any((t == [c["dh"][i, 0], c["dh"][i, 1], c["acc"][j]]).all() for t in c["trip"][:c["off"][1]])
    else:
        assert not any((p == [i, j]).all() for p in c["pairs"][:c["off"][1]])


@pytest.mark.parametrize("case", S.CELLGRID, ids=S.case_id)
def test_cellgrid_cases_keep_the_band_small_and_agree_with_the_brute_force(case):
    from test_cellgrid import _brute_force
    c = S.build("cellgrid", case)
    pairs64, d64, _, per = _brute_force(c["asm"])
    assert np.array_equal(pairs64, c["pairs64"]) and min(per) >= 0 and sum(per) > 0
    if S.parse(case[0])[0] != "lattice":
        print(f"{S.case_id(case)}: {c['n_near']} pairs within {S.BAND} of r_thr, {pairs64.shape[0]} contacts")
        assert c["n_near"] <= 0.01 * pairs64.shape[0], case
    # outside the band the float32 chain decides like the brute force, and its d is the float64 one to float32 rounding
    key = lambda p: p[:, 0] * (1 << 32) + p[:, 1]       # noqa: E731
    far64 = pairs64[~c["near64"]]
    assert np.isin(key(far64), key(c["pairs"])).all()
    extra = c["pairs"][~np.isin(key(c["pairs"]), key(pairs64))]
    assert extra.shape[0] <= c["n_near"]
    both = np.isin(key(pairs64), key(c["pairs"]))
    scale = max(np.abs(a[np.isfinite(a)]).max() for a, _ in c["asm"])
    assert np.abs(c["d"][np.isin(key(c["pairs"]), key(pairs64))].astype(np.float64) - d64[both]).max() <= 8 * S.EPS32 * max(scale, S.R_THR)
    # a tie flag needs a partner at exactly r_thr in float32
    assert c["ties"].dtype == np.uint8 and c["ties"].size == sum(a.shape[0] for a, _ in c["asm"])


def test_superposition_cases_are_degenerate_exactly_where_they_were_built_to_be():
    by_family = {}
    for case in S.SUPERPOSE:
        c = S.build("superpose", case)
        kind = S.parse(case[0])[0]
        print(f"{S.case_id(case)}: determined {c['determined'].astype(int).tolist()}, rmsd {np.array2string(c['rmsd64'], precision=3)}")
        assert np.array_equal(c["determined"], c["design"]), (case, c["determined"], c["design"])
        n, F = by_family.get(kind, (0, 0))
        by_family[kind] = (n + int((~c["determined"]).sum()), F + c["determined"].size)
        assert np.abs(np.linalg.det(c["R64"]) - 1).max() < 1e-9
        if kind in ("identity", "rot180"):
            assert c["rmsd64"].max() < 1e-5
        if kind == "mirror":
            assert c["rmsd64"].min() > 1e-3                                      # a reflection no rotation undoes
        assert np.linalg.norm(c["dock_r"][c["design"]], axis=1).max() < 2.5 and np.isfinite(c["dock_t"]).all()
    print("undetermined frames by family:", {k: v for k, v in by_family.items() if v[0]})
    assert {k for k, v in by_family.items() if v[0]} == set(S.DEGENERATE)
    assert all(3 * n <= F for n, F in by_family.values()), by_family


def test_case_lists_cover_every_edge_set():
    table = S.coverage()
    for key in sorted(table, key=str):
        print(f"{key[0]:10s} {key[1]:24s} {sorted(table[key], key=str)}")
    print("cases per list:", {k: len(v) for k, v in S.CASES.items()})
    for key, need in S.REQUIRED.items():
        assert need <= table[key], (key, need - table[key])
    ids = [S.case_id(c) for _, c in ALL]
    assert len(set(ids)) == len(ids) and len({c[1] for _, c in ALL}) == len(ALL)          # every case a name and a seed of its own
    # about a quarter of the cases carry a NaN, and every group one infinite coordinate
    sweep = [(e, c) for e, c in ALL if e != "superpose"]
    share = sum("nan" in c[0] for _, c in sweep) / len(sweep)
    assert 0.2 <= share <= 0.3, share
    for group, entries in GROUPS.items():
        assert sum("inf" in c[0] for e, c in sweep if e in entries) >= 1, group
    # every third case of a list runs from host arrays too: each list has one
    assert all(any(S.every_third(e, c) for c in cases) for e, cases in S.CASES.items())


@pytest.mark.parametrize("case", [c for c in S.SASA if sum(c[2][0]) <= 200], ids=S.case_id)
def test_sasa_counts_are_the_definition(case):
    c = S.build("sasa", case)
    for f in range(c["X"].shape[0]):
        assert np.array_equal(definition_counts(c["X"][f], c["R"], c["S"], c["sizes"]), c["counts"][f])


def test_dense_sasa_case_exceeds_the_candidate_tile():
    """every atom of the 300-atom cluster lies within R_i + R_j of every other: 299 candidate records, more than the 256 of one LDS tile"""
    c = S.build("sasa", S.SASA[-1])
    x, r = c["X"][0].astype(np.float64), c["R"].astype(np.float64)
    d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    assert ((d < r[:, None] + r[None, :]).sum(1) - 1).min() > 256
