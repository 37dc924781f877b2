"""GPU tests of pesto_amd.surface (pesto_surface.hip) against the NumPy restatement of tests/test_surface_fixture.py, which the CPU suite
pins to the reference's notebook. Every comparison is exact equality (indices, integer sums, the bits of distances, scores and AUCs).
Shapes are the smallest at which the kernels can go wrong: one element, the vertex tile (256) - 1 / + 0 / + 1 against the atom tile (256)
and the slab (512) - 1 / + 0 / + 1 and two slabs + 1, batches whose structures meet inside a tile, exact ties within a tile, across tiles
and across slabs on lattice coordinates, full-mantissa coordinates near the origin and 9000 angstroms away, non-finite coordinates."""
import numpy as np
import pytest

from conftest import golden
from analysis_sweep import FAR, lattice_points, rough_points
from test_surface_fixture import (ATILE, CHAINS, FIXED, PREDICTORS, SLAB, VTILE, areas_def, auc_def, chain_def, check_against_fixture, gather_def,
                                  keys_def, nearest_def, residues_def, same, scored_def, stored_runs)

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def offs(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def check_nearest(vertices, xyz, vo=None, ao=None, **kw):
    from pesto_amd import surface as S
    index, distance = S.nearest_atoms(vertices, xyz, vo, ao, **kw)
    want = nearest_def(vertices, xyz, offs([vertices.shape[0]]) if vo is None else vo, offs([xyz.shape[0]]) if ao is None else ao)
    assert isinstance(index, np.ndarray) and index.dtype == np.int32 and distance.dtype == np.float32
    assert np.array_equal(index, want[0]) and same(distance, want[1])
    return index, distance


def test_constants_mirror_the_kernels():
    from pesto_amd import surface as S
    assert (S.VERTEX_TILE, S.ATOM_TILE, S.SLAB) == (VTILE, ATILE, SLAB) and SLAB == 2 * ATILE


def test_nearest_one_vertex_one_atom():
    v, x = np.array([[1.5, -2.0, 0.25]], np.float32), np.array([[4.5, 2.0, 0.25]], np.float32)
    index, distance = check_nearest(v, x)
    assert index[0] == 0 and distance[0] == 5.0


@pytest.mark.parametrize("V", [VTILE - 1, VTILE, VTILE + 1])
def test_nearest_at_the_tile_and_slab_edges(V):
    rng = np.random.default_rng([7, V])
    for N in (ATILE - 1, ATILE, ATILE + 1, 2 * ATILE + 1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 1):
        v, x = rough_points(rng, (V, 3), 20.0), rough_points(rng, (N, 3), 20.0)
        x[N - 1] = v[V - 1] + np.float32(0.125)                    # the last atom is the last vertex's nearest: the edge element is used
        index, _ = check_nearest(v, x)
        assert index[V - 1] == N - 1


def test_nearest_batch_keeps_structures_apart():
    """three structures whose vertex and atom ranges end inside a tile; foreign atoms sit ON vertices of the neighbouring structures"""
    rng = np.random.default_rng(11)
    vs, ns = (300, 212, 700), (600, 257, 1100)
    vo, ao = offs(vs), offs(ns)
    v, x = rough_points(rng, (sum(vs), 3), 25.0), rough_points(rng, (sum(ns), 3), 25.0)
    x[ao[1]] = v[vo[1] - 1]           # first atom of structure 1 on the last vertex of structure 0
    x[ao[1] - 1] = v[vo[1]]           # last atom of structure 0 on the first vertex of structure 1
    x[ao[2] + 5] = v[vo[2] - 1]       # an atom of structure 2 on the last vertex of structure 1
    x[ao[2] - 1] = v[vo[2] + 255]     # last atom of structure 1 on a vertex of structure 2
    index, distance = check_nearest(v, x, vo, ao)
    for s in range(3):
        assert np.all((index[vo[s]:vo[s + 1]] >= ao[s]) & (index[vo[s]:vo[s + 1]] < ao[s + 1]))
    assert np.all(distance[[vo[1] - 1, vo[1], vo[2] - 1, vo[2] + 255]] > 0)
    # one structure at a time gives the same rows; so does every slab size
    for s in range(3):
        one = check_nearest(v[vo[s]:vo[s + 1]], x[ao[s]:ao[s + 1]])
        assert np.array_equal(one[0] + ao[s], index[vo[s]:vo[s + 1]]) and same(one[1], distance[vo[s]:vo[s + 1]])
    for slab in (ATILE, 4 * ATILE, 2 ** 20):
        again = check_nearest(v, x, vo, ao, slab=slab)
        assert same(again[0], index) and same(again[1], distance)


def test_nearest_exact_ties_take_the_lowest_index():
    """lattice coordinates (multiples of 1/16): the keys are exact, ties are real. Planted: a vertex equidistant from atoms k and k + 1 (one
    tile), from k and k + tile + 1 inside one slab, and from k and k + tile + 1 across two slabs"""
    rng = np.random.default_rng(13)
    V, N = 600, 2 * SLAB + 76
    v, x = lattice_points(rng, (V, 3), 4.0), lattice_points(rng, (N, 3), 4.0)
    step = np.float32(1 / 16)
    for vi, k, other, axis in ((0, 20, 21, 0), (1, 10, 10 + ATILE + 1, 1), (2, 300, 300 + ATILE + 1, 2), (3, 500, 2 * SLAB + 3, 0)):
        v[vi] = np.float32([40 + 3 * vi, 40, 40])                  # away from the cloud: the planted pair is the nearest
        x[k], x[other] = v[vi], v[vi]
        x[k, axis] += step
        x[other, axis] -= step
    keys = keys_def(v, x)
    tied = keys == keys.min(axis=1, keepdims=True)
    assert tied.sum(axis=1).max() >= 2
    first, last = np.argmax(tied, axis=1), N - 1 - np.argmax(tied[:, ::-1], axis=1)
    multi = tied.sum(axis=1) >= 2
    assert np.any(multi & (first // ATILE == last // ATILE))       # a tie within a tile
    assert np.any(multi & (first // SLAB != last // SLAB))         # a tie across slabs
    assert np.any(multi & (first // ATILE != last // ATILE) & (first // SLAB == last // SLAB))
    assert np.array_equal(first[:4], [20, 10, 300, 500])
    index, _ = check_nearest(v, x)
    assert np.array_equal(index, first)
    for slab in (ATILE, 2 ** 20):
        check_nearest(v, x, slab=slab)


@pytest.mark.parametrize("far", [False, True], ids=["origin", "9000A"])
def test_nearest_full_mantissa_coordinates(far):
    rng = np.random.default_rng([17, int(far)])
    vs, ns = (700, 130), (1300, 90)
    v, x = rough_points(rng, (sum(vs), 3), 30.0), rough_points(rng, (sum(ns), 3), 30.0)
    if far:
        v, x = v + FAR, x + FAR
    check_nearest(v, x, offs(vs), offs(ns))


def test_nearest_non_finite_coordinates_never_match():
    rng = np.random.default_rng(19)
    vs, ns = (260, 40), (300, 20)
    vo, ao = offs(vs), offs(ns)
    v, x = rough_points(rng, (sum(vs), 3), 10.0), rough_points(rng, (sum(ns), 3), 10.0)
    x[5, 1], x[270, 0], v[100, 2] = np.nan, np.inf, np.nan
    x[5, [0, 2]], x[270, [1, 2]] = v[3, [0, 2]], v[4, [1, 2]]       # both would be very near without the bad coordinate
    x[ao[1]:] = np.nan                                              # the second structure has no usable atom
    index, distance = check_nearest(v, x, vo, ao)
    assert index[100] == -1 and np.isnan(distance[100]) and 5 not in index and 270 not in index
    assert np.all(index[vo[1]:] == -1) and np.all(np.isnan(distance[vo[1]:])) and np.all(index[:vo[1]][np.arange(260) != 100] >= 0)
    big = np.float32([[3e38, 0, 0]])                                # a finite coordinate whose key overflows: no match either
    index, distance = check_nearest(np.zeros((1, 3), np.float32), big)
    assert index[0] == -1 and np.isnan(distance[0])


# ------------------------------------------------------------------ areas
def fan_mesh(rng, lattice):
    """structure 0: vertex 0 in 300 faces, a degenerate face, vertices without a face; structure 1: a few faces with local indices"""
    pts = lattice_points if lattice else rough_points
    V0, V1 = 310, 9
    v = pts(rng, (V0 + V1, 3), 8.0)
    f0 = [(0, i, i + 1) for i in range(1, 301)] + [(3, 3, 5), (302, 303, 304)]      # vertices 305 .. 309 have no face
    if lattice:                                                     # three lattice points on a line: an exactly degenerate face
        v[302], v[303], v[304] = np.float32([1, 1, 1]), np.float32([2, 2, 2]), np.float32([4, 4, 4])
    f1 = [(0, 1, 2), (2, 1, 3), (8, 7, 6), (0, 8, 4)]                # vertex 5 of structure 1 has no face
    return v, np.array(f0 + f1, np.int32), offs([V0, V1]), offs([len(f0), len(f1)])


@pytest.mark.parametrize("lattice", [True, False], ids=["lattice", "rough"])
def test_vertex_areas_equal_the_definition(lattice):
    from pesto_amd import surface as S
    v, f, vo, fo = fan_mesh(np.random.default_rng(23), lattice)
    want = areas_def(v, f, vo, fo)
    got = S.vertex_areas_fixed(v, f, vo, fo)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.all(got[305:310] == 0) and got[vo[1] + 5] == 0 and got[0] > 0 and (not lattice or got[303] == 0)
    assert same(S.vertex_areas(v, f, vo, fo), want.astype(np.float64) / FIXED)
    assert same(S.vertex_areas_fixed(v, f, vo, fo), got)             # the same bits from call to call
    assert same(host(S.vertex_areas_fixed(dev(v), dev(f), vo, fo)), got)
    # a structure without faces, and no face at all
    fo2 = offs([0, fo[2] - fo[1]])
    assert np.array_equal(S.vertex_areas_fixed(v, f[fo[1]:], vo, fo2), np.r_[np.zeros(vo[1], np.int64), want[vo[1]:]])
    assert np.array_equal(S.vertex_areas_fixed(v, f[:0], vo, offs([0, 0])), np.zeros(v.shape[0], np.int64))


def test_face_index_out_of_range_is_refused():
    from pesto_amd import _lib
    from pesto_amd import surface as S
    v, f, vo, fo = fan_mesh(np.random.default_rng(29), True)
    for bad, where in ((310, 5), (-1, 7), (9, fo[1] + 1), (2 ** 31 - 1, 0)):      # 310: a vertex of the NEXT structure; 9: past the last one
        g = f.copy()
        g[where, 1] = bad
        with pytest.raises(_lib.PestoError) as e:
            S.vertex_areas_fixed(v, g, vo, fo)
        assert e.value.code == -1 and b"face index" in _lib.load().pesto_surface_last_error()
    assert np.array_equal(S.vertex_areas_fixed(v, f, vo, fo), areas_def(v, f, vo, fo))       # and the next call succeeds
    w = v.copy()
    w[1, 0] = np.nan
    with pytest.raises(_lib.PestoError, match="not finite"):
        S.vertex_areas_fixed(w, f, vo, fo)


# ------------------------------------------------------------------ residue table
def one(x):
    return int(round(x * FIXED))


def edge_table():
    """two structures. Structure 0 (atoms 0 .. 9, one per residue 0 .. 9): residue 0 has iface_area == 5.0 exactly (area 10), residue 1 has
    ratio == 0.04 (6 of 150), residue 2 is one unit of 2^-40 above 5.0, residue 3 one unit above the ratio 0.04, residue 4 has no vertex,
    residues 5 .. 8 carry the max_score cases, residue 9 has vertices whose nearest is -1 only. Structure 1: two residues, three atoms."""
    rows = []                                                       # (nearest atom, area, iface, score)
    rows += [(0, one(1.0), 1, 0.5)] * 5 + [(0, one(5.0), 0, 0.25)]
    rows += [(1, one(6.0), 1, -1.0), (1, one(144.0), 0, -2.0)]
    rows += [(2, one(5.0) + 1, 1, 1.0), (2, one(5.0) - 1, 0, 3.0)]
    rows += [(3, one(6.0) + 1, 1, 1.0), (3, one(144.0) - 1, 0, 0.0)]
    rows += [(5, one(0.5), 0, -3.5), (5, one(0.5), 1, -0.25), (5, 0, 0, -7.0)]          # negative scores only
    rows += [(6, one(0.5), 0, -0.0), (6, one(0.5), 0, 0.0), (6, one(0.5), 0, -0.0)]     # -0.0 against +0.0
    rows += [(7, one(0.5), 0, -0.0)]                                                    # -0.0 alone
    rows += [(8, one(7.0), 1, -1e-42)]                                                  # one vertex, a denormal
    rows += [(-1, one(9.0), 1, 9.0)] * 2
    n0 = len(rows)
    rows += [(10, one(3.0), 1, 2.0), (12, one(4.0), 1, -2.0), (11, one(1.0), 0, 5.0)]
    rng = np.random.default_rng(31)
    order = np.r_[rng.permutation(n0), n0 + rng.permutation(3)]
    rows = [rows[i] for i in order]
    nearest, area, iface = np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int64), np.array([r[2] for r in rows], np.uint8)
    score = np.array([r[3] for r in rows], np.float32)
    atom_res = np.r_[np.arange(10), [0, 0, 1]].astype(np.int32)
    return nearest, atom_res, area, iface, score, offs([n0, 3]), offs([10, 3]), offs([10, 2])


def check_table(got, want):
    for k in ("n_vertices", "area_fixed", "iface_area_fixed", "area", "iface_area", "label", "max_score"):
        if want[k] is None:
            assert got[k] is None
        else:
            assert same(host(got[k]), want[k]), k


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_residue_table_edges(on_device):
    from pesto_amd import surface as S
    nearest, atom_res, area, iface, score, vo, ao, ro = edge_table()
    want = residues_def(nearest, atom_res, area, iface, score, vo, ao, ro)
    assert list(want["label"][:4]) == [0, 0, 1, 1] and want["iface_area"][0] == 5.0 and want["iface_area"][1] / want["area"][1] == 0.04
    assert want["n_vertices"][4] == 0 and want["n_vertices"][9] == 0 and np.isnan(want["max_score"][[4, 9]]).all()
    assert same(want["max_score"][5:9], np.float32([-0.25, 0.0, 0.0, -1e-42]))
    put = (lambda a: dev(a)) if on_device else (lambda a: a)
    got = S.residue_surface(put(nearest), put(atom_res), put(area), put(iface), put(score), vo, ao, ro)
    assert got["label"].is_cuda if on_device else isinstance(got["label"], np.ndarray)
    check_table(got, want)
    none = S.residue_surface(put(nearest), put(atom_res), put(area), put(iface), None, vo, ao, ro)
    check_table(none, residues_def(nearest, atom_res, area, iface, None, vo, ao, ro))
    # the order of the vertices (of the atomics) does not matter
    perm = np.r_[np.arange(vo[1])[::-1], vo[1] + np.arange(3)[::-1]]
    check_table(S.residue_surface(put(nearest[perm]), put(atom_res), put(area[perm]), put(iface[perm]), put(score[perm]), vo, ao, ro), want)


def test_residue_table_refuses_what_the_device_sees():
    from pesto_amd import _lib
    from pesto_amd import surface as S
    nearest, atom_res, area, iface, score, vo, ao, ro = edge_table()
    for bad in (np.nan, np.inf, -np.inf):
        s = score.copy()
        s[3] = bad
        with pytest.raises(_lib.PestoError, match="non-finite"):
            S.residue_surface(nearest, atom_res, area, iface, s, vo, ao, ro)
    n = nearest.copy()
    n[0] = 11                                                      # an atom of the other structure
    with pytest.raises(_lib.PestoError, match="nearest-atom index"):
        S.residue_surface(n, atom_res, area, iface, score, vo, ao, ro)
    n[0] = 13                                                      # no atom at all
    with pytest.raises(_lib.PestoError, match="nearest-atom index"):
        S.residue_surface(n, atom_res, area, iface, score, vo, ao, ro)
    a = atom_res.copy()
    a[12] = 2                                                      # structure 1 has two residues
    with pytest.raises(_lib.PestoError, match="atom_residue"):
        S.residue_surface(nearest, a, area, iface, score, vo, ao, ro)
    check_table(S.residue_surface(nearest, atom_res, area, iface, score, vo, ao, ro), residues_def(nearest, atom_res, area, iface, score, vo, ao, ro))


def test_vertex_scores_gather():
    from pesto_amd import _lib
    from pesto_amd import surface as S
    rng = np.random.default_rng(37)
    p = rng.normal(0, 1, 50).astype(np.float32)
    nearest = rng.integers(-1, 50, 777).astype(np.int32)
    assert (nearest == -1).any()
    for put in (lambda a: a, dev):
        assert same(host(S.vertex_scores(put(nearest), put(p))), gather_def(nearest, p))
    nearest[5] = 50
    with pytest.raises(_lib.PestoError):
        S.vertex_scores(nearest, p)


# ------------------------------------------------------------------ scored residues
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_scored_residues_with_an_empty_structure_in_the_middle(on_device):
    from pesto_amd import surface as S
    rng = np.random.default_rng(41)
    rs = (VTILE + 3, 7, 2 * VTILE, 1)
    ro, R = offs(rs), sum(rs)
    n = rng.integers(0, 3, R).astype(np.int32)
    label, p = (rng.random(R) < 0.3).astype(np.uint8), rng.normal(0, 1, R).astype(np.float32)
    valid = rng.random(R) < 0.7
    valid[ro[1]:ro[2]] = False                                     # nothing of structure 1 counts
    n[ro[3]], valid[ro[3]] = 2, True
    put = dev if on_device else (lambda a: a)
    table = {"n_vertices": put(n), "label": put(label), "r_offsets": ro}
    for va in (valid, None):
        want = scored_def(n, label, p, va, ro)
        got = S.scored_residues(table, put(p), None if va is None else put(va))
        assert isinstance(got[0], np.ndarray) and got[0].dtype == np.int32 and np.array_equal(got[0], want[0])
        assert all(same(host(g), w) for g, w in zip(got[1:], want[1:]))
    off = S.scored_residues(table, put(p), put(valid))[0]
    assert off[1] == off[2] and off[1] > 0 and off[4] == off[3] + 1


def tiny_item(rng, valid):
    """a closed little mesh around a few atoms: an octahedron of 6 vertices, 8 faces, with 4 atoms in 2 residues"""
    v = np.float32([[6, 0, 0], [-6, 0, 0], [0, 6, 0], [0, -6, 0], [0, 0, 6], [0, 0, -6]]) + rough_points(rng, (6, 3), 0.1)
    f = np.int32([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    x = np.float32([[3, 0, 0], [1, 1, 0], [-3, 0, 0], [-1, -1, 0]])
    return {"vertices": v, "faces": f, "iface": np.uint8([1, 0, 1, 0, 1, 0]), "xyz": x, "atom_residue": np.int32([0, 0, 1, 1]),
            "p_atom": np.float32([0.9, 0.9, 0.2, 0.2]), "p_res": np.float32([0.9, 0.2]), "valid": np.array([valid, valid])}


def test_driver_refuses_a_structure_without_scored_residues():
    from pesto_amd import surface as S
    rng = np.random.default_rng(43)
    items = [tiny_item(rng, True), tiny_item(rng, False), tiny_item(rng, True)]
    with pytest.raises(ValueError, match="structure 1"):
        S.benchmark_surfaces(items)
    out = S.benchmark_surfaces([items[0], items[2]])
    assert out["point_auc"].shape == (2,) and np.array_equal(out["offsets"], [0, 2, 4])


# ------------------------------------------------------------------ end to end
def as_item(kw):
    it = {k: kw[k] for k in ("vertices", "faces", "iface", "xyz", "atom_residue") if k in kw}
    it["n_residues"] = kw["n_res"]
    it.update({k: kw[k] for k in ("p_atom", "p_res", "valid", "vertex_score") if kw.get(k) is not None})
    return it


def out_of(res, s=0):
    """structure s of a driver result as chain_def's dict (indices local to the structure)"""
    vo, ro, off = res["v_offsets"], res["table"]["r_offsets"], res["offsets"]
    vs, rs, ks = slice(vo[s], vo[s + 1]), slice(ro[s], ro[s + 1]), slice(off[s], off[s + 1])
    a0 = res["a_offsets"][s]
    near = host(res["nearest"])[vs]
    table = {k: (None if res["table"][k] is None else host(res["table"][k])[rs]) for k in ("n_vertices", "area_fixed", "iface_area_fixed", "label", "max_score")}
    return {"nearest": np.where(near >= 0, near - a0, -1).astype(np.int32), "distance": host(res["distance"])[vs], "area_fixed": host(res["area_fixed"])[vs],
            "table": table, "vertex_score": host(res["vertex_score"])[vs], "residue": (host(res["residue"])[ks] - ro[s]).astype(np.int32),
            "y": host(res["y"])[ks], "p": host(res["p"])[ks], "point_auc": float(res["point_auc"][s]), "residue_auc": float(res["residue_auc"][s])}


@pytest.mark.parametrize("tag", PREDICTORS + ("masif",))
def test_stored_chains_batched_equal_the_fixture(tag):
    from pesto_amd import surface as S
    g = golden("surface")
    runs = [dict(stored_runs(name))[tag] for name in CHAINS]
    res = S.benchmark_surfaces([as_item(kw) for kw in runs], "max" if tag == "masif" else "given")
    for s, name in enumerate(CHAINS):
        check_against_fixture(g, name, tag, out_of(res, s))
    # pooled and medians: the same integers over the concatenated columns
    iface, pv = np.concatenate([kw["iface"] for kw in runs]), host(res["vertex_score"])
    assert res["pooled_point_auc"] == auc_def(iface != 0, pv) and res["pooled_residue_auc"] == auc_def(host(res["y"]), host(res["p"]))
    assert res["median_point_auc"] == np.median(res["point_auc"]) and res["median_residue_auc"] == np.median(res["residue_auc"])


@pytest.mark.parametrize("tag", ["sppider", "masif"])
def test_one_stored_chain_on_rocm_tensors(tag):
    import torch
    from pesto_amd import surface as S
    g, name = golden("surface"), CHAINS[2]
    kw = dict(stored_runs(name))[tag]
    item = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in as_item(kw).items()}
    res = S.benchmark_surfaces([item], "max" if tag == "masif" else "given")
    for k in ("nearest", "distance", "area_fixed", "residue", "y", "p", "vertex_score"):
        assert torch.is_tensor(res[k]) and res[k].is_cuda, k
    assert res["table"]["label"].is_cuda
    check_against_fixture(g, name, tag, out_of(res))
    want = chain_def(**kw)
    assert res["point_auc"][0] == want["point_auc"] and res["residue_auc"][0] == want["residue_auc"]
