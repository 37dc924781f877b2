"""CPU checks of the clustering fixture (tests/golden/make_clustering_golden.py) and of the host side of pesto_amd.clustering, and the
yardsticks the GPU tests import: pairwise_rmsd64 (an explicit float64 superposition by np.linalg.svd followed by the RMS coordinate
difference - deliberately NOT the G - 2 sum(s) formula of the kernel), pinned here to the reference's recorded float32 results within
their recorded deviation e_ref; gromos_def, the integer definition of the GROMOS clustering, pinned by hand-worked matrices; and the
tolerances. Bad arguments raise ValueError before any launch."""
import numpy as np
import pytest

from conftest import golden

EPS32 = float(np.finfo(np.float32).eps)
RMSD_CASES = ["md29_all", "md29_sel", "md29_rect", "mirror", "near", "tiny_n1", "tiny_n2", "tiny_n3", "tiny_n4"]
# what the generator printed for the three recorded cutoffs (sizes, centres)
RECORDED_CLUSTERS = [([14, 8, 2, 1, 1, 1, 1, 1], [13, 2, 27, 0, 7, 12, 17, 24]), ([24, 3, 2], [11, 6, 22]), ([28, 1], [21, 0])]


def case_inputs(g, case):
    """(xyz_a, xyz_b or None for the self form, sel or None, scale) as pairwise_rmsd takes them"""
    X = golden("frames_md_1JTG_uL")["X_frames"]
    sel = g["sel7"].astype(np.int64)
    if case == "md29_all":
        return X, None, None, 1.0
    if case == "md29_sel":
        return X, None, sel, 1.0
    if case == "md29_rect":
        return X[g["md29_rect_ia"]], X[g["md29_rect_ib"]], None, 1.0
    if case == "mirror":
        return X[5:6], X[5:6] * np.array([1, 1, -1], np.float32), sel, 1.0
    if case == "near":
        return X[0:1], g["near_b"], None, 1.0
    return g[case + "_a"], g[case + "_b"], None, 1.0


def pairwise_rmsd64(a, b=None, sel=None, scale=1.0):
    """float64 [Fa, Fb]: every b_j rotated onto every a_i by the optimal proper rotation (SVD in float64 of the centred covariance,
    the reflection folded into the last right vector), then scale * sqrt(mean |b_j R - a_i|^2) from the coordinates themselves"""
    b = a if b is None else b
    if sel is not None:
        a, b = a[:, sel], b[:, sel]
    a, b = a.astype(np.float64), b.astype(np.float64)
    a, b = a - a.mean(1, keepdims=True), b - b.mean(1, keepdims=True)
    D = np.zeros((a.shape[0], b.shape[0]))
    for i in range(a.shape[0]):
        U, _, Vt = np.linalg.svd(np.einsum("na,fnb->fab", a[i], b))
        Vt[:, 2] *= np.sign(np.linalg.det(U) * np.linalg.det(Vt))[:, None]
        gap = np.einsum("fna,fac->fnc", b, np.einsum("fka,fbk->fab", Vt, U)) - a[i][None]
        D[i] = np.sqrt((gap * gap).sum(-1).mean(-1)) * scale
    return D


def gromos_def(D, cutoff):
    """(labels int32 [F], centers int32 [C], sizes int32 [C]) of the definition: adj = D <= float32(cutoff) or i == j; while a frame is
    active, the active frame with the most active neighbours (np.argmax: the first of them) takes them as the next cluster"""
    D = np.asarray(D, np.float32)
    F = D.shape[0]
    with np.errstate(invalid="ignore"):
        adj = (D <= np.float32(cutoff)) | np.eye(F, dtype=bool)
    active, labels, centers, sizes = np.ones(F, bool), np.full(F, -1, np.int32), [], []
    while active.any():
        cnt = np.where(active, (adj & active[None]).sum(1), -1)
        c = int(np.argmax(cnt))
        mem = adj[c] & active
        labels[mem] = len(centers)
        centers.append(c)
        sizes.append(int(mem.sum()))
        active &= ~mem
    return labels, np.array(centers, np.int32), np.array(sizes, np.int32)


def rg_of(a, b=None, sel=None):
    """the largest RMS radius of the selected atoms about their mean over the frames of a case"""
    out = 0.0
    for x in (a,) if b is None else (a, b):
        x = (x if sel is None else x[:, sel]).astype(np.float64)
        out = max(out, float(np.sqrt(np.square(x - x.mean(1, keepdims=True)).sum(-1).mean(-1)).max()))
    return out


def tolerance(g, case, value64, scale, rg):
    """a recorded case: max(4 e_ref, 4 eps32 max(max|value|, scale * rg))"""
    return max(4.0 * float(g[case + "_eref"]), 4.0 * EPS32 * max(float(np.max(np.abs(value64))), scale * rg))


def sweep_tolerance(g, value64, scale, rg):
    """a seeded case without a reference run: max(4 eps32 max(max|value|, scale * rg), E_floor), E_floor the smallest recorded e_ref"""
    return max(4.0 * EPS32 * max(float(np.max(np.abs(value64))), scale * rg), float(g["e_floor"]))


def duplicate_bound(scale, rg):
    """a pair of bitwise equal frames"""
    return 4.0 * EPS32 * scale * rg


def from_adjacency(F, edges, cutoff=1.0):
    """a symmetric float32 matrix with D <= cutoff exactly on the listed pairs"""
    D = np.full((F, F), 2.0 * cutoff, np.float32)
    for i, j in edges:
        D[i, j] = D[j, i] = 0.5 * cutoff
    np.fill_diagonal(D, 0.0)
    return D


def recount_chain():
    """(D, cutoff, labels, centers, sizes): 0 holds 1..4, 5 holds 3, 4 and 6, 7 holds 8 and 9. Once the first cluster (0..4) has left,
    5 keeps only 6, so the second centre is 7; the counts of the first round would make it 5."""
    D = from_adjacency(10, [(0, 1), (0, 2), (0, 3), (0, 4), (5, 3), (5, 4), (5, 6), (7, 8), (7, 9)])
    return D, 1.0, [0, 0, 0, 0, 0, 2, 2, 1, 1, 1], [0, 7, 5], [5, 3, 2]


def count_tie():
    """(D, cutoff, labels, centers, sizes): 2 holds 1 and 3, 4 holds 0 and 5: both count 3, the lower index goes first"""
    D = from_adjacency(6, [(2, 1), (2, 3), (4, 0), (4, 5)])
    return D, 1.0, [1, 0, 0, 0, 1, 1], [2, 4], [3, 3]


HAND_WORKED = {"recount_chain": recount_chain, "count_tie": count_tie}


@pytest.mark.parametrize("case", RMSD_CASES)
def test_rmsd64_is_pinned_to_the_reference(case):
    g = golden("clustering")
    a, b, sel, scale = case_inputs(g, case)
    v = pairwise_rmsd64(a, b, sel, scale)
    assert v.shape == g[case + "_ref"].shape and g[case + "_ref"].dtype == np.float32
    assert np.allclose(g[case + "_f64"], v, rtol=1e-9, atol=1e-9)
    assert np.abs(g[case + "_ref"].astype(np.float64) - v).max() <= float(g[case + "_eref"]) * (1 + 1e-6) + 1e-9


def test_recorded_cases_are_what_they_claim():
    g = golden("clustering")
    assert float(g["e_floor"]) == min(float(g[c + "_eref"]) for c in RMSD_CASES) > 0
    assert g["mirror_f64"][0, 0] > 1.0                                          # a proper rotation cannot undo the mirror
    assert 1e-6 < g["near_f64"][0, 0] < 4e-6 and 1e-4 < g["near_f64"][0, 1] < 3e-4 and 1e-2 < g["near_f64"][0, 2] < 3e-2
    ia, ib = g["md29_rect_ia"], g["md29_rect_ib"]
    assert sorted(set(ia) & set(ib)) == [3, 4]
    a, b, _, _ = case_inputs(g, "tiny_n1")
    assert not a.any() and not b.any() and not g["tiny_n1_f64"].any()
    for case, rank in (("tiny_n2", 1), ("tiny_n3", 1), ("tiny_n4", 2)):
        a, b, _, _ = case_inputs(g, case)
        assert a.shape[1] == int(case[-1])
        for x in list(a) + list(b):
            assert np.linalg.matrix_rank(x.astype(np.float64) - x.astype(np.float64).mean(0), tol=1e-5) == rank


def test_gromos_def_hand_worked():
    for make in HAND_WORKED.values():
        D, cut, labels, centers, sizes = make()
        got = gromos_def(D, cut)
        assert got[0].tolist() == labels and got[1].tolist() == centers and got[2].tolist() == sizes
    # the counts of the first round alone would pick 5 second
    D = recount_chain()[0]
    first = ((D <= 1.0) | np.eye(10, dtype=bool)).sum(1)
    assert first[5] == 4 and first[7] == 3
    # a NaN is no neighbour, whatever the comparison is written as
    D = np.array([[0, np.nan, 9], [np.nan, 0, 9], [9, 9, 0]], np.float32)
    got = gromos_def(D, 1.0)
    assert got[0].tolist() == [0, 1, 2] and got[1].tolist() == [0, 1, 2] and got[2].tolist() == [1, 1, 1]
    # <= is inclusive; the cutoff is rounded to float32 first
    D = np.array([[0, 0.1], [0.1, 0]], np.float32)
    assert gromos_def(D, 0.1)[0].tolist() == [0, 0] and gromos_def(D, float(np.float32(0.1)))[0].tolist() == [0, 0]
    assert gromos_def(D, float(np.nextafter(np.float32(0.1), np.float32(0))))[0].tolist() == [0, 1]
    assert gromos_def(np.zeros((1, 1), np.float32), 0.0)[2].tolist() == [1]


def test_recorded_clusters():
    g = golden("clustering")
    D = g["md29_all_f64"]
    entries = np.sort(D[np.triu_indices(29, 1)])
    X = golden("frames_md_1JTG_uL")["X_frames"]
    tol = tolerance(g, "md29_all", D, 1.0, rg_of(X))
    for k, cut in enumerate(g["cutoffs"]):
        labels, centers, sizes = gromos_def(D, cut)
        assert np.array_equal(labels, g[f"cl{k}_labels"]) and np.array_equal(centers, g[f"cl{k}_centers"]) and np.array_equal(sizes, g[f"cl{k}_sizes"])
        assert sizes.tolist() == RECORDED_CLUSTERS[k][0] and centers.tolist() == RECORDED_CLUSTERS[k][1]
        assert np.all(np.diff(sizes) <= 0) and sizes.sum() == 29 and np.array_equal(labels[centers], np.arange(len(centers)))
        below, above = entries[entries <= cut].max(), entries[entries > cut].min()
        assert above - below > 100.0 * tol                                     # every matrix within tolerance has this adjacency


def test_arguments_raise_before_any_launch():
    from pesto_amd import clustering as C
    m = object()                # no handle: the checks must come first
    x, y = np.zeros((4, 5, 3), np.float32), np.zeros((3, 6, 3), np.float32)
    for bad in (x[0], x[:, :, :2], np.zeros((0, 5, 3), np.float32)):
        with pytest.raises(ValueError):
            C.pairwise_rmsd(bad, model=m)
        with pytest.raises(ValueError):
            C.pairwise_rmsd(x, bad, model=m)
        with pytest.raises(ValueError):
            C.cluster_frames(bad, 1.0, model=m)
    with pytest.raises(ValueError, match="atoms"):
        C.pairwise_rmsd(x, y, model=m)
    for sel in ([0, 5], [-1, 2], [], np.zeros(5, bool), np.ones(4, bool), [0.5, 1.0]):
        with pytest.raises(ValueError, match="sel"):
            C.pairwise_rmsd(x, sel=sel, model=m)
        with pytest.raises(ValueError, match="sel"):
            C.cluster_frames(x, 1.0, sel=sel, model=m)
    with pytest.raises(ValueError, match="scale"):
        C.pairwise_rmsd(x, scale=np.inf, model=m)
    # shapes alone decide these: the views below repeat one element
    many = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (C.MAX_FRAMES + 1, 1, 3), (0, 0, 0))
    assert C.MAX_PAIRS == 2 ** 28 and C.MAX_FRAMES ** 2 == C.MAX_PAIRS
    with pytest.raises(ValueError, match="2\\*\\*28"):
        C.pairwise_rmsd(many, model=m)
    with pytest.raises(ValueError, match="2\\*\\*28"):
        C.pairwise_rmsd(many[:2 ** 14], many, model=m)
    with pytest.raises(ValueError):
        C.cluster_frames(many, 1.0, model=m)
    D = np.zeros((4, 4), np.float32)
    for bad in (D[:3], D[0], D[None], np.zeros((0, 0), np.float32)):
        with pytest.raises(ValueError, match="square"):
            C.gromos_clusters(bad, 1.0, model=m)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (C.MAX_FRAMES + 1, C.MAX_FRAMES + 1), (0, 0))
    with pytest.raises(ValueError, match="frames"):
        C.gromos_clusters(big, 1.0, model=m)
    for cut in (np.nan, np.inf, -np.inf, 1e39):
        with pytest.raises(ValueError, match="cutoff"):
            C.gromos_clusters(D, cut, model=m)
        with pytest.raises(ValueError, match="cutoff"):
            C.cluster_frames(x, cut, model=m)
