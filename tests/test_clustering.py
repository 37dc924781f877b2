"""GPU tests of pesto_amd.clustering (pesto_cluster.hip). The RMSD matrix: every recorded case of tests/golden/clustering.npz within
`tolerance` of pairwise_rmsd64 (test_clustering_fixture.py: an explicit float64 superposition, pinned there to the reference's recorded
results), through host arrays and ROCm tensors; the self form bitwise symmetric with a zero diagonal and bit-equal off the diagonal to the
rectangular call on a copy; identical bits from run to run; exact duplicates below the duplicate bound; a seeded sweep over the tile
edges (frames mod 4 and mod 16, atoms mod 4 and mod the 16-atom stage) and over contiguous, strided and permuted selections. The
clustering: the recorded integers at the three recorded cutoffs, seeded and hand-worked matrices against gromos_def exactly, an
asymmetric matrix refused, cluster_frames against its parts, and Model.forward_frames followed by cluster_frames on one ROCm tensor."""
import numpy as np
import pytest

from conftest import golden, md_frames, weights
from test_clustering_fixture import (HAND_WORKED, RMSD_CASES, case_inputs, duplicate_bound, from_adjacency, gromos_def, pairwise_rmsd64, rg_of,
                                     sweep_tolerance, tolerance)

pytestmark = pytest.mark.gpu

ON = pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
# (Fa, Fb; Fb None: the self form): every residue of the 4-frame MFMA rows and of the 16-frame tile, one and several tiles a side
SWEEP_PAIRS = [(1, 1), (1, 65), (65, 1), (3, 4), (4, 3), (5, 15), (15, 16), (16, 17), (17, 5), (63, 64), (64, 65), (65, 63), (16, 16), (4, 64),
               (64, 4), (3, 63), (1, None), (5, None), (17, None), (64, None), (65, None)]
SWEEP_ATOMS = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 257]
CLUSTER_FRAMES = [1, 2, 63, 64, 65, 129, 200]


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def place(on_device, *arrays):
    return [dev(a) if on_device else a for a in arrays]


def bits(a):
    return host(a).view(np.uint32)


def same_clusters(got, want):
    assert len(got) == 3
    for v, w in zip(got, want):
        v = host(v)
        assert v.dtype == np.int32 and np.array_equal(v, np.asarray(w, np.int32)), (v, w)


_rmsd_cache = {}


def recorded(case, on_device):
    """(inputs, the library's matrix as a host array, the float64 yardstick, the bound) of a recorded case, computed once"""
    from pesto_amd import clustering as C
    if (case, on_device) not in _rmsd_cache:
        g = golden("clustering")
        a, b, sel, scale = case_inputs(g, case)
        want = pairwise_rmsd64(a, b, sel, scale)
        da, db = place(on_device, a, b)
        D = C.pairwise_rmsd(da, db, sel=sel, scale=scale)
        assert (D.is_cuda if on_device else isinstance(D, np.ndarray)) and tuple(D.shape) == want.shape
        assert host(D).dtype == np.float32
        _rmsd_cache[case, on_device] = ((da, db, sel, scale), host(D), want, tolerance(g, case, want, scale, rg_of(a, b, sel)))
    return _rmsd_cache[case, on_device]


@ON
@pytest.mark.parametrize("case", RMSD_CASES)
def test_recorded_cases_within_tolerance(case, on_device):
    _, D, want, tol = recorded(case, on_device)
    err = float(np.abs(D.astype(np.float64) - want).max())
    print(f"{case}: max deviation {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (case, err, tol)
    if case == "mirror":
        assert D[0, 0] > 1.0


@ON
@pytest.mark.parametrize("case", ["md29_all", "md29_sel"])
def test_self_form_is_symmetric_and_equals_the_rectangular_call(case, on_device):
    from pesto_amd import clustering as C
    (a, _, sel, scale), D, _, _ = recorded(case, on_device)
    assert np.array_equal(D.view(np.uint32), D.T.view(np.uint32)) and not np.diag(D).view(np.uint32).any()
    again = C.pairwise_rmsd(a, sel=sel, scale=scale)
    assert np.array_equal(bits(again), D.view(np.uint32))
    copy = a.clone() if on_device else a.copy()
    R = host(C.pairwise_rmsd(a, copy, sel=sel, scale=scale))
    off = ~np.eye(D.shape[0], dtype=bool)
    assert np.array_equal(R.view(np.uint32)[off], D.view(np.uint32)[off])
    assert np.array_equal(bits(C.pairwise_rmsd(a, copy, sel=sel, scale=scale)), R.view(np.uint32))
    # the other side's result is the same matrix
    other = host(C.pairwise_rmsd(*place(not on_device, host(a)), sel=sel, scale=scale))
    assert np.array_equal(other.view(np.uint32), D.view(np.uint32))


@ON
def test_exact_duplicates_lie_below_the_duplicate_bound(on_device):
    g = golden("clustering")
    (a, b, sel, scale), D, want, _ = recorded("md29_rect", on_device)
    ia, ib = g["md29_rect_ia"], g["md29_rect_ib"]
    bound = duplicate_bound(scale, rg_of(host(a), host(b)))
    pairs = [(i, j) for i in range(len(ia)) for j in range(len(ib)) if ia[i] == ib[j]]
    assert len(pairs) == 2
    for i, j in pairs:
        print(f"duplicate ({ia[i]}, {ib[j]}): {D[i, j]:.3e}, bound {bound:.3e}")
        assert 0.0 <= D[i, j] <= bound and want[i, j] <= bound


def sweep_selection(kind, n, N, rng):
    if kind == "contiguous":
        return np.arange(3, 3 + n)
    if kind == "strided":
        return np.arange(1, 2 * n + 1, 2)
    return rng.permutation(N)[:n]


@pytest.mark.parametrize("kind", ["contiguous", "strided", "permuted"])
@pytest.mark.parametrize("Fa,Fb", SWEEP_PAIRS)
def test_tile_edge_sweep(Fa, Fb, kind):
    from pesto_amd import clustering as C
    g = golden("clustering")
    rng = np.random.default_rng(1000 * Fa + 10 * (Fb or 0) + len(kind))
    scale = 10.0
    for k, n in enumerate(SWEEP_ATOMS):
        N = 2 * n + 3
        a = (rng.normal(0.0, 1.5, (Fa, N, 3)) + rng.normal(0.0, 2.0, (Fa, 1, 3))).astype(np.float32)
        b = None if Fb is None else (rng.normal(0.0, 1.5, (Fb, N, 3)) + rng.normal(0.0, 2.0, (Fb, 1, 3))).astype(np.float32)
        sel = sweep_selection(kind, n, N, rng)
        want = pairwise_rmsd64(a, b, sel, scale)
        tol = sweep_tolerance(g, want, scale, rg_of(a, b, sel))
        on_device = (k + Fa) % 2 == 0
        D = host(C.pairwise_rmsd(*place(on_device, a, b), sel=place(on_device and k % 3 == 0, sel)[0], scale=scale))
        err = float(np.abs(D.astype(np.float64) - want).max())
        assert D.shape == want.shape and err <= tol, (Fa, Fb, n, kind, err, tol)
        if Fb is None:
            assert np.array_equal(D.view(np.uint32), D.T.view(np.uint32)) and not np.diag(D).view(np.uint32).any(), (Fa, n, kind)


def test_mask_selection_and_trajectory_objects():
    from pesto_amd import clustering as C

    class Traj:
        def __init__(self, xyz):
            self.xyz = xyz
    g = golden("clustering")
    a, _, sel, scale = case_inputs(g, "md29_sel")
    mask = np.zeros(a.shape[1], bool)
    mask[sel] = True
    _, D, _, _ = recorded("md29_sel", False)
    assert np.array_equal(bits(C.pairwise_rmsd(Traj(a), sel=mask, scale=scale)), D.view(np.uint32))
    # the selection applied by the caller is the same problem
    assert np.array_equal(bits(C.pairwise_rmsd(np.ascontiguousarray(a[:, sel]), scale=scale)), D.view(np.uint32))
    ten = host(C.pairwise_rmsd(a[:4], sel=sel))                                # the default scale: nanometres in, angstroms out
    assert np.abs(ten - 10.0 * D[:4, :4]).max() <= 4 * np.finfo(np.float32).eps * ten.max()


@ON
def test_recorded_clusters(on_device):
    from pesto_amd import clustering as C
    g = golden("clustering")
    D = place(on_device, g["md29_all_f64"].astype(np.float32))[0]
    for k, cut in enumerate(g["cutoffs"]):
        got = C.gromos_clusters(D, float(cut))
        assert all(v.is_cuda if on_device else isinstance(v, np.ndarray) for v in got)
        same_clusters(got, (g[f"cl{k}_labels"], g[f"cl{k}_centers"], g[f"cl{k}_sizes"]))


def seeded_matrices(F):
    """name -> (D, cutoff): symmetric float32 matrices with a zero diagonal"""
    rng = np.random.default_rng(F)
    U = np.triu(rng.uniform(0.5, 2.0, (F, F)).astype(np.float32), 1)
    U = U + U.T
    out = {"one_cluster": (U, 2.5), "singletons": (U, 0.25)}
    for q in (0.02, 0.2, 0.6):
        if F > 2:
            out[f"quantile_{q}"] = (U, float(np.quantile(U[np.triu_indices(F, 1)], q)))
    # cliques of three: every count is 3 (the last clique may be smaller), so every round is a tie
    T = from_adjacency(F, [(i, j) for i in range(F) for j in range(i + 1, F) if i // 3 == j // 3])
    out["count_tie"] = (T, 1.0)
    # paths of three taken from the top: the middles tie at 3, their ends at 2
    P = from_adjacency(F, [(F - 1 - i, F - 2 - i) for i in range(F - 1) if i % 3 != 2])
    out["tie_from_the_top"] = (P, 1.0)
    if F >= 63:                 # the hand-worked matrices at the word boundary, everything else a singleton
        for name, make in HAND_WORKED.items():
            d, cut, _, _, _ = make()
            at = 60 if F >= 70 else F - d.shape[0]
            E = np.full((F, F), 2.0 * cut, np.float32)
            E[at:at + d.shape[0], at:at + d.shape[0]] = d
            np.fill_diagonal(E, 0.0)
            out[name] = (E, cut)
    nan = U.copy()
    if F > 2:
        nan[0, 1] = nan[1, 0] = np.nan
        out["nan_entry"] = (nan, 2.5)
    return out


@pytest.mark.parametrize("F", CLUSTER_FRAMES)
def test_seeded_matrices_equal_the_definition(F):
    from pesto_amd import clustering as C
    for k, (name, (D, cut)) in enumerate(seeded_matrices(F).items()):
        want = gromos_def(D, cut)
        got = C.gromos_clusters(place((k + F) % 2 == 0, D)[0], cut)
        same_clusters(got, want)
        if name == "one_cluster":
            assert host(got[2]).tolist() == [F]
        if name == "singletons":
            assert host(got[1]).tolist() == list(range(F))
        if name == "quantile_0.2" and F >= 63:
            assert 2 < len(want[1]) < F and want[2][0] > 2
    for name, make in HAND_WORKED.items():
        D, cut, labels, centers, sizes = make()
        same_clusters(C.gromos_clusters(D, cut), (labels, centers, sizes))


def test_many_rounds():
    """pairs (2 i, 2 i + 1) with counts of 2 throughout: F / 2 rounds, several batches of rounds between two reads of the done flag"""
    from pesto_amd import clustering as C
    F = 200
    D = from_adjacency(F, [(2 * i, 2 * i + 1) for i in range(F // 2)])
    same_clusters(C.gromos_clusters(dev(D), 1.0), gromos_def(D, 1.0))
    assert len(gromos_def(D, 1.0)[1]) == F // 2


@ON
def test_an_asymmetric_matrix_is_refused(on_device):
    from pesto_amd import clustering as C
    rng = np.random.default_rng(5)
    U = np.triu(rng.uniform(0.5, 2.0, (70, 70)).astype(np.float32), 1)
    U = U + U.T
    for i, j, v in ((0, 1, 0.75), (69, 3, 0.75), (64, 65, np.nan), (10, 40, None)):
        D = U.copy()
        D[i, j] = np.nextafter(D[i, j], np.float32(0)) if v is None else v
        with pytest.raises(ValueError, match="symmetric"):
            C.gromos_clusters(place(on_device, D)[0], 1.0)
    Z = np.zeros((3, 3), np.float32)
    Z[0, 1] = -0.0                                                              # the same value, other bits
    with pytest.raises(ValueError, match="symmetric"):
        C.gromos_clusters(place(on_device, Z)[0], 1.0)
    same_clusters(C.gromos_clusters(place(on_device, U)[0], 1.0), gromos_def(U, 1.0))


@ON
def test_cluster_frames_is_its_two_parts(on_device):
    from pesto_amd import clustering as C
    g = golden("clustering")
    (a, _, _, scale), D, _, _ = recorded("md29_all", on_device)
    for k, cut in enumerate(g["cutoffs"]):
        labels, centers, sizes, Dk = C.cluster_frames(a, float(cut), scale=scale)
        assert all(v.is_cuda if on_device else isinstance(v, np.ndarray) for v in (labels, centers, sizes, Dk))
        assert np.array_equal(bits(Dk), D.view(np.uint32))
        same_clusters((labels, centers, sizes), gromos_def(host(Dk), cut))
        same_clusters((labels, centers, sizes), (g[f"cl{k}_labels"], g[f"cl{k}_centers"], g[f"cl{k}_sizes"]))
    sel = g["sel7"].astype(np.int64)
    labels, centers, sizes, Ds = C.cluster_frames(a, 1.2, sel=sel, scale=scale)
    assert np.array_equal(bits(Ds), recorded("md29_sel", on_device)[1].view(np.uint32))
    same_clusters((labels, centers, sizes), gromos_def(host(Ds), 1.2))


def test_forward_frames_then_cluster_frames_on_the_device():
    from pesto_amd import Model
    from pesto_amd import clustering as C
    from pesto_amd.config import CONFIGS
    import torch
    f = md_frames()
    m = Model(CONFIGS["i_v4_0"]).to("cuda:0")
    m.load_state_dict(weights("i_v4_0"))
    X = dev(f["X_frames"])
    roa = dev(f["res_of_atom"])
    M = torch.zeros((X.shape[1], f["R"]), device=X.device)
    M[torch.arange(X.shape[1], device=X.device), roa.long()] = 1.0
    z = m.forward_frames(X, dev(f["ids"]), dev(f["q0"]), M)
    cut = float(golden("clustering")["cutoffs"][0])
    labels, centers, sizes, D = C.cluster_frames(X, cut, scale=1.0, model=m)
    assert z.is_cuda and labels.is_cuda and centers.is_cuda and sizes.is_cuda and D.is_cuda
    picked = z[centers.long()]                                                  # the centres' logits, never off the device
    assert picked.is_cuda and tuple(picked.shape) == (len(centers), f["R"], z.shape[2])
    assert np.abs(host(picked) - f["z"][host(centers)]).max() < 1e-4
    g = golden("clustering")
    same_clusters((labels, centers, sizes), (g["cl0_labels"], g["cl0_centers"], g["cl0_sizes"]))
