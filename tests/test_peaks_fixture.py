"""CPU checks of the host side of pesto_amd.peaks, and the yardsticks the GPU tests import: the definitions of the density-peak clustering in
NumPy. pdist32 (the float32 distance whose bits the kernels reproduce), quantile_rank and dc_of (np.partition), centers_def (math.fsum),
peaks_def (rho, delta, the nearest denser point, centres, labels, sizes and halo; ``rho=`` evaluates everything after the density from a
given rho), pinned here by two hand-worked cases; the seeded sweep inputs; and the bounds.

Bounds, with eps32 = 2^-23 and u = 2^-52:
    centers  eps32 |want| + R u A, A = sum w |x| / sum w of that coordinate: the one rounding to float32, and R additions of terms whose
             absolute values sum to sum w |x|, each product exact in double, divided by S (the division's rounding is inside R u A)
    rg       eps32 want + (R + 8) u want + sqrt(3) R u max_coordinate(A): sum w |x - c'|^2 = sum w |x - c|^2 + S |c' - c|^2 for any c', so
             a centre off by |dc| <= sqrt(3) R u max(A) adds at most |dc| to the root; the sum itself has non-negative terms, hence a
             relative error of at most (R + 8) u (R additions, the few roundings of one term, the division and the root), half of it
             after the root; and the one rounding to float32
    gaussian rho   tol_i = 2 (2 a_max + n + 8) u rho64_i, a_max the largest (d / d_c)^2 below 745 (beyond it exp gives 0): the argument's two
             roundings amplified by exp, exp's own ulp and n additions, on both sides. A case is decisive iff every gap between
             consecutive sorted rho64 is at least 4 tol: then any rho within tol has the order of rho64, and everything after the
             density is the same.
"""
import math

import numpy as np
import pytest

EPS32 = float(np.finfo(np.float32).eps)
U = 2.0 ** -52
SWEEP_N = [2, 3, 63, 64, 65, 129, 255, 256, 257, 513, 1000]    # the 64-row block and the 256-column tile from both sides, several tiles
SWEEP_D = [1, 2, 3, 8]
SWEEP_PDC = 2.0


# ---- definitions
def pdist32(X):
    """float32 [n, n]: s = dx0*dx0; s = s + dx1*dx1; ...; sqrt(s), every operation rounded to float32"""
    X = np.asarray(X, np.float32)
    dx = X[:, None, 0] - X[None, :, 0]
    s = dx * dx
    for c in range(1, X.shape[1]):
        dx = X[:, None, c] - X[None, :, c]
        s = s + dx * dx
    assert s.dtype == np.float32
    return np.sqrt(s)


def quantile_rank(n, pdc):
    M = n * (n - 1) // 2
    return min(M - 1, max(0, math.ceil(M * pdc / 100.0) - 1))


def dc_of(D, k):
    """the k-th smallest (0-based) entry of D above the diagonal"""
    v = np.asarray(D, np.float32)[np.triu_indices(D.shape[0], 1)]
    return np.partition(v, k)[k]


def centers_def(Xp, W):
    """(centers float64 [F, 3], wsum float64 [F], rg float64 [F]) of the weights W >= 0 by math.fsum; NaN, 0, NaN where the weights sum to 0"""
    Xp, W = np.asarray(Xp, np.float64), np.asarray(W, np.float64)
    F = Xp.shape[0]
    c, S, rg = np.full((F, 3), np.nan), np.zeros(F), np.full(F, np.nan)
    for f in range(F):
        on = np.nonzero(W[f] > 0)[0]
        S[f] = math.fsum(W[f, on])
        if S[f] > 0:
            c[f] = [math.fsum(W[f, on] * Xp[f, on, a]) / S[f] for a in range(3)]
            rg[f] = math.sqrt(math.fsum(W[f, on] * np.square(Xp[f, on] - c[f]).sum(1)) / S[f])
    return c, S, rg


def centers_tolerance(Xp, W, want_c, want_rg):
    """(the bound of centers [F, 3], the bound of rg [F]) as the module's docstring derives them; rows whose weights sum to 0 get 0"""
    Xp, W = np.asarray(Xp, np.float64), np.asarray(W, np.float64)
    R = Xp.shape[1]
    W = np.where(W > 0, W, 0.0)
    S = W.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        A = np.where(S[:, None] > 0, (W[:, :, None] * np.abs(np.nan_to_num(Xp))).sum(1) / S[:, None], 0.0)
    tol_c = EPS32 * np.abs(np.nan_to_num(want_c)) + R * U * A
    tol_rg = EPS32 * np.nan_to_num(want_rg) + (R + 8) * U * np.nan_to_num(want_rg) + math.sqrt(3.0) * R * U * A.max(1)
    return tol_c, tol_rg


def gaussian_rho64(D, dc):
    """(rho64 [n], a_max): sum_{j != i} exp(-(d_ij / d_c)^2) in float64 from the float32 d_ij and d_c, by math.fsum"""
    D = np.asarray(D, np.float32)
    a = D.astype(np.float64) / np.float64(np.float32(dc))
    a2 = a * a
    e = np.exp(-a2)
    np.fill_diagonal(e, 0.0)
    off = a2[~np.eye(D.shape[0], dtype=bool)]
    below = off[off < 745.0]
    return np.array([math.fsum(r) for r in e]), float(below.max()) if below.size else 0.0


def gaussian_tolerance(rho64, a_max):
    return 2.0 * (2.0 * a_max + rho64.size + 8.0) * U * rho64


def decisive(rho64, a_max):
    """every gap between consecutive sorted rho64 is at least 4 tol (of the larger of the two)"""
    order = np.argsort(rho64)
    r, t = rho64[order], gaussian_tolerance(rho64, a_max)[order]
    return bool(np.all(np.diff(r) >= 4.0 * t[1:]))


def peaks_def(D, dc, kernel, n_clusters=None, rho_min=0.0, delta_min=None, rho=None):
    """dict(rho float64, delta float32, nh, labels, halo, centers, sizes) of the definition over the float32 matrix D (the diagonal is
    ignored). "Denser" is key(j) > key(i): rho_j > rho_i, or rho_j == rho_i and j < i."""
    D = np.asarray(D, np.float32)
    n = D.shape[0]
    dc = np.float32(dc)
    off = ~np.eye(n, dtype=bool)
    if rho is None:
        rho = ((D < dc) & off).sum(1).astype(np.float64) if kernel == "cutoff" else gaussian_rho64(D, dc)[0]
    rho = np.asarray(rho, np.float64)
    order = np.lexsort((np.arange(n), -rho))                # from the densest to the least dense by key
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    masked = np.where(pos[None, :] < pos[:, None], D, np.float32(np.inf))
    nh = masked.argmin(1).astype(np.int32)                  # the first of the minima: the lowest j among equal distances
    delta = masked.min(1)
    top = int(order[0])
    nh[top] = -1
    delta[top] = D[top][off[top]].max() if n > 1 else 0.0
    if n_clusters is not None:
        gamma = rho * delta.astype(np.float64)
        others = sorted((i for i in range(n) if i != top), key=lambda i: (-gamma[i], i))
        chosen = [top] + others[:n_clusters - 1]
    else:
        chosen = [i for i in range(n) if i == top or (rho[i] >= rho_min and delta[i] >= np.float32(delta_min))]
    centers = np.array(sorted(chosen, key=lambda i: pos[i]), np.int32)
    labels = np.full(n, -1, np.int32)
    labels[centers] = np.arange(centers.size)
    for i in order:
        if labels[i] < 0:
            labels[i] = labels[nh[i]]
    sizes = np.bincount(labels, minlength=centers.size).astype(np.int32)
    border = (labels[:, None] != labels[None, :]) & (D < dc)
    mean = np.where(border, (rho[:, None] + rho[None, :]) / 2.0, 0.0)
    rho_b = np.zeros(centers.size)
    np.maximum.at(rho_b, labels, mean.max(1))
    return dict(rho=rho, delta=delta.astype(np.float32), nh=nh, labels=labels, halo=rho < rho_b[labels], centers=centers, sizes=sizes)


# ---- hand-worked cases: (points, dc, rho, delta or None, nh, [(rule, centers, labels or None, sizes, halo indices)])
CASE_A = dict(X=np.array([[0.0], [1.0], [2.5], [10.0], [11.0], [12.5], [30.0]], np.float32), dc=1.6,
              rho=[1, 2, 1, 1, 2, 1, 0], delta=[1, 29, 1.5, 1, 10, 1.5, 17.5], nh=[1, -1, 1, 4, 1, 4, 5],
              rules=[(dict(n_clusters=2), [1, 4], [0, 0, 0, 1, 1, 1, 1], [3, 4], []),
                     (dict(rho_min=1.0, delta_min=5.0), [1, 4], [0, 0, 0, 1, 1, 1, 1], [3, 4], []),
                     (dict(rho_min=0.0, delta_min=5.0), [1, 4, 6], [0, 0, 0, 1, 1, 1, 2], [3, 3, 1], [])])
CASE_B = dict(X=np.array([(0, 0), (0.5, 0), (0, 0.5), (0.5, 0.5), (0.25, 0.25), (1.4, 0.25), (2.3, 0.25), (3.2, 0), (3.7, 0), (3.2, 0.5), (3.7, 0.5),
                          (3.45, 0.25), (3.45, 0.6)], np.float32), dc=1.0,
              rho=[4, 5, 4, 5, 4, 3, 3, 6, 5, 6, 5, 5, 5], delta=None, nh=[1, 7, 0, 1, 0, 1, 5, -1, 7, 7, 8, 7, 9],
              rules=[(dict(n_clusters=2), [7, 1], None, [6, 7], [0, 2, 4, 5, 6])])
HAND_WORKED = {"A": CASE_A, "B": CASE_B}


# ---- the seeded sweep
def sweep_points(n, d):
    """float32 [n, d]: blobs of unit variance around min(3, n) centres drawn at scale 6. (The seed base is one under which every case
    with d >= 2 and n >= 3 is decisive: at n = 3 d_c is the smallest distance, and a far third point leaves the near pair exactly tied.)"""
    rng = np.random.default_rng(7060 + 10 * n + d)
    k = min(3, n)
    centres = rng.normal(0.0, 6.0, (k, d))
    return (centres[rng.integers(0, k, n)] + rng.normal(0.0, 1.0, (n, d))).astype(np.float32)


SWEEP = [(n, d) for n in SWEEP_N for d in SWEEP_D]
_sweep_cache = {}


def sweep_case(n, d):
    """dict(X, D = pdist32(X), dc at SWEEP_PDC, rho64, a_max, tol, decisive), computed once"""
    if (n, d) not in _sweep_cache:
        X = sweep_points(n, d)
        D = pdist32(X)
        dc = dc_of(D, quantile_rank(n, SWEEP_PDC))
        case = dict(X=X, D=D, dc=float(dc))
        if dc > 0:
            rho64, a_max = gaussian_rho64(D, dc)
            case.update(rho64=rho64, a_max=a_max, tol=gaussian_tolerance(rho64, a_max), decisive=decisive(rho64, a_max))
        _sweep_cache[n, d] = case
    return _sweep_cache[n, d]


def grid_points(side=9):
    """a regular side x side grid: exact ties in distance and, under the cut-off kernel, in rho"""
    g = np.arange(side, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)


# ---- tests
def test_quantile_rank_and_dc_of():
    from pesto_amd import peaks as K
    for (n, pdc), k in (((29, 2), 8), ((2, 2), 0), ((1000, 100), 499499), ((5, 0.001), 0), ((5, 50), 4), ((5, 100), 9), ((4, 17), 1)):
        assert quantile_rank(n, pdc) == k == K.quantile_rank(n, pdc)
    D = sweep_case(65, 3)["D"]
    full = np.sort(D[np.triu_indices(65, 1)])
    for k in (0, 1, 41, 1000, full.size - 1):
        assert dc_of(D, k) == full[k]


def test_pdist32_is_float32_throughout():
    X = sweep_points(65, 3)
    D = pdist32(X)
    assert D.dtype == np.float32 and np.array_equal(D.view(np.uint32), D.T.view(np.uint32)) and not np.diag(D).any()
    i, j = 3, 40
    dx = X[i] - X[j]
    want = np.sqrt((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2])
    assert want.dtype == np.float32 and D[i, j] == want
    # the zero padding of a staged point leaves the sum unchanged
    assert np.array_equal(pdist32(np.concatenate([X, np.zeros((65, 5), np.float32)], 1)).view(np.uint32), D.view(np.uint32))
    assert not np.allclose(D, np.sqrt(((X[:, None].astype(np.float64) - X[None]) ** 2).sum(-1)), rtol=0, atol=0)


@pytest.mark.parametrize("name", sorted(HAND_WORKED))
def test_hand_worked_cases(name):
    case = HAND_WORKED[name]
    D = pdist32(case["X"])
    for rule, centers, labels, sizes, halo in case["rules"]:
        got = peaks_def(D, case["dc"], "cutoff", **rule)
        assert got["rho"].tolist() == case["rho"] and got["nh"].tolist() == case["nh"]
        if case["delta"] is not None:
            assert got["delta"].tolist() == case["delta"]
        assert got["centers"].tolist() == centers and got["sizes"].tolist() == sizes
        if labels is not None:
            assert got["labels"].tolist() == labels
        assert np.nonzero(got["halo"])[0].tolist() == halo
        assert np.array_equal(got["labels"][got["centers"]], np.arange(len(centers)))
        # everything after the density from a given rho
        again = peaks_def(D, case["dc"], "cutoff", rho=np.array(case["rho"], np.float64), **rule)
        assert all(np.array_equal(again[k], got[k]) for k in got)


def test_ties_are_resolved_by_index():
    D = pdist32(grid_points())
    got = peaks_def(D, 1.5, "cutoff", n_clusters=1)
    assert set(got["rho"].tolist()) == {3.0, 5.0, 8.0}                   # corners, edges, interior
    assert got["centers"].tolist() == [10] and got["nh"][10] == -1        # the first interior point is the densest
    assert got["nh"][11] == 10 and got["nh"][19] == 10
    assert got["nh"][20] == 11                                            # 11 and 19 are both denser (lower index) at distance 1
    assert got["nh"][40] == 31 and got["delta"][40] == np.float32(1.0)    # 31 and 39 likewise


def test_planted_clusters_are_recovered():
    rng = np.random.default_rng(11)
    centres = np.array([[0.0, 0.0, 0.0], [12.0, 0.0, 0.0], [0.0, 12.0, 0.0]])
    member = np.repeat(np.arange(3), 40)
    X = (centres[member] + rng.normal(0.0, 1.0, (120, 3))).astype(np.float32)
    D = pdist32(X)
    dc = dc_of(D, quantile_rank(120, 2.0))
    for kernel in ("cutoff", "gaussian"):
        got = peaks_def(D, dc, kernel, n_clusters=3)
        assert got["sizes"].tolist() == [40, 40, 40]
        for c in range(3):
            assert len(set(member[got["labels"] == c])) == 1
    by_radius = peaks_def(D, dc, "gaussian", delta_min=np.float32(6.0 * dc))
    assert np.array_equal(by_radius["labels"], peaks_def(D, dc, "gaussian", n_clusters=3)["labels"])


@pytest.mark.parametrize("n,d", SWEEP)
def test_sweep_cases_are_decisive(n, d):
    case = sweep_case(n, d)
    assert case["dc"] > 0
    order = np.sort(case["rho64"])
    gap = np.diff(order) / np.maximum(gaussian_tolerance(case["rho64"], case["a_max"])[np.argsort(case["rho64"])][1:], 1e-300) if n > 1 else np.array([np.inf])
    print(f"n = {n}, d = {d}: dc {case['dc']:.4g}, a_max {case['a_max']:.4g}, smallest gap {gap.min():.3g} tol, decisive {case['decisive']}")
    if d >= 2 and n >= 3:
        assert case["decisive"]


def test_centers_def_and_bounds():
    Xp = np.array([[[1, 2, 3], [3, 2, 1], [5, 5, 5], [np.nan, 0, 0]], [[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4]]], np.float32)
    P = np.array([[0.9, 0.6, 0.1, 0.2], [0.1, np.nan, 0.5, 0.2]], np.float32)
    with np.errstate(invalid="ignore"):
        W = (P > np.float32(0.5)).astype(np.float32)
    c, S, rg = centers_def(Xp, W)
    assert S.tolist() == [2.0, 0.0] and c[0].tolist() == [2.0, 2.0, 2.0] and rg[0] == math.sqrt(2.0)
    assert np.isnan(c[1]).all() and np.isnan(rg[1])
    tol_c, tol_rg = centers_tolerance(Xp, W, c, rg)
    assert tol_c.shape == (2, 3) and 0 < tol_c[0].max() < 1e-6 and 0 < tol_rg[0] < 1e-6 and not tol_c[1].any() and tol_rg[1] == 0
    c, S, rg = centers_def(Xp[1:], np.array([[1.0, 0.0, 3.0, 0.0]]))
    assert S[0] == 4.0 and c[0].tolist() == [2.5, 2.5, 2.5] and abs(rg[0] - math.sqrt(3 * 0.75)) < 1e-15


def test_the_package_exports_the_module():
    import pesto_amd
    from pesto_amd import peaks as K
    for name in ("peaks", "interface_centers", "weighted_centers", "distance_quantile", "density_peaks", "cluster_interface_frames"):
        assert name in pesto_amd.__all__ and getattr(pesto_amd, name) is (K if name == "peaks" else getattr(K, name))


def test_arguments_raise_before_any_launch():
    from pesto_amd import peaks as K
    m = object()                # no handle: the checks must come first
    X = sweep_points(10, 3)
    D = pdist32(X)
    for bad in (dict(), dict(X=X, D=D), dict(X=X[0]), dict(X=np.zeros((4, 9), np.float32)), dict(X=np.zeros((4, 0), np.float32)), dict(D=D[:5]),
                dict(D=D[0]), dict(X=np.zeros((0, 3), np.float32))):
        with pytest.raises(ValueError):
            K.distance_quantile(model=m, **bad)
        with pytest.raises(ValueError):
            K.density_peaks(dc=1.0, n_clusters=1, model=m, **bad)
    for pdc in (0.0, -1.0, 100.5, np.nan):
        with pytest.raises(ValueError, match="pdc"):
            K.distance_quantile(X, pdc=pdc, model=m)
        with pytest.raises(ValueError, match="pdc"):
            K.density_peaks(X, pdc=pdc, n_clusters=2, model=m)
    for idx in ([0, 10], [-1, 2], [], np.zeros(9, bool), [0.5, 1.0]):
        with pytest.raises(ValueError, match="idx"):
            K.distance_quantile(X, idx=idx, model=m)
        with pytest.raises(ValueError, match="idx"):
            K.density_peaks(D=D, dc=1.0, n_clusters=1, idx=idx, model=m)
    with pytest.raises(ValueError, match="2 selected"):
        K.distance_quantile(X, idx=[3], model=m)
    with pytest.raises(ValueError, match="give dc"):
        K.density_peaks(X, idx=[3], n_clusters=1, model=m)
    for dc in (0.0, -1.0, np.inf, np.nan, 1e-60, 1e39):
        with pytest.raises(ValueError, match="dc"):
            K.density_peaks(X, dc=dc, n_clusters=2, model=m)
    for rule in (dict(), dict(n_clusters=2, delta_min=1.0), dict(delta_min=1.0, delta_factor=2.0), dict(n_clusters=2, delta_factor=2.0)):
        with pytest.raises(ValueError, match="exactly one"):
            K.density_peaks(X, dc=1.0, model=m, **rule)
    for K_ in (0, 11, -1, 2.5):
        with pytest.raises(ValueError, match="n_clusters"):
            K.density_peaks(X, dc=1.0, n_clusters=K_, model=m)
    with pytest.raises(ValueError, match="n_clusters"):
        K.density_peaks(X, dc=1.0, n_clusters=4, idx=[0, 1, 2], model=m)
    with pytest.raises(ValueError, match="kernel"):
        K.density_peaks(X, dc=1.0, n_clusters=2, kernel="epanechnikov", model=m)
    for bad in (dict(delta_min=np.nan), dict(delta_factor=-1.0), dict(delta_factor=np.inf), dict(delta_min=1.0, rho_min=np.nan)):
        with pytest.raises(ValueError):
            K.density_peaks(X, dc=1.0, model=m, **bad)
    many = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (K.MAX_POINTS + 1, 3), (0, 0))
    with pytest.raises(ValueError, match="points"):
        K.distance_quantile(many, model=m)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (K.MAX_FRAMES + 1, K.MAX_FRAMES + 1), (0, 0))
    with pytest.raises(ValueError, match="rows"):
        K.density_peaks(D=big, dc=1.0, n_clusters=1, model=m)
    assert K.MAX_POINTS == 1 << 17 and K.MAX_CLUSTERS == 1024 and K.MAX_DIM == 8
    # the interface centres
    Xp, P = np.zeros((4, 5, 3), np.float32), np.zeros((4, 5), np.float32)
    for bx, bp in ((Xp[0], P), (Xp, P[0]), (Xp, P[:3]), (Xp[:, :, :2], P), (np.zeros((0, 5, 3), np.float32), np.zeros((0, 5), np.float32))):
        with pytest.raises(ValueError):
            K.interface_centers(bx, bp, model=m)
        with pytest.raises(ValueError):
            K.weighted_centers(bx, bp, model=m)
        with pytest.raises(ValueError):
            K.cluster_interface_frames(bx, bp, n_clusters=1, model=m)
    with pytest.raises(ValueError, match="p_thr"):
        K.interface_centers(Xp, P, p_thr=np.nan, model=m)
    with pytest.raises(ValueError, match="unknown"):
        K.cluster_interface_frames(Xp, P, cutoff=1.0, model=m)
