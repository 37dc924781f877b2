"""GPU tests of pesto_amd.dynamics (pesto_dynamics.hip) against the float64 yardstick of test_dynamics_fixture.py. Bounds are formulas:
mean, rmsf, DCCM and projections (float32, rounded once) within 1 ulp32 (DCCM: of 1.0), projections against the float64 product with the
RETURNED components within scale gamma_3n (|D| |v|) + 1 ulp32; the covariance entrywise within Yardstick.cov_bound; a PCA result through
check_pca (orthonormality, the sign rule, rank, residuals, converged, Weyl, the total variance). A seeded sweep runs every F against every
n at the edges of the 64-wide tile, the 16-deep stage and the K step of 4; then selections, ddof, both sides, the named cases of
tests/golden/dynamics.npz (planted and flat spectra, the cancellation case, the md29 frames, rank-deficient inputs) and bitwise
repeatability."""
import numpy as np
import pytest

from conftest import golden
from test_dynamics_fixture import EPS32, PCA_CASES, Yardstick, check_pca, planted, ratio_to, ulp32_ratio, yard

pytestmark = pytest.mark.gpu

SWEEP_F = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 129]
SWEEP_N = [1, 2, 21, 22, 64, 65]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def sweep_frames(F, n):
    """decaying spectrum over every direction there is (0.8^i), no noise: the first min(F - 1, 3n, 32) eigenvalues are distinct"""
    return planted(F, n, min(max(F - 1, 1), 3 * n, 40), 0.0, 0.3, 1000 * F + n)


_sweep = {}


def swept(F, n, ddof):
    if (F, n, ddof) not in _sweep:
        xyz = sweep_frames(F, n)
        _sweep[F, n, ddof] = (xyz, Yardstick(xyz, None, 10.0, ddof))
    return _sweep[F, n, ddof]


def check_basics(dy, xyz, y, sel, label, ddofs):
    """fluctuations, covariance and cross_correlation of one input against its yardstick; returns the largest ratio of error to bound"""
    mean, rm = dy.fluctuations(xyz, sel=sel, scale=y.scale)
    mean, rm = host(mean), host(rm)
    n = y.m // 3
    assert mean.dtype == np.float32 and mean.shape == (n, 3) and rm.dtype == np.float32 and rm.shape == (n,)
    r_mean, r_rmsf = ulp32_ratio(mean.reshape(-1), y.mean), ulp32_ratio(rm, y.rmsf)
    assert r_mean <= 1.0 and r_rmsf <= 1.0, (label, r_mean, r_rmsf)
    assert np.array_equal(host(dy.rmsf(xyz, sel=sel, scale=y.scale)).view(np.uint32), rm.view(np.uint32))
    worst = 0.0
    for ddof in ddofs:
        yd = y if ddof == y.ddof else Yardstick(host(xyz), sel, y.scale, ddof)
        C = host(dy.covariance(xyz, sel=sel, scale=y.scale, ddof=ddof))
        assert C.dtype == np.float64 and C.shape == (y.m, y.m)
        assert np.array_equal(C.view(np.uint64), C.T.view(np.uint64)), label
        ratio = ratio_to(np.abs(C - yd.C), yd.cov_bound(yd.e_ref_sum()))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (label, ddof, ratio)
    M = host(dy.cross_correlation(xyz, sel=sel))
    assert M.dtype == np.float32 and M.shape == (n, n)
    assert np.array_equal(M.view(np.uint32), M.T.view(np.uint32)) and np.all(np.diag(M) == 1.0) and np.all(np.isfinite(M))
    assert np.abs(M.astype(np.float64) - y.dccm()).max() <= EPS32, label
    return worst


@pytest.mark.parametrize("n", SWEEP_N)
def test_sweep_fluctuations_covariance_dccm(n):
    from pesto_amd import dynamics as dy
    worst = 0.0
    for F in SWEEP_F:
        xyz, y = swept(F, n, 0 if F == 1 else 1)
        worst = max(worst, check_basics(dy, xyz, y, None, (F, n), [0] if F == 1 else [0, 1]))
    print(f"n = {n}: largest covariance error / bound {worst:.3e}")


@pytest.mark.parametrize("n", SWEEP_N)
def test_sweep_pca_and_project(n):
    from pesto_amd import dynamics as dy
    m = 3 * n
    for F in SWEEP_F:
        ddof = 0 if F == 1 else 1
        xyz, y = swept(F, n, ddof)
        e_ref, dev_eigh = y.e_ref_eig(), y.eigh_orth_dev()
        for k in sorted({kk for kk in (1, 5, 32, m) if kk <= min(32, m)}):
            res = dy.pca(xyz, n_components=k, ddof=ddof)
            lam = y.eig()[0]
            rank = min(k, F - 1, m)
            # the rank is pinned where no eigenvalue among the first k sits near the null threshold
            sure = not np.any((lam[:k] > 1e-14 * lam[0]) & (lam[:k] < 1e-10 * lam[0])) if lam[0] > 0 else True
            if sure and lam[0] > 0:
                rank = int((lam[:k] > 1e-12 * lam[0]).sum())
            check_pca(res, y, k, 1e-9, e_ref, dev_eigh, True, rank if sure else None, f"F={F} n={n} k={k}")
            assert ulp32_ratio(np.asarray(res.mean).reshape(-1), y.mean) <= 1.0
            r = y.proj_check(res.projections, res.components)
            assert r <= 1.0, (F, n, k, r)
            if k == min(5, m):
                p2 = dy.project(xyz, res.mean, res.components)
                assert p2.dtype == np.float32 and p2.shape == (F, k)
                r2 = y.proj_check(p2, res.components, mean32=res.mean)
                assert r2 <= 1.0, (F, n, k, r2)


@pytest.mark.parametrize("case", sorted(PCA_CASES))
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_named_cases(case, on_device):
    from pesto_amd import dynamics as dy
    g = golden("dynamics")
    (xyz, sel, scale, ddof, k), y = yard(case)
    x = dev(xyz) if on_device else xyz
    res = dy.pca(x, sel=sel, n_components=k, scale=scale, ddof=ddof)
    for v in (res.eigenvalues, res.components, res.projections, res.mean, res.residuals):
        assert v.is_cuda if on_device else isinstance(v, np.ndarray)
    res = res._replace(**{f: host(getattr(res, f)) for f in ("eigenvalues", "components", "projections", "mean", "residuals")})
    c = PCA_CASES[case]
    fig = check_pca(res, y, k, 1e-9, float(g[case + "_e_ref_eig"]), float(g[case + "_orth_dev"]), c["converge"], c.get("rank"), case)
    if c["converge"]:
        assert fig["iterations"] <= 64
    r = y.proj_check(res.projections, res.components)
    print(case, "projection error / bound", r)
    assert r <= 1.0
    assert ulp32_ratio(res.mean.reshape(-1), y.mean) <= 1.0
    if case == "identical_5x22":
        assert not res.eigenvalues.any() and not res.components.any() and not res.projections.any() and res.total_variance == 0.0
    worst = check_basics(dy, x, y, sel, case, [0, 1])
    print(case, "largest covariance error / bound", worst)
    if case + "_rmsf" in g.files:
        assert ulp32_ratio(host(dy.rmsf(x, sel=sel, scale=scale)), g[case + "_rmsf"]) <= 1.0


def test_identical_frames_and_one_moving_atom_dccm():
    from pesto_amd import dynamics as dy
    M = dy.cross_correlation(yard("identical_5x22")[0][0])
    assert np.array_equal(M, np.eye(22, dtype=np.float32))
    M = dy.cross_correlation(yard("one_atom_17x21")[0][0])
    assert np.array_equal(M, np.eye(21, dtype=np.float32))
    assert not dy.rmsf(yard("identical_5x22")[0][0]).any()


def test_selections_agree_with_a_gathered_copy():
    from pesto_amd import dynamics as dy
    xyz = planted(17, 65, 10, 1e-3, 0.3, 7)
    idx = np.array([64, 3, 17, 5, 40, 41, 42, 0, 9, 33, 2, 8, 21, 22, 23, 63, 50, 31, 30, 12, 13, 60])          # permuted, n = 22
    mask = np.zeros(65, bool)
    mask[idx] = True
    for sel, gathered in ((idx, xyz[:, idx]), (mask, xyz[:, np.nonzero(mask)[0]]), (None, xyz)):
        a, b = dy.covariance(xyz, sel=sel), dy.covariance(np.ascontiguousarray(gathered))
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        for fa, fb in zip(dy.fluctuations(xyz, sel=sel), dy.fluctuations(np.ascontiguousarray(gathered))):
            assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
        assert np.array_equal(dy.cross_correlation(xyz, sel=sel).view(np.uint32), dy.cross_correlation(np.ascontiguousarray(gathered)).view(np.uint32))
        pa, pb = dy.pca(xyz, sel=sel, n_components=5), dy.pca(np.ascontiguousarray(gathered), n_components=5)
        assert np.array_equal(pa.components.view(np.uint64), pb.components.view(np.uint64))
        assert np.array_equal(pa.projections.view(np.uint32), pb.projections.view(np.uint32))
    # an object with .xyz, and a list as the selection
    class Traj:
        pass
    t = Traj()
    t.xyz = xyz
    assert np.array_equal(dy.rmsf(t, sel=list(idx)).view(np.uint32), dy.rmsf(xyz, sel=idx).view(np.uint32))


def test_two_calls_and_two_sides_give_the_same_bits():
    from pesto_amd import dynamics as dy
    (xyz, sel, scale, ddof, k), _ = yard("planted_65x22")
    d = dev(xyz)

    def everything(x):
        p = dy.pca(x, n_components=k)
        out = list(dy.fluctuations(x)) + [dy.covariance(x), dy.cross_correlation(x), p.eigenvalues, p.components, p.projections, p.mean, p.residuals,
                                          dy.project(x, p.mean, p.components)]
        return [host(v).tobytes() for v in out] + [p.total_variance, p.rank, p.iterations, p.converged]

    first = everything(xyz)
    assert everything(xyz) == first and everything(d) == first


def test_fit_superposes_first_and_project_takes_other_frames():
    from pesto_amd import dynamics as dy, trajectory as tr
    (xyz, sel, scale, ddof, k), _ = yard("md29_sel")
    res = dy.pca(xyz, sel=sel, n_components=3, scale=scale, fit=0)
    sup = tr.superpose(xyz[:1], xyz, sel, sel)
    want = dy.pca(sup, sel=sel, n_components=3, scale=scale)
    assert np.array_equal(res.components.view(np.uint64), want.components.view(np.uint64))
    ref = np.ascontiguousarray(xyz[0, sel])
    res2 = dy.pca(xyz, sel=sel, n_components=3, scale=scale, fit=ref)
    assert np.allclose(res2.eigenvalues, want.eigenvalues, rtol=1e-5)           # (the same fit from a gathered reference)
    # other frames on the basis: the first 5 superposed frames give the rows of the full projection, bit for bit
    p = dy.project(np.ascontiguousarray(sup[:5]), want.mean, want.components, sel=sel, scale=scale)
    y = Yardstick(sup[:5], sel, scale, 1)
    assert y.proj_check(p, want.components, mean32=want.mean) <= 1.0


def test_non_convergence_is_reported_not_raised():
    from pesto_amd import dynamics as dy
    (xyz, sel, scale, ddof, k), y = yard("flat_200x70")
    g = golden("dynamics")
    res = dy.pca(xyz, n_components=k, max_iter=1)
    assert res.iterations == 1 and not res.converged
    check_pca(res, y, k, 1e-9, float(g["flat_200x70_e_ref_eig"]), float(g["flat_200x70_orth_dev"]), False, None, "flat, one iteration")
    loose = dy.pca(xyz, n_components=k, tol=10.0)         # |C v - theta v| <= lambda_0 / 2 for any Ritz pair
    assert loose.converged and loose.iterations == 1
