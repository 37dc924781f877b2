"""CPU tests of pesto_amd.dynamics and the yardstick its GPU tests (test_dynamics.py) measure against: a float64 restatement of the
definition (mean, centred frames, covariance, RMSF, DCCM, eigenpairs by LAPACK), the named cases of tests/golden/dynamics.npz (generated
by tests/golden/make_dynamics_golden.py from seeds and frame indices, no reference code involved) with their e_ref, the disagreement of
two independent float64 routes, the bounds as formulas, and check_pca, the properties every PCA result must have. Here: the yardstick's
self-consistency, the recorded values, check_pca against a NumPy restatement of the solver, every argument check (ValueError before
the library is loaded) and the module's exports."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden

EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
RANK_TOL = 1e-12            # pesto_dynamics.hip: a Ritz value at or below RANK_TOL x the largest is a null direction

# name -> recipe. planted: offset 5 + noise N(0, 1) + a rank-r part with singular scale amp 0.8^i on random orthonormal directions (the
# solver's prototype cases); converge: the case must report converged within max_iter
PCA_CASES = {
    "planted_129x65": dict(kind="planted", F=129, n=65, r=40, noise=1e-3, amp=0.3, k=32, seed=101, converge=True),
    "planted_300x100": dict(kind="planted", F=300, n=100, r=12, noise=1e-2, amp=0.3, k=10, seed=102, converge=True),
    "planted_29x290": dict(kind="planted", F=29, n=290, r=28, noise=1e-3, amp=0.3, k=10, seed=103, converge=True),
    "planted_17x21": dict(kind="planted", F=17, n=21, r=5, noise=1e-3, amp=0.3, k=5, seed=104, converge=True),
    "planted_65x22": dict(kind="planted", F=65, n=22, r=30, noise=1e-3, amp=0.3, k=32, seed=105, converge=True),
    "flat_200x70": dict(kind="planted", F=200, n=70, r=0, noise=1.0, amp=0.0, k=8, seed=106, converge=False),
    # coordinates some nm from the origin, fluctuations of 1e-3 nm: what centring before multiplying exists for
    "cancel_65x22": dict(kind="planted", F=65, n=22, r=12, noise=1e-6, amp=1e-3, k=5, seed=107, converge=True, spread=3.0),
    "md29_sel": dict(kind="md29", k=10, converge=True),
    "identical_5x22": dict(kind="identical", F=5, n=22, k=5, seed=108, converge=True, rank=0),
    "one_atom_17x21": dict(kind="one_atom", F=17, n=21, k=5, seed=109, converge=True, rank=3),
    "few_frames_4x22": dict(kind="planted", F=4, n=22, r=3, noise=1e-3, amp=0.3, k=10, seed=110, converge=True, rank=3),
}


def gamma(p):
    return p * EPS64 / (1.0 - p * EPS64)


def planted(F, n, r, noise, amp, seed, spread=0.0):
    """float32 [F, n, 3]: 5 (+ a per-coordinate offset of up to `spread`) + noise N(0, 1) + a planted rank-r part"""
    rng = np.random.default_rng(seed)
    m = 3 * n
    A = 5.0 + spread * rng.uniform(-1, 1, (1, m)) + noise * rng.standard_normal((F, m))
    if r:
        A = A + (rng.standard_normal((F, r)) * (amp * 0.8 ** np.arange(r))) @ np.linalg.qr(rng.standard_normal((m, r)))[0].T
    return np.ascontiguousarray(A.astype(np.float32).reshape(F, n, 3))


def case_inputs(case):
    """(xyz float32 [F, N, 3], sel, scale, ddof, k) of a named case"""
    c = PCA_CASES[case]
    if c["kind"] == "md29":
        return np.ascontiguousarray(golden("frames_md_1JTG_uL")["X_frames"], np.float32), np.arange(0, 2030, 7), 1.0, 1, c["k"]
    if c["kind"] == "planted":
        return planted(c["F"], c["n"], c["r"], c["noise"], c["amp"], c["seed"], c.get("spread", 0.0)), None, 10.0, 1, c["k"]
    rng = np.random.default_rng(c["seed"])
    x = np.repeat(rng.uniform(2, 8, (1, c["n"], 3)).astype(np.float32), c["F"], 0)
    if c["kind"] == "one_atom":
        x[:, 7] += rng.standard_normal((c["F"], 3)).astype(np.float32) * np.float32(0.1)
    return np.ascontiguousarray(x), None, 10.0, 1, c["k"]


def selected(xyz, sel):
    x = np.asarray(xyz, np.float32)
    if sel is not None:
        s = np.asarray(sel)
        x = x[:, np.nonzero(s)[0] if s.dtype == np.bool_ else s]
    return x.reshape(x.shape[0], -1).astype(np.float64)


class Yardstick:
    """the definition in float64: x [F, m], mean, D = x - mean, C, rmsf, dccm, and (lazily) the eigenpairs of C by LAPACK"""

    def __init__(self, xyz, sel=None, scale=10.0, ddof=1):
        self.x = selected(xyz, sel)
        self.F, self.m = self.x.shape
        self.scale, self.ddof = float(scale), int(ddof)
        self.mean = self.x.mean(0)
        self.D = self.x - self.mean
        self.C = scale * scale * (self.D.T @ self.D) / (self.F - ddof) if self.F - ddof >= 1 else None
        sq = (self.D * self.D).sum(0).reshape(-1, 3).sum(1)
        self.rmsf = scale * np.sqrt(sq / self.F)
        self._eig = None

    def dccm(self):
        G = self.D.T @ self.D
        n = self.m // 3
        tr = G.reshape(n, 3, n, 3).diagonal(axis1=1, axis2=3).sum(-1)
        d = np.diag(tr)
        with np.errstate(divide="ignore", invalid="ignore"):
            M = tr / np.sqrt(np.outer(d, d))
        M[~np.isfinite(M)] = 0.0
        M[np.outer(d, d) <= 0.0] = 0.0
        np.fill_diagonal(M, 1.0)
        return M

    def eig(self):
        if self._eig is None:
            lam, V = np.linalg.eigh(self.C)
            self._eig = lam[::-1].copy(), V[:, ::-1].copy()
        return self._eig

    def e_ref_eig(self):
        """eigvalsh of C against the squared singular values of the centred, scaled frames / (F - ddof)"""
        lam = self.eig()[0]
        sv = np.linalg.svd(self.scale * self.D, compute_uv=False) ** 2 / (self.F - self.ddof)
        sv = np.pad(sv, (0, max(0, self.m - sv.size)))[:self.m]
        return float(np.abs(lam - sv).max())

    def e_ref_sum(self):
        """C in float64 against C summed in np.longdouble"""
        xl = self.x.astype(np.longdouble)
        Dl = xl - xl.mean(0)
        Cl = np.longdouble(self.scale) ** 2 * (Dl.T @ Dl) / (self.F - self.ddof)
        return float(np.abs(self.C - Cl.astype(np.float64)).max())

    def eigh_orth_dev(self):
        V = self.eig()[1]
        return float(np.abs(V.T @ V - np.eye(self.m)).max())

    def cov_bound(self, e_ref):
        """entrywise: scale^2 [gamma_{F+4} (|D|^T |D|)_ij + u (sum_f |d_fi| + sum_f |d_fj|)] / (F - ddof) + 4 e_ref, u = gamma_F max|x| the
        mean's own rounding; holds for any order of summation"""
        A = np.abs(self.D)
        s = A.sum(0)
        u = gamma(self.F) * np.abs(self.x).max()
        return self.scale ** 2 * (gamma(self.F + 4) * (A.T @ A) + u * (s[:, None] + s[None, :])) / (self.F - self.ddof) + 4.0 * e_ref

    def proj_check(self, got, components, mean32=None):
        """(largest ratio of error to bound) of float32 projections against scale D v in float64 with the GIVEN components; the bound is
        scale gamma_{3n} (|D| |v|) plus 1 ulp32 of the value. mean32: the basis' own float32 mean (project); None: this yardstick's."""
        D = self.D if mean32 is None else self.x - np.asarray(mean32, np.float64).reshape(-1)
        V = np.asarray(components, np.float64).reshape(len(components), -1).T
        want = self.scale * (D @ V)
        bound = abs(self.scale) * gamma(self.m) * (np.abs(D) @ np.abs(V)) + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        return ratio_to(np.abs(np.asarray(got, np.float64) - want), bound)


def ratio_to(err, bound):
    """largest err / bound; an error of 0 against a bound of 0 counts 0, any other error against it inf"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0.0, err / np.where(bound > 0.0, bound, 1.0), np.where(err == 0.0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def ulp32_ratio(got, want):
    """largest |got - want| in units of the float32 spacing at |want|"""
    want = np.asarray(want, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)).max())


def check_pca(res, y, k, tol, e_ref, orth_dev, must_converge, rank=None, label=""):
    """Every property a PCA result must have, in float64 from the returned arrays against the yardstick y; returns the figures."""
    F, m, n = y.F, y.m, y.m // 3
    th = np.asarray(res.eigenvalues, np.float64)
    V = np.asarray(res.components, np.float64).reshape(k, m)
    rs = np.asarray(res.residuals, np.float64)
    assert th.shape == (k,) and V.shape == (k, m) and rs.shape == (k,) and np.asarray(res.projections).shape == (F, k)
    assert np.asarray(res.projections).dtype == np.float32 and np.asarray(res.mean).dtype == np.float32
    assert np.all(np.isfinite(th)) and np.all(np.isfinite(V)) and np.all(th >= 0.0) and np.all(np.diff(th) <= 0.0)
    r = int(res.rank)
    assert 0 <= r <= min(k, max(F - 1, 0), m)
    if rank is not None:
        assert r == rank, (label, r, rank)
    assert np.all(th[:r] > 0.0) and not th[r:].any() and not V[r:].any() and not rs[r:].any()
    # orthonormal rows (the null rows are zero)
    G = V @ V.T
    target = np.diag((np.arange(k) < r).astype(np.float64))
    orth = float(np.abs(G - target).max())
    orth_bound = 4.0 * orth_dev
    # sign rule: the entry of largest magnitude is positive, the lowest index on ties
    for i in range(r):
        assert V[i, int(np.argmax(np.abs(V[i])))] > 0.0, (label, i)
    # residuals, recomputed with the test's own C, agree within the 2-norm of the covariance bound
    cb = float(np.linalg.norm(y.cov_bound(e_ref), 2))
    # (in np.longdouble: a float64 product of C rounds by some gamma_m |C|, more than a residual of a few ulp of theta that it is to measure)
    Rl = y.C.astype(np.longdouble) @ V.T.astype(np.longdouble) - V.T.astype(np.longdouble) * th.astype(np.longdouble)
    rec = np.sqrt((Rl * Rl).sum(0)).astype(np.float64)
    res_gap = float(np.abs(rec - rs)[:r].max()) if r else 0.0
    th0 = th[0] if k else 0.0
    assert bool(res.converged) == bool(rs.max() <= tol * th0), (label, rs.max(), tol * th0)
    assert 1 <= int(res.iterations)
    tv_gap = abs(float(res.total_variance) - float(np.trace(y.C)))
    tv_bound = float(np.trace(y.cov_bound(e_ref)))
    lam = y.eig()[0][:k]
    weyl = 0.0
    if res.converged:       # Weyl, index by index: |theta_i - lambda_i| <= residual_i + 4 e_ref, the residual against the test's own C
        lam_r = np.where(np.arange(k) < r, lam, th)         # (a null direction claims only lambda <= RANK_TOL theta_0, below)
        weyl = float((np.abs(th - lam_r) / (rec + 4.0 * e_ref + 1e-300)).max())
        assert np.all(lam[r:] <= 2.0 * RANK_TOL * max(th0, lam[0]) + 4.0 * e_ref)
    figures = dict(orth=orth, orth_bound=orth_bound, res_gap=res_gap, res_bound=cb, tv_gap=tv_gap, tv_bound=tv_bound, weyl_ratio=weyl,
                   iterations=int(res.iterations), converged=bool(res.converged), rank=r)
    print(label, figures)
    assert orth <= orth_bound, (label, orth, orth_bound)
    assert res_gap <= cb, (label, res_gap, cb)
    assert tv_gap <= tv_bound, (label, tv_gap, tv_bound)
    assert weyl <= 1.0, (label, weyl)
    if must_converge:
        assert res.converged, (label, "not converged", figures)
    return figures


# ---- a NumPy restatement of the solver (float64), to test check_pca and the recorded iteration counts
def _ortho(Y):
    for _ in range(2):
        W = Y.T @ Y
        d = np.diag(W)
        di = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
        s, U = np.linalg.eigh(W * np.outer(di, di))
        keep = s > s.max() * 1e-13 if s.max() > 0 else np.zeros_like(s, bool)
        Q = np.zeros_like(Y)
        Q[:, keep] = ((Y * di) @ U[:, keep]) / np.sqrt(s[keep])
        Y = Q
    return Y


def pca64(xyz, sel, k, scale=10.0, ddof=1, tol=1e-9, max_iter=64):
    from pesto_amd.dynamics import PCA
    y = Yardstick(xyz, sel, scale, ddof)
    F, m = y.F, y.m
    D = scale * y.D
    rng = np.random.default_rng(1)
    Q = _ortho(rng.uniform(-1, 1, (m, 64)))
    for it in range(1, max_iter + 1):
        Y = D.T @ (D @ Q) / (F - ddof)
        T = Q.T @ Y
        th, V = np.linalg.eigh((T + T.T) / 2)
        o = np.argsort(-th, kind="stable")
        th, V = th[o], V[:, o]
        X, Z = Q @ V, Y @ V
        live = (th > RANK_TOL * th[0]) & (th[0] > 0)
        res = np.where(live, np.linalg.norm(Z - X * th, axis=0), 0.0)
        conv = res[:k].max() <= tol * max(th[0], 0.0)
        if conv:
            break
        Q = _ortho(Z)
    th, X, res, live = th[:k], X[:, :k].T.copy(), res[:k], live[:k]
    th, X = np.where(live, th, 0.0), X * live[:, None]
    for i in range(k):
        if live[i] and X[i, int(np.argmax(np.abs(X[i])))] < 0:
            X[i] = -X[i]
    proj = (D @ X.T).astype(np.float32)
    return PCA(th, X.reshape(k, m // 3, 3), proj, y.mean.astype(np.float32).reshape(-1, 3), float(np.trace(y.C)), res, int(live.sum()), it, bool(conv))


_yard = {}


def yard(case):
    """(inputs, Yardstick) of a named case, computed once"""
    if case not in _yard:
        xyz, sel, scale, ddof, k = case_inputs(case)
        _yard[case] = ((xyz, sel, scale, ddof, k), Yardstick(xyz, sel, scale, ddof))
    return _yard[case]


# ---- the tests
@pytest.mark.parametrize("case", sorted(PCA_CASES))
def test_recorded_values_and_e_ref(case):
    g = golden("dynamics")
    (xyz, sel, scale, ddof, k), y = yard(case)
    lam = y.eig()[0]
    scale_l = max(lam[0], 1e-300)
    rec = g[case + "_lam"]
    assert rec.shape == (min(33, y.m),)
    # LAPACK builds differ by rounding: the recorded eigenvalues within 64 eps of the largest, and e_ref of the size it was recorded with
    assert np.abs(rec - lam[:rec.size]).max() <= 64 * EPS64 * scale_l
    for key, now in (("_e_ref_eig", y.e_ref_eig()), ("_e_ref_sum", y.e_ref_sum())):
        was = float(g[case + key])
        print(case, key, was, now)
        assert 0.0 <= was <= 1e-12 * scale_l + 1e-300 and now <= 16.0 * max(was, EPS64 * scale_l)
    assert float(g[case + "_orth_dev"]) <= 64 * EPS64
    assert abs(float(g[case + "_total"]) - np.trace(y.C)) <= 64 * EPS64 * np.trace(y.C) + 1e-300
    if PCA_CASES[case]["converge"] and lam[0] > 0:
        # distinct eigenvalues among the significant first k + 1: far apart against residual + 4 e_ref (Weyl matches index by index)
        sig = lam[:k + 1][lam[:k + 1] > 1e-11 * lam[0]]
        if sig.size > 1:
            assert float(g[case + "_min_gap"]) > 10.0 * (1e-9 * lam[0] + 4.0 * float(g[case + "_e_ref_eig"]))
            assert (-np.diff(sig)).min() >= 0.5 * float(g[case + "_min_gap"])
        # no eigenvalue near the null threshold: the rank is not a matter of rounding
        assert not np.any((lam[:k] > 1e-14 * lam[0]) & (lam[:k] < 1e-10 * lam[0]))


def test_yardstick_is_self_consistent():
    (xyz, sel, scale, ddof, k), y = yard("md29_sel")
    assert y.F == 29 and y.m == 870
    assert np.array_equal(y.C, y.C.T) or np.abs(y.C - y.C.T).max() <= 4 * EPS64 * np.abs(y.C).max()
    assert np.allclose(y.C, scale ** 2 * np.cov(y.x.T, ddof=ddof), rtol=1e-12, atol=1e-12 * np.abs(y.C).max())
    n = y.m // 3
    assert np.allclose(y.rmsf ** 2 * y.F / (y.F - ddof), np.diag(y.C).reshape(n, 3).sum(1), rtol=1e-12)
    M = y.dccm()
    assert np.all(np.diag(M) == 1.0) and np.abs(M).max() <= 1.0 + 1e-12 and np.allclose(M, M.T, atol=1e-15)
    lam, V = y.eig()
    assert lam[28] < 1e-12 * lam[0] < lam[27]           # 29 frames: rank 28
    assert abs(lam.sum() - np.trace(y.C)) <= 1e-12 * lam.sum()
    # the bound is far below the values it guards and above the yardstick's own disagreement
    b = y.cov_bound(y.e_ref_sum())
    assert b.max() < 1e-9 * np.abs(y.C).max() and b.min() >= 4 * y.e_ref_sum()
    # zero variance gives 0 off the diagonal
    y1 = yard("one_atom_17x21")[1]
    M1 = y1.dccm()
    assert np.array_equal(M1, np.eye(21)) and y1.rmsf[7] > 0 and not np.delete(y1.rmsf, 7).any()


@pytest.mark.parametrize("case", ["planted_17x21", "planted_65x22", "md29_sel", "identical_5x22", "one_atom_17x21", "few_frames_4x22", "cancel_65x22"])
def test_check_pca_accepts_the_numpy_solver(case):
    (xyz, sel, scale, ddof, k), y = yard(case)
    g = golden("dynamics")
    res = pca64(xyz, sel, k, scale, ddof)
    fig = check_pca(res, y, k, 1e-9, float(g[case + "_e_ref_eig"]), float(g[case + "_orth_dev"]), True, PCA_CASES[case].get("rank"), case)
    assert fig["iterations"] <= 14
    assert y.proj_check(res.projections, res.components) <= 1.0
    # and refuses a wrong one: a component off by 1e-6, an eigenvalue scaled by F / (F - 1)
    if res.rank:
        bad = res._replace(eigenvalues=np.asarray(res.eigenvalues) * y.F / (y.F - 1.0))
        with pytest.raises(AssertionError):
            check_pca(bad, y, k, 1e-9, float(g[case + "_e_ref_eig"]), float(g[case + "_orth_dev"]), True, None, case)


def test_argument_checks_come_before_the_library(monkeypatch):
    from pesto_amd import _lib, dynamics as dy

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(dy, "_model_of", lambda *a: no_load())
    x = np.zeros((4, 5, 3), np.float32)
    bad = [
        lambda: dy.fluctuations(np.zeros((4, 5), np.float32)),
        lambda: dy.fluctuations(np.zeros((0, 5, 3), np.float32)),
        lambda: dy.fluctuations(x, sel=[5]),
        lambda: dy.fluctuations(x, sel=[-1]),
        lambda: dy.fluctuations(x, sel=np.zeros(4, bool)),
        lambda: dy.fluctuations(x, sel=np.zeros(5, bool)),
        lambda: dy.fluctuations(x, sel=np.array([0.5])),
        lambda: dy.rmsf(x, scale=float("nan")),
        lambda: dy.covariance(x, scale=float("inf")),
        lambda: dy.covariance(x, ddof=2),
        lambda: dy.covariance(x, ddof=-1),
        lambda: dy.covariance(x, ddof=True),
        lambda: dy.covariance(x[:1], ddof=1),
        lambda: dy.pca(x[:1], n_components=1, ddof=1),
        lambda: dy.cross_correlation(np.zeros((4, 5, 2), np.float32)),
        lambda: dy.pca(x, n_components=0),
        lambda: dy.pca(x, n_components=16),              # k <= 3n = 15
        lambda: dy.pca(np.zeros((4, 20, 3), np.float32), n_components=33),
        lambda: dy.pca(x, n_components=2, tol=-1.0),
        lambda: dy.pca(x, n_components=2, tol=float("nan")),
        lambda: dy.pca(x, n_components=2, max_iter=0),
        lambda: dy.pca(x, n_components=2, fit=4),
        lambda: dy.pca(x, n_components=2, fit=np.zeros((4, 3), np.float32)),
        lambda: dy.project(x, np.zeros((4, 3), np.float32), np.zeros((2, 5, 3))),
        lambda: dy.project(x, np.zeros((5, 3), np.float32), np.zeros((2, 4, 3))),
        lambda: dy.project(x, np.zeros((5, 3), np.float32), np.zeros((65, 5, 3))),
        lambda: dy.project(x, np.zeros((5, 3), np.float32), np.zeros((5, 3))),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")
    # (3n)^2 <= 2^27 without touching an array of that size
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2, 3862, 3), (0, 0, 0))
    for call in (lambda: dy.covariance(big), lambda: dy.cross_correlation(big)):
        with pytest.raises(ValueError):
            call()
    assert (3 * 3861) ** 2 <= dy.MAX_COV < (3 * 3862) ** 2


def test_exports_header_and_abi():
    import pesto_amd
    from pesto_amd import _lib, dynamics as dy
    from pesto_amd.csrc import build
    names = ["fluctuations", "rmsf", "covariance", "cross_correlation", "pca", "project", "PCA"]
    assert sorted(dy.__all__) == sorted(names)
    for nme in names + ["dynamics"]:
        assert nme in pesto_amd.__all__ and getattr(pesto_amd, nme) is (dy if nme == "dynamics" else getattr(dy, nme))
    assert dy.PCA._fields == ("eigenvalues", "components", "projections", "mean", "total_variance", "residuals", "rank", "iterations", "converged")
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    for sym in ("pesto_fluctuations", "pesto_covariance", "pesto_cross_correlation", "pesto_pca", "pesto_project"):
        assert sym in _lib.ABI_SYMBOLS and re.search(r"\bint " + sym + r"\(pesto_model\* m,", hdr)
    assert "pesto_dynamics_last_error" in _lib.ABI_SYMBOLS and re.search(r"const char\* pesto_dynamics_last_error\(void\);", hdr)
    for name, value in (("MAX_FRAMES", dy.MAX_FRAMES), ("MAX_ATOMS", dy.MAX_ATOMS), ("MAX_COV", dy.MAX_COV)):
        sh = re.search(r"PESTO_DYNAMICS_" + name + r" = 1 << (\d+)", hdr)
        assert sh and 1 << int(sh.group(1)) == value
    assert re.search(r"PESTO_DYNAMICS_MAX_COMPONENTS = (\d+)", hdr).group(1) == str(dy.MAX_COMPONENTS)
    assert "pesto_dynamics.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "pesto_amd", "csrc", "pesto_dynamics.hip")).read()
    tile = open(os.path.join(ROOT, "pesto_amd", "csrc", "pesto_mma64.h")).read()           # the f64 MFMA tile k_dyn_mma is built on
    assert '#include "pesto_mma64.h"' in src and "mma64_loop<" in src and "_mfma_f64_" in tile
    assert "atomicAdd" not in src and "atomicAdd" not in tile
    assert float(re.search(r"RANK_TOL = ([0-9.e+-]+);", src).group(1)) == RANK_TOL
