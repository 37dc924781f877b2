"""CPU tests of pesto_amd.normalmodes and the yardstick its GPU tests (test_normalmodes.py) measure against: a float64 restatement of the
definition (the pair loop, H64, Gamma64 and b, eigh on the complement of R, the sign rule and the zero threshold), the generators (a
seeded self-avoiding 3.8 A chain rounded to float32, the hand-worked networks), the named cases of tests/golden/normalmodes.npz
(written by tests/golden/make_normalmodes_golden.py from seeds and the project's own 1thf_D fixture) with their e_ref, the disagreement
of two float64 routes (eigvalsh of H against the squared singular values of the incidence matrix B, H = B^T B), the bounds as formulas,
and check_modes, the properties every result of anm / gnm must have. Here: the generators' assertions, the hand-worked spectra, the
strictness of the cut-off, the recorded values, every argument check and the exports."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden

EPS64 = 2.0 ** -52
FLOPPY = 1e-10              # pesto_enm.hip: a Ritz value at or below FLOPPY b is a floppy direction


def gamma(p):
    return p * EPS64 / (1.0 - p * EPS64)


def ratio_to(err, bound):
    """largest err / bound; an error of 0 against a bound of 0 counts 0, any other error against it inf"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0.0, err / np.where(bound > 0.0, bound, 1.0), np.where(err == 0.0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


# ---- generators
def chain(n, seed, step=3.8, clash=3.7):
    """float32 [n, 3]: a seeded self-avoiding walk of 3.8 A steps (no two nodes two or more apart along it nearer than `clash`)"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 3))
    i = 1
    while i < n:
        u = rng.standard_normal(3)
        p = x[i - 1] + step * u / np.linalg.norm(u)
        if i < 2 or np.linalg.norm(x[:i - 1] - p, axis=1).min() >= clash:
            x[i] = p
            i += 1
    return np.ascontiguousarray(x.astype(np.float32))


def ca_1thf():
    g = golden("io_1thf_D")
    return np.ascontiguousarray(g["final_xyz"][np.char.strip(g["final_name"].astype(str)) == "CA"], np.float32)


HAND = {
    # name -> (coordinates, cutoff, the non-zero eigenvalues, the floppy directions); gamma 1, p 0, scale 1, all pairs within the cut-off
    "triangle": (np.eye(3, dtype=np.float32), 2.0, [1.5, 1.5, 3.0], 0),
    "tetrahedron": (np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32), 3.0, [1, 1, 2, 2, 2, 4], 0),
    "square": (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), 1.5, [2, 2, 2, 2, 4], 1),
}


def chain_plus_one():
    """a 30-node chain at cut-off 12 and one more node held by a single spring to the chain's last node: 2 floppy directions"""
    x = chain(30, 11).astype(np.float64)
    out = x[29] - x.mean(0)
    return np.ascontiguousarray(np.vstack([x, x[29] + 11.5 * out / np.linalg.norm(out)]).astype(np.float32))


def two_components():
    """two 8-node chains 200 A apart: 6 floppy directions"""
    return np.ascontiguousarray(np.vstack([chain(8, 12), chain(8, 13) + np.float32(200.0)]))


# name -> (coordinates, kind, cutoff, scale, p, k, n_zero)
def named_cases():
    ca = ca_1thf()
    cases = {name: (x, "anm", c, 1.0, 0, min(32, 3 * len(x) - 6), nz) for name, (x, c, _, nz) in HAND.items()}
    cases["chain_plus_one"] = (chain_plus_one(), "anm", 12.0, 1.0, 0, 20, 2)
    cases["two_components"] = (two_components(), "anm", 12.0, 1.0, 0, 20, 6)
    cases["1thf_c8"] = (ca, "anm", 8.0, 1.0, 0, 20, 0)
    cases["1thf_c15"] = (ca, "anm", 15.0, 1.0, 0, 20, 0)
    cases["1thf_gnm_c10"] = (ca, "gnm", 10.0, 1.0, 0, 20, 0)
    return cases


# ---- the yardstick
def springs(x32, cutoff, scale):
    """bool [n, n]: the pair test of the definition in float32, as lddt.reference_pairs makes it"""
    x = np.asarray(x32, np.float32)
    d = x[:, None, :] - x[None, :, :]
    sq = d * d
    s2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    dist = np.sqrt(s2.astype(np.float64)).astype(np.float32) * np.float32(scale)
    return (dist < np.float32(cutoff)) & (s2 > 0)


class Network:
    """the definition in float64 for the selected nodes x32 [n, 3]: the springs, k, H64 or Gamma64, b, R, and (lazily) the eigenpairs on the
    complement of R by LAPACK"""

    def __init__(self, x32, kind="anm", cutoff=15.0, scale=10.0, gamma_=1.0, p=0):
        self.x32 = np.asarray(x32, np.float32)
        self.n, self.dim = len(self.x32), 3 if kind == "anm" else 1
        self.m = self.dim * self.n
        n = self.n
        self.mask = springs(self.x32, cutoff, scale)
        x = self.x32.astype(np.float64)
        r = float(scale) * (x[None, :, :] - x[:, None, :])                 # r[i, j] = scale (x_j - x_i)
        r2 = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            k = np.where(self.mask, float(gamma_) / r2 if p == 2 else float(gamma_), 0.0)
            uu = np.where(self.mask[..., None, None], r[..., :, None] * r[..., None, :] / r2[..., None, None], 0.0)
        self.k, self.r = k, r
        self.rowsum = np.cumsum(k, axis=1)[:, -1] if n else np.zeros(0)          # in ascending j
        self.b = 2.0 * float(self.rowsum.max())
        self.n_springs = int(self.mask.sum()) // 2
        self.deg = self.mask.sum(1)
        if self.dim == 3:
            blocks = -k[..., None, None] * uu
            blocks[np.arange(n), np.arange(n)] = -blocks.sum(1)
            self.M = blocks.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n)
        else:
            self.M = -k + np.diag(self.rowsum)
        self.M = 0.5 * (self.M + self.M.T)
        self.R = self._rigid(float(scale) * x)
        self._eig = None

    def _rigid(self, xs):
        """R, evaluated in np.longdouble (modified Gram-Schmidt twice, a column that loses all but 1e-10 of its norm dropped) and rounded
        to float64 once. R_dev: the sine of the largest angle between that space and the one float64 arithmetic gives from the same
        coordinates (LAPACK's SVD): how well float64 can know R at all. Two bodies far apart make three nearly dependent rotations, and
        their common part is lost to the rounding of x - centroid; every float64 evaluation of R carries an error of that size."""
        self.R_dev = 0.0
        if self.dim == 1:
            return np.full((self.n, 1), 1.0 / np.sqrt(self.n))

        def raw_of(x):
            c = x - x.mean(0)
            raw = np.zeros((self.m, 6), x.dtype)
            for a in range(3):
                raw[a::3, a] = 1.0
                e = np.zeros(3, x.dtype)
                e[a] = 1.0
                raw[:, 3 + a] = np.cross(e, c).reshape(-1)
            return raw
        raw, cols = raw_of(xs.astype(np.longdouble)), []
        for c in range(6):
            v = raw[:, c].copy()
            n0 = (v * v).sum()
            for _ in range(2):
                for w in cols:
                    v = v - (w * v).sum() * w
            n1 = (v * v).sum()
            if n0 > 0 and n1 > np.longdouble(1e-20) * n0:
                cols.append(v / np.sqrt(n1))
        Rl = np.stack(cols, 1)
        U, sv, _ = np.linalg.svd(raw_of(xs), full_matrices=False)
        R64 = U[:, sv > 1e-10 * sv.max()].astype(np.longdouble)
        if R64.shape[1] == Rl.shape[1]:
            self.R_dev = float(np.linalg.norm((Rl - R64 @ (R64.T @ Rl)).astype(np.float64), 2))
        return Rl.astype(np.float64)

    def csr(self):
        off = np.concatenate([[0], np.cumsum(self.deg)]).astype(np.int64)
        i, j = np.nonzero(self.mask)
        return off, j.astype(np.int32), self.k[i, j]

    def entry_bound(self):
        """entrywise bound on a dense matrix against M: 8 eps k_ij off the diagonal blocks, gamma_{deg_i + 8} sum_j k_ij on them"""
        E = 8.0 * EPS64 * np.repeat(np.repeat(self.k, self.dim, 0), self.dim, 1)
        d = np.array([gamma(int(g) + 8) for g in self.deg]) * self.rowsum
        for i in range(self.n):
            E[self.dim * i:self.dim * (i + 1), self.dim * i:self.dim * (i + 1)] = d[i]
        return E

    def eig(self):
        """(lambda ascending [m - rank R], W [m, m - rank R]): eigh of P M P + 2 b R R^T, whose lowest m - rank R pairs are M's on the
        complement of R (the rigid motions sit at 2 b)"""
        if self._eig is None:
            P = np.eye(self.m) - self.R @ self.R.T
            A = P @ self.M @ P + 2.0 * max(self.b, 1.0) * (self.R @ self.R.T)
            lam, W = np.linalg.eigh(0.5 * (A + A.T))
            q = self.m - self.R.shape[1]
            self._eig = lam[:q].copy(), W[:, :q].copy()
        return self._eig

    def e_ref(self):
        """The yardstick's own error in an eigenvalue, the largest of: eigvalsh of M against the squared singular values of the incidence
        matrix B (rows sqrt(k) u^T (e_j - e_i)), M = B^T B; the eigenvalues on the complement of R (eig(), which multiplies M by the
        projector in float64) against the squared singular values of B N, N a basis of the complement; and eps lambda_max, one unit
        roundoff of the matrix' norm, below which no backward-stable eigensolver knows an eigenvalue (the two routes of a 12 x 12 matrix
        can agree by luck to a fraction of it)."""
        i, j = np.nonzero(np.triu(self.mask))
        B = np.zeros((len(i), self.m))
        w = np.sqrt(self.k[i, j])
        for a in range(self.dim):
            u = self.r[i, j, a] / np.sqrt((self.r[i, j] ** 2).sum(1)) if self.dim == 3 else np.ones(len(i))
            B[np.arange(len(i)), self.dim * j + a] = w * u
            B[np.arange(len(i)), self.dim * i + a] = -w * u

        def squares(A, size):
            sv = np.zeros(size)
            if A.shape[0] and size:
                s = np.linalg.svd(A, compute_uv=False) ** 2
                sv[:min(len(s), size)] = s[:size]
            return np.sort(sv)
        full = np.sort(np.linalg.eigvalsh(self.M))
        N = np.linalg.svd(self.R, full_matrices=True)[0][:, self.R.shape[1]:]
        lam = self.eig()[0]
        return float(max(np.abs(full - squares(B, self.m)).max(), np.abs(lam - squares(B @ N, len(lam))).max() if len(lam) else 0.0,
                         EPS64 * np.abs(full).max()))

    def lapack_dev(self):
        """(|W^T W - I|, |R^T W|): what LAPACK's own eigenvectors show through the products check_modes forms. Each is at least eps: the
        products are sums of terms of unit size evaluated in float64, so a deviation below one unit roundoff is not measured but met by
        luck (2e-17 for the 2 x 2 Kirchhoff matrix of two nodes). The second is at least R_dev: LAPACK's vectors are orthogonal to the
        very R they were projected with, which says nothing of how well float64 knows R."""
        W = self.eig()[1]
        return max(float(np.abs(W.T @ W - np.eye(W.shape[1])).max()), EPS64), max(float(np.abs(self.R.T @ W).max()), EPS64, self.R_dev)


def check_modes(res, net, k, tol, e_ref, dev, n_zero=None, must_converge=True, label=""):
    """Every property a result of anm / gnm must have, in float64 from the returned arrays against the yardstick; returns the figures."""
    m, b = net.m, net.b
    th = np.asarray(res.eigenvalues, np.float64)
    V = np.asarray(res.modes, np.float64).reshape(k, m)
    rs = np.asarray(res.residuals, np.float64)
    assert th.shape == (k,) and rs.shape == (k,) and np.asarray(res.modes).shape == ((k, net.n, 3) if net.dim == 3 else (k, net.n))
    assert np.all(np.isfinite(th)) and np.all(np.isfinite(V)) and np.all(np.isfinite(rs)) and np.all(th >= 0.0) and np.all(np.diff(th) >= 0.0)
    assert float(res.bound) == b, (label, res.bound, b)
    assert int(res.n_springs) == net.n_springs
    nz = int(res.n_zero)
    assert nz == int((th == 0.0).sum()) and not np.any((th > 0.0) & (th <= FLOPPY * b))
    if n_zero is not None:
        assert nz == n_zero, (label, nz, n_zero)
    orth = float(np.abs(V @ V.T - np.eye(k)).max())
    rigid = float(np.abs(net.R.T @ V.T).max())
    for i in range(k):          # sign rule: the entry of largest magnitude is positive, the lowest index on ties
        assert V[i, int(np.argmax(np.abs(V[i])))] > 0.0, (label, i)
    # residuals, recomputed with the test's own matrix in np.longdouble, agree within the 2-norm of the matrix' bound
    hb = float(np.linalg.norm(net.entry_bound(), 2)) + 4.0 * e_ref          # (the yardstick's own error enters once, on the norm)
    Vl, Ml, Rl = V.T.astype(np.longdouble), net.M.astype(np.longdouble), net.R.astype(np.longdouble)
    Y = Ml @ Vl
    Y = Y - Rl @ (Rl.T @ Y)
    D = Y - Vl * th.astype(np.longdouble)
    rec = np.sqrt((D * D).sum(0)).astype(np.float64)
    res_gap = float(np.abs(rec - rs).max())
    assert bool(res.converged) == bool(rs.max() <= tol * b), (label, rs.max(), tol * b)
    assert 1 <= int(res.iterations) <= int(res.applies)
    lam = net.eig()[0][:k]
    weyl = float((np.abs(th - lam) / (rec + 4.0 * e_ref + 1e-300)).max()) if res.converged else 0.0
    figures = dict(orth=orth, orth_bound=4.0 * dev[0], rigid=rigid, rigid_bound=4.0 * dev[1], res_gap=res_gap, res_bound=hb, weyl_ratio=weyl,
                   worst_residual_over_b=float(rs.max() / b) if b else 0.0, iterations=int(res.iterations), applies=int(res.applies), n_zero=nz,
                   converged=bool(res.converged))
    print(label, figures)
    assert orth <= 4.0 * dev[0], (label, orth, 4.0 * dev[0])
    assert rigid <= 4.0 * dev[1], (label, rigid, 4.0 * dev[1])
    assert res_gap <= hb, (label, res_gap, hb)
    assert weyl <= 1.0, (label, weyl)
    if must_converge:
        assert res.converged, (label, "not converged", figures)
    return figures


def modes64(net, k):
    """a NumPy restatement of what anm / gnm return (LAPACK on the complement), to test check_modes"""
    from pesto_amd.normalmodes import Modes
    lam, W = net.eig()
    th, V = lam[:k].copy(), W[:, :k].T.copy()
    for i in range(k):
        if V[i, int(np.argmax(np.abs(V[i])))] < 0:
            V[i] = -V[i]
    Y = net.M @ V.T
    Y -= net.R @ (net.R.T @ Y)
    rs = np.linalg.norm(Y - V.T * th, axis=0)
    floppy = th <= FLOPPY * net.b
    th[floppy] = 0.0
    return Modes(th, V.reshape((k, net.n, 3) if net.dim == 3 else (k, net.n)), rs, net.b, int(floppy.sum()), 1, 1, net.n_springs,
                 bool(rs.max() <= 1e-10 * net.b))


_nets = {}


def named(case):
    """(recipe, Network, recorded values) of a named case, computed once"""
    if case not in _nets:
        x, kind, cutoff, scale, p, k, nz = named_cases()[case]
        g = golden("normalmodes")
        rec = {f: g[case + "/" + f] for f in ("x", "e_ref", "dev", "lam", "b", "n_springs")}
        _nets[case] = ((x, kind, cutoff, scale, p, k, nz), Network(x, kind, cutoff, scale, 1.0, p), rec)
    return _nets[case]


NAMES = ["triangle", "tetrahedron", "square", "chain_plus_one", "two_components", "1thf_c8", "1thf_c15", "1thf_gnm_c10"]


# ---- the tests
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_worked_spectra(name):
    x, cutoff, want, floppy = HAND[name]
    net = Network(x, "anm", cutoff, 1.0)
    assert net.mask.sum() == len(x) * (len(x) - 1)                   # all pairs within the cut-off
    lam = np.linalg.eigvalsh(net.M)
    zero = lam[np.abs(lam) <= 1e-12 * net.b]
    assert len(zero) == 6 + floppy and np.allclose(lam[len(zero):], sorted(want), rtol=0, atol=1e-12)
    lc = net.eig()[0]
    assert int((lc <= FLOPPY * net.b).sum()) == floppy and np.allclose(lc[floppy:], sorted(want), rtol=0, atol=1e-12)


def test_two_nodes_and_floppy_generators():
    net = Network(np.array([[0, 0, 0], [0, 3, 4]], np.float32), "anm", 6.0, 1.0)
    assert np.allclose(np.linalg.eigvalsh(net.M), [0, 0, 0, 0, 0, 2], rtol=0, atol=1e-15) and net.b == 2.0
    for case, floppy in (("chain_plus_one", 2), ("two_components", 6)):
        (x, kind, cutoff, scale, p, k, nz), net, _ = named(case)
        assert nz == floppy and int((net.eig()[0] <= FLOPPY * net.b).sum()) == floppy
    assert named("chain_plus_one")[1].deg[30] == 1 and named("two_components")[1].R.shape[1] == 6
    assert Network(np.array([[0, 0, 0], [1, 0, 0], [2.5, 0, 0]], np.float32), "anm", 9.0, 1.0).R.shape[1] == 5          # collinear: rank 5


@pytest.mark.parametrize("case", NAMES)
def test_generator_assertions_and_recorded_values(case):
    (x, kind, cutoff, scale, p, k, nz), net, rec = named(case)
    assert np.array_equal(rec["x"], x) and float(rec["b"]) == net.b and int(rec["n_springs"]) == net.n_springs
    e_ref = net.e_ref()
    assert e_ref <= 64 * EPS64 * net.b and float(rec["e_ref"]) <= 64 * EPS64 * net.b
    lam = net.eig()[0]
    # no non-zero eigenvalue between 1e-14 b and 1e-6 b: the floppy threshold of 1e-10 b decides nothing by rounding
    assert not np.any((lam > 1e-14 * net.b) & (lam < 1e-6 * net.b)), lam[:8] / net.b
    assert np.abs(lam[:k] - rec["lam"]).max() <= 4.0 * max(e_ref, float(rec["e_ref"]))
    assert all(d <= 256 * EPS64 for d in net.lapack_dev()) and all(d <= 256 * EPS64 for d in rec["dev"])
    # eigenvalues matched index by index are more than 10 e_ref apart, or form a known multiplet (the hand-worked networks')
    if case not in HAND:
        live = lam[:k + 1][lam[:k + 1] > FLOPPY * net.b]
        assert np.all(np.diff(live) > 10.0 * e_ref), (case, np.diff(live).min(), e_ref)


@pytest.mark.parametrize("case", ["tetrahedron", "chain_plus_one", "1thf_gnm_c10"])
def test_check_modes_accepts_the_lapack_solution(case):
    (x, kind, cutoff, scale, p, k, nz), net, rec = named(case)
    dev = tuple(4.0 * d for d in net.lapack_dev())                  # (the same vectors: no margin to spend)
    check_modes(modes64(net, k), net, k, 1e-10, net.e_ref(), dev, n_zero=nz, label=case)


def test_cutoff_is_strict():
    # a pair planted at exactly the cut-off on dyadic coordinates is no spring; one float32 step nearer it is
    at = np.array([[0, 0, 0], [8, 0, 0]], np.float32)
    assert not springs(at, 8.0, 1.0).any() and not springs(at / 8, 8.0, 8.0).any()
    near = at.copy()
    near[1, 0] = np.nextafter(np.float32(8), np.float32(0))
    assert springs(near, 8.0, 1.0).sum() == 2
    assert not springs(np.zeros((2, 3), np.float32), 8.0, 1.0).any()           # coincident nodes share no spring


def test_chain_generator_is_self_avoiding_and_seeded():
    x = chain(65, 3).astype(np.float64)
    d = np.linalg.norm(x[:, None] - x[None], axis=2)
    assert np.allclose(np.diag(d, 1), 3.8, atol=1e-5) and d[np.triu_indices(65, 2)].min() >= 3.7 - 1e-5
    assert np.array_equal(chain(65, 3), chain(65, 3)) and not np.array_equal(chain(65, 3), chain(65, 4))


def test_host_helpers():
    from pesto_amd import normalmodes as nm
    A = nm.sample_amplitudes([0.0, 1.0, 4.0], 200, rmsd=1.5, seed=7, n_nodes=10)
    assert A.shape == (200, 3) and not A[:, 0].any() and np.isclose(np.sqrt(np.mean((A * A).sum(1)) / 10), 1.5)
    assert np.array_equal(A, nm.sample_amplitudes([0.0, 1.0, 4.0], 200, rmsd=1.5, seed=7, n_nodes=10))
    assert np.isclose(A[:, 1].std() / A[:, 2].std(), 2.0, rtol=0.3)
    P = nm.mode_path(4, 2, 5, rmsd=1.0, n_nodes=9)
    assert P.shape == (5, 4) and np.allclose(P[:, 2], [-3, -1.5, 0, 1.5, 3]) and not P[:, [0, 1, 3]].any()
    assert np.allclose(nm.cumulative_overlap(np.array([0.6, 0.8])), [0.6, 1.0])
    with pytest.raises(ValueError):
        nm.mode_path(4, 4, 5, n_nodes=3)
    with pytest.raises(ValueError):
        nm.sample_amplitudes([1.0], 0, n_nodes=3)
    with pytest.raises(TypeError):          # n_nodes has no default: a per-node rmsd is undefined without it
        nm.sample_amplitudes([1.0], 4)
    with pytest.raises(TypeError):
        nm.mode_path(4, 1, 5)


def test_argument_checks_come_before_the_library(monkeypatch):
    from pesto_amd import _lib, normalmodes as nm

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    x = chain(8, 1)
    bad = [lambda: nm.anm(x[:2]), lambda: nm.anm(x, n_modes=0), lambda: nm.anm(x, n_modes=19), lambda: nm.anm(x, n_modes=33),
           lambda: nm.gnm(x[:1]), lambda: nm.gnm(x, n_modes=8), lambda: nm.anm(x, cutoff=0.0), lambda: nm.anm(x, cutoff=float("nan")),
           lambda: nm.anm(x, scale=-1.0), lambda: nm.anm(x, gamma=0.0), lambda: nm.anm(x, gamma=float("inf")), lambda: nm.anm(x, p=1),
           lambda: nm.anm(x, tol=-1.0), lambda: nm.anm(x, max_iter=0), lambda: nm.anm(x, sel=[0, 1, 9]), lambda: nm.anm(x.reshape(-1)),
           lambda: nm.network(np.zeros((2, 8, 3), np.float32)), lambda: nm.hessian(x, sel=np.ones(7, bool)), lambda: nm.kirchhoff(x, p=True),
           lambda: nm.mode_fluctuations(np.ones(3), np.zeros((2, 8, 3))), lambda: nm.mode_fluctuations(np.ones(2), np.zeros((2, 8, 3)), factor=np.inf),
           lambda: nm.mode_correlation(np.ones(2), np.zeros((2, 8, 2))), lambda: nm.overlap(np.zeros((2, 8, 3)), np.zeros((2, 7, 3))),
           lambda: nm.deform(x, np.zeros((2, 7, 3)), np.zeros((4, 2))), lambda: nm.deform(x, np.zeros((2, 8, 3)), np.zeros((4, 3))),
           lambda: nm.deform(x, np.zeros((2, 3, 3)), np.zeros((4, 2)), node_of_atom=[0, 1, 2, 3, 0, 1, 2, 0]),
           lambda: nm.structure_modes({"xyz": x}, kind="enm")]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"call {i} was accepted")


def test_exports_header_and_abi():
    import pesto_amd
    from pesto_amd import _lib, normalmodes as nm
    from pesto_amd.csrc import build
    names = ["Modes", "network", "hessian", "kirchhoff", "anm", "gnm", "mode_fluctuations", "mode_correlation", "overlap", "cumulative_overlap",
             "deform", "sample_amplitudes", "mode_path", "structure_modes"]
    assert sorted(nm.__all__) == sorted(names)
    for nme in names + ["normalmodes"]:
        assert nme in pesto_amd.__all__ and getattr(pesto_amd, nme) is (nm if nme == "normalmodes" else getattr(nm, nme))
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    for sym in ("pesto_enm_network", "pesto_enm_matrix", "pesto_enm_modes", "pesto_enm_fluctuations", "pesto_enm_overlap", "pesto_enm_deform"):
        assert sym in _lib.ABI_SYMBOLS and re.search(r"\bint " + sym + r"\(pesto_model\* m,", hdr)
    assert "pesto_enm_last_error" in _lib.ABI_SYMBOLS and re.search(r"const char\* pesto_enm_last_error\(void\);", hdr)
    for name, value in (("NODES", nm.MAX_NODES), ("SPRINGS", nm.MAX_SPRINGS), ("DENSE", nm.MAX_DENSE), ("MODES", nm.MAX_MODES)):
        found = re.search(r"PESTO_ENM_MAX_" + name + r" = (1 << )?(\d+)", hdr)
        assert (1 << int(found.group(2)) if found.group(1) else int(found.group(2))) == value
    assert "pesto_enm.hip" in build.SOURCES and "pesto_ritz.h" in build.HEADERS
    src = open(os.path.join(ROOT, "pesto_amd", "csrc", "pesto_enm.hip")).read()
    # one text of the Rayleigh-Ritz machinery: the ENM translation unit includes it and defines none of it
    assert '#include "pesto_ritz.h"' in src and not re.search(r"void k_dyn_\w+\(", src)
    # the tile skeleton both solvers multiply with is built on the f64 MFMA tile of pesto_mma64.h; since it moved, that is read in the
    # header (the assertion of test_dynamics_fixture.py on pesto_dynamics.hip now meets that file's comment on where the skeleton went)
    ritz = open(os.path.join(ROOT, "pesto_amd", "csrc", "pesto_ritz.h")).read()
    dyn = open(os.path.join(ROOT, "pesto_amd", "csrc", "pesto_dynamics.hip")).read()
    assert '#include "pesto_mma64.h"' in ritz and "mma64_loop<f64x4, false>(lds" in ritz and "void k_dyn_jacobi(" in ritz
    assert '#include "pesto_ritz.h"' in dyn and not re.search(r"void k_dyn_(mma|jacobi|rotate|polish|resid)\(", dyn)
    assert float(re.search(r"FLOPPY = ([0-9.e-]+);", src).group(1)) == FLOPPY
