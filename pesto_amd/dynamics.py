"""Essential dynamics of MD frames on the GPU: what an MD user looks at after the RMSD curve (pesto_dynamics.hip).

The reference contains none of this (its notebooks stop at the clustering); what stands here is the standard set of tools (Amadei et
al. 1993; ``gmx covar`` / ``gmx anaeig``, mdtraj + sklearn's PCA, MDAnalysis.analysis.pca):
    fluctuations / rmsf   the mean structure and the root-mean-square fluctuation of every atom
    covariance            the positional covariance matrix, float64 [3n, 3n]
    cross_correlation     the dynamic cross-correlation map (DCCM), float32 [n, n]
    pca                   the leading principal components of the frames and the frames projected on them
    project               other frames on a given basis (the bound ensemble on the unbound run's modes)
Calling conventions are those of pesto_amd.clustering: float32 [F, N, 3] arrays or objects with ``.xyz``; ``sel`` an index array or a
mask; ``scale`` multiplies coordinates (10: nanometres in, angstroms out); the first array decides where a call runs (_lib.Side: ROCm
tensors in, ROCm tensors out on torch's current stream; NumPy in, NumPy out); ``model`` lends its device handle, without one a
weightless handle is used; arguments are checked before any launch (ValueError); there is no CPU fallback.

Definition, with x_f the selected coordinates of frame f flattened to m = 3n values, all in double from the float32 inputs:
    mean = (1/F) sum_f x_f          d_f = (double)x_f - mean   (centred BEFORE multiplying)
    C    = scale^2 sum_f d_f d_f^T / (F - ddof),  ddof 0 or 1 (default 1), F - ddof >= 1
    rmsf_i  = scale sqrt((1/F) sum_f |d_f,i|^2)                                       rounded to float32 once
    DCCM_ij = tr(C_ij) / sqrt(tr(C_ii) tr(C_jj)) over the 3 x 3 blocks of C           rounded once; 1 on the diagonal; 0, never NaN, for
                                                                                      an atom without variance
    pca: the k leading eigenpairs (theta_i, v_i) of C by block subspace iteration with Rayleigh-Ritz on 64 vectors, matrix-free (C is
    never formed, so any F against 3n works without m^2 memory); projections = scale d_f . v_i rounded once
Every sum runs in an order fixed by the shapes alone, so every output is bit-identical from call to call. The covariance evaluates only
the tiles i <= j and mirrors them: C and the DCCM are bitwise symmetric.

Measured on an MI355X: profiles/bench_dynamics.py -> profiles/dynamics.json; DESIGN.md section 4.23 has the kernels, the bounds of the
tests and what was not done (mass weighting, iterative fitting to the mean, quasi-harmonic entropies, tICA).
"""
import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib
from .trajectory import _model_of, _selection, _xyz

MAX_FRAMES = 2 ** 24        # PESTO_DYNAMICS_MAX_FRAMES
MAX_ATOMS = 2 ** 24         # PESTO_DYNAMICS_MAX_ATOMS
MAX_COV = 2 ** 27           # PESTO_DYNAMICS_MAX_COV: (3n)^2 of covariance and cross_correlation
MAX_COMPONENTS = 32         # PESTO_DYNAMICS_MAX_COMPONENTS
MAX_BASIS = 64              # components of project
F32_MAX = float(np.finfo(np.float32).max)

__all__ = ["PCA", "fluctuations", "rmsf", "covariance", "cross_correlation", "pca", "project"]


class PCA(NamedTuple):
    """eigenvalues float64 [k], descending, >= 0; components float64 [k, n, 3], orthonormal rows, in each the entry of largest magnitude
    positive (lowest index on ties); projections float32 [F, k] = scale d_f . v_i; mean float32 [n, 3] (input units); total_variance =
    tr C; residuals float64 [k] = |C v_i - theta_i v_i|; rank: the directions among the k with an eigenvalue above 1e-12 of the largest
    (the others have eigenvalue 0 and an all-zero component); iterations; converged = (max residual <= tol * eigenvalues[0])."""
    eigenvalues: object
    components: object
    projections: object
    mean: object
    total_variance: float
    residuals: object
    rank: int
    iterations: int
    converged: bool


def _check(xyz, sel, scale, ddof=None, cov=False):
    a = _xyz(xyz)
    F, N = int(a.shape[0]), int(a.shape[1])
    if F > MAX_FRAMES or N > MAX_ATOMS:
        raise ValueError(f"at most 2**24 frames and 2**24 atoms, got {F} and {N}")
    s, n = _selection(sel, N, "sel", least=1)
    sc = float(scale)
    if not (np.isfinite(sc) and abs(sc) <= F32_MAX):
        raise ValueError(f"scale must be finite, got {scale!r}")
    if ddof is not None:
        if isinstance(ddof, bool) or ddof not in (0, 1):
            raise ValueError(f"ddof must be 0 or 1, got {ddof!r}")
        if F - int(ddof) < 1:
            raise ValueError(f"F - ddof must be at least 1, got {F} frames with ddof={ddof}")
    if cov and (3 * n) ** 2 > MAX_COV:
        raise ValueError(f"(3n)**2 must not exceed 2**27 entries, got n = {n}")
    return a, F, N, s, n, sc


def _call(a, model):
    model = _model_of(model, a)
    return model, _lib.Side(a, model._gpu), _lib.load()


def fluctuations(xyz, sel=None, scale=10.0, model=None):
    """(mean float32 [n, 3], rmsf float32 [n]): the mean position of every selected atom over the frames, in the input's unit (unscaled, so
    it can be fed back as the reference of trajectory.superpose), and its root-mean-square fluctuation about it times scale."""
    a, F, N, s, n, sc = _check(xyz, sel, scale)
    model, side, lib = _call(a, model)
    x = side.put(a, np.float32)
    sd = None if s is None else side.put(s, np.int32)
    mean, out = side.empty((n, 3), np.float32), side.empty((n,), np.float32)
    _lib.check(lib.pesto_fluctuations(model.handle, F, N, n, side.ptr(x), side.ptr(sd), sc, side.ptr(mean), side.ptr(out), side.kind, side.stream),
               lib.pesto_dynamics_last_error)
    return side.result(mean), side.result(out)


def rmsf(xyz, sel=None, scale=10.0, model=None):
    """float32 [n]: the second element of fluctuations."""
    return fluctuations(xyz, sel, scale, model)[1]


def covariance(xyz, sel=None, scale=10.0, ddof=1, model=None):
    """float64 [3n, 3n]: C = scale^2 sum_f d_f d_f^T / (F - ddof), bitwise symmetric. (3n)^2 <= MAX_COV entries (1 GiB)."""
    a, F, N, s, n, sc = _check(xyz, sel, scale, ddof, cov=True)
    model, side, lib = _call(a, model)
    x = side.put(a, np.float32)
    sd = None if s is None else side.put(s, np.int32)
    C = side.empty((3 * n, 3 * n), np.float64)
    _lib.check(lib.pesto_covariance(model.handle, F, N, n, side.ptr(x), side.ptr(sd), sc, int(ddof), side.ptr(C), side.kind, side.stream),
               lib.pesto_dynamics_last_error)
    return side.result(C)


def cross_correlation(xyz, sel=None, model=None):
    """float32 [n, n]: the dynamic cross-correlation map, bitwise symmetric with a diagonal of exactly 1; an atom without variance gets 0
    off the diagonal. The covariance behind it is device scratch: (3n)^2 <= MAX_COV."""
    a, F, N, s, n, _ = _check(xyz, sel, 1.0, cov=True)
    model, side, lib = _call(a, model)
    x = side.put(a, np.float32)
    sd = None if s is None else side.put(s, np.int32)
    M = side.empty((n, n), np.float32)
    _lib.check(lib.pesto_cross_correlation(model.handle, F, N, n, side.ptr(x), side.ptr(sd), side.ptr(M), side.kind, side.stream),
               lib.pesto_dynamics_last_error)
    return side.result(M)


def pca(xyz, sel=None, n_components=10, scale=10.0, ddof=1, tol=1e-9, max_iter=64, fit=None, model=None):
    """PCA of the frames on the selected atoms: the n_components <= min(MAX_COMPONENTS, 3n) leading eigenpairs of the covariance and the
    frames projected on them. ``fit``: a frame index or an [n, 3] array (the selected atoms of a reference); the frames are first superposed
    on it by trajectory.superpose on ``sel``. Without it the caller's frames are taken as they are. Non-convergence within max_iter is
    reported (``converged``), never raised."""
    return _pca(xyz, sel, n_components, scale, ddof, tol, max_iter, fit, model)[0]


def _pca(xyz, sel, n_components, scale, ddof, tol, max_iter, fit, model):
    """(PCA, the most sweeps one of the call's 64 x 64 Jacobi runs took: a diagnostic for profiles/bench_dynamics.py)"""
    a, F, N, s, n, sc = _check(xyz, sel, scale, ddof)
    k = int(n_components)
    if not 1 <= k <= min(MAX_COMPONENTS, 3 * n):
        raise ValueError(f"n_components must lie in 1 .. min({MAX_COMPONENTS}, 3n = {3 * n}), got {n_components!r}")
    tl, mi = float(tol), int(max_iter)
    if not (np.isfinite(tl) and tl >= 0.0):
        raise ValueError(f"tol must be finite and >= 0, got {tol!r}")
    if mi < 1:
        raise ValueError(f"max_iter must be at least 1, got {max_iter!r}")
    if fit is not None:
        a = _fitted(a, fit, F, N, s, n, model)
    model, side, lib = _call(a, model)
    x = side.put(a, np.float32)
    sd = None if s is None else side.put(s, np.int32)
    eig, comp = side.empty((k,), np.float64), side.empty((k, n, 3), np.float64)
    proj, mean, res = side.empty((F, k), np.float32), side.empty((n, 3), np.float32), side.empty((k,), np.float64)
    total, info = ctypes.c_double(0.0), (ctypes.c_int32 * 4)()
    _lib.check(lib.pesto_pca(model.handle, F, N, n, side.ptr(x), side.ptr(sd), k, sc, int(ddof), tl, mi, side.ptr(eig), side.ptr(comp), side.ptr(proj),
                             side.ptr(mean), side.ptr(res), ctypes.byref(total), info, side.kind, side.stream), lib.pesto_dynamics_last_error)
    r = side.result
    return PCA(r(eig), r(comp), r(proj), r(mean), float(total.value), r(res), int(info[0]), int(info[1]), bool(info[2])), int(info[3])


def _fitted(a, fit, F, N, s, n, model):
    """the frames superposed on ``fit`` (a frame index, or the [n, 3] selected atoms of a reference) on the selection"""
    from .trajectory import superpose
    if isinstance(fit, (int, np.integer)) and not isinstance(fit, bool):
        if not -F <= int(fit) < F:
            raise ValueError(f"fit: frame index {fit} out of range for {F} frames")
        i = int(fit) % F
        return superpose(a[i:i + 1], a, s, s, model=model)
    ref = fit if _lib.is_torch(fit) else np.asarray(fit, np.float32)
    if tuple(ref.shape) != (n, 3):
        raise ValueError(f"fit must be a frame index or an [n = {n}, 3] array, got shape {list(ref.shape)}")
    return superpose(ref.reshape(1, n, 3), a, None, s, model=model)


def project(xyz, mean, components, sel=None, scale=10.0, model=None):
    """float32 [F, k] = scale ((double)x_f - mean) . components_i: the frames of xyz on a given basis (mean [n, 3], components [k, n, 3], as
    pca returns them; k <= MAX_BASIS)."""
    a, F, N, s, n, sc = _check(xyz, sel, scale)
    mean = mean if _lib.is_torch(mean) else np.asarray(mean, np.float32)
    components = components if _lib.is_torch(components) else np.asarray(components, np.float64)
    if tuple(mean.shape) != (n, 3):
        raise ValueError(f"mean must be [n = {n}, 3], got {list(mean.shape)}")
    shp = tuple(components.shape)
    if len(shp) != 3 or shp[1:] != (n, 3) or not 1 <= shp[0] <= MAX_BASIS:
        raise ValueError(f"components must be [1 <= k <= {MAX_BASIS}, n = {n}, 3], got {list(shp)}")
    k = int(shp[0])
    model, side, lib = _call(a, model)
    x = side.put(a, np.float32)
    sd = None if s is None else side.put(s, np.int32)
    mu, co = side.put(mean, np.float32), side.put(components, np.float64)
    out = side.empty((F, k), np.float32)
    _lib.check(lib.pesto_project(model.handle, F, N, n, side.ptr(x), side.ptr(sd), k, side.ptr(mu), side.ptr(co), sc, side.ptr(out), side.kind,
                                 side.stream), lib.pesto_dynamics_last_error)
    return side.result(out)
