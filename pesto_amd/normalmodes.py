"""Elastic-network normal modes of ONE structure on the GPU (pesto_enm.hip): what a user with a structure and no trajectory puts in the
place of MD. The anisotropic network model (ANM, Atilgan et al. 2001) and the Gaussian network model (GNM, Bahar et al. 1997), as ProDy,
ElNemo and WEBnm@ offer them, turn the structure into collective modes, predicted fluctuations and an ensemble of deformed conformers
that Model.forward_frames, peaks.cluster_interface_frames and dynamics.pca take as frames:
    network                       the spring list, a CSR
    hessian / kirchhoff           the dense matrices, float64
    anm / gnm                     the lowest modes without the rigid motions (Modes)
    mode_fluctuations / mode_correlation   the predicted B-factor profile and cross-correlation map of a set of modes
    overlap / cumulative_overlap  modes against modes (dynamics.pca's components) or against a displacement between two conformers
    deform                        conformers x + sum_k A[f, k] v_k, every atom of a residue moving with its node
    sample_amplitudes / mode_path amplitudes for deform (host-only helpers)
    structure_modes               the CA network of a structure file or Structure
Calling conventions are those of pesto_amd.dynamics: ``xyz`` float32 [N, 3] or [1, N, 3]; ``sel`` an index array or a mask selecting the
n nodes; ``scale`` multiplies distances (10: nanometres in, angstroms in the definition); the first array decides where a call runs
(_lib.Side: ROCm tensors in, ROCm tensors out on torch's current stream; NumPy in, NumPy out); ``model`` lends its device handle;
arguments are checked on the host (ValueError) and again by the device's verdict before anything is written (PestoError); there is no
CPU or PyTorch fallback.

Definition (this library's own; no equality with ProDy is claimed).
    Springs: the ordered pairs (i, j), i != j, of selected nodes with fl32(sqrt_rn(dist2(i, j))) * fl32(scale) < fl32(cutoff), strict,
    the float32 distance of lddt.reference_pairs, and dist2 > 0 (coincident nodes share no spring). A non-finite selected coordinate
    refuses the call. Stiffness k_ij = gamma |r|^-p with r = scale ((double)x_j - (double)x_i), p 0 (the classic network, k = gamma
    exactly) or 2 (the parameter-free form of Yang et al. 2009 inside the cut-off); gamma > 0 and finite. Defaults: cutoff 15 (ANM) and
    10 (GNM), gamma 1, p 0.
    Hessian (ANM), float64 [3n, 3n]: H_ij = -k_ij r r^T / |r|^2 for a spring, H_ii = -sum_j H_ij in ascending j.
    Kirchhoff (GNM), float64 [n, n]: Gamma_ij = -k_ij, Gamma_ii = sum_j k_ij.
    Bound: b = 2 max_i sum_j k_ij >= lambda_max(Gamma) by Gershgorin, and H <= Gamma (x) I_3 because u u^T <= I for every spring: b
    bounds both spectra and is a function of the list alone.
    Modes: R is the rigid-body basis, three translations and three rotations about the centroid, [3n, 6], orthonormalised in double with
    null directions dropped (GNM: the constant vector). anm / gnm return the k lowest eigenpairs of H (Gamma) restricted to the
    complement of R; k <= min(32, 3n - 6) with n >= 3 (ANM), k <= min(32, n - 1) with n >= 2 (GNM). Eigenvalues ascend. A Ritz value
    <= 1e-10 b is a floppy direction (a node held by one spring, a second component, a planar or collinear network): its eigenvalue is
    reported as exactly 0, it is kept as a mode and counted in n_zero; the threshold is a definition. Modes are float64 [k, n, 3]
    ([k, n]) with orthonormal rows; in each the entry of largest magnitude is positive, lowest index on ties.
    residuals_i = |(I - R R^T) H v_i - theta_i v_i|_2; converged = (max_i residuals_i <= tol b); non-convergence is reported, never raised.
Every sum runs in an order fixed by the shapes and the list alone (no float atomics): every output repeats its bits from call to call
and between host and device inputs.

Measured on an MI355X: profiles/bench_normalmodes.py -> profiles/normalmodes.json; DESIGN.md section 4.29 has the kernels, the solver's
schedule, the bounds of the tests and what was not built (per-frame modes and ragged batches, mass weighting, user-supplied spring
lists, other stiffness forms, nucleic-acid nodes, rotation-translation blocks, more than 32 modes).
"""
import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib
from .trajectory import _model_of, _selection

MAX_NODES = 2 ** 24         # PESTO_ENM_MAX_NODES
MAX_SPRINGS = 2 ** 27       # PESTO_ENM_MAX_SPRINGS
MAX_DENSE = 2 ** 27         # PESTO_ENM_MAX_DENSE
MAX_MODES = 32              # PESTO_ENM_MAX_MODES
MAX_GIVEN = 64              # modes given to mode_fluctuations, mode_correlation, overlap and deform
F32_MAX = float(np.finfo(np.float32).max)

__all__ = ["Modes", "network", "hessian", "kirchhoff", "anm", "gnm", "mode_fluctuations", "mode_correlation", "overlap", "cumulative_overlap",
           "deform", "sample_amplitudes", "mode_path", "structure_modes"]


class Modes(NamedTuple):
    """eigenvalues float64 [k], ascending, a floppy direction exactly 0; modes float64 [k, n, 3] (anm) or [k, n] (gnm), orthonormal rows, in
    each the entry of largest magnitude positive (lowest index on ties); residuals float64 [k]; bound = b; n_zero: the floppy directions
    among the k; iterations: Rayleigh-Ritz steps; applies: operator applications on the block of 64 vectors; n_springs: the springs
    (unordered pairs); converged = (max residual <= tol * bound)."""
    eigenvalues: object
    modes: object
    residuals: object
    bound: float
    n_zero: int
    iterations: int
    applies: int
    n_springs: int
    converged: bool


def _nodes(xyz, name="xyz"):
    """the [N, 3] array of a structure argument ([1, N, 3] is taken too)"""
    a = getattr(xyz, "xyz", xyz)
    if not (_lib.is_torch(a) or isinstance(a, np.ndarray)):
        a = np.asarray(a, np.float32)
    shp = tuple(a.shape)
    if len(shp) == 3 and shp[0] == 1 and shp[2] == 3:
        a, shp = a.reshape(shp[1], 3), shp[1:]
    if len(shp) != 2 or shp[1] != 3 or shp[0] < 1:
        raise ValueError(f"{name} must be [N >= 1, 3] or [1, N, 3], got {list(shp)}")
    if shp[0] > MAX_NODES:
        raise ValueError(f"at most 2**24 atoms, got {shp[0]}")
    return a


def _springs(cutoff, scale, gamma, p):
    c, s, g = float(cutoff), float(scale), float(gamma)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        q = np.float32(c) / np.float32(s) if s else np.float32("nan")
    if not (np.isfinite(c) and np.isfinite(s) and c > 0 and s > 0 and abs(c) <= F32_MAX and abs(s) <= F32_MAX and np.isfinite(q) and q > 0):
        raise ValueError(f"cutoff and scale must be positive and finite (and cutoff / scale a float32), got {cutoff!r}, {scale!r}")
    if not (np.isfinite(g) and g > 0):
        raise ValueError(f"gamma must be positive and finite, got {gamma!r}")
    if isinstance(p, bool) or p not in (0, 2):
        raise ValueError(f"p must be 0 or 2, got {p!r}")
    return c, s, g, int(p)


def _setup(xyz, sel, cutoff, scale, gamma, p, model, least=1):
    a = _nodes(xyz)
    N = int(a.shape[0])
    s, n = _selection(sel, N, "sel", least=least)
    c, sc, g, pp = _springs(cutoff, scale, gamma, p)
    model = _model_of(model, a)
    side = _lib.Side(a, model._gpu)
    x = side.put(a, np.float32)
    sd = None if s is None else side.put(s, np.int32)
    return model, side, _lib.load(), x, sd, N, n, c, sc, g, pp


def network(xyz, sel=None, cutoff=15.0, scale=10.0, gamma=1.0, p=0, model=None):
    """(offsets int64 [n + 1], j int32 [K], k float64 [K]): the springs as a CSR over the selected nodes in the selection's numbering; row
    i = offsets[i]:offsets[i + 1] holds node i's partners j, ascending, with k_ij. Every spring stands twice (K = 2 n_springs)."""
    model, side, lib, x, sd, N, n, c, sc, g, pp = _setup(xyz, sel, cutoff, scale, gamma, p, model)
    off = side.empty((n + 1,), np.int64)
    K, b = ctypes.c_int64(0), ctypes.c_double(0.0)

    def call(cap, j, k):
        _lib.check(lib.pesto_enm_network(model.handle, N, n, side.ptr(x), side.ptr(sd), c, sc, g, pp, cap, side.ptr(off), side.ptr(j), side.ptr(k),
                                         ctypes.byref(K), ctypes.byref(b), side.kind, side.stream), lib.pesto_enm_last_error)
    call(0, None, None)
    j, k = side.empty((int(K.value),), np.int32), side.empty((int(K.value),), np.float64)
    if K.value:
        call(int(K.value), j, k)
    return side.result(off), side.result(j), side.result(k)


def _matrix(xyz, sel, cutoff, scale, gamma, p, model, dim):
    model, side, lib, x, sd, N, n, c, sc, g, pp = _setup(xyz, sel, cutoff, scale, gamma, p, model)
    if (dim * n) ** 2 > MAX_DENSE:
        raise ValueError(f"({dim} n)**2 must not exceed 2**27 entries, got n = {n}")
    out = side.empty((dim * n, dim * n), np.float64)
    _lib.check(lib.pesto_enm_matrix(model.handle, N, n, side.ptr(x), side.ptr(sd), c, sc, g, pp, dim, side.ptr(out), side.kind, side.stream),
               lib.pesto_enm_last_error)
    return side.result(out)


def hessian(xyz, sel=None, cutoff=15.0, scale=10.0, gamma=1.0, p=0, model=None):
    """float64 [3n, 3n]: the ANM Hessian, bitwise symmetric, every diagonal 3 x 3 block included. (3n)^2 <= MAX_DENSE entries (1 GiB)."""
    return _matrix(xyz, sel, cutoff, scale, gamma, p, model, 3)


def kirchhoff(xyz, sel=None, cutoff=10.0, scale=10.0, gamma=1.0, p=0, model=None):
    """float64 [n, n]: the GNM Kirchhoff matrix, bitwise symmetric. n^2 <= MAX_DENSE entries."""
    return _matrix(xyz, sel, cutoff, scale, gamma, p, model, 1)


def _modes(xyz, n_modes, sel, cutoff, scale, gamma, p, tol, max_iter, model, dim):
    a = _nodes(xyz)
    _, n = _selection(sel, int(a.shape[0]), "sel", least=3 if dim == 3 else 2)
    k = int(n_modes)
    room = 3 * n - 6 if dim == 3 else n - 1
    if not 1 <= k <= min(MAX_MODES, room):
        raise ValueError(f"n_modes must lie in 1 .. min({MAX_MODES}, {'3n - 6' if dim == 3 else 'n - 1'} = {room}), got {n_modes!r}")
    tl, mi = float(tol), int(max_iter)
    if not (np.isfinite(tl) and tl >= 0.0):
        raise ValueError(f"tol must be finite and >= 0, got {tol!r}")
    if mi < 1:
        raise ValueError(f"max_iter must be at least 1, got {max_iter!r}")
    model, side, lib, x, sd, N, n, c, sc, g, pp = _setup(a, sel, cutoff, scale, gamma, p, model)
    eig, res = side.empty((k,), np.float64), side.empty((k,), np.float64)
    modes = side.empty((k, n, 3) if dim == 3 else (k, n), np.float64)
    b, K, info = ctypes.c_double(0.0), ctypes.c_int64(0), (ctypes.c_int32 * 6)()
    _lib.check(lib.pesto_enm_modes(model.handle, N, n, side.ptr(x), side.ptr(sd), c, sc, g, pp, dim, k, tl, mi, side.ptr(eig), side.ptr(modes),
                                   side.ptr(res), ctypes.byref(b), ctypes.byref(K), info, side.kind, side.stream), lib.pesto_enm_last_error)
    r = side.result
    return Modes(r(eig), r(modes), r(res), float(b.value), int(info[0]), int(info[1]), int(info[3]), int(K.value) // 2, bool(info[2])), int(info[4])


def anm(xyz, n_modes=20, sel=None, cutoff=15.0, scale=10.0, gamma=1.0, p=0, tol=1e-10, max_iter=32, model=None):
    """Modes: the n_modes <= min(MAX_MODES, 3n - 6) lowest non-rigid modes of the anisotropic network on the n >= 3 selected nodes."""
    return _modes(xyz, n_modes, sel, cutoff, scale, gamma, p, tol, max_iter, model, 3)[0]


def gnm(xyz, n_modes=20, sel=None, cutoff=10.0, scale=10.0, gamma=1.0, p=0, tol=1e-10, max_iter=32, model=None):
    """Modes: the n_modes <= min(MAX_MODES, n - 1) lowest non-constant modes of the Gaussian network on the n >= 2 selected nodes."""
    return _modes(xyz, n_modes, sel, cutoff, scale, gamma, p, tol, max_iter, model, 1)[0]


def _given(eigenvalues, modes, model):
    """(model, side, eigenvalues, modes, k, n, dim) of modes as anm / gnm return them"""
    shp = tuple(modes.shape)
    if len(shp) not in (2, 3) or (len(shp) == 3 and shp[2] != 3) or not 1 <= shp[0] <= MAX_GIVEN or shp[1] < 1:
        raise ValueError(f"modes must be [1 <= k <= {MAX_GIVEN}, n, 3] or [k, n], got {list(shp)}")
    k, n, dim = int(shp[0]), int(shp[1]), 3 if len(shp) == 3 else 1
    if eigenvalues is not None and tuple(np.shape(eigenvalues) if not _lib.is_torch(eigenvalues) else eigenvalues.shape) != (k,):
        raise ValueError(f"eigenvalues must be [k = {k}], one for every mode")
    lead = modes if _lib.is_torch(modes) else np.asarray(modes, np.float64)
    model = _model_of(model, lead)
    side = _lib.Side(lead, model._gpu)
    mo = side.put(lead, np.float64)
    ev = None
    if eigenvalues is not None:
        ev = side.put(eigenvalues, np.float64, (k,), "eigenvalues")
    return model, side, ev, mo, k, n, dim


def mode_fluctuations(eigenvalues, modes, factor=1.0, model=None):
    """float64 [n] = factor sum_k |v_k,i|^2 / lambda_k over lambda_k > 0, ascending k: the predicted B-factor profile up to
    8 pi^2 / 3 kT / gamma."""
    fc = float(factor)
    if not np.isfinite(fc):
        raise ValueError(f"factor must be finite, got {factor!r}")
    model, side, ev, mo, k, n, dim = _given(eigenvalues, modes, model)
    lib = _lib.load()
    out = side.empty((n,), np.float64)
    _lib.check(lib.pesto_enm_fluctuations(model.handle, k, n, dim, side.ptr(ev), side.ptr(mo), fc, side.ptr(out), None, side.kind, side.stream),
               lib.pesto_enm_last_error)
    return side.result(out)


def mode_correlation(eigenvalues, modes, model=None):
    """float32 [n, n]: sum_k (v_k,i . v_k,j) / lambda_k normalised like the DCCM and rounded once; bitwise symmetric, a diagonal of
    exactly 1; a node without fluctuation gets 0, never NaN. n^2 <= MAX_DENSE."""
    model, side, ev, mo, k, n, dim = _given(eigenvalues, modes, model)
    if n * n > MAX_DENSE:
        raise ValueError(f"n**2 must not exceed 2**27 entries, got n = {n}")
    lib = _lib.load()
    out = side.empty((n, n), np.float32)
    _lib.check(lib.pesto_enm_fluctuations(model.handle, k, n, dim, side.ptr(ev), side.ptr(mo), 1.0, None, side.ptr(out), side.kind, side.stream),
               lib.pesto_enm_last_error)
    return side.result(out)


def overlap(modes_a, modes_b, model=None):
    """float64 [ka, kb] = |v_a . v_b| for two sets of modes on the same nodes (anm(...).modes against dynamics.pca(...).components). A
    [n, 3] (or [n]) displacement, open -> closed, may stand for modes_b: it is normalised and the result is [ka, 1]; its cumulative
    overlap is cumulative_overlap(result[:, 0]) = sqrt(cumsum(overlap^2))."""
    model, side, _, A, ka, n, dim = _given(None, modes_a, model)
    shp = tuple(modes_b.shape)
    single = shp == ((n, 3) if dim == 3 else (n,))
    if not single and not (len(shp) == len(tuple(A.shape)) and shp[1:] == tuple(A.shape)[1:] and 1 <= shp[0] <= MAX_GIVEN):
        raise ValueError(f"modes_b must be [1 <= kb <= {MAX_GIVEN}, {', '.join(map(str, tuple(A.shape)[1:]))}] or one displacement, got {list(shp)}")
    lib = _lib.load()
    B = side.put(modes_b, np.float64)
    kb = 1 if single else int(shp[0])
    out = side.empty((ka, kb), np.float64)
    _lib.check(lib.pesto_enm_overlap(model.handle, ka, kb, n * dim, side.ptr(A), side.ptr(B), 1 if single else 0, side.ptr(out), side.kind, side.stream),
               lib.pesto_enm_last_error)
    return side.result(out)


def cumulative_overlap(ov):
    """sqrt(cumsum(ov^2)) along the first axis: how much of a displacement the first 1, 2, ... modes span."""
    if _lib.is_torch(ov):
        return (ov * ov).cumsum(0).sqrt()
    ov = np.asarray(ov, np.float64)
    return np.sqrt(np.cumsum(ov * ov, axis=0))


def deform(xyz, modes, amplitudes, node_of_atom=None, model=None):
    """float32 [F, N, 3] = fl32((double)x_a + sum_k A[f, k] v_k[node_of_atom[a]]), the sum in ascending k, in double, rounded once.
    modes float64 [k, n, 3]; amplitudes [F, k] in xyz's unit; without node_of_atom atoms are nodes (n = N), with it (int [N], values in
    [0, n)) every atom of a residue moves with its CA. The result feeds Model.forward_frames, dynamics.pca and
    clustering.pairwise_rmsd without a host round trip."""
    a = _nodes(xyz)
    N = int(a.shape[0])
    shp = tuple(modes.shape)
    if len(shp) != 3 or shp[2] != 3 or not 1 <= shp[0] <= MAX_GIVEN:
        raise ValueError(f"modes must be [1 <= k <= {MAX_GIVEN}, n, 3], got {list(shp)}")
    k, n = int(shp[0]), int(shp[1])
    amp = amplitudes if _lib.is_torch(amplitudes) else np.asarray(amplitudes, np.float64)
    if len(amp.shape) != 2 or int(amp.shape[1]) != k or not 1 <= int(amp.shape[0]) <= MAX_NODES:
        raise ValueError(f"amplitudes must be [F >= 1, k = {k}], got {list(amp.shape)}")
    F = int(amp.shape[0])
    if F * N * 3 > 2 ** 36:
        raise ValueError("F * N * 3 must not exceed 2**36 values a call: pass the amplitudes in batches")
    nd = None
    if node_of_atom is None:
        if n != N:
            raise ValueError(f"modes have {n} nodes and xyz {N} atoms: pass node_of_atom")
    else:
        nd = _lib.host(node_of_atom).reshape(-1)
        if nd.size != N or not np.issubdtype(nd.dtype, np.integer):
            raise ValueError(f"node_of_atom must hold {N} integers, got {nd.size} of {nd.dtype}")
        if nd.min() < 0 or nd.max() >= n:
            raise ValueError(f"node_of_atom must lie in 0 .. {n - 1}")
    lib = _lib.load()
    model = _model_of(model, a)
    side = _lib.Side(a, model._gpu)
    x, mo, am = side.put(a, np.float32), side.put(modes, np.float64), side.put(amp, np.float64)
    ndd = None if nd is None else side.put(nd, np.int32)
    out = side.empty((F, N, 3), np.float32)
    _lib.check(lib.pesto_enm_deform(model.handle, F, N, n, k, side.ptr(x), side.ptr(mo), side.ptr(am), side.ptr(ndd), side.ptr(out), side.kind,
                                    side.stream), lib.pesto_enm_last_error)
    return side.result(out)


def sample_amplitudes(eigenvalues, n_frames, rmsd=1.0, seed=0, *, n_nodes):
    """float64 [n_frames, k] (NumPy, host only): Gaussian draws of numpy.random.default_rng(seed) with standard deviation 1 / sqrt(lambda_k),
    amplitude 0 for a zero eigenvalue, scaled so that the root-mean-square displacement of a node over all frames,
    sqrt(mean_f sum_k A[f, k]^2 / n_nodes) for modes with orthonormal rows, is ``rmsd``. n_nodes has no default: the eigenvalues do not tell it, and a
    forgotten one would make the frames sqrt(n) too small (n_nodes = 1 gives the RMS length of the whole displacement vector)."""
    ev = np.asarray(_lib.host(eigenvalues), np.float64).reshape(-1)
    F, n = int(n_frames), int(n_nodes)
    if F < 1 or n < 1 or not np.isfinite(float(rmsd)) or float(rmsd) < 0:
        raise ValueError("n_frames and n_nodes must be at least 1 and rmsd finite and >= 0")
    sd = np.zeros_like(ev)
    sd[ev > 0] = 1.0 / np.sqrt(ev[ev > 0])
    A = np.random.default_rng(seed).standard_normal((F, ev.size)) * sd
    ms = float(np.mean(np.sum(A * A, axis=1))) / n
    return A * (float(rmsd) / np.sqrt(ms)) if ms > 0 else A


def mode_path(n_modes, mode, n_steps, rmsd=1.0, *, n_nodes):
    """float64 [n_steps, n_modes] (NumPy, host only): amplitudes along one mode in n_steps equal steps between the two conformers whose
    root-mean-square node displacement is ``rmsd``: from -rmsd sqrt(n_nodes) to +rmsd sqrt(n_nodes)."""
    k, i, S, n = int(n_modes), int(mode), int(n_steps), int(n_nodes)
    if not (1 <= k and 0 <= i < k and S >= 1 and n >= 1):
        raise ValueError("need n_modes >= 1, 0 <= mode < n_modes, n_steps >= 1 and n_nodes >= 1")
    top = float(rmsd) * np.sqrt(n)
    A = np.zeros((S, k))
    A[:, i] = np.linspace(-top, top, S) if S > 1 else top
    return A


def structure_modes(structure, kind="anm", **kw):
    """(Modes, xyz float32 [N, 3], node_of_atom int32 [N]): the network on the CA atoms of the protein residues of a structure (a PDB
    path, a structure_io.Structure or a structure dict, whatever structalign.ca_traces takes), in angstroms (scale 1), with all the
    structure's atoms and the node each moves with in deform: its own residue's CA; an atom outside the protein residues moves with the
    protein residue before it in the file."""
    if kind not in ("anm", "gnm"):
        raise ValueError(f"kind must be 'anm' or 'gnm', got {kind!r}")
    if "scale" in kw or "sel" in kw:
        raise ValueError("structure_modes selects the CA atoms itself, in angstroms: scale and sel are not taken")
    from .lddt import _structure_dict
    from .structalign import ca_traces
    d = _structure_dict(structure)
    xyz = np.ascontiguousarray(np.asarray(d["xyz"], np.float32).reshape(-1, 3))
    traces = ca_traces(d)
    if not traces:
        raise ValueError("the structure has no protein chain")
    ca = np.concatenate([t[1] for t in traces])
    first = np.concatenate([np.asarray(t[3], np.int64) for t in traces])
    order = np.argsort(first, kind="stable")
    node = order[np.clip(np.searchsorted(first[order], np.arange(xyz.shape[0]), "right") - 1, 0, None)].astype(np.int32)
    out = (anm if kind == "anm" else gnm)(ca, scale=1.0, **kw)
    return out, xyz, node
