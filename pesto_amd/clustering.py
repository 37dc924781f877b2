"""Pairwise RMSD and frame clustering on the GPU: the clustering step that ends the reference's MD workflow.

The reference's notebooks (md_analysis/apply_model_with_clustering.ipynb, clustering_analysis.ipynb) run the model over the frames,
superpose them, cluster them and keep the cluster centres. Their clusterer is a third-party package that the reference does not contain;
what stands here instead is the standard pair of tools, the minimal RMSD of every frame against every other frame and the GROMOS
clustering (Daura et al. 1999, ``gmx cluster -method gromos``) over such a matrix (pesto_cluster.hip):
    pairwise_rmsd      float32 [Fa, Fb]: trajectory_utils.superpose_transform + the rmsd expression for every pair of frames at once
    gromos_clusters    labels, centres and sizes from a symmetric distance matrix and a cutoff
    cluster_frames     the two in a row, the matrix staying on the device
Calling conventions are those of pesto_amd.trajectory: float32 [F, N, 3] arrays or objects with ``.xyz``; the first array decides where
a call runs (_lib.Side: ROCm tensors in, ROCm tensors out on torch's current stream; NumPy in, NumPy out); ``model`` lends its device
handle, without one a weightless handle is used; arguments are checked before any launch (ValueError); there is no CPU fallback.

Definition, for a_i = xyz_a[i, sel], b_j = xyz_b[j, sel] (n atoms each, t their means):
    D[i, j]  = scale * sqrt(mean_n |R_ij (b_j - t_b) - (a_i - t_a)|^2),  R_ij the optimal PROPER rotation (never a reflection)
             = scale * sqrt(max((G_a + G_b - 2 (s0 + s1 + sign(det H) s2)) / n, 0))
    G        = sum |x - t|^2 of a frame, H = (a_i - t_a)^T (b_j - t_b), s0 >= s1 >= s2 its singular values
evaluated in double from the float32 coordinates and rounded to float32 once. H of all pairs is one matrix product
[4 Fa x n] . [n x 4 Fb] of rows (x, y, z, 1) on v_mfma_f64_16x16x4_f64: the products of float32 values are exact in double, only the
accumulation rounds; the ones row brings the coordinate sums and n, and H is centred as H - s_a s_b^T / n. The singular values come
from a one-sided Jacobi. An exactly duplicated frame therefore gives about 1e-7 of its radius of gyration rather than 0 (except on the
diagonal of the self form, which is 0 by construction).
    adj[i, j] = D[i, j] <= float32(cutoff) or i == j              a NaN compares false
    repeat while a frame is active: cnt[i] = active j with adj[i, j]; the centre is the active i with the largest cnt (lowest index on
    ties); the active j with adj[centre, j] get label c = 0, 1, ... and become inactive; centers[c] = centre, sizes[c] = their number
The clustering is all integers once the adjacency is fixed and equals its definition exactly.

The reference's own float32 route (superpose_transform + rmsd, pair by pair) deviates from a float64 restatement by
(tests/golden/make_clustering_golden.py, e_ref; the tests allow max(4 e_ref, 4 eps32 max(max|value|, scale * rg))):
    md29_all 1.6e-06   md29_sel 1.8e-06   md29_rect 1.2e-06   mirror 1.8e-06   near 2.1e-05   tiny 1.4e-07
Every output is bit-identical from call to call.

Measured on an MI355X (profiles/bench_clustering.py -> profiles/clustering.json; whole calls on ROCm tensors, device events, medians):
pairwise_rmsd, self form, at (F, n) = (512, 290) / (512, 2030) / (4096, 290): 0.243 / 0.553 / 2.75 ms, against 44.9 / 47.0 / 586 ms for F
calls of trajectory.rmsd; the covariance kernel alone (kernel trace) 81 / 462 / 2590 us = 15.7 / 19.0 / 30.4 TFLOP/s of the arithmetic it
executes, its per-pair finish 18 / 17 / 505 us of that. gromos_clusters at F = 4096: 0.526 ms at the median cutoff (9 clusters),
0.486 ms with every frame its own cluster. DESIGN.md section 4.19 has the split and what was not tried.
"""
import ctypes

import numpy as np

from . import _lib
from .trajectory import _model_of, _selection, _xyz

MAX_PAIRS = 2 ** 28         # PESTO_CLUSTER_MAX_PAIRS: Fa * Fb of pairwise_rmsd
MAX_FRAMES = 16384          # PESTO_CLUSTER_MAX_FRAMES: F of gromos_clusters
F32_MAX = float(np.finfo(np.float32).max)


def _check_rmsd(xyz_a, xyz_b, sel, scale):
    a = _xyz(xyz_a, "xyz_a")
    b = None if xyz_b is None else _xyz(xyz_b, "xyz_b")
    Fa, N = int(a.shape[0]), int(a.shape[1])
    Fb = Fa if b is None else int(b.shape[0])
    if b is not None and int(b.shape[1]) != N:
        raise ValueError(f"xyz_a has {N} atoms and xyz_b {int(b.shape[1])}")
    if Fa * Fb > MAX_PAIRS:
        raise ValueError(f"at most 2**28 frame pairs, got {Fa} * {Fb}")
    s, n = _selection(sel, N, "sel", least=1)
    sc = float(scale)
    if not (np.isfinite(sc) and abs(sc) <= F32_MAX):
        raise ValueError(f"scale must be finite, got {scale!r}")
    return a, b, Fa, Fb, N, s, n, sc


def _check_matrix(D):
    if not (_lib.is_torch(D) or isinstance(D, np.ndarray)):
        D = np.asarray(D, np.float32)
    shp = tuple(D.shape)
    if len(shp) != 2 or shp[0] != shp[1] or shp[0] < 1:
        raise ValueError(f"D must be a square [F >= 1, F] matrix, got {list(shp)}")
    if shp[0] > MAX_FRAMES:
        raise ValueError(f"at most {MAX_FRAMES} frames, got {shp[0]}")
    return D, int(shp[0])


def _check_cutoff(cutoff):
    with np.errstate(over="ignore"):
        c = float(np.float32(float(cutoff)))
    if not np.isfinite(c):
        raise ValueError(f"cutoff must be a finite float32 value, got {cutoff!r}")
    return c


def _rmsd(side, model, a, b, Fa, Fb, N, s, n, sc):
    xa = side.put(a, np.float32)
    xb = None if b is None else side.put(b, np.float32)
    sd = None if s is None else side.put(s, np.int32)
    D = side.empty((Fa, Fb), np.float32)
    lib = _lib.load()
    _lib.check(lib.pesto_pairwise_rmsd(model.handle, Fa, Fb, N, n, side.ptr(xa), side.ptr(xb), side.ptr(sd), sc, side.ptr(D), side.kind, side.stream),
               lib.pesto_cluster_last_error)
    return D


def _gromos(side, model, D, F, c):
    d = side.put(D, np.float32)
    labels, centers, sizes = (side.empty((F,), np.int32) for _ in range(3))
    nc = ctypes.c_int32(0)
    lib = _lib.load()
    try:
        _lib.check(lib.pesto_gromos_clusters(model.handle, F, side.ptr(d), c, side.ptr(labels), side.ptr(centers), side.ptr(sizes), ctypes.byref(nc),
                                             side.kind, side.stream), lib.pesto_cluster_last_error)
    except _lib.PestoError as err:
        if err.code == -1:          # PESTO_ERR_INVALID: the one argument check made on the device, the symmetry of D
            raise ValueError(str(err)) from None
        raise
    return labels, centers[:nc.value], sizes[:nc.value]


def pairwise_rmsd(xyz_a, xyz_b=None, sel=None, scale=10.0, model=None):
    """float32 [Fa, Fb]: the minimal RMSD of every frame of xyz_a [Fa, N, 3] against every frame of xyz_b [Fb, N, 3], fitted and measured
    on the atoms ``sel`` (an index array or a mask; None: all atoms), times scale (10: nanometres in, angstroms out). xyz_b=None: xyz_a
    against itself; only the pairs i <= j are evaluated and mirrored, so D is bitwise symmetric with a diagonal of exactly 0 and has, off
    the diagonal, the bits of pairwise_rmsd(xyz_a, a copy of xyz_a). Fa * Fb <= MAX_PAIRS; finite coordinates are the caller's contract."""
    a, b, Fa, Fb, N, s, n, sc = _check_rmsd(xyz_a, xyz_b, sel, scale)
    model = _model_of(model, a)
    side = _lib.Side(a, model._gpu)
    return side.result(_rmsd(side, model, a, b, Fa, Fb, N, s, n, sc))


def gromos_clusters(D, cutoff, model=None):
    """(labels int32 [F], centers int32 [C], sizes int32 [C]): the GROMOS clusters of the bitwise symmetric float32 [F, F] matrix D
    (F <= MAX_FRAMES; ValueError if it is not symmetric, the call's one check on the device) at ``cutoff`` (rounded to float32; D <= cutoff
    is a neighbour). labels[f] is the cluster of frame f, numbered in order of extraction; centers[c] its centre frame and sizes[c] its
    number of members, never increasing."""
    D, F = _check_matrix(D)
    c = _check_cutoff(cutoff)
    model = _model_of(model, D)
    side = _lib.Side(D, model._gpu)
    return tuple(side.result(v) for v in _gromos(side, model, D, F, c))


def cluster_frames(xyz, cutoff, sel=None, scale=10.0, model=None):
    """(labels, centers, sizes, D): pairwise_rmsd(xyz, sel=sel, scale=scale) followed by gromos_clusters(D, cutoff), the matrix staying on
    the device between the two (host arrays are copied to the device once, the four results back once)."""
    a, _, F, _, N, s, n, sc = _check_rmsd(xyz, None, sel, scale)
    if F > MAX_FRAMES:
        raise ValueError(f"at most {MAX_FRAMES} frames, got {F}")
    c = _check_cutoff(cutoff)
    model = _model_of(model, a)
    lead = a
    if not (_lib.is_torch(a) and a.is_cuda):
        import torch
        lead = torch.from_numpy(np.ascontiguousarray(_lib.host(a), np.float32)).to(f"cuda:{model._gpu}")
    side = _lib.Side(lead, model._gpu)
    D = _rmsd(side, model, lead, None, F, F, N, s, n, sc)
    out = _gromos(side, model, D, F, c) + (D,)
    if lead is a:
        return out
    out = tuple(v.cpu() for v in out)
    return out if _lib.is_torch(a) else tuple(v.numpy() for v in out)
