"""Density-peak clustering of MD frames by the centre of their predicted interface, on the GPU: steps 3 to 5 of the clustering in the
reference's notebooks.

The notebooks (md_analysis/apply_model_with_clustering.ipynb, cell lines 263-343, and clustering_analysis.ipynb) run the model on every
n-th frame (P [F, R]), superpose the residue centroids of those frames (Xp [F, R, 3]), take the centre of the predicted interface of
every frame (T = P > p_thr, Xc = sum_r Xp T / sum_r T, frames without a residue above the threshold dropped), cluster the points Xc and
keep the cluster centres as frame indices. Their clusterer is CLoNe, a third-party package that the reference does not contain and whose
source is not available: CLoNe is NOT reproduced here and no equality with its results is claimed. What stands in its place is the
published algorithm it derives from, density peaks (Rodriguez and Laio, Science 344, 2014), in full (pesto_peaks.hip):
    interface_centers / weighted_centers    centre, weight sum and radius of the predicted interface of every frame
    distance_quantile                       d_c: the pair distance at the percentile pdc, exactly
    density_peaks                           rho, delta, the nearest denser point, centres, labels and halo, over points or over a matrix
    cluster_interface_frames                the notebook's step in one call, the centres staying on the device
Model.forward_frames, trajectory.residue_centroids and trajectory.superpose give P and Xp; ranking.scores the per-frame AUC. Over a
precomputed matrix density_peaks is a second clusterer for clustering.pairwise_rmsd. Calling conventions are those of
pesto_amd.clustering: the first array decides where a call runs (_lib.Side: ROCm tensors in, ROCm tensors out on torch's current stream;
NumPy in, NumPy out); ``model`` lends its device handle, without one a weightless handle is used; arguments are checked before any launch
(ValueError); there is no CPU fallback.

Definition. Centres of a frame f: w_r = 1 if P[f, r] > float32(p_thr) else 0 (a NaN compares false), or the given weights;
S = sum w_r, c = sum w_r x_r / S, rg = sqrt(sum w_r |x_r - c|^2 / S), all sums in double in a fixed order with terms of weight 0 skipped,
each output rounded to float32 once; S = 0 gives c = rg = NaN.
Distances: points X float32 [F, d], 1 <= d <= 8: s = dx0*dx0; s = s + dx1*dx1; ...; dist = sqrt(s), every operation rounded to float32
(NumPy gives the same bits); or a float32 [F, F] matrix, bitwise symmetric, finite and >= 0 off the diagonal, the diagonal ignored.
d_c: with M = n (n - 1) / 2 pairs i < j, the k-th smallest distance (0-based), k = min(M - 1, max(0, ceil(M pdc / 100) - 1)).
"Denser" is the total order key(j) > key(i): rho_j > rho_i, or rho_j == rho_i and j < i.
    rho     cutoff: the number of j != i with d_ij < d_c (strictly); gaussian: sum_{j != i} exp(-(d_ij / d_c)^2) in double
    nh, delta   the denser j with the smallest d_ij (the lowest j among equal distances) and that distance; the densest point has
            nh = -1 and delta = max_j d_ij (0 for n = 1)
    centres the densest point always; n_clusters = K: plus the K - 1 others with the largest gamma = rho * delta (one double multiply;
            the lower index first among equal ones); delta_min: plus every point with rho >= rho_min and delta >= delta_min;
            delta_factor: delta_min = float32(delta_factor * dc), a centre then being a point without a denser one within that radius.
            Listed from the densest to the least dense by key
    labels  labels[centers[c]] = c, labels[i] = labels[nh[i]]; sizes[c] the members of c
    halo    rho_i < rho_b[labels[i]], rho_b[c] = max (rho_i + rho_j) / 2 over the pairs i in c, j not in c with d_ij < d_c (else 0)
Everything but the Gaussian rho is exact (integers, comparisons, minima and maxima of float32 values); the Gaussian rho is summed in a
fixed order. Every output is bit-identical from call to call. DESIGN.md section 4.20 has the kernels, limits and measurements.
"""
import ctypes
import math
from typing import Any, NamedTuple

import numpy as np

from . import _lib
from .clustering import MAX_FRAMES
from .trajectory import _model_of, _selection

MAX_POINTS = 1 << 17        # PESTO_PEAKS_MAX_POINTS: n over points
MAX_CLUSTERS = 1024         # PESTO_PEAKS_MAX_CLUSTERS: n_clusters
MAX_DIM = 8                 # PESTO_PEAKS_MAX_DIM
MAX_CENTER_FRAMES = 1 << 23  # PESTO_PEAKS_MAX_FRAMES: F of interface_centers
THRESHOLD, WEIGHTS = 0, 1
KERNELS = {"cutoff": 0, "gaussian": 1}
F32_MAX = float(np.finfo(np.float32).max)


class Peaks(NamedTuple):
    """density_peaks' result over the n selected rows"""
    dc: float
    rho: Any                # float64 [n]
    delta: Any              # float32 [n]
    nearest_higher: Any     # int32 [n], -1 for the densest point
    labels: Any             # int32 [n]
    halo: Any               # bool [n]
    centers: Any            # int32 [C], from the densest to the least dense
    sizes: Any              # int32 [C]


class InterfaceClusters(NamedTuple):
    """cluster_interface_frames' result over all F frames: Peaks' fields with frame indices (labels -1, halo False, rho and delta NaN,
    nearest_higher -1 for a frame without a predicted interface), and interface_centers' three outputs"""
    dc: float
    rho: Any
    delta: Any
    nearest_higher: Any
    labels: Any
    halo: Any
    centers: Any
    sizes: Any
    Xc: Any                 # float32 [F, 3]
    wsum: Any               # float64 [F]
    rg: Any                 # float32 [F]


def _array(a, name, ndim):
    if not (_lib.is_torch(a) or isinstance(a, np.ndarray)):
        a = np.asarray(a, np.float32)
    if len(tuple(a.shape)) != ndim:
        raise ValueError(f"{name} must have {ndim} axes, got {list(a.shape)}")
    return a


def _check_centers(Xp, PW, name):
    x = _array(Xp, "Xp", 3)
    w = _array(PW, name, 2)
    F, R = int(x.shape[0]), int(x.shape[1])
    if x.shape[2] != 3 or F < 1 or R < 1:
        raise ValueError(f"Xp must be [F >= 1, R >= 1, 3], got {list(x.shape)}")
    if tuple(w.shape) != (F, R):
        raise ValueError(f"{name} must be [{F}, {R}], got {list(w.shape)}")
    if F > MAX_CENTER_FRAMES:
        raise ValueError(f"at most {MAX_CENTER_FRAMES} frames, got {F}")
    return x, w, F, R


def _centers(side, model, x, w, F, R, mode, p_thr):
    xd, wd = side.put(x, np.float32), side.put(w, np.float32)
    centers, wsum, rg = side.empty((F, 3), np.float32), side.empty((F,), np.float64), side.empty((F,), np.float32)
    lib = _lib.load()
    try:
        _lib.check(lib.pesto_weighted_centers(model.handle, F, R, side.ptr(xd), side.ptr(wd), mode, p_thr, side.ptr(centers), side.ptr(wsum),
                                              side.ptr(rg), side.kind, side.stream), lib.pesto_peaks_last_error)
    except _lib.PestoError as err:
        if err.code == -1:          # PESTO_ERR_INVALID: the weights are checked on the device
            raise ValueError(str(err)) from None
        raise
    return centers, wsum, rg


def _check_p_thr(p_thr):
    t = float(np.float32(float(p_thr)))
    if math.isnan(t):
        raise ValueError("p_thr must not be NaN")
    return t


def interface_centers(Xp, P, p_thr=0.5, model=None):
    """(centers float32 [F, 3], wsum float64 [F], rg float32 [F]): per frame the mean position of the residues with P > p_thr (p_thr
    rounded to float32; a NaN in P compares false), their number, and their RMS distance from that centre - the notebook's Xc and, at
    p_thr = 0.3, its interface radius r_int, for every frame at once. A frame with no residue above the threshold gets NaN, 0, NaN.
    Xp float32 [F, R, 3], P float32 [F, R]."""
    x, w, F, R = _check_centers(Xp, P, "P")
    t = _check_p_thr(p_thr)
    model = _model_of(model, x)
    side = _lib.Side(x, model._gpu)
    return tuple(side.result(v) for v in _centers(side, model, x, w, F, R, THRESHOLD, t))


def weighted_centers(Xp, W, model=None):
    """interface_centers with the weights W float32 [F, R] >= 0 given directly (the notebook's commented-out soft weighting W = P):
    centre, weight sum and weighted RMS radius per frame. A negative or non-finite weight raises ValueError and nothing is written."""
    x, w, F, R = _check_centers(Xp, W, "W")
    model = _model_of(model, x)
    side = _lib.Side(x, model._gpu)
    return tuple(side.result(v) for v in _centers(side, model, x, w, F, R, WEIGHTS, 0.0))


def quantile_rank(n, pdc):
    """k of d_c: the 0-based rank, among the n (n - 1) / 2 pair distances, of the percentile pdc"""
    M = n * (n - 1) // 2
    return min(M - 1, max(0, math.ceil(M * pdc / 100.0) - 1))


def _check_source(X, D, idx):
    """(the array, is it a matrix, F, d, idx as int32 or None, n)"""
    if (X is None) == (D is None):
        raise ValueError("exactly one of X and D must be given")
    if X is not None:
        a = _array(X, "X", 2)
        F, d = int(a.shape[0]), int(a.shape[1])
        if F < 1 or not 1 <= d <= MAX_DIM:
            raise ValueError(f"X must be [F >= 1, 1 <= d <= {MAX_DIM}], got {list(a.shape)}")
        if F > (2 ** 31 - 1) // MAX_DIM:
            raise ValueError(f"at most {(2 ** 31 - 1) // MAX_DIM} points in X, got {F}")
    else:
        a = _array(D, "D", 2)
        F, d = int(a.shape[0]), 0
        if a.shape[0] != a.shape[1] or F < 1:
            raise ValueError(f"D must be a square [F >= 1, F] matrix, got {list(a.shape)}")
        if F > MAX_FRAMES:
            raise ValueError(f"at most {MAX_FRAMES} rows in D, got {F}")
    if idx is None:
        s, n = None, F
    else:
        try:
            s, n = _selection(idx, F, "sel", least=1)
        except ValueError as err:
            raise ValueError(str(err).replace("sel", "idx").replace("atoms", "rows").replace("atom", "row")) from None
    if X is not None and n > MAX_POINTS:
        raise ValueError(f"at most {MAX_POINTS} selected points, got {n}")
    return a, X is None, F, d, s, n


def _check_pdc(pdc):
    p = float(pdc)
    if not 0.0 < p <= 100.0:
        raise ValueError(f"pdc must lie in (0, 100], got {pdc!r}")
    return p


def _invalid(err):
    if err.code == -1:              # PESTO_ERR_INVALID: the checks made on the device (symmetry, finiteness, sign)
        raise ValueError(str(err)) from None
    raise err


def _rank(side, model, a, matrix, F, d, s, n, k):
    ad = side.put(a, np.float32)
    sd = None if s is None else side.put(s, np.int32)
    out = ctypes.c_float(0.0)
    lib = _lib.load()
    try:
        _lib.check(lib.pesto_pair_distance_rank(model.handle, F, d, None if matrix else side.ptr(ad), side.ptr(ad) if matrix else None, n, side.ptr(sd),
                                                k, ctypes.byref(out), side.kind, side.stream), lib.pesto_peaks_last_error)
    except _lib.PestoError as err:
        _invalid(err)
    return float(out.value), ad, sd


def distance_quantile(X=None, D=None, pdc=2.0, idx=None, model=None):
    """float: d_c, the pair distance at the percentile ``pdc`` (0 < pdc <= 100) - the k-th smallest, k = quantile_rank(n, pdc), of the
    n (n - 1) / 2 distances between the n >= 2 selected rows (idx: an index array or a mask; None: all) of the points X float32 [F, d <= 8]
    or of the distance matrix D float32 [F, F]. Exact: the float32 value a full sort would give."""
    a, matrix, F, d, s, n = _check_source(X, D, idx)
    p = _check_pdc(pdc)
    if n < 2:
        raise ValueError(f"at least 2 selected rows, got {n}")
    model = _model_of(model, a)
    side = _lib.Side(a, model._gpu)
    return _rank(side, model, a, matrix, F, d, s, n, quantile_rank(n, p))[0]


def _check_rule(n, n_clusters, rho_min, delta_min, delta_factor):
    """(n_clusters or 0, rho_min, delta_min or None while it hangs on a d_c still to be computed)"""
    if sum(v is not None for v in (n_clusters, delta_min, delta_factor)) != 1:
        raise ValueError("exactly one of n_clusters, delta_min and delta_factor must be given")
    r = float(rho_min)
    if math.isnan(r):
        raise ValueError("rho_min must not be NaN")
    if n_clusters is not None:
        K = int(n_clusters)
        if K != n_clusters or not 1 <= K <= min(n, MAX_CLUSTERS):
            raise ValueError(f"n_clusters must lie in 1 .. min(n = {n}, {MAX_CLUSTERS}), got {n_clusters!r}")
        return K, r, 0.0
    if delta_min is not None:
        with np.errstate(over="ignore"):
            t = float(np.float32(float(delta_min)))
        if math.isnan(t):
            raise ValueError("delta_min must not be NaN")
        return 0, r, t
    f = float(delta_factor)
    if not (math.isfinite(f) and f >= 0.0):
        raise ValueError(f"delta_factor must be finite and >= 0, got {delta_factor!r}")
    return 0, r, None


def _check_dc(dc):
    with np.errstate(over="ignore"):
        v = float(np.float32(float(dc)))
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"dc must be a finite float32 value > 0, got {dc!r}")
    return v


def _peaks(side, model, a, matrix, F, d, s, n, dc, pdc, kernel, K, r_min, d_min, delta_factor):
    if dc is None:
        dc, ad, sd = _rank(side, model, a, matrix, F, d, s, n, quantile_rank(n, pdc))
        if not dc > 0.0:
            raise ValueError(f"the pair distance at pdc = {pdc} is 0 (duplicated rows): give dc or a larger pdc")
        if not math.isfinite(dc):
            raise ValueError(f"the pair distance at pdc = {pdc} is not finite")
    else:
        ad = side.put(a, np.float32)
        sd = None if s is None else side.put(s, np.int32)
    if d_min is None:
        with np.errstate(over="ignore"):
            d_min = float(np.float32(float(delta_factor) * dc))
    rho, delta = side.empty((n,), np.float64), side.empty((n,), np.float32)
    nh, labels, centers, sizes = (side.empty((n,), np.int32) for _ in range(4))
    halo = side.empty((n,), np.bool_)
    nc = ctypes.c_int32(0)
    lib = _lib.load()
    try:
        _lib.check(lib.pesto_density_peaks(model.handle, F, d, None if matrix else side.ptr(ad), side.ptr(ad) if matrix else None, n, side.ptr(sd), dc, kernel,
                                           K, r_min, d_min, side.ptr(rho), side.ptr(delta), side.ptr(nh), side.ptr(labels), side.ptr(halo),
                                           side.ptr(centers), side.ptr(sizes), ctypes.byref(nc), side.kind, side.stream), lib.pesto_peaks_last_error)
    except _lib.PestoError as err:
        _invalid(err)
    return Peaks(dc, rho, delta, nh, labels, halo, centers[:nc.value], sizes[:nc.value])


def _check_peaks(X, D, dc, pdc, kernel, n_clusters, rho_min, delta_min, delta_factor, idx):
    a, matrix, F, d, s, n = _check_source(X, D, idx)
    if kernel not in KERNELS:
        raise ValueError(f"kernel must be one of {sorted(KERNELS)}, got {kernel!r}")
    if dc is None:
        p = _check_pdc(pdc)
        if n < 2:
            raise ValueError(f"d_c from pdc needs at least 2 selected rows, got {n}: give dc")
    else:
        p, dc = None, _check_dc(dc)
    K, r_min, d_min = _check_rule(n, n_clusters, rho_min, delta_min, delta_factor)
    return (a, matrix, F, d, s, n, dc, p, KERNELS[kernel], K, r_min, d_min, delta_factor)


def density_peaks(X=None, D=None, dc=None, pdc=2.0, kernel="gaussian", n_clusters=None, rho_min=0.0, delta_min=None, delta_factor=None, idx=None,
                  model=None):
    """Peaks(dc, rho, delta, nearest_higher, labels, halo, centers, sizes): the density-peak clustering (see the module's definition) of the
    n selected rows (idx: an index array or a mask; None: all) of the points X float32 [F, d <= 8] or of the distance matrix D float32
    [F, F]. dc: the kernel's width, finite and > 0; None: distance_quantile at ``pdc`` (a d_c of 0 raises ValueError). kernel: "gaussian" or
    "cutoff". Exactly one centre rule: n_clusters (1 .. min(n, 1024)), delta_min (with rho_min), or delta_factor (delta_min =
    float32(delta_factor * dc), with rho_min). All indices in the result count the selected rows. An asymmetric matrix, a negative or
    non-finite entry or coordinate raise ValueError from the device's check, nothing written."""
    args = _check_peaks(X, D, dc, pdc, kernel, n_clusters, rho_min, delta_min, delta_factor, idx)
    model = _model_of(model, args[0])
    side = _lib.Side(args[0], model._gpu)
    out = _peaks(side, model, *args)
    return Peaks(out.dc, *(side.result(v) for v in out[1:]))


def cluster_interface_frames(Xp, P, p_thr=0.5, model=None, **density_peaks_kwargs):
    """InterfaceClusters: the notebook's step in one call. interface_centers(Xp, P, p_thr); the frames with a predicted interface
    (wsum > 0); density_peaks on their centres (density_peaks_kwargs: dc, pdc, kernel, n_clusters, rho_min, delta_min, delta_factor);
    the result mapped back to all F frames: labels -1, halo False, rho and delta NaN, nearest_higher -1 for a frame without a predicted
    interface, centers and nearest_higher as frame indices. With ROCm tensors the centres stay on the device between the two calls (host
    arrays are copied to the device once, the results back once); only wsum is read to choose the frames."""
    for key in density_peaks_kwargs:
        if key not in ("dc", "pdc", "kernel", "n_clusters", "rho_min", "delta_min", "delta_factor"):
            raise ValueError(f"unknown argument {key!r}")
    x, w, F, R = _check_centers(Xp, P, "P")
    t = _check_p_thr(p_thr)
    model = _model_of(model, x)
    import torch
    on_device = _lib.is_torch(x) and x.is_cuda
    lead = x if on_device else torch.from_numpy(np.ascontiguousarray(_lib.host(x), np.float32)).to(f"cuda:{model._gpu}")
    side = _lib.Side(lead, model._gpu)
    Xc, wsum, rg = _centers(side, model, lead, w, F, R, THRESHOLD, t)
    keep = torch.nonzero(wsum > 0).reshape(-1)
    n = int(keep.numel())
    if n < 1:
        raise ValueError(f"no frame has a residue above p_thr = {p_thr!r}")
    args = _check_peaks(Xc, None, density_peaks_kwargs.pop("dc", None), density_peaks_kwargs.pop("pdc", 2.0), density_peaks_kwargs.pop("kernel", "gaussian"),
                        density_peaks_kwargs.pop("n_clusters", None), density_peaks_kwargs.pop("rho_min", 0.0), density_peaks_kwargs.pop("delta_min", None),
                        density_peaks_kwargs.pop("delta_factor", None), keep.cpu().numpy() if n < F else None)
    pk = _peaks(side, model, *args)
    if n < F:
        kl = keep.long()
        rho = torch.full((F,), float("nan"), dtype=torch.float64, device=lead.device)
        delta = torch.full((F,), float("nan"), dtype=torch.float32, device=lead.device)
        nh, labels = (torch.full((F,), -1, dtype=torch.int32, device=lead.device) for _ in range(2))
        halo = torch.zeros((F,), dtype=torch.bool, device=lead.device)
        rho[kl], delta[kl], labels[kl], halo[kl] = pk.rho, pk.delta, pk.labels, pk.halo
        k32 = keep.to(torch.int32)
        nh[kl] = torch.where(pk.nearest_higher >= 0, k32[pk.nearest_higher.clamp(min=0).long()], pk.nearest_higher)
        pk = Peaks(pk.dc, rho, delta, nh, labels, halo, k32[pk.centers.long()], pk.sizes)
    out = tuple(pk[1:]) + (Xc, wsum, rg)
    if not on_device:
        out = tuple(v.cpu() for v in out)
        if not _lib.is_torch(x):
            out = tuple(v.numpy() for v in out)
    return InterfaceClusters(pk.dc, *out)
