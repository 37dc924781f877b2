"""MD ensemble analysis on the GPU: what the reference's MD notebooks do with the frames of a trajectory once the model has run over them.

The reference (md_analysis/mdtraj_utils/statistical_contacts_model.py, trajectory_utils.py, the tail of apply_model_md.ipynb) runs a
Python loop over the frames that materialises a [Na, Nb, bins] tensor per frame, a Python double loop over residue pairs for fnat and a
batched NumPy SVD for the superposition. Here every function is one launch sequence over all frames (pesto_contact_counts and the other
entry points of pesto_trajectory.hip):
    contact_counts / contacts_distribution        binned pair-distance counts over the frames and their distribution P
    StatisticalContactsModel, div_KL, interface_ensemble_comparison     the reference's model: fit, per-frame log-likelihood, divergence
    residue_contact_maps / native_contacts / fnat residue-residue contact maps per frame and the fraction of native contacts
    superpose_transform / superpose / rmsd        optimal rigid superposition of every frame onto a reference
    residue_centroids                             the mean position of every residue's atoms per frame (X M / count)
Trajectories are float32 [F, N, 3] arrays (mdtraj's layout) or any object with an ``.xyz`` attribute of that shape; everything is
unit-agnostic except where a ``scale`` is named (mdtraj keeps nanometres, the reference multiplies by 10 for angstroms). The first
trajectory decides where a call runs (_lib.Side): ROCm tensors stay on the device (device pointers, torch's current stream, ROCm tensors
out); NumPy arrays and CPU tensors are staged and NumPy arrays come back. ``model`` lends its device handle; without one a weightless
handle is used. Arguments are checked before any launch (ValueError). There is no CPU or PyTorch fallback.

Definition, for xyz0 [F, Na, 3], xyz1 [F, Nb, 3] and bins (B + 1 strictly increasing finite float64 edges, 1 <= B <= MAX_BINS = 128):
    d[f,i,j]     = sqrt((dx*dx + dy*dy) + dz*dz)            float32, every operation rounded as written, correctly rounded sqrt
    hit(f,i,j)   = the b with bins[b] <= d < bins[b+1]      compared in float64; none if outside or NaN
    count[i,j,b] = number of frames with hit = b
    P[i,j,b]     = float32(count) / (float32(sum_b count) + 1e-6f)
    L[f]         = -mean over (i,j,b) of log(1 - PQ + floor(PQ)),  PQ = P[i,j,b] if hit(f,i,j) = b else 0
    KL(P,Q)[i,j] = -sum_b P log(R),  R = Q / (P + 1e-6f), R = 1 where R < 1e-6f
Counts, P, contact maps, native contacts and fnat equal the reference exactly. L, KL, the superposition, rmsd and the centroids are
evaluated in double from the float32 inputs and rounded once, so they lie within half a float32 unit of a float64 restatement; the
reference's own float32 results deviate from that restatement by (tests/golden/make_trajectory_golden.py, e_ref; the tests allow
max(4 e_ref, 4 eps32 max|value|)):
    iface   L0 4.5e-10   L 4.5e-10   L / mean(L0) 3.7e-07   KL 2.1e-07
    superposition of 29 MD frames of 2,030 atoms (all atoms | a 290-atom selection | one mirrored frame):
            t 4.1e-06 | 1.8e-06 | 1.6e-06    R 2.5e-07 | 1.6e-07 | 3.4e-07    t_ref 1.3e-06 | 1.8e-06 | 1.3e-06
            superposed xyz 8.5e-06 | 5.6e-06 | 1.5e-05    rmsd 1.0e-05 | 7.2e-06 | 8.1e-06
    residue centroids (float32 X M / count) 4.0e-06
Every output is bit-identical from call to call.
"""
import numpy as np

from . import _lib
from .patches import _default_model

MAX_BINS = 128              # PESTO_TRAJECTORY_MAX_BINS
MAX_FRAMES = 2 ** 24        # PESTO_TRAJECTORY_MAX_FRAMES: the reference counts frames in float32
MAX_MAP_ATOMS = 12288       # PESTO_TRAJECTORY_MAX_MAP_ATOMS: Na + Nb of residue_contact_maps
F32_MAX = float(np.finfo(np.float32).max)


def _xyz(t, name="xyz"):
    """the [F, N, 3] array of a trajectory argument (its .xyz, if it has one)"""
    a = getattr(t, "xyz", t)
    if not (_lib.is_torch(a) or isinstance(a, np.ndarray)):
        a = np.asarray(a, np.float32)
    shp = tuple(a.shape)
    if len(shp) != 3 or shp[2] != 3 or shp[0] < 1 or shp[1] < 1:
        raise ValueError(f"{name} must be [F >= 1, N >= 1, 3], got {list(shp)}")
    return a


def _model_of(model, lead):
    if model is None:
        model = _default_model(lead.device.index if _lib.is_torch(lead) and lead.is_cuda else 0)
    return model


def _edges(bins):
    e = np.ascontiguousarray(np.asarray(_lib.host(bins), np.float64).reshape(-1))
    B = e.size - 1
    if not 1 <= B <= MAX_BINS:
        raise ValueError(f"1 to {MAX_BINS} bins (2 to {MAX_BINS + 1} edges), got {e.size} edges")
    if not np.all(np.isfinite(e)) or np.any(np.abs(e) > F32_MAX):
        raise ValueError("bins must be finite edges within the float32 range")
    if not np.all(e[1:] > e[:-1]):
        raise ValueError("bins must increase strictly")
    return e, B


def _pair(xyz0, xyz1, B):
    a = _xyz(xyz0, "xyz0")
    b = a if xyz1 is None else _xyz(xyz1, "xyz1")
    F, Na, Nb = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
    if int(b.shape[0]) != F:
        raise ValueError(f"the two sides have {F} and {int(b.shape[0])} frames")
    if F > MAX_FRAMES:
        raise ValueError(f"at most 2**24 frames, got {F}")
    if Na * Nb * B >= 2 ** 31:
        raise ValueError(f"output too large to index: Na * Nb * bins = {Na} * {Nb} * {B} must stay below 2**31")
    return a, b, F, Na, Nb


def _counts(xyz0, xyz1, bins, model, want_p, frame_splits=None):
    e, B = _edges(bins)
    a, b, F, Na, Nb = _pair(xyz0, xyz1, B)
    splits = 0 if frame_splits is None else int(frame_splits)
    if splits < 0:
        raise ValueError(f"frame_splits must be positive, got {frame_splits!r}")
    model = _model_of(model, a)
    h = model.handle
    side = _lib.Side(a, model._gpu)
    xa = side.put(a, np.float32)
    xb = xa if b is a else side.put(b, np.float32)
    counts = side.empty((Na, Nb, B), np.uint32)
    P = side.empty((Na, Nb, B), np.float32) if want_p else None
    lib = _lib.load()
    _lib.check(lib.pesto_contact_counts(h, F, Na, Nb, side.ptr(xa), side.ptr(xb), B, e.ctypes.data, side.ptr(counts), side.ptr(P), splits,
                                        side.kind, side.stream), lib.pesto_trajectory_last_error)
    return counts, P


def contact_counts(xyz0, xyz1=None, bins=None, model=None, frame_splits=None):
    """uint32 [Na, Nb, B]: for every atom pair the number of frames whose distance falls into each bin (xyz1=None: xyz0 against itself).
    On the device the counts come back as the int32 tensor of the same bits. frame_splits: the number of frame ranges counted by separate
    workgroups and added as integers (default: chosen from the sizes; the result does not depend on it)."""
    if bins is None:
        raise ValueError("bins: give the B + 1 bin edges")
    return _counts(xyz0, xyz1, bins, model, False, frame_splits)[0]


def contacts_distribution(xyz0, xyz1, bins, model=None, frame_splits=None):
    """The reference's contacts_distribution(xyz0, xyz1, bins): float32 [Na, Nb, B], the distribution of every atom pair's distance over
    the bins, P = count / (sum of the pair's counts + 1e-6)."""
    return _counts(xyz0, xyz1, bins, model, True, frame_splits)[1]


def _loglik(xyz0, xyz1, bins, P, model):
    e, B = _edges(bins)
    a, b, F, Na, Nb = _pair(xyz0, xyz1, B)
    if tuple(P.shape) != (Na, Nb, B):
        raise ValueError(f"P must be [{Na}, {Nb}, {B}], got {list(P.shape)}")
    model = _model_of(model, a)
    h = model.handle
    side = _lib.Side(a, model._gpu)
    xa = side.put(a, np.float32)
    xb = xa if b is a else side.put(b, np.float32)
    p = side.put(P, np.float32)
    L = side.empty((F,), np.float32)
    lib = _lib.load()
    _lib.check(lib.pesto_contact_loglik(h, F, Na, Nb, side.ptr(xa), side.ptr(xb), B, e.ctypes.data, side.ptr(p), side.ptr(L), side.kind, side.stream),
               lib.pesto_trajectory_last_error)
    return L


class StatisticalContactsModel:
    """The reference's StatisticalContactsModel(xmin, xmax, num_bins): bins = linspace(xmin, xmax, num_bins), i.e. num_bins - 1 bins."""

    def __init__(self, xmin, xmax, num_bins, model=None):
        self.bins = np.linspace(xmin, xmax, num_bins)
        _edges(self.bins)
        self.model = model
        self.P = None

    def fit(self, traj, other_traj=None):
        """Sets P float32 [Na, Nb, B]: the contacts distribution of traj against other_traj (against itself without one)."""
        self.P = contacts_distribution(traj, other_traj, self.bins, self.model)

    def loglikelihood(self, traj, other_traj=None):
        """float32 [F]: the negative mean log-likelihood of every frame under the fitted P. Device scratch: one double per 32 x 32 tile
        of atom pairs and frame, at most 64 MB (the frames go through in passes), whatever F is."""
        if self.P is None:
            raise ValueError("fit the model first")
        return _loglik(traj, other_traj, self.bins, self.P, self.model)


def div_KL(P, Q, model=None):
    """The reference's div_KL(P, Q): float32 [Na, Nb] = -sum_b P log(Q / (P + 1e-6)), terms with a ratio below 1e-6 dropped."""
    shp = tuple(P.shape)
    if len(shp) < 2 or tuple(Q.shape) != shp or min(shp) < 1:
        raise ValueError(f"P and Q must have the same shape [..., B >= 1], got {list(shp)} and {list(Q.shape)}")
    n = int(np.prod(shp[:-1]))
    if n * shp[-1] >= 2 ** 31:
        raise ValueError("P is too large to index: its size must stay below 2**31")
    model = _model_of(model, P)
    h = model.handle
    side = _lib.Side(P, model._gpu)
    p, q = side.put(P, np.float32), side.put(Q, np.float32)
    D = side.empty(shp[:-1], np.float32)
    lib = _lib.load()
    _lib.check(lib.pesto_contact_div_kl(h, n, int(shp[-1]), side.ptr(p), side.ptr(q), side.ptr(D), side.kind, side.stream),
               lib.pesto_trajectory_last_error)
    return D


def interface_ensemble_comparison(xyz_bound_R, xyz_bound_L, xyz_R, xyz_L, xmin=0.0, xmax=10.0, num_bins=21, model=None):
    """The core of the reference's interface_ensemble_comparison on already selected interface atoms (receptor R, ligand L; the bound
    ensemble and the one compared with it): returns (L0, L / mean(L0), D) with L0 the log-likelihood of the bound frames under the model
    fitted on them, L that of the other ensemble's frames under the same model, and D = div_KL(P_other, P_bound) [Na, Nb].
    The reference fits its second model with the literal bins (0, 10, 21) whatever it was given; here both models use the given bins,
    which is the same thing for the default arguments."""
    bound = StatisticalContactsModel(xmin, xmax, num_bins, model)
    bound.fit(xyz_bound_R, xyz_bound_L)
    L0 = bound.loglikelihood(xyz_bound_R, xyz_bound_L)
    L = bound.loglikelihood(xyz_R, xyz_L)
    other = StatisticalContactsModel(xmin, xmax, num_bins, model)
    other.fit(xyz_R, xyz_L)
    # a mean of F values the caller reads next; float32 like the reference's np.mean of its float32 L0
    return L0, L / L0.mean(), div_KL(other.P, bound.P, model)


def _residue_order(res, n_atoms, name, n_rows=None, need_all=True):
    """(perm int32 [N]: the atoms ordered by residue row, ascending within a row; off int32 [R + 1]; R). Made on the host on every call: a
    ROCm ``res`` is copied to the host (one synchronising copy of N integers) and perm / off go back to the device; only the coordinates
    and the outputs of residue_contact_maps / residue_centroids never leave the device."""
    r = _lib.host(res).reshape(-1)
    if r.size != n_atoms or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"{name} must be {n_atoms} integer residue rows, got {r.dtype} [{r.size}]")
    if r.min() < 0:
        raise ValueError(f"{name}: negative residue row")
    R = int(r.max()) + 1 if n_rows is None else int(n_rows)
    if R < 1 or int(r.max()) >= R:
        raise ValueError(f"{name}: rows must lie in 0 .. {R - 1}")
    cnt = np.bincount(r, minlength=R)
    if need_all and np.any(cnt == 0):
        raise ValueError(f"{name}: residue row {int(np.argmin(cnt != 0))} has no atom")
    off = np.zeros(R + 1, np.int32)
    off[1:] = np.cumsum(cnt)
    return np.argsort(r, kind="stable").astype(np.int32), off, R


def residue_contact_maps(xyz_a, xyz_b, res_a, res_b, r_thr=5.0, scale=10.0, model=None):
    """uint8 [F, Ra, Rb]: map[f, r, s] = 1 where an atom of residue r of A and an atom of residue s of B have
    float32(d * scale) < float32(r_thr) in frame f - NumPy's float32 evaluation of pairwise_distance_matrix(...) < r_thr in the
    reference's fnat. res_a [Na], res_b [Nb]: the residue row of each atom, 0 .. Ra - 1 / 0 .. Rb - 1, every row non-empty (they need
    not be contiguous). Na + Nb <= MAX_MAP_ATOMS."""
    a, b = _xyz(xyz_a, "xyz_a"), _xyz(xyz_b, "xyz_b")
    F, Na, Nb = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
    if int(b.shape[0]) != F:
        raise ValueError(f"the two sides have {F} and {int(b.shape[0])} frames")
    if Na + Nb > MAX_MAP_ATOMS:
        raise ValueError(f"at most {MAX_MAP_ATOMS} atoms on the two sides together, got {Na} + {Nb}")
    thr, sc = float(r_thr), float(scale)
    if not (np.isfinite(thr) and abs(thr) <= F32_MAX) or not (0 < sc <= F32_MAX and np.float32(sc) > 0):
        raise ValueError(f"r_thr must be finite and scale positive and finite, got {r_thr!r}, {scale!r}")
    pa, oa, Ra = _residue_order(res_a, Na, "res_a")
    pb, ob, Rb = _residue_order(res_b, Nb, "res_b")
    if F * Ra * Rb >= 2 ** 40:
        raise ValueError("output too large: F * Ra * Rb must stay below 2**40")
    model = _model_of(model, a)
    h = model.handle
    side = _lib.Side(a, model._gpu)
    xa, xb = side.put(a, np.float32), side.put(b, np.float32)
    pa, oa, pb, ob = (side.put(v, np.int32) for v in (pa, oa, pb, ob))
    maps = side.empty((F, Ra, Rb), np.uint8)
    lib = _lib.load()
    _lib.check(lib.pesto_residue_contact_maps(h, F, Na, Nb, side.ptr(xa), side.ptr(xb), Ra, Rb, side.ptr(pa), side.ptr(oa), side.ptr(pb), side.ptr(ob),
                                              thr, sc, side.ptr(maps), side.kind, side.stream), lib.pesto_trajectory_last_error)
    return maps


def _native(maps_ref, maps, model):
    sr, sm = tuple(maps_ref.shape), tuple(maps.shape)
    if len(sm) != 3 or len(sr) != 3 or sr[1:] != sm[1:] or sr[0] not in (1, sm[0]) or min(sm) < 1:
        raise ValueError(f"maps must be [F, Ra, Rb] and maps_ref [1 or F, Ra, Rb], got {list(sm)} and {list(sr)}")
    if sm[1] * sm[2] >= 2 ** 31:
        raise ValueError("too many residue pairs: Ra * Rb must stay below 2**31")
    model = _model_of(model, maps)
    h = model.handle
    side = _lib.Side(maps, model._gpu)
    flags = lambda v: v if str(v.dtype).endswith("uint8") else v != 0           # (the kernel tests uint8 entries against 0)
    m, r = side.put(flags(maps), np.uint8), side.put(flags(maps_ref), np.uint8)
    nat, tot = side.empty((sm[0],), np.int64), side.empty((1,), np.int64)
    lib = _lib.load()
    _lib.check(lib.pesto_native_contacts(h, sm[0], sr[0], sm[1] * sm[2], side.ptr(r), side.ptr(m), side.ptr(nat), side.ptr(tot), side.kind, side.stream),
               lib.pesto_trajectory_last_error)
    return nat, tot


def native_contacts(maps_ref, maps, model=None):
    """int64 [F]: the number of residue pairs in contact in both maps[f] and maps_ref[f] (maps_ref [1 or F, Ra, Rb])."""
    return _native(maps_ref, maps, model)[0]


def fnat(maps_ref, maps, model=None):
    """float64 [F]: the fraction of native contacts, native_contacts / sum(maps_ref) - the reference's expression, whose denominator
    counts every frame of maps_ref."""
    nat, tot = _native(maps_ref, maps, model)
    if _lib.is_torch(nat):
        return nat.double() / tot.double()
    return nat / tot[0]


def _selection(sel, n_atoms, name, least=0):
    """(int32 indices or None for all atoms, their number) of a selection given as indices or as a mask; least > 0: it must hold that many."""
    if sel is None:
        return None, n_atoms
    s = _lib.host(sel).reshape(-1)
    if s.dtype == np.bool_:
        if s.size != n_atoms:
            raise ValueError(f"{name}: a mask must have {n_atoms} entries, got {s.size}")
        s = np.nonzero(s)[0]
    if not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f"{name} must hold atom indices or be a mask, got {s.dtype}")
    if least and not least <= s.size <= n_atoms:
        raise ValueError(f"{name} must select {least} to {n_atoms} atoms, got {s.size}")
    if s.size and (s.min() < 0 or s.max() >= n_atoms):
        raise ValueError(f"{name}: atom indices must lie in 0 .. {n_atoms - 1}")
    return s.astype(np.int32), int(s.size)


def _superpose(xyz_ref, xyz, sel_ref, sel, scale, model, want_xyz):
    y, x = _xyz(xyz_ref, "xyz_ref"), _xyz(xyz, "xyz")
    Fr, Nr, F, N = int(y.shape[0]), int(y.shape[1]), int(x.shape[0]), int(x.shape[1])
    if Fr not in (1, F):
        raise ValueError(f"xyz_ref must have 1 or {F} frames, got {Fr}")
    sr, nr = _selection(sel_ref, Nr, "sel_ref")
    s, n = _selection(sel, N, "sel")
    if nr != n:
        raise ValueError(f"the selections differ in length: {nr} atoms of the reference, {n} of the trajectory")
    if n < 3:
        raise ValueError(f"a superposition needs at least 3 atoms, got {n}")
    if want_xyz and Nr != N and sel_ref is None and sel is None:
        raise ValueError(f"xyz_ref has {Nr} atoms and xyz {N}")
    if F * N * 3 >= 2 ** 40:
        raise ValueError("trajectory too large: F * N * 3 must stay below 2**40")
    model = _model_of(model, x)
    h = model.handle
    side = _lib.Side(x, model._gpu)
    xd, yd = side.put(x, np.float32), side.put(y, np.float32)
    srd = None if sr is None else side.put(sr, np.int32)
    sd = None if s is None else side.put(s, np.int32)
    t, R, tr = side.empty((F, 1, 3), np.float32), side.empty((F, 3, 3), np.float32), side.empty((Fr, 1, 3), np.float32)
    out = side.empty((F, N, 3), np.float32) if want_xyz else None
    dev = side.empty((F,), np.float32)
    lib = _lib.load()
    _lib.check(lib.pesto_superpose(h, F, Fr, Nr, N, n, side.ptr(yd), side.ptr(xd), side.ptr(srd), side.ptr(sd), float(scale), side.ptr(t), side.ptr(R),
                                   side.ptr(tr), side.ptr(out), side.ptr(dev), side.kind, side.stream), lib.pesto_trajectory_last_error)
    return t, R, tr, out, dev


def superpose_transform(xyz_ref, xyz, model=None):
    """The reference's superpose_transform(xyz_ref, xyz) on all atoms: (t [F, 1, 3], R [F, 3, 3], t_ref [Fr, 1, 3]) float32 with
    (xyz - t) @ R + t_ref on xyz_ref; t, t_ref the means over the atoms, R = Vt^T diag(1, 1, det(U) det(Vt)) U^T of
    U, S, Vt = svd((xyz_ref - t_ref)^T (xyz - t)). xyz_ref has one frame or one per frame of xyz. (The reference returns R as float64.)"""
    return _superpose(xyz_ref, xyz, None, None, 1.0, model, False)[:3]


def superpose(xyz_ref, xyz, sel_ref=None, sel=None, model=None):
    """float32 [F, N, 3]: every frame of xyz superposed onto xyz_ref, fitted on the selected atoms (index arrays or masks of the same
    number of atoms; None: all atoms) and applied to all atoms. A selection that does not determine the rotation (collinear or coincident
    atoms) gets some proper rotation that fits it as well as any other, as an SVD library would give; never NaN."""
    return _superpose(xyz_ref, xyz, sel_ref, sel, 1.0, model, True)[3]


def rmsd(xyz_ref, xyz, sel_ref=None, sel=None, scale=10.0, model=None):
    """float32 [F]: superpose on the selection, then sqrt(mean over the selected atoms of the squared deviation) * scale (the
    reference's rmsd; scale 10: nanometres in, angstroms out)."""
    return _superpose(xyz_ref, xyz, sel_ref, sel, scale, model, False)[4]


def residue_centroids(X_frames, res_of_atom, R, model=None):
    """float32 [F, R, 3]: the mean position of each residue's atoms per frame - X M / count at the end of the reference's
    apply_model_md notebook, for the X_frames and res_of_atom a Model.forward_frames caller holds (NaN for a row without atoms). X_frames stays on the device;
    res_of_atom is ordered on the host (see _residue_order)."""
    x = _xyz(X_frames, "X_frames")
    F, N = int(x.shape[0]), int(x.shape[1])
    perm, off, R = _residue_order(res_of_atom, N, "res_of_atom", n_rows=R, need_all=False)
    model = _model_of(model, x)
    h = model.handle
    side = _lib.Side(x, model._gpu)
    xd, pd, od = side.put(x, np.float32), side.put(perm, np.int32), side.put(off, np.int32)
    out = side.empty((F, R, 3), np.float32)
    lib = _lib.load()
    _lib.check(lib.pesto_residue_centroids(h, F, N, R, side.ptr(xd), side.ptr(pd), side.ptr(od), side.ptr(out), side.kind, side.stream),
               lib.pesto_trajectory_last_error)
    return out
