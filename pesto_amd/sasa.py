"""Solvent-accessible surface area on the GPU: the reference's two uses of ``md.shrake_rupley`` without mdtraj.

The reference computes SASA over every structure of a store in a two-process pool (interfaceome/solvent_accessible_surface_area.py) and
frame by frame in a Python loop (sasa, md_analysis/mdtraj_utils/trajectory_utils.py:428-438). Here one call (pesto_sasa,
pesto_sasa.hip) takes all frames of a trajectory, or a ragged batch of structures, in one launch sequence:
    sphere_points / atomic_radii    the golden-spiral points mdtraj generates; van der Waals radii of the project's element vocabulary
    shrake_rupley                   areas per atom or per residue of [N,3] / [F,N,3] coordinates, several structures per call (sizes)
    sasa                            the reference's trajectory_utils.sasa: float32 [F, N], all frames in one call
    structure_sasa                  the reference's wrapper on the structure dicts of structure_io (one, or a list in one launch)
    save_sasa                       the reference's store layout through h5store
    buried_area                     per atom, the SASA of its subunit alone minus its SASA in the complex, in one launch
The first array decides where a call runs (_lib.Side): a ROCm tensor keeps everything on the device and on torch's current stream, NumPy
comes back as NumPy. ``model`` lends its device handle; without one a weightless handle is used. Arguments are checked before the library is
loaded (ValueError). There is no CPU or PyTorch fallback.

Definition, for X float32 [F,N,3], R float32 [N] = float32(radius) + float32(probe) and the P sphere points S, every operation rounded to
float32 as written (no fused multiply-add):
    t = X[f,i] + (R[i] * S[k]);  d = t - X[f,j];  q = (d.x*d.x + d.y*d.y) + d.z*d.z
    point k of atom i is buried when some j != i of i's structure (with finite coordinates and radius) has q < R[j]*R[j]
    count[f,i] = the number of points that are not buried
    area[f,i]  = float32(((c0 * count) * R[i]) * R[i]) in double, c0 = 4 pi / P;  a residue's area is the double sum over its atoms, in atom
                 order, rounded once
This is mdtraj's algorithm with an exact, integer result: count does not depend on the order of the neighbours, on the other structures
of the call or on the kernel's pruning, and every output is bit-identical from call to call. An atom with a NaN or infinite coordinate or
radius buries nothing and counts all P points; coincident atoms are not an error (mdtraj exits the process on them). mdtraj evaluates the
area in float32, so its values may differ from these by a couple of units in the last place (not checkable without mdtraj). Areas are in
the square of xyz's unit; radii and probe_radius must be in that unit (mdtraj works in nanometres: 1 nm^2 = 100 A^2).
"""
import os

import numpy as np

from . import _lib
from .patches import _default_model

MAX_POINTS = 8192           # PESTO_SASA_MAX_POINTS

# van der Waals radii in angstroms. H, C, N, O, F, P, S: A. Bondi, J. Phys. Chem. 68 (1964) 441. Se, Mg, Cl, Zn, Na, I, K, Br, Cu, Cd, Ni,
# Hg, As, Pt: Bondi's table as well. Ca, Sr, Ba, B: M. Mantina et al., J. Phys. Chem. A 113 (2009) 5806 (main-group elements Bondi left
# out). Fe, Mn, Co, W, Mo (in neither): S. Alvarez, Dalton Trans. 42 (2013) 8617. mdtraj's own table may differ for the metals: pass
# ``radii=`` where its values are needed.
VDW_RADII = {
    "H": 1.20, "C": 1.70, "N": 1.55, "O": 1.52, "F": 1.47, "P": 1.80, "S": 1.80,
    "Se": 1.90, "Mg": 1.73, "Cl": 1.75, "Zn": 1.39, "Na": 2.27, "I": 1.98, "K": 2.75, "Br": 1.85, "Cu": 1.40, "Cd": 1.58, "Ni": 1.63,
    "Hg": 1.55, "As": 1.85, "Pt": 1.75,
    "Ca": 2.31, "Sr": 2.49, "Ba": 2.68, "B": 1.92,
    "Fe": 2.44, "Mn": 2.45, "Co": 2.40, "W": 2.57, "Mo": 2.45,
}
_UNITS = {"A": 1.0, "nm": 0.1}


def sphere_points(n=960):
    """float32 [n, 3]: the golden-spiral unit points of mdtraj's Shrake-Rupley code, computed in float64 and rounded once:
    y_k = k (2 / n) - 1 + 1 / n, r = sqrt(1 - y^2), phi = k pi (3 - sqrt 5), point (cos(phi) r, y, sin(phi) r)."""
    n = int(n)
    if not 1 <= n <= MAX_POINTS:
        raise ValueError(f"n_sphere_points must be in 1 .. {MAX_POINTS}, got {n}")
    k = np.arange(n, dtype=np.float64)
    y = k * (2.0 / n) - 1.0 + 1.0 / n
    r = np.sqrt(1.0 - y * y)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([np.cos(phi) * r, y, np.sin(phi) * r], 1).astype(np.float32)


def atomic_radii(elements, unit="A"):
    """float32 [N]: the van der Waals radius of every atom (VDW_RADII) in angstroms (unit="A") or nanometres ("nm"). elements: element
    symbols in any letter case, or integer indices into the project's STD_ELEMENTS (dataset.py; the first block of q). An element without
    an entry - the vocabulary's "unknown" index included - raises ValueError: pass ``radii=`` to shrake_rupley for those."""
    if unit not in _UNITS:
        raise ValueError(f"unit must be 'A' or 'nm', got {unit!r}")
    e = _lib.host(elements).reshape(-1)
    if np.issubdtype(e.dtype, np.integer):
        from .dataset import STD_ELEMENTS
        if e.size and (e.min() < 0 or e.max() >= len(STD_ELEMENTS)):
            bad = int(e[(e < 0) | (e >= len(STD_ELEMENTS))][0])
            raise ValueError(f"element index {bad} has no radius (0 .. {len(STD_ELEMENTS) - 1} index STD_ELEMENTS): pass radii=")
        e = STD_ELEMENTS[e]
    names, inverse = np.unique(np.char.strip(np.asarray(e).astype(str)), return_inverse=True)
    table = np.empty(names.size, np.float64)
    for k, name in enumerate(names):
        if name.capitalize() not in VDW_RADII:
            raise ValueError(f"element {name!r} has no radius in VDW_RADII: pass radii=")
        table[k] = VDW_RADII[name.capitalize()] * _UNITS[unit]
    return table[inverse.reshape(-1)].astype(np.float32)


def _coordinates(xyz):
    """(the [F, N, 3] array, whether it came as one [N, 3] frame)"""
    a = getattr(xyz, "xyz", xyz)
    if not (_lib.is_torch(a) or isinstance(a, np.ndarray)):
        a = np.asarray(a, np.float32)
    shp = tuple(a.shape)
    if len(shp) not in (2, 3) or shp[-1] != 3 or min(shp) < 1:
        raise ValueError(f"xyz must be [N >= 1, 3] or [F >= 1, N >= 1, 3], got {list(shp)}")
    return (a[None], True) if len(shp) == 2 else (a, False)


def _total_radius(radii, elements, probe_radius, n_atoms):
    """float32 [N] atomic + probe radius, added in float32 (a ROCm ``radii`` stays on its device)"""
    probe = float(probe_radius)
    if not (np.isfinite(probe) and probe >= 0.0):
        raise ValueError(f"probe_radius must be finite and not negative, got {probe_radius!r}")
    if radii is None:
        if elements is None:
            raise ValueError("give radii= (one per atom) or elements= (symbols, or indices into STD_ELEMENTS)")
        radii = atomic_radii(elements)
    if int(np.prod(tuple(radii.shape) if hasattr(radii, "shape") else np.shape(radii))) != n_atoms:
        raise ValueError(f"{'radii' if elements is None else 'radii / elements'} must have one entry per atom ({n_atoms})")
    if _lib.is_torch(radii):
        import torch
        return radii.detach().reshape(-1).to(torch.float32) + float(np.float32(probe))
    return np.asarray(radii, np.float32).reshape(-1) + np.float32(probe)


def _groups(residue, n_atoms):
    """(perm, off, R) of the residue rows, as trajectory._residue_order builds them (rows need not be contiguous; every row has an atom)"""
    from .trajectory import _residue_order
    if residue is None:
        raise ValueError("mode='residue' needs residue=: the residue row of every atom")
    return _residue_order(residue, n_atoms, "residue")


def _run(x, R, n_points, sizes, groups, model, want_counts, want_area):
    """One pesto_sasa call: (counts [F,N] int32 or None, area [F,N] float32 or None, group sums [F,G] float32 or None), all checked."""
    F, N = int(x.shape[0]), int(x.shape[1])
    pts = sphere_points(n_points)
    if F * N >= 2 ** 31:
        raise ValueError(f"too large to index: F * N = {F} * {N} must stay below 2**31")
    if sizes is None:
        sizes = [N]
    sizes = [int(v) for v in np.asarray(_lib.host(sizes)).reshape(-1)]
    if not sizes or min(sizes) < 1 or sum(sizes) != N:
        raise ValueError(f"sizes must be positive atom counts that add up to {N}, got {sizes if len(sizes) <= 8 else sizes[:8] + ['...']}")
    if groups is not None and F * groups[2] >= 2 ** 31:
        raise ValueError("too many residue sums: F * R must stay below 2**31")
    if model is None:
        model = _default_model(x.device.index if _lib.is_torch(x) and x.is_cuda else 0)
    h = model.handle
    side = _lib.Side(x, model._gpu)
    xd, rd, sd = side.put(x, np.float32), side.put(R, np.float32), side.put(pts, np.float32)
    offs = _lib.offsets(sizes)
    counts = side.empty((F, N), np.int32) if want_counts else None
    area = side.empty((F, N), np.float32) if want_area else None
    pd = od = gsum = None
    G = 0
    if groups is not None:
        G = groups[2]
        pd, od = side.put(groups[0], np.int32), side.put(groups[1], np.int32)
        gsum = side.empty((F, G), np.float32)
    lib = _lib.load()
    _lib.check(lib.pesto_sasa(h, F, N, len(sizes), offs.ctypes.data, side.ptr(xd), side.ptr(rd), int(n_points), side.ptr(sd),
                              4.0 * np.pi / int(n_points), side.ptr(counts), side.ptr(area), G, side.ptr(pd), side.ptr(od), side.ptr(gsum),
                              side.kind, side.stream), lib.pesto_sasa_last_error)
    return side.result(counts), side.result(area), side.result(gsum)


def shrake_rupley(xyz, radii=None, elements=None, probe_radius=1.4, n_sphere_points=960, mode="atom", residue=None, sizes=None, model=None,
                  return_counts=False):
    """md.shrake_rupley(traj, probe_radius, n_sphere_points, mode) on coordinates: float32 [F, N] areas per atom (mode="atom") or
    [F, R] per residue (mode="residue", with residue= the residue row 0 .. R - 1 of every atom; rows need not be contiguous), in the
    square of xyz's unit. xyz: [F, N, 3], one frame [N, 3] (then the result has no frame axis) or anything with ``.xyz``.
    radii: the atomic radius of every atom in xyz's unit (without the probe); without it, elements= (symbols, or indices into
    STD_ELEMENTS) looks them up in VDW_RADII, which is in angstroms. sizes: atom counts of independent structures laid end to end along
    N, computed in one launch, none seeing another. return_counts: also the int32 [F, N] numbers of exposed sphere points.
    Note mdtraj's defaults are nanometres (probe_radius=0.14); here the default probe is 1.4 for angstrom coordinates."""
    x, single = _coordinates(xyz)
    if mode not in ("atom", "residue"):
        raise ValueError(f"mode must be 'atom' or 'residue', got {mode!r}")
    sphere_points(n_sphere_points)
    N = int(x.shape[1])
    R = _total_radius(radii, elements, probe_radius, N)
    groups = _groups(residue, N) if mode == "residue" else None
    counts, area, gsum = _run(x, R, n_sphere_points, sizes, groups, model, return_counts, groups is None)
    out = area if groups is None else gsum
    if single:
        out, counts = out[0], (None if counts is None else counts[0])
    return (out, counts) if return_counts else out


def sasa(traj, radii=None, elements=None, probe_radius=1.4, n_sphere_points=960, model=None):
    """The reference's sasa(traj) (md_analysis/mdtraj_utils/trajectory_utils.py:428-438): float32 [F, N], the solvent-accessible area of
    every atom in every frame - all frames in one call instead of one md.shrake_rupley per frame. traj: [F, N, 3] or anything with
    ``.xyz``; radii / elements / probe_radius as in shrake_rupley (mdtraj trajectories are in nanometres: pass radii and probe in nm,
    e.g. atomic_radii(elements, "nm") and 0.14)."""
    x, single = _coordinates(traj)
    if single:
        raise ValueError("sasa takes a trajectory [F, N, 3]; use shrake_rupley for one frame")
    return shrake_rupley(x, radii, elements, probe_radius, n_sphere_points, model=model)


def _concatenated(item):
    """(xyz [N,3], element [N], residue row [N]) of a structure dict or a dict of subunits (concatenated in order, as the reference's
    concatenate_chains does)"""
    from .structure_io import Structure
    if isinstance(item, Structure):
        item = item.to_dict()
    if not isinstance(item, dict) or not item:
        raise ValueError("a structure is a dict with 'xyz' and 'element', or a dict of such subunits")
    parts = [item] if "xyz" in item and not isinstance(item["xyz"], dict) else list(item.values())
    for p in parts:
        if not isinstance(p, dict) or "xyz" not in p or "element" not in p:
            raise ValueError("a structure is a dict with 'xyz' and 'element', or a dict of such subunits")
    xyz = np.concatenate([np.asarray(p["xyz"], np.float32).reshape(-1, 3) for p in parts])
    if xyz.shape[0] < 1:
        raise ValueError("a structure without atoms")
    element = np.concatenate([np.asarray(p["element"]).astype(str).reshape(-1) for p in parts])
    rows, start = [], 0
    for c, p in enumerate(parts):
        n = np.asarray(p["xyz"]).reshape(-1, 3).shape[0]
        keys = [np.full(n, c, np.int64), np.asarray(p["resid"]).reshape(-1).astype(np.int64)] if "resid" in p else [np.full(n, c, np.int64), np.arange(n)]
        if "chain_name" in p:
            keys.insert(1, np.unique(np.asarray(p["chain_name"]).astype(str), return_inverse=True)[1].reshape(-1).astype(np.int64))
        _, r = np.unique(np.stack(keys, 1), axis=0, return_inverse=True)
        rows.append(r.reshape(-1) + start)
        start += int(r.max()) + 1 if n else 0
    return xyz, element, np.concatenate(rows).astype(np.int32)


def structure_sasa(subunits_or_structure, radii=None, probe_radius=1.4, n_sphere_points=960, mode="atom", model=None):
    """The reference's wrapper_solvent_accessible_surface_area (interfaceome/solvent_accessible_surface_area.py:27-31) on what
    structure_io.read_pdb / StructuresDataset return: a structure dict, or a dict of subunits that is concatenated in order. float32 [N]
    areas per atom in A^2 (mode="residue": per residue, in order of chain and residue number), from the 'element' column and VDW_RADII
    unless radii= is given. A list or tuple of structures goes through ONE launch and comes back as a list. The reference converts to
    nanometres first, so its numbers are these / 100."""
    many = isinstance(subunits_or_structure, (list, tuple))
    items = [_concatenated(s) for s in (subunits_or_structure if many else [subunits_or_structure])]
    if not items:
        return []
    sizes = [it[0].shape[0] for it in items]
    xyz = np.concatenate([it[0] for it in items])
    if radii is None:
        radii = atomic_radii(np.concatenate([it[1] for it in items]))
    elif many:
        radii = np.concatenate([np.asarray(_lib.host(r), np.float32).reshape(-1) for r in radii])
    residue, start = None, 0
    if mode == "residue":
        rows = []
        for it in items:
            rows.append(it[2] + start)
            start += int(it[2].max()) + 1
        residue = np.concatenate(rows)
    out = shrake_rupley(xyz, radii, None, probe_radius, n_sphere_points, mode, residue, sizes, model)
    if not many:
        return out
    cuts = np.cumsum(sizes if mode == "atom" else [int(it[2].max()) + 1 for it in items])[:-1]
    return np.split(out, cuts)


def save_sasa(path, results):
    """Write {key: areas} in the layout of the reference's store (interfaceome/solvent_accessible_surface_area.py:42-52):
    ``hf[key] = sasa.ravel().astype(np.string_)`` per key - fixed-length byte strings of the float32 values' text - and the keys as
    ``metadata/keys``. The reference's values are nm^2, which is A^2 / 100: divide what structure_sasa returns by 100 for a store that
    its readers take as theirs. Needs the HDF5 C library (h5store.H5Unavailable otherwise; nothing is written in another format)."""
    from . import h5store
    h5store.load()
    path = os.fspath(path)
    tmp = path + ".tmp"
    try:
        with h5store.H5Store(tmp, "w") as hf:
            keys = []
            for key, v in results.items():
                hf.create_dataset(str(key), np.asarray(_lib.host(v), np.float32).ravel().astype(bytes))
                keys.append(str(key))
            hf.create_dataset("metadata/keys", np.array(keys).astype(bytes) if keys else np.zeros(0, "S1"))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def load_sasa(path):
    """{key: float32 areas} of a store written by save_sasa or by the reference's script."""
    from . import h5store
    with h5store.H5Store(os.fspath(path)) as hf:
        keys = [k.decode() for k in hf.read("metadata/keys")] if "metadata/keys" in hf else []
        return {k: hf.read(k).astype(np.float32) for k in keys}


def buried_area(xyz, radii, subunit, probe_radius=1.4, n_sphere_points=960, model=None):
    """(counts, areas) per atom: the exposed sphere points / the SASA the atom has in its subunit alone minus what it has in the complex,
    int32 and float32 [N] (or [F, N] for xyz [F, N, 3]). subunit: an integer label per atom. One launch over the ragged batch
    [complex, subunit 0, subunit 1, ...]; the differences are taken here. A count difference is never negative: the complex's occluders
    are a superset of the subunit's."""
    x, single = _coordinates(xyz)
    N = int(x.shape[1])
    lab = _lib.host(subunit).reshape(-1)
    if lab.size != N or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"subunit must be {N} integer labels, got {lab.dtype} [{lab.size}]")
    R = _total_radius(radii, None, probe_radius, N)
    sphere_points(n_sphere_points)
    order = np.argsort(lab, kind="stable")
    sizes = [N] + [int(v) for v in np.unique(lab, return_counts=True)[1]]
    gather = np.concatenate([np.arange(N), order])
    if _lib.is_torch(x):
        import torch
        gather_x = torch.as_tensor(gather, device=x.device)
        gather_r = torch.as_tensor(gather, device=R.device) if _lib.is_torch(R) else gather
        back = torch.as_tensor(np.argsort(order), device=x.device)
    else:
        gather_x = gather_r = gather
        back = np.argsort(order)
    counts, area, _ = _run(x[:, gather_x], R[gather_r], n_sphere_points, sizes, None, model, True, True)
    dc = counts[:, N:][:, back] - counts[:, :N]
    da = area[:, N:][:, back] - area[:, :N]
    return (dc[0], da[0]) if single else (dc, da)
