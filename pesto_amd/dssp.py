"""DSSP secondary structure on the GPU: the reference's ``md.compute_dssp`` without mdtraj.

The reference runs ``md.compute_dssp(traj, simplified=False)`` on every structure of the AlphaFold store in a 12-process pool and writes
the codes to HDF5 (interfaceome/secondary_structures.py:27-31, wrapper_secondary_structure). Here one call (pesto_dssp, pesto_dssp.hip)
takes all frames of a trajectory, or a ragged batch of structures, in one launch sequence:
    backbone_table      host helper: the N / CA / C / O atom rows, proline flags and chain numbers of a reader's structure dict
    compute_dssp        md.compute_dssp on coordinates: a '<U2' array [F, R] (or [R] for one frame), full or simplified alphabet
    kabsch_sander       the hydrogen-bond tables: every residue's two best acceptors and two best donors with their energies
    structure_dssp      the reference's wrapper on the structure dicts of structure_io (one, or a list in ONE launch)
    save_dssp/load_dssp the reference's store layout through h5store
The coordinates decide where a call runs (_lib.Side): a ROCm tensor keeps everything on the device and on torch's current stream and
gives the uint8 codes back as a tensor, NumPy comes back as NumPy. ``model`` lends its device handle; without one a weightless handle
is used. Arguments are checked before the library is loaded (ValueError). There is no CPU or PyTorch fallback.

The definition (the contract)
-----------------------------
Kabsch & Sander 1983 as the DSSP 2.x program, which mdtraj ports, applies it. mdtraj is not available to this project, so agreement
with it is not checkable here; what is written below is what the kernels compute and what tests/golden/make_dssp_golden.py restates.

Arithmetic. All arithmetic is in double. Inputs are float32 coordinates times ``scale`` (to angstroms). Sums are evaluated left to
right as written, every operation rounded on its own, no fused multiply-add; sqrt and division are IEEE. |a - b| is
sqrt(dx*dx + dy*dy + dz*dz) of the component differences.

Residue order and continuity. Residues are indexed in order within one structure; structures of a batch never see each other. A
residue without all four backbone atoms is 'NA' and takes part in nothing. cont(i) holds when i - 1 and i have all four atoms and the
same chain number and |C(i-1) - N(i)| <= 2.5. nobreak(a, b) means cont holds for every step a+1 .. b (and 0 <= a <= b < R).

1. Hydrogen positions. H(i) = N(i) + (C(i-1) - O(i-1)) / |C(i-1) - O(i-1)| when cont(i) holds and i is not proline; otherwise H(i) = N(i).

2. Hydrogen-bond energy. For every ordered pair donor d != acceptor a, both complete, with |CA(d) - CA(a)| < 9.0, d not proline and
   a != d - 1 (d -> d + 1 is evaluated and d -> d - 1 is not, as in the program):
       e = -27.888/|H(d)O(a)| + 27.888/|H(d)C(a)| - 27.888/|N(d)C(a)| + 27.888/|N(d)O(a)|
   If any of the four distances is < 0.5, e_m = -9900; otherwise e_m = round-half-away-from-zero(1000 e), clamped below at -9900. Only
   e_m < 0 is kept. A donor's two acceptors are the two smallest (e_m, a), ordered lexicographically; an acceptor's two donors are
   chosen likewise (this equals the program's strict-less update in its visiting order and does not depend on the order of the
   threads). bond(d, a) holds when a is one of d's two acceptors with e_m < -500.

3. Bridges. For i >= 1, j >= i + 3, j + 1 < R, with nobreak(i-1, i+1) and nobreak(j-1, j+1): parallel if (bond(i+1, j) and
   bond(j, i-1)) or (bond(j+1, i) and bond(i, j-1)); else antiparallel if (bond(i+1, j-1) and bond(j+1, i-1)) or (bond(j, i) and
   bond(i, j)).

4. Ladders and bulge linking. Ladders are maximal runs of same-type bridges (i+1, j+1) for parallel, (i+1, j-1) for antiparallel;
   j_begin / j_end of a ladder are its smallest / largest j. Ladder B continues ladder A of the same type through a bulge when both
   strands are unbroken across the gap (nobreak(i_end(A), i_begin(B)), and nobreak(j_end(A), j_begin(B)) for parallel,
   nobreak(j_end(B), j_begin(A)) for antiparallel), both gaps are non-negative, and one gap is <= 1 while the other is <= 4, with
   gi = i_begin(B) - i_end(A) - 1 and gj = j_begin(B) - j_end(A) - 1 (parallel) or j_begin(A) - j_end(B) - 1 (antiparallel). Linking
   is transitive. The DSSP program omits the lower bound on gj and through that links a hairpin to the next strand of a meander: on
   1OL5, without the bound 35 consecutive residues become E across two turns; with it the familiar
   EEEEEEEEEETTEEEEEEEETTT  EEEEEEEE appears. The bound is THIS PROJECT'S documented choice - the paper's wording - and it is not
   checkable against mdtraj here. Every residue from the first to the last of each strand of a linked set of ladders, gaps included,
   gets E if the set has more than one bridge, otherwise B; E is never overwritten by B.

5. Turns and helices. start_n(i), n = 3, 4, 5, holds when nobreak(i, i+n) and bond(i+n, i). In this order: H on i .. i+3 when
   start_4(i-1) and start_4(i) (overrides E / B); G on i .. i+2 when start_3(i-1) and start_3(i) and all three are blank or G; I on
   i .. i+4 when start_5(i-1) and start_5(i) and all five are blank or I. Then for blank i in 1 .. R-2: T if start_n(i-k) for some n
   and 1 <= k < n; else S if nobreak(i-2, i+2) and cos kappa < cos 70 deg = 0.3420201433256687, cos kappa = u.v / sqrt((u.u)(v.v)),
   u = CA(i) - CA(i-2), v = CA(i+2) - CA(i).

A NaN coordinate makes every comparison it enters false. Every output is an integer, bit-identical from call to call.

How it compares with the authors' records: on the five assemblies of tests/golden/pdb the simplified codes agree with the files'
HELIX / SHEET records on 0.86 (1ZNS), 0.82 (1H9D), 0.88 (1OL5), 0.92 (6O1T) and 0.91 (7KHT) of the residues, and every SHEET residue is E
(measured by tests/golden/make_dssp_golden.py; no test asserts these).
"""
import os

import numpy as np

from . import _lib
from .patches import _default_model

MAX_RESIDUES = 65535        # PESTO_DSSP_MAX_RESIDUES, per structure
CODES = np.array([" ", "H", "B", "E", "G", "I", "T", "S", "NA"])             # enum pesto_dssp_code
SIMPLIFIED = np.array(["C", "H", "E", "E", "H", "H", "C", "C", "NA"])        # H, G, I -> H;  B, E -> E;  the rest -> C
_BACKBONE = ("N", "CA", "C", "O")


def _text(a):
    a = np.asarray(a)
    return np.char.strip(a.astype(str)) if a.dtype.kind in "SUO" else a


def _one_table(d, first_chain):
    """(table [R, 4], proline [R], chain [R]) of one structure dict; residues are runs of atoms with one (chain_name, resid, resname,
    icode), in file order"""
    for key in ("name", "resname", "resid"):
        if not isinstance(d, dict) or key not in d:
            raise ValueError("a structure is a dict with 'name', 'resname', 'resid' (and 'chain_name'), or a dict of such subunits")
    name, resname = _text(d["name"]).reshape(-1), _text(d["resname"]).reshape(-1)
    resid = np.asarray(d["resid"]).reshape(-1).astype(np.int64)
    n = name.size
    if n < 1 or resname.size != n or resid.size != n:
        raise ValueError("'name', 'resname' and 'resid' must have one entry per atom, and at least one")
    cols = [resid != np.roll(resid, 1), resname != np.roll(resname, 1)]
    chain_name = _text(d["chain_name"]).reshape(-1) if "chain_name" in d else np.zeros(n, np.int64)
    if chain_name.size != n:
        raise ValueError("'chain_name' must have one entry per atom")
    cols.append(chain_name != np.roll(chain_name, 1))
    if "icode" in d:
        icode = _text(d["icode"]).reshape(-1)
        if icode.size != n:
            raise ValueError("'icode' must have one entry per atom")
        cols.append(icode != np.roll(icode, 1))
    first = np.logical_or.reduce(cols)
    first[0] = True
    row = np.cumsum(first) - 1
    starts = np.nonzero(first)[0]
    R = starts.size
    table = np.full((R, 4), -1, np.int32)
    for k, atom in enumerate(_BACKBONE):
        at = np.nonzero(name == atom)[0][::-1]              # reversed: the first atom of a name in a residue is written last and stays
        table[row[at], k] = at
    names, where = np.unique(chain_name[starts], return_index=True)
    order = np.argsort(np.argsort(where))                   # chains numbered in order of first appearance
    chain = order[np.searchsorted(names, chain_name[starts])].astype(np.int32) + first_chain
    return table, (resname[starts] == "PRO").astype(np.uint8), chain


def backbone_table(structure_or_subunits):
    """(table int32 [R, 4], proline uint8 [R], chain int32 [R], R) of what structure_io.read_pdb / StructuresDataset return: the rows of
    'xyz' that hold the N, CA, C and O of every residue (-1 for a missing atom; the first atom of a name counts), whether the residue
    is a proline, and its chain number. Residues are runs of consecutive atoms with one (chain_name, resid, resname, icode), in file
    order - every residue of the file, hetero groups and nucleotides included (they lack the four atoms and come out as 'NA', as in
    mdtraj). Chains are numbered in order of first appearance. A dict of subunits is concatenated in order, as the reference's
    concatenate_chains does; every subunit's chains get numbers of their own."""
    from .structure_io import Structure
    item = structure_or_subunits
    if isinstance(item, Structure):
        item = item.to_dict()
    if not isinstance(item, dict) or not item:
        raise ValueError("a structure is a dict with 'name', 'resname', 'resid' (and 'chain_name'), or a dict of such subunits")
    parts = [item] if "name" in item and not isinstance(item["name"], dict) else list(item.values())
    tables, pros, chains, atoms, first_chain = [], [], [], 0, 0
    for p in parts:
        t, pr, ch = _one_table(p, first_chain)
        tables.append(np.where(t >= 0, t + atoms, -1).astype(np.int32))
        pros.append(pr)
        chains.append(ch)
        atoms += np.asarray(p["name"]).reshape(-1).size
        first_chain = int(ch.max()) + 1
    table = np.concatenate(tables)
    return table, np.concatenate(pros), np.concatenate(chains), int(table.shape[0])


def _coordinates(xyz):
    """(the [F, N, 3] array, whether it came as one [N, 3] frame)"""
    a = getattr(xyz, "xyz", xyz)
    if not (_lib.is_torch(a) or isinstance(a, np.ndarray)):
        a = np.asarray(a, np.float32)
    shp = tuple(a.shape)
    if len(shp) not in (2, 3) or shp[-1] != 3 or min(shp) < 1:
        raise ValueError(f"xyz must be [N >= 1, 3] or [F >= 1, N >= 1, 3], got {list(shp)}")
    return (a[None], True) if len(shp) == 2 else (a, False)


def _checked_table(table, n_atoms):
    """(table int32 [R, 4], proline uint8 [R], chain int32 [R]) of backbone_table's tuple (R optional), or of a bare [R, 4] table"""
    pro = chain = None
    if isinstance(table, (tuple, list)) and len(table) in (3, 4) and np.ndim(table[0]) == 2:
        if len(table) == 4 and int(table[3]) != np.shape(table[0])[0]:
            raise ValueError(f"table: the residue count {table[3]} is not the table's {np.shape(table[0])[0]} rows")
        table, pro, chain = table[0], table[1], table[2]
    t = _lib.host(table)
    if t.ndim != 2 or t.shape[1] != 4 or t.shape[0] < 1 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"table must be integer [R >= 1, 4] atom rows (N, CA, C, O), got {t.dtype} {list(t.shape)}")
    R = t.shape[0]
    if t.min() < -1 or t.max() >= n_atoms:
        raise ValueError(f"table names atom rows outside -1 .. {n_atoms - 1}")
    pro = np.zeros(R, np.uint8) if pro is None else _lib.host(pro).reshape(-1)
    chain = np.zeros(R, np.int32) if chain is None else _lib.host(chain).reshape(-1)
    if pro.size != R or chain.size != R:
        raise ValueError(f"proline flags and chain numbers must have one entry per residue ({R})")
    if not np.issubdtype(chain.dtype, np.integer):
        raise ValueError("chain numbers must be integers")
    return np.ascontiguousarray(t, np.int32), np.ascontiguousarray(pro != 0, np.uint8), np.ascontiguousarray(chain, np.int32)


def _run(xyz, table, sizes, scale, model, want_codes, want_bonds):
    """One pesto_dssp call: (codes uint8 [F, R] or None, partners int32 [F, R, 4] or None, energies int32 [F, R, 4] or None, single)"""
    x, single = _coordinates(xyz)
    F, N = int(x.shape[0]), int(x.shape[1])
    t, pro, chain = _checked_table(table, N)
    R = t.shape[0]
    scale = float(scale)
    if not np.isfinite(scale):
        raise ValueError(f"scale must be finite, got {scale!r}")
    if F * N >= 2 ** 31 or F * R >= 2 ** 31:
        raise ValueError(f"too large to index: F * N = {F} * {N} and F * R = {F} * {R} must stay below 2**31")
    sizes = [R] if sizes is None else [int(v) for v in np.asarray(_lib.host(sizes)).reshape(-1)]
    if not sizes or min(sizes) < 1 or sum(sizes) != R:
        raise ValueError(f"sizes must be positive residue counts that add up to {R}, got {sizes if len(sizes) <= 8 else sizes[:8] + ['...']}")
    if max(sizes) > MAX_RESIDUES:
        raise ValueError(f"a structure has {max(sizes)} residues, at most {MAX_RESIDUES}")
    if model is None:
        model = _default_model(x.device.index if _lib.is_torch(x) and x.is_cuda else 0)
    h = model.handle
    side = _lib.Side(x, model._gpu)
    xd = side.put(x, np.float32)
    offs = _lib.offsets(sizes)
    codes = side.empty((F, R), np.uint8) if want_codes else None
    partners = side.empty((F, R, 4), np.int32) if want_bonds else None
    energies = side.empty((F, R, 4), np.int32) if want_bonds else None
    lib = _lib.load()
    _lib.check(lib.pesto_dssp(h, F, N, side.ptr(xd), scale, R, len(sizes), offs.ctypes.data, t.ctypes.data, pro.ctypes.data, chain.ctypes.data,
                              side.ptr(codes), side.ptr(partners), side.ptr(energies), side.kind, side.stream), lib.pesto_dssp_last_error)
    return side.result(codes), side.result(partners), side.result(energies), single


def letters(codes, simplified=True):
    """The '<U2' letters of uint8 codes (enum pesto_dssp_code): the full alphabet 'H B E G I T S', ' ' and 'NA', or the simplified one
    'H' (H, G, I), 'E' (B, E), 'C' (the rest) and 'NA'."""
    c = _lib.host(codes)
    if not np.issubdtype(c.dtype, np.integer) or (c.size and (c.min() < 0 or c.max() >= len(CODES))):
        raise ValueError(f"codes must be integers in 0 .. {len(CODES) - 1}")
    return (SIMPLIFIED if simplified else CODES)[c.astype(np.int64)]


def compute_dssp(xyz, table, simplified=True, sizes=None, scale=1.0, model=None, return_codes=False):
    """md.compute_dssp(traj, simplified) on coordinates: a '<U2' array [F, R], or [R] for one frame [N, 3], as mdtraj gives it.
    xyz: [F, N, 3], [N, 3] or anything with ``.xyz``; scale multiplies it to angstroms (10.0 for mdtraj's nanometres).
    table: what backbone_table returns, or a bare int [R, 4] table of N / CA / C / O atom rows (-1: missing; then no residue is a
    proline and all share one chain). sizes: residue counts of independent structures laid end to end along R, computed in one launch,
    none seeing another. Full alphabet (simplified=False): 'H', 'B', 'E', 'G', 'I', 'T', 'S', ' ' and 'NA' for a residue without all
    four backbone atoms; simplified: 'H', 'E', 'C', 'NA'. return_codes (and always for a ROCm tensor, which stays on its device and
    stream): the uint8 codes of enum pesto_dssp_code instead - letters() turns them into either alphabet."""
    codes, _, _, single = _run(xyz, table, sizes, scale, model, True, False)
    if single:
        codes = codes[0]
    if return_codes or (_lib.is_torch(codes) and codes.is_cuda):
        return codes
    return letters(codes, simplified)


def kabsch_sander(xyz, table, sizes=None, scale=1.0, model=None):
    """(partners int32 [F, R, 4], energies float32 [F, R, 4]; no frame axis for one frame): every residue's two best acceptors of its
    N-H (columns 0, 1) and two best donors to its C=O (columns 2, 3), best first, as residue indices within the residue's structure, -1
    for none, with the energies in kcal/mol (the definition's integer thousandths / 1000; 0 for none)."""
    _, partners, energies, single = _run(xyz, table, sizes, scale, model, False, True)
    if _lib.is_torch(energies):
        import torch
        energies = energies.to(torch.float32) / 1000.0
    else:
        energies = energies.astype(np.float32) / np.float32(1000.0)
    return (partners[0], energies[0]) if single else (partners, energies)


def structure_dssp(structure_or_list, simplified=False, model=None):
    """The reference's wrapper_secondary_structure (interfaceome/secondary_structures.py:27-31) on what structure_io.read_pdb /
    StructuresDataset return: a structure dict, or a dict of subunits that is concatenated in order. A '<U2' array [1, R] as
    md.compute_dssp gives for the one-frame trajectory the reference builds (full alphabet by default, as the reference asks for).
    A list or tuple of structures goes through ONE launch and comes back as a list."""
    many = isinstance(structure_or_list, (list, tuple))
    items = list(structure_or_list) if many else [structure_or_list]
    if not items:
        return []
    tabs, xyzs, atoms = [], [], 0
    for it in items:
        t, pro, chain, _ = backbone_table(it)
        d = it.to_dict() if hasattr(it, "to_dict") else it
        parts = [d] if "xyz" in d and not isinstance(d["xyz"], dict) else list(d.values())
        if any(not isinstance(p, dict) or "xyz" not in p for p in parts):
            raise ValueError("a structure needs 'xyz'")
        xyz = np.concatenate([np.asarray(p["xyz"], np.float32).reshape(-1, 3) for p in parts])
        if xyz.shape[0] <= int(t.max()):
            raise ValueError("'xyz' has fewer rows than 'name'")
        tabs.append((np.where(t >= 0, t + atoms, -1).astype(np.int32), pro, chain))
        xyzs.append(xyz)
        atoms += xyz.shape[0]
    table = (np.concatenate([t[0] for t in tabs]), np.concatenate([t[1] for t in tabs]), np.concatenate([t[2] for t in tabs]))
    sizes = [t[0].shape[0] for t in tabs]
    out = compute_dssp(np.concatenate(xyzs)[None], table, simplified, sizes, 1.0, model)
    if not many:
        return out
    return [o for o in np.split(out, np.cumsum(sizes)[:-1], axis=1)]


def save_dssp(path, results):
    """Write {key: codes} in the layout of the reference's store (interfaceome/secondary_structures.py:42-52):
    ``hf[key] = ss.ravel().astype(np.string_)`` per key - the ravelled letters as fixed-length byte strings - and the keys as
    ``metadata/keys``. Needs the HDF5 C library (h5store.H5Unavailable otherwise; nothing is written in another format)."""
    from . import h5store
    h5store.load()
    path = os.fspath(path)
    tmp = path + ".tmp"
    try:
        with h5store.H5Store(tmp, "w") as hf:
            keys = []
            for key, v in results.items():
                v = np.asarray(v)
                if v.dtype.kind not in "US":
                    v = letters(v, simplified=False)
                hf.create_dataset(str(key), v.ravel().astype("S2"))
                keys.append(str(key))
            hf.create_dataset("metadata/keys", np.array(keys).astype(bytes) if keys else np.zeros(0, "S1"))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def load_dssp(path):
    """{key: '<U2' letters [R]} of a store written by save_dssp or by the reference's script."""
    from . import h5store
    with h5store.H5Store(os.fspath(path)) as hf:
        keys = [k.decode() for k in hf.read("metadata/keys")] if "metadata/keys" in hf else []
        return {k: np.asarray(hf.read(k)).astype("U2") for k in keys}
