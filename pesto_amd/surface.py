"""Surface-vertex benchmark scoring on the GPU: the reference's comparison of per-residue predictors with MaSIF-site on surface meshes
(masif-site_benchmark/masif_sppider_Intpred_comp.ipynb), without pyflann, pymesh or Biopython.

A ground-truth mesh carries an interface flag per vertex. Every vertex is tied to its nearest atom; predictions travel atom -> vertex for
the per-point ROC AUC, labels travel vertex -> residue through an area rule for the per-residue ROC AUC, and MaSIF's per-vertex scores
travel vertex -> residue as a maximum. Here (pesto_surface.hip), over a ragged batch of S structures:
    nearest_atoms          (index int32 [V], distance float32 [V]): the nearest atom of every vertex
    vertex_areas           float64 [V]: pymesh's vertex_area, a third of every adjacent triangle (vertex_areas_fixed: the int64 sums)
    residue_surface        the residue table: n_vertices, area, iface_area, label (the notebook's is_res_iface), max_score
    vertex_scores          float32 [V]: a per-atom prediction gathered at the vertices
    scored_residues        (offsets int32 [S + 1], residue int32 [K], y uint8 [K], p float32 [K]): residues with a vertex and a prediction
    benchmark_surfaces     the driver: per-structure, pooled and median ROC AUCs per point and per residue, through ranking.scores
    read_ply / write_ply / structure_atoms / ca_prediction      host I/O (no kernel)
The batch is described by offsets (int32 [S + 1], strictly rising from 0, on the host): ``v_offsets`` over V vertices, ``a_offsets`` over N
atoms, ``r_offsets`` over R residues, and ``f_offsets`` over F faces, where alone a structure may be empty. Face indices and
``atom_residue`` are local to their structure; nearest-atom indices and everything returned per vertex or per residue are in batch order.
One structure needs no offsets. The first array decides where a call runs (_lib.Side): ROCm tensors stay on the device (device pointers,
torch's current stream, ROCm tensors out); NumPy arrays and CPU tensors are staged. ``model`` lends its device handle; without one a
weightless handle is used. Arguments are checked before any launch (ValueError); what only the device can see - a face index or an
``atom_residue`` out of range, a non-finite vertex score - raises PestoError. There is no CPU or PyTorch fallback.

A DELIBERATE DEPARTURE from the reference: the nearest atom is exact and in float32 - the key is the squared distance
fma(rz, rz, fma(ry, ry, rx * rx)) of the float32 differences, the smallest key wins, the lowest atom index among equal keys - where the
reference casts to float64 and asks FLANN for an APPROXIMATE neighbour (a randomised kd-tree). Areas and their sums are 64-bit integers in
units of 2^-40 (each face adds llrint(area / 3 * 2^40) to its corners), so every output is the same bits from call to call and equals the
NumPy restatement of tests/test_surface_fixture.py exactly. Not covered: binary PLY, faces that are not triangles, building the mesh itself
(MSMS / PyMesh), sample-weighted AUC.
"""
import numpy as np

from . import _lib, ranking
from .trajectory import _model_of

VERTEX_TILE = 256           # PESTO_SURFACE_VERTEX_TILE: the vertices one workgroup of the search owns
ATOM_TILE = 256             # PESTO_SURFACE_ATOM_TILE: the atoms it holds in LDS at a time
SLAB = 512                  # PESTO_SURFACE_SLAB: the atoms of one structure one workgroup walks
FIXED_ONE = 2.0 ** 40       # the areas' fixed point
IFACE_MIN_AREA = 5.0        # is_res_iface: iface_area > 5.0 and iface_area / area > 0.04
IFACE_MIN_RATIO = 0.04
INT_MAX = 2 ** 31 - 1


def _dtype_name(a):
    return str(a.dtype).replace("torch.", "")


def _array(a, name):
    if not hasattr(a, "dtype") or not hasattr(a, "shape"):
        a = np.asarray(a)
    return a


def _shape(a, name, tail, dtypes):
    """the leading length of ``a`` after the checks of its rank, its trailing axes and its type"""
    shape = tuple(int(v) for v in a.shape)
    want = "[n" + "".join(f", {t}" for t in tail) + "]"
    if len(shape) != 1 + len(tail) or shape[1:] != tuple(tail):
        raise ValueError(f"{name} must be {want}, got {list(shape)}")
    if _dtype_name(a) not in dtypes:
        raise ValueError(f"{name} must be {' or '.join(dtypes)}, got {_dtype_name(a)}")
    if shape[0] > INT_MAX:
        raise ValueError(f"{name} has {shape[0]} rows: at most 2**31 - 1")
    return shape[0]


def _offsets(offsets, total, name, may_be_empty=False):
    """int32 [S + 1] from 0 to total, strictly rising (rising, for the faces); None: one structure"""
    if offsets is None:
        if total < 1 and not may_be_empty:
            raise ValueError(f"{name}: an empty structure")
        return np.array([0, total], np.int32)
    o = _lib.host(offsets).reshape(-1)
    ok = o.size >= 2 and np.issubdtype(o.dtype, np.integer) and o[0] == 0 and o[-1] == total
    if ok:
        d = np.diff(o.astype(np.int64))
        ok = bool(np.all(d >= 0)) if may_be_empty else bool(np.all(d > 0))
    if not ok:
        raise ValueError(f"{name} must be integers rising {'' if may_be_empty else 'strictly '}from 0 to {total}")
    return np.ascontiguousarray(o, np.int32)


def _same_structures(*offs):
    if len({o.size for o in offs}) != 1:
        raise ValueError(f"the offsets describe {[o.size - 1 for o in offs]} structures")
    return offs[0].size - 1


def _flags(side, a, name, n):
    """a 0 / non-zero array (bool or an integer type) of n rows as uint8 on the call's side"""
    a = _array(a, name)
    _shape(a, name, (), ("bool", "uint8", "int8", "int16", "int32", "int64", "float32", "float64"))
    if int(a.shape[0]) != n:
        raise ValueError(f"{name} must be [{n}], got {list(a.shape)}")
    return side.put(a != 0, np.uint8)


def _call(fn, *args):
    lib = _lib.load()
    _lib.check(getattr(lib, fn)(*args), lib.pesto_surface_last_error)


# ------------------------------------------------------------------------------------------------ the kernels' entry points
def nearest_atoms(vertices, xyz, v_offsets=None, a_offsets=None, model=None, slab=None):
    """(index int32 [V], distance float32 [V]): for every vertex (float32 [V, 3]) the nearest atom (float32 [N, 3]) of its own structure, as
    its batch index, and the distance. The key is the float32 squared distance fma(rz, rz, fma(ry, ry, rx * rx)) of the float32
    differences; the smallest key wins, the lowest atom index among equal keys; distance = sqrt(key) in float32. A pair whose key is not
    finite - a NaN or infinite coordinate on either side - never matches; a vertex without a match gets index -1 and distance NaN.
    This is exact, unlike the reference (float64 coordinates, FLANN's approximate neighbour; see the module docstring).
    slab: the atoms of one structure one workgroup walks, a multiple of ATOM_TILE (default SLAB); the result does not depend on it."""
    vertices, xyz = _array(vertices, "vertices"), _array(xyz, "xyz")
    V, N = _shape(vertices, "vertices", (3,), ("float32",)), _shape(xyz, "xyz", (3,), ("float32",))
    vo, ao = _offsets(v_offsets, V, "v_offsets"), _offsets(a_offsets, N, "a_offsets")
    S = _same_structures(vo, ao)
    slab = 0 if slab is None else int(slab)
    if slab < 0 or slab % ATOM_TILE or slab > INT_MAX:
        raise ValueError(f"slab must be a positive multiple of {ATOM_TILE}, got {slab}")
    model = _model_of(model, vertices)
    side = _lib.Side(vertices, model._gpu)
    vd, xd = side.put(vertices, np.float32), side.put(xyz, np.float32)
    index, distance = side.empty((V,), np.int32), side.empty((V,), np.float32)
    _call("pesto_surface_nearest", model.handle, S, vo.ctypes.data, ao.ctypes.data, side.ptr(vd), side.ptr(xd), slab, side.ptr(index),
          side.ptr(distance), side.kind, side.stream)
    return side.result(index), side.result(distance)


def vertex_areas_fixed(vertices, faces, v_offsets=None, f_offsets=None, model=None):
    """int64 [V]: the vertex areas in units of 2^-40 - the sum over the faces at a vertex of llrint(area / 3 * 2^40) - which
    residue_surface takes. See vertex_areas."""
    vertices, faces = _array(vertices, "vertices"), _array(faces, "faces")
    V, F = _shape(vertices, "vertices", (3,), ("float32",)), _shape(faces, "faces", (3,), ("int32",))
    vo, fo = _offsets(v_offsets, V, "v_offsets"), _offsets(f_offsets, F, "f_offsets", may_be_empty=True)
    S = _same_structures(vo, fo)
    model = _model_of(model, vertices)
    side = _lib.Side(vertices, model._gpu)
    vd, fd = side.put(vertices, np.float32), side.put(faces, np.int32)
    out = side.empty((V,), np.int64)
    _call("pesto_surface_areas", model.handle, S, vo.ctypes.data, fo.ctypes.data, side.ptr(vd), side.ptr(fd) if F else None, side.ptr(out), side.kind,
          side.stream)
    return side.result(out)


def vertex_areas(vertices, faces, v_offsets=None, f_offsets=None, model=None):
    """float64 [V]: pymesh's vertex_area, a third of the area of every triangle at the vertex. faces: int32 [F, 3], vertex indices local to
    the structure. A face's area is 0.5 * sqrt(cx cx + cy cy + cz cz) of the cross product of its edge vectors (corner 1 - corner 0,
    corner 2 - corner 0), in float64 from the float32 coordinates without contraction; each face adds llrint(area / 3 * 2^40) to its
    three vertices as a 64-bit integer and the result is sum * 2^-40: the same bits on every run, whatever the order of the faces. A
    degenerate face adds 0, a vertex without a face has area 0. A face index outside its structure, or a face area that is not finite,
    raises PestoError; nothing out of range is read."""
    a = vertex_areas_fixed(vertices, faces, v_offsets, f_offsets, model)
    return a.double() / FIXED_ONE if _lib.is_torch(a) else a.astype(np.float64) / FIXED_ONE


def residue_surface(nearest, atom_residue, area_fixed, iface, vertex_score=None, v_offsets=None, a_offsets=None, r_offsets=None, model=None):
    """The residue table, a dict of arrays over the R residues of the batch:
        n_vertices int32     the vertices whose nearest atom (``nearest`` int32 [V], batch index; -1: none) lies in the residue
                             (``atom_residue`` int32 [N], local to the structure)
        area, iface_area     float64: the exact integer sums of ``area_fixed`` (int64 [V], vertex_areas_fixed) over those vertices and
                             over those with ``iface`` != 0, times 2^-40 (area_fixed, iface_area_fixed: the int64 sums themselves)
        label uint8          iface_area > 5.0 and iface_area / area > 0.04 - the notebook's is_res_iface
        max_score float32    the maximum of ``vertex_score`` (float32 [V]) over those vertices, as compute_pred_labels_per_residue takes it;
                             NaN for a residue without a vertex, -0.0 reported as +0.0; None without vertex_score
        r_offsets int32      [S + 1], on the host
    r_offsets=None with one structure: R = max(atom_residue) + 1. A non-finite vertex score raises PestoError, as ranking refuses it.
    Every value is an integer sum or an integer maximum: the same bits whatever the order the atomics land in."""
    nearest, atom_residue, area_fixed = _array(nearest, "nearest"), _array(atom_residue, "atom_residue"), _array(area_fixed, "area_fixed")
    V, N = _shape(nearest, "nearest", (), ("int32",)), _shape(atom_residue, "atom_residue", (), ("int32",))
    if _shape(area_fixed, "area_fixed", (), ("int64",)) != V:
        raise ValueError(f"area_fixed must be [{V}], got {list(area_fixed.shape)}")
    if r_offsets is None and v_offsets is None and a_offsets is None and N:
        r_offsets = [0, int(_lib.host(atom_residue).max()) + 1]
    if r_offsets is None:
        raise ValueError("a batch needs r_offsets")
    ro = _lib.host(r_offsets).reshape(-1)
    R = int(ro[-1]) if ro.size else 0
    vo, ao, ro = _offsets(v_offsets, V, "v_offsets"), _offsets(a_offsets, N, "a_offsets"), _offsets(ro, R, "r_offsets")
    S = _same_structures(vo, ao, ro)
    model = _model_of(model, nearest)
    side = _lib.Side(nearest, model._gpu)
    nd, rd, fd = side.put(nearest, np.int32), side.put(atom_residue, np.int32), side.put(area_fixed, np.int64)
    yd = _flags(side, iface, "iface", V)
    sd = None
    if vertex_score is not None:
        vertex_score = _array(vertex_score, "vertex_score")
        if _shape(vertex_score, "vertex_score", (), ("float32",)) != V:
            raise ValueError(f"vertex_score must be [{V}], got {list(vertex_score.shape)}")
        sd = side.put(vertex_score, np.float32)
    n, area, iarea, label = side.empty((R,), np.int32), side.empty((R,), np.int64), side.empty((R,), np.int64), side.empty((R,), np.uint8)
    mx = side.empty((R,), np.float32) if sd is not None else None
    _call("pesto_surface_residues", model.handle, S, vo.ctypes.data, ao.ctypes.data, ro.ctypes.data, side.ptr(nd), side.ptr(rd), side.ptr(fd),
          side.ptr(yd), side.ptr(sd), side.ptr(n), side.ptr(area), side.ptr(iarea), side.ptr(label), side.ptr(mx), side.kind, side.stream)
    n, area, iarea, label, mx = (side.result(a) for a in (n, area, iarea, label, mx))
    f64 = (lambda a: a.double() / FIXED_ONE) if _lib.is_torch(area) else (lambda a: a.astype(np.float64) / FIXED_ONE)
    return {"n_vertices": n, "area": f64(area), "iface_area": f64(iarea), "area_fixed": area, "iface_area_fixed": iarea, "label": label,
            "max_score": mx, "r_offsets": ro}


def vertex_scores(nearest, p_atom, model=None):
    """float32 [V]: p_atom[nearest] (``p_atom`` float32 [N], ``nearest`` batch indices), NaN where nearest is -1. The notebook's
    atoms[r[vi]].bfactor * alpha, with alpha applied by the caller."""
    nearest, p_atom = _array(nearest, "nearest"), _array(p_atom, "p_atom")
    V, N = _shape(nearest, "nearest", (), ("int32",)), _shape(p_atom, "p_atom", (), ("float32",))
    if V < 1 or N < 1:
        raise ValueError(f"at least one vertex and one atom, got {V} and {N}")
    model = _model_of(model, nearest)
    side = _lib.Side(nearest, model._gpu)
    nd, pd = side.put(nearest, np.int32), side.put(p_atom, np.float32)
    out = side.empty((V,), np.float32)
    _call("pesto_surface_vertex_scores", model.handle, V, N, side.ptr(nd), side.ptr(pd), side.ptr(out), side.kind, side.stream)
    return side.result(out)


def scored_residues(table, p_res, valid=None, model=None):
    """(offsets int32 [S + 1] on the host, residue int32 [K], y uint8 [K], p float32 [K]): the residues of ``table`` (residue_surface) with
    n_vertices > 0 and a valid prediction - the notebook's ``key in res_pred and key in labels_per_residue`` - compacted on the device in
    residue order: their batch index, their label and ``p_res`` (float32 [R]). valid: bool [R], None for all. A structure may come out
    empty here; ranking, and so benchmark_surfaces, refuses an empty segment."""
    n, label, ro = table["n_vertices"], table["label"], table["r_offsets"]
    R, S = int(ro[-1]), ro.size - 1
    p_res = _array(p_res, "p_res")
    if _shape(p_res, "p_res", (), ("float32",)) != R:
        raise ValueError(f"p_res must be [{R}], got {list(p_res.shape)}")
    model = _model_of(model, n)
    side = _lib.Side(n, model._gpu)
    nd, ld, pd = side.put(n, np.int32, (R,), "n_vertices"), side.put(label, np.uint8, (R,), "label"), side.put(p_res, np.float32)
    vd = None if valid is None else _flags(side, valid, "valid", R)
    off = side.empty((S + 1,), np.int64)
    res, y, p = side.empty((R,), np.int32), side.empty((R,), np.uint8), side.empty((R,), np.float32)
    sz = np.zeros(1, np.int64)
    _call("pesto_surface_scored", model.handle, S, ro.ctypes.data, side.ptr(nd), side.ptr(ld), side.ptr(pd), side.ptr(vd), R, side.ptr(off),
          side.ptr(res), side.ptr(y), side.ptr(p), sz.ctypes.data, side.kind, side.stream)
    K = int(sz[0])
    return (_lib.host(off).astype(np.int32),) + tuple(side.result(a[:K]) for a in (res, y, p))


# ------------------------------------------------------------------------------------------------ the driver
def _roc(y, p, offsets, model):
    return _lib.host(ranking.scores(y, p, offsets, model)["scores"])[:, 0, 0].astype(np.float64)


def benchmark_surfaces(items, residue_score="given", model=None):
    """What the notebook prints for one predictor over a set of chains. ``items``: one dict per structure with
        vertices float32 [V, 3], faces int32 [F, 3], iface [V] (0 / non-zero), xyz float32 [N, 3], atom_residue int32 [N]
    and, for residue_score="given" (SPPIDER, PSIVER, IntPred, PeSTo: predictions per residue, written on the atoms),
        p_atom float32 [N]         the prediction at every atom, gathered at the vertices for the per-point score
        p_res float32 [R]          the prediction of every residue, for the per-residue score; valid bool [R] (optional): which count
    or, for residue_score="max" (MaSIF's direction: predictions per vertex),
        vertex_score float32 [V]   the per-point prediction; the residue's prediction is the maximum over its vertices
    and optionally n_residues (default max(atom_residue) + 1). Returns a dict: point_auc, residue_auc float64 [S] (ROC AUC per structure,
    ranking.scores over the vertices with the flags of ``iface`` and over the scored residues with their labels), pooled_point_auc,
    pooled_residue_auc (all structures as one segment), median_point_auc, median_residue_auc, and the intermediate arrays (nearest,
    distance, area_fixed, table, offsets, residue, y, p, vertex_score, v_offsets, a_offsets). A structure without a scored residue raises ValueError: the
    reference's ``except: 0.5`` is not reproduced. The first item's vertices decide where the batch runs."""
    if residue_score not in ("given", "max"):
        raise ValueError(f'residue_score must be "given" or "max", got {residue_score!r}')
    items = list(items)
    if not items:
        raise ValueError("no structure")
    need = ["vertices", "faces", "iface", "xyz", "atom_residue"] + (["p_atom", "p_res"] if residue_score == "given" else ["vertex_score"])
    for i, it in enumerate(items):
        missing = [k for k in need if it.get(k) is None]
        if missing:
            raise ValueError(f"item {i} lacks {missing}")
    lead = items[0]["vertices"]
    model = _model_of(model, lead)
    side = _lib.Side(lead, model._gpu)
    n_res = [int(it["n_residues"]) if it.get("n_residues") is not None else int(_lib.host(it["atom_residue"]).max()) + 1 for it in items]
    vo, fo = _lib.offsets(it["vertices"].shape[0] for it in items), _lib.offsets(it["faces"].shape[0] for it in items)
    ao, ro = _lib.offsets(it["xyz"].shape[0] for it in items), _lib.offsets(n_res)
    cat = lambda key, dtype: side.cat([it[key] for it in items], dtype)          # noqa: E731
    vertices, faces, xyz, atom_res = cat("vertices", np.float32), cat("faces", np.int32), cat("xyz", np.float32), cat("atom_residue", np.int32)
    iface = side.cat([_lib.host(it["iface"]) != 0 for it in items], np.uint8)
    nearest, distance = nearest_atoms(vertices, xyz, vo, ao, model)
    area = vertex_areas_fixed(vertices, faces, vo, fo, model)
    if residue_score == "given":
        p_vertex = vertex_scores(nearest, cat("p_atom", np.float32), model)
        table = residue_surface(nearest, atom_res, area, iface, None, vo, ao, ro, model)
        for i, it in enumerate(items):
            if int(it["p_res"].shape[0]) != n_res[i]:
                raise ValueError(f"item {i}: p_res must be [{n_res[i]}], got {list(it['p_res'].shape)}")
        valid = None
        if any(it.get("valid") is not None for it in items):
            valid = np.concatenate([np.ones(n_res[i], bool) if it.get("valid") is None else _lib.host(it["valid"]) != 0 for i, it in enumerate(items)])
        p_res = cat("p_res", np.float32)
    else:
        p_vertex = cat("vertex_score", np.float32)
        table = residue_surface(nearest, atom_res, area, iface, p_vertex, vo, ao, ro, model)
        p_res, valid = table["max_score"], None
    offsets, residue, y, p = scored_residues(table, p_res, valid, model)
    empty = np.nonzero(np.diff(offsets) == 0)[0]
    if empty.size:
        raise ValueError(f"structure {int(empty[0])} has no residue with a vertex and a valid prediction")
    point = _roc(iface, p_vertex, vo, model)
    res = _roc(y, p, offsets, model)
    out = {"point_auc": point, "residue_auc": res, "pooled_point_auc": float(_roc(iface, p_vertex, None, model)[0]),
           "pooled_residue_auc": float(_roc(y, p, None, model)[0]), "median_point_auc": float(np.median(point)),
           "median_residue_auc": float(np.median(res)), "nearest": nearest, "distance": distance, "area_fixed": area, "table": table,
           "offsets": offsets, "residue": residue, "y": y, "p": p, "vertex_score": p_vertex, "v_offsets": vo, "a_offsets": ao}
    return out


# ------------------------------------------------------------------------------------------------ host I/O
def read_ply(path):
    """An ASCII PLY 1.0 mesh as PyMesh writes it: {"vertices": float32 [V, 3], "faces": int32 [F, 3], "attributes": {name: float32 [V]}}
    (every vertex property but x, y, z, in the file's order). Vertex properties must be float, the faces ``property list uchar int
    vertex_indices`` and triangles. Binary PLY, other elements and other faces are refused."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    nl = data.find(b"\n", end)
    header = data[:end].decode("ascii", "replace").splitlines()
    counts, props, element, fmt = {}, [], None, None
    for line in header[1:]:
        t = line.split()
        if not t or t[0] == "comment":
            continue
        if t[0] == "format":
            fmt = t[1:]
        elif t[0] == "element":
            element = t[1]
            if element not in ("vertex", "face") or element in counts:
                raise ValueError(f"{path}: element {element!r}: only one vertex and one face element are read")
            counts[element] = int(t[2])
        elif t[0] == "property" and element == "vertex":
            if len(t) != 3 or t[1] not in ("float", "float32"):
                raise ValueError(f"{path}: vertex property {' '.join(t[1:])!r}: only float properties are read")
            props.append(t[2])
        elif t[0] == "property" and element == "face":
            if t[1:] != ["list", "uchar", "int", "vertex_indices"] and t[1:] != ["list", "uint8", "int32", "vertex_indices"]:
                raise ValueError(f"{path}: face property {' '.join(t[1:])!r}: only 'list uchar int vertex_indices' is read")
        else:
            raise ValueError(f"{path}: header line {line!r}")
    if fmt != ["ascii", "1.0"]:
        raise ValueError(f"{path}: format {' '.join(fmt or ['?'])}: only 'ascii 1.0' is read (binary PLY is not)")
    if props[:3] != ["x", "y", "z"] or "vertex" not in counts or list(counts)[0] != "vertex":
        raise ValueError(f"{path}: the vertex element must come first, with x, y, z as its first properties")
    V, F, P = counts["vertex"], counts.get("face", 0), len(props)
    tokens = data[nl + 1:].split()
    if len(tokens) < V * P + 4 * F:
        raise ValueError(f"{path}: {len(tokens)} values for {V} vertices of {P} properties and {F} triangles")
    vert = np.array(tokens[:V * P], dtype="S").astype(np.float64).astype(np.float32).reshape(V, P) if V else np.zeros((0, P), np.float32)
    rest = tokens[V * P:]
    if F and (len(rest) != 4 * F or any(t != b"3" for t in rest[::4])):
        raise ValueError(f"{path}: a face that is not a triangle")
    faces = np.array(rest, dtype="S").astype(np.int64).reshape(F, 4)[:, 1:].astype(np.int32) if F else np.zeros((0, 3), np.int32)
    if F and (faces.min() < 0 or faces.max() >= V):
        raise ValueError(f"{path}: a face index outside [0, {V})")
    return {"vertices": np.ascontiguousarray(vert[:, :3]), "faces": np.ascontiguousarray(faces),
            "attributes": {name: np.ascontiguousarray(vert[:, 3 + k]) for k, name in enumerate(props[3:])}}


def _ply_number(v):
    """the shortest decimal that reads back as the same float32 (integers without a point, as PyMesh writes them)"""
    v = np.float32(v)
    s = np.format_float_positional(v, unique=True, trim="-") if 1e-4 <= abs(float(v)) < 1e16 or v == 0 else np.format_float_scientific(v, unique=True, trim="-")
    return s


def write_ply(path, vertices, faces, attributes=None):
    """Writes the dialect read_ply reads (ASCII PLY 1.0, float vertex properties x, y, z and one per attribute, triangles), so that a
    prediction can be painted on a MaSIF mesh. Every number is the shortest decimal that reads back as the same float32:
    read_ply(write_ply(mesh)) is the mesh bit for bit."""
    vertices = np.asarray(_lib.host(vertices), np.float32)
    faces = np.asarray(_lib.host(faces))
    attributes = {} if attributes is None else {str(k): np.asarray(_lib.host(v), np.float32).reshape(-1) for k, v in attributes.items()}
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertices must be [V, 3], got {list(vertices.shape)}")
    if faces.size == 0:
        faces = np.zeros((0, 3), np.int32)
    if faces.ndim != 2 or faces.shape[1] != 3 or not np.issubdtype(faces.dtype, np.integer):
        raise ValueError(f"faces must be integers [F, 3] (triangles), got {faces.dtype} {list(faces.shape)}")
    V = vertices.shape[0]
    if faces.size and (faces.min() < 0 or faces.max() >= V):
        raise ValueError(f"a face index outside [0, {V})")
    for k, v in attributes.items():
        if v.shape != (V,) or not k or any(c.isspace() for c in k) or k in ("x", "y", "z"):
            raise ValueError(f"attribute {k!r} must be [{V}] under a name without blanks other than x, y, z")
    cols = np.concatenate([vertices] + [v[:, None] for v in attributes.values()], axis=1)
    lines = ["ply", "format ascii 1.0", "comment Generated by pesto_amd", f"element vertex {V}"]
    lines += [f"property float {k}" for k in ["x", "y", "z"] + list(attributes)]
    lines += [f"element face {faces.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    lines += [" ".join(_ply_number(v) for v in row) for row in cols]
    lines += [f"3 {a} {b} {c}" for a, b, c in faces.tolist()]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def structure_atoms(structure):
    """The atoms of a PDB file (a path) or a structure_io.Structure, as they stand (no preprocessing): {"xyz": float32 [N, 3],
    "atom_residue": int32 [N], "bfactor": float32 [N], "ca_index": int32 [R] (the residue's first atom named CA, -1 without one),
    "n_residues": R}. Residues are consecutive runs of (chain, resid, icode, het_flag)."""
    from .structure_io import Structure
    st = Structure.read_pdb(structure) if isinstance(structure, (str, bytes)) or hasattr(structure, "__fspath__") else structure
    d = st.to_dict()
    n = len(st)
    icode = d["icode"] if "icode" in d else np.zeros(n, "U1")
    keys = [np.asarray(d["chain_name"]), np.asarray(d["resid"]), np.asarray(icode), np.asarray(d["het_flag"])]
    new = np.zeros(n, bool)
    if n:
        new[0] = True
        for k in keys:
            new[1:] |= k[1:] != k[:-1]
    atom_res = (np.cumsum(new) - 1).astype(np.int32)
    R = int(atom_res[-1]) + 1 if n else 0
    ca = np.full(R, -1, np.int32)
    is_ca = np.nonzero(np.char.strip(np.asarray(d["name"]).astype(str)) == "CA")[0]
    rows, first = np.unique(atom_res[is_ca], return_index=True)
    ca[rows] = is_ca[first].astype(np.int32)
    return {"xyz": np.ascontiguousarray(d["xyz"], np.float32), "atom_residue": atom_res, "bfactor": st.bfactor(), "ca_index": ca, "n_residues": R}


def ca_prediction(atoms, alpha=1e-2):
    """(p_atom float32 [N], p_res float32 [R], valid bool [R]) from the b-factors of structure_atoms(...): the notebook's reading of a
    predictor's PDB file. p_atom = bfactor * alpha; a residue's prediction is its CA's, valid where the residue has a CA whose b-factor is
    not negative (IntPred marks the residues it ignored with a negative one)."""
    bf, ca = np.asarray(atoms["bfactor"], np.float32), np.asarray(atoms["ca_index"])
    has = ca >= 0
    b_res = np.where(has, bf[np.where(has, ca, 0)], np.float32(-1)).astype(np.float32)
    a = np.float32(alpha)
    return (bf * a).astype(np.float32), (b_res * a).astype(np.float32), has & (b_res >= 0)
