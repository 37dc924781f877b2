"""Structure-based alignment of CA traces on the GPU: the residue correspondence of two chains and the superposition that goes with it,
found together (pesto_structalign.hip).

The package could score a model against a reference only when it already knew which residue pairs with which: from residue numbers
(lddt.structure_lddt, tmscore.structure_tmscore) or from a sequence alignment (sequences.match_atoms). Two proteins of one fold with
little sequence identity, a chain and a homologue, the two halves of a duplicated domain could not be compared at all. Structural
alignment is the alternation of the two halves the package has: under a superposition, the dynamic programme of sequences.py over scores
made of inter-residue distances gives an alignment; the TM-score search of tmscore.py on the aligned pairs gives the next superposition.
    align_structures     StructAlign(map, map_offsets, n_aligned, n_ident, dp_score, unit, round, tm_a, tm_b, rotation, translation, rmsd,
                         history) of P pairs of chains
    tm_matrix            all against all: float32 [S, S], entry (i, j) normalised by the length of j; 1 - min(T, T.T) feeds
                         clustering.gromos_clusters
    ca_traces            the CA trace and the codes of every protein chain of a structure
    structure_align      two structures or PDB paths, chain by chain, with an atom match that lddt.lddt and tmscore.tm_score take unchanged
coords holds the float32 CA coordinates of S structures back to back (or is a list of [L, 3] arrays; then sizes is not given), sizes
their lengths; a pair (a, b) moves a of m residues onto b of n residues. scale multiplies distances (the default 10 turns nanometres
into angstroms). The lead argument decides where a call runs (_lib.Side): NumPy in, NumPy out; ROCm tensors in, ROCm tensors out on torch's
current stream. sizes, pairs and init are read on the host. There is no CPU or PyTorch fallback; arguments are checked on the host before
any launch (ValueError).

Definition (our own, stated in full; no equality with the TM-align program is claimed). Per pair: Lmin = min(m, n), d0s =
tmscore.default_d0(Lmin), Q = 1024.
    cell score     under a transform (R, t), in double from the float32 inputs: x'_i = x_i R + t, u = |x'_i - y_j|^2 scale^2 / d0s^2,
                   s_ij = int32(floor(Q / (1 + u) + 0.5))
    DP(R, t, g)    the recursion, the ties D, U, L, the end rule and the canonical path of sequences.py in "overlap" mode, with s_ij in the
                   place of matrix[a[i-1]][b[j-1]], gap_open = g and gap_extend = 0; integer throughout: a map, its score, its n_aligned
    I1, threading  every offset k (a_i on b_(i+k)) whose overlap has at least max(3, ceil(Lmin / 2)) residues: one Kabsch fit of the
                   overlap (the fit of tmscore.py, as x' = x R + t), the sum of s over the overlap under it; the largest sum wins, ties to
                   the smallest k; the alignment is the overlap itself
    I2, fragments  f = min(Lmin, max(4, min(20, Lmin // 3))); starts in each chain 0, stride, 2 stride, ... <= len - f, plus len - f, with
                   stride = max(1, ceil((len - f) / (frag_starts - 1))); for every pair of fragments the fit of a's onto b's and the score
                   of DP(fit, 0) of the whole chains; the largest score wins, ties to the lowest (start in a, start in b); the alignment
                   is the map of that DP
    I3             the caller's init map, if given (for example sequences.align_maps')
    units          (initial alignment i, gap g) with g = round(gap_open Q), then 0: unit 2 i + (1 if g is the zero gap else 0); 4 or 6 a pair.
                   A unit whose alignment has fewer than 3 pairs is dead.
    a round        a live unit (1) searches: tm_score on its aligned pairs, a's residues onto b's, norm_len = Lmin, d0 = d0s, step = max(1,
                   n_aligned >> 3): tm_r (float32), R, t; (2) runs DP(R, t, its gap): the new map; (3) is done if the new map equals the
                   old one (integer compare), dead if it aligns fewer than 3 pairs. All units run up to ``rounds`` rounds.
    result         the alignment SEARCHED in the (unit, round) with the largest tm_r, ties to the lowest (unit, round)
    map            int32 [sum of m]: the index in b or -1; map_offsets int64 [P + 1] (host) says where a pair's rows begin
    n_aligned, n_ident (aligned pairs with equal codes; 0 without codes), dp_score (the score of the winning round's DP), unit, round
    tm_a, tm_b     float32: the winning pairs scored by tm_score at step 1, normalised by m with d0(m) and by n with d0(n): bit for bit
                   tmscore.tm_score called by hand on the gathered pairs; rmsd likewise
    rotation, translation   float64: those of the search normalised by the shorter chain (with m = n, tm_a's): x' = x @ R + t
    history        float64 [P, units, rounds, 3] = (tm_r, the score of the round's DP, n_aligned of the alignment searched); NaN where a
                   unit did not run: convergence is read from it
No unit ever alive: tm 0, n_aligned 0, map -1, the identity transform, rmsd NaN, unit and round -1. A non-finite coordinate in either
chain: NaN scores and transform, map -1, unit -1. Every output is bit-identical from call to call and between host and device inputs.

Not built: secondary-structure initial alignments, TM-align's distance trimming before the final search, circular permutation, multiple
structure alignment, nucleic acids, a device-resident round loop (the host reads 8 bytes a unit once per round). The chain permutation
of an oligomer whose entities are known is chainmap.py's.

Limits: 3 <= length <= MAX_LENGTH = 4096, P <= 2**20, rounds <= 64, 2 <= frag_starts <= 64, 0 <= gap_open <= 1. Every excess raises
ValueError.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from .tmscore import default_d0
from .trajectory import _model_of

Q = 1024                        # PESTO_STRUCTALIGN_Q
MIN_LENGTH = 3                  # PESTO_STRUCTALIGN_MIN_LENGTH
MAX_LENGTH = 4096               # PESTO_STRUCTALIGN_MAX_LENGTH
MAX_PAIRS = 2 ** 20             # PESTO_STRUCTALIGN_MAX_PAIRS
MAX_ROUNDS = 64                 # PESTO_STRUCTALIGN_MAX_ROUNDS
MIN_FRAG_STARTS, MAX_FRAG_STARTS = 2, 64

StructAlign = namedtuple("StructAlign", "map map_offsets n_aligned n_ident dp_score unit round tm_a tm_b rotation translation rmsd history")


def _int(value, lo, hi, name):
    if isinstance(value, bool) or value != int(value) or not lo <= value <= hi:
        raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {value!r}")
    return int(value)


def _layout(coords, sizes):
    """(coords [N, 3] as given or concatenated on the lead's side, sizes list)"""
    if isinstance(coords, (list, tuple)):
        if sizes is not None:
            raise ValueError("a list of traces brings its own sizes")
        parts = list(coords)
        if not parts:
            raise ValueError("no structures")
        sizes = [int(p.shape[0]) for p in parts]
        if _lib.is_torch(parts[0]):
            import torch
            coords = torch.cat([p.reshape(-1, 3) for p in parts])
        else:
            coords = np.concatenate([np.asarray(p).reshape(-1, 3) for p in parts])
    else:
        if sizes is None:
            raise ValueError("sizes: the lengths of the structures in coords")
        sizes = [int(v) for v in np.asarray(_lib.host(sizes)).reshape(-1)]
    if len(coords.shape) != 2 or coords.shape[1] != 3:
        raise ValueError(f"coords must be [N, 3], got {list(coords.shape)}")
    if not sizes or sum(sizes) != int(coords.shape[0]):
        raise ValueError(f"sizes must add up to {int(coords.shape[0])} residues")
    if min(sizes) < MIN_LENGTH or max(sizes) > MAX_LENGTH:
        raise ValueError(f"every structure must have {MIN_LENGTH} to {MAX_LENGTH} residues, got {min(sizes)} .. {max(sizes)}")
    return coords, sizes


def align_structures(coords, sizes=None, pairs=None, *, codes=None, init=None, gap_open=0.6, rounds=20, frag_starts=16, scale=10.0, model=None):
    """StructAlign of the listed pairs (int32 [P, 2]; None: all i < j in row-major order): see the module's definition. codes uint8 [N]:
    residue codes, for n_ident; init: one initial map per pair (a list of int arrays of length m, or their concatenation)."""
    coords, sizes = _layout(coords, sizes)
    S = len(sizes)
    if pairs is None:
        pairs = np.array([(i, j) for i in range(S) for j in range(i + 1, S)], np.int32).reshape(-1, 2)
    pairs = np.ascontiguousarray(np.asarray(_lib.host(pairs)).reshape(-1, 2))
    if not np.issubdtype(pairs.dtype, np.integer):
        raise ValueError("pairs must hold integers")
    P = pairs.shape[0]
    if not 1 <= P <= MAX_PAIRS:
        raise ValueError(f"1 to {MAX_PAIRS} pairs, got {P}")
    if pairs.min() < 0 or pairs.max() >= S:
        raise ValueError(f"pairs must name structures 0 .. {S - 1}")
    pairs = pairs.astype(np.int32)
    go = float(gap_open)
    if not 0.0 <= go <= 1.0:
        raise ValueError(f"0 <= gap_open <= 1 expected, got {gap_open!r}")
    rounds = _int(rounds, 1, MAX_ROUNDS, "rounds")
    frag_starts = _int(frag_starts, MIN_FRAG_STARTS, MAX_FRAG_STARTS, "frag_starts")
    sc = float(scale)
    if not (np.isfinite(sc) and sc > 0):
        raise ValueError(f"scale must be positive and finite, got {scale!r}")
    lens = np.asarray(sizes, np.int64)
    m, n = lens[pairs[:, 0]], lens[pairs[:, 1]]
    moff = np.zeros(P + 1, np.int64)
    moff[1:] = np.cumsum(m)
    if init is not None:
        if isinstance(init, (list, tuple)):
            init = np.concatenate([np.asarray(_lib.host(v)).reshape(-1) for v in init]) if len(init) else np.zeros(0)
        init = np.asarray(_lib.host(init)).reshape(-1)
        if init.size != moff[-1] or not np.issubdtype(init.dtype, np.integer):
            raise ValueError(f"init must hold one integer map per pair, {int(moff[-1])} entries in all, got {init.size}")
        if init.size and (init.min() < -1 or np.any(init >= np.repeat(n, m))):
            raise ValueError("init: an entry is -1 or an index of b")
        for p in range(P):
            hit = init[moff[p]:moff[p + 1]]
            if np.any(np.diff(hit[hit >= 0]) <= 0):
                raise ValueError(f"init: the aligned residues of pair {p} must map to ascending indices of b")
        init = np.ascontiguousarray(init, np.int32)
    d0 = np.ascontiguousarray(np.stack([default_d0(np.minimum(m, n)), default_d0(m), default_d0(n)], 1), np.float64)
    offs = _lib.offsets(sizes)
    if codes is not None and tuple(codes.shape if hasattr(codes, "shape") else np.shape(codes)) != (int(offs[-1]),):
        raise ValueError(f"codes must be [{int(offs[-1])}]")
    model = _model_of(model, coords)
    side = _lib.Side(coords, model._gpu)
    xd = side.put(coords, np.float32)
    cd = None
    if codes is not None:
        cd = side.put(codes, np.uint8)
    NU = 6 if init is not None else 4
    amap = side.empty((int(moff[-1]),), np.int32)
    na, ni, ds, un, ro = (side.empty((P,), np.int32) for _ in range(5))
    tm, rot, tr = side.empty((P, 2), np.float32), side.empty((P, 3, 3), np.float64), side.empty((P, 3), np.float64)
    rmsd, hist = side.empty((P,), np.float32), side.empty((P, NU, rounds, 3), np.float64)
    lib = _lib.load()
    _lib.check(lib.pesto_structalign(model.handle, S, offs.ctypes.data, side.ptr(xd), side.ptr(cd), P, pairs.ctypes.data,
                                     None if init is None else init.ctypes.data, d0.ctypes.data, go, rounds, frag_starts, sc, side.ptr(amap),
                                     side.ptr(na), side.ptr(ni), side.ptr(ds), side.ptr(un), side.ptr(ro), side.ptr(tm), side.ptr(rot), side.ptr(tr),
                                     side.ptr(rmsd), side.ptr(hist), side.kind, side.stream), lib.pesto_structalign_last_error)
    r = side.result
    return StructAlign(r(amap), moff, r(na), r(ni), r(ds), r(un), r(ro), r(tm)[:, 0], r(tm)[:, 1], r(rot), r(tr), r(rmsd), r(hist))


def tm_matrix(coords, sizes=None, **kw):
    """float32 [S, S] (on the lead's side): the structures aligned all against all; entry (i, j) is the TM-score of the pair normalised
    by the length of j, the diagonal 1. D = 1 - min(T, T.T) is a symmetric distance for clustering.gromos_clusters."""
    coords, sizes = _layout(coords, sizes)
    S = len(sizes)
    if S < 2:
        raise ValueError("a matrix needs at least two structures")
    if "pairs" in kw or "init" in kw:
        raise ValueError("tm_matrix aligns all pairs itself: pairs and init are not taken")
    out = align_structures(coords, sizes, None, **kw)
    iu = np.triu_indices(S, 1)
    if _lib.is_torch(out.tm_a):
        import torch
        T = torch.eye(S, dtype=torch.float32, device=out.tm_a.device)
        i, j = (torch.from_numpy(v).to(T.device) for v in iu)
    else:
        T = np.eye(S, dtype=np.float32)
        i, j = iu
    T[i, j] = out.tm_b          # the pair (i, j) moves i onto j: tm_b is normalised by j's length
    T[j, i] = out.tm_a
    return T


def ca_traces(structure):
    """[(chain_name, xyz float32 [R_c, 3], codes uint8 [R_c], first-atom index of each residue int64 [R_c])] per protein chain of a
    structure (whatever lddt.structure_lddt takes), in the order of first appearance: the residues sequences.structure_sequences lists,
    each with the coordinates of its (first) CA atom, in the structure's own unit (angstroms for a PDB file: scale 1)."""
    from .lddt import _structure_dict
    from .sequences import structure_sequences
    d = _structure_dict(structure)
    xyz = np.asarray(d["xyz"], np.float32).reshape(-1, 3)
    is_ca = np.char.strip(np.asarray(d["name"]).astype(str)) == "CA"
    ca_at = np.nonzero(is_ca)[0]
    out = []
    for chain, codes, first in structure_sequences(d):
        at = ca_at[np.searchsorted(ca_at, first, "left")]       # the first CA at or after a residue's first atom: its own
        out.append((chain, np.ascontiguousarray(xyz[at]), codes, first))
    return out


def structure_align(reference, predicted, model=None, **kw):
    """(StructAlign, chains, match): ``predicted`` aligned onto ``reference`` by structure, chain by chain. Each is a PDB path, a
    structure_io.Structure, a structure dict or a dict of subunits, in angstroms (scale 1). Every protein chain of the model (a) is
    aligned with every protein chain of the reference (b) in one align_structures call; chains are paired greedily by descending tm_b
    (normalised by the reference chain), then ascending (reference chain, model chain), each chain once, and a pairing is kept with
    n_aligned >= 3. StructAlign holds the kept pairs, ``chains`` their (reference chain, model chain) names in the same order, and
    ``match`` is sequences.match_atoms' five results with the residues paired by these alignments, for lddt.lddt and tmscore.tm_score."""
    from .sequences import _matched
    if "scale" in kw or "pairs" in kw or "init" in kw:
        raise ValueError("structure_align lists the chain pairs itself, in angstroms: scale, pairs and init are not taken")
    ta, tb = ca_traces(predicted), ca_traces(reference)
    ta, tb = [t for t in ta if len(t[2]) >= MIN_LENGTH], [t for t in tb if len(t[2]) >= MIN_LENGTH]
    if not ta or not tb:
        raise ValueError("each structure needs a protein chain of at least 3 residues")
    na = len(ta)
    coords = np.concatenate([t[1] for t in ta + tb])
    codes = np.concatenate([t[2] for t in ta + tb])
    sizes = [len(t[2]) for t in ta + tb]
    pairs = np.array([(i, na + j) for j in range(len(tb)) for i in range(na)], np.int32)
    out = align_structures(coords, sizes, pairs, codes=codes, scale=1.0, model=model, **kw)
    tm_b, aligned = np.asarray(out.tm_b, np.float64), np.asarray(out.n_aligned)
    order = np.lexsort((pairs[:, 0], pairs[:, 1], -np.nan_to_num(tm_b, nan=-1.0)))
    used_a, used_b, chosen = set(), set(), []
    for p in order:
        i, j = int(pairs[p, 0]), int(pairs[p, 1])
        if i in used_a or j in used_b or aligned[p] < 3:
            continue
        used_a.add(i)
        used_b.add(j)
        chosen.append(int(p))
    chosen = sorted(chosen)

    def partner_of(a, b, fa, fb):
        row_a = {int(f): r for r, f in enumerate(fa)}           # (a: the reference's dict here, as in sequences._matched)
        row_b = {int(f): r for r, f in enumerate(fb)}
        partner = np.full(fa.size, -1, np.int64)
        for p in chosen:
            i, j = int(pairs[p, 0]), int(pairs[p, 1]) - na
            rows = out.map[out.map_offsets[p]:out.map_offsets[p + 1]]
            hit = np.nonzero(rows >= 0)[0]
            ref_rows = np.array([row_a[int(f)] for f in tb[j][3][rows[hit]]], np.int64)
            partner[ref_rows] = [row_b[int(f)] for f in ta[i][3][hit]]
        return partner
    match = _matched(reference, predicted, model, partner_of)[:5]
    sel = np.array(chosen, np.int64)
    moff = np.zeros(sel.size + 1, np.int64)
    lens = np.diff(out.map_offsets)[sel]
    moff[1:] = np.cumsum(lens)
    amap = np.concatenate([out.map[out.map_offsets[p]:out.map_offsets[p + 1]] for p in chosen]) if chosen else np.zeros(0, np.int32)
    kept = StructAlign(amap, moff, *(np.asarray(v)[sel] for v in out[2:]))
    return kept, [(tb[int(pairs[p, 1]) - na][0], ta[int(pairs[p, 0])][0]) for p in chosen], match
