"""Chain mapping of oligomers on the GPU: which chain of a model lies on which chain of the reference, for every frame of a run or every
decoy of a set, so that lddt, dockq and tm_score see the copies of an entity in the reference's order.

The scorers of this package score a model for a GIVEN pairing of chains, and the only pairing the package made was greedy and by
sequence (sequences.match_atoms) or by per-chain TM-score (structalign.structure_align): for a homodimer, a C4 channel or an A2B2 complex
every copy of an entity ties, so chain A went on chain A whatever the arrangement. OpenStructure's ChainMapper, DockQ v2, MM-align and
US-align solve the pairing first; this module does (pesto_chainmap.hip):
    chain_map            ChainMap(score, mapping, chain_score, n_mapped, seed, round, rotation, translation) of F frames
    apply_mapping        the model's chains gathered into the reference's chain order, NaN where unmapped: feeds lddt, tm_score, dockq
    structure_chainmap   two structures or two PDB paths: entities by sequence clustering, slots by alignment, then chain_map
    seed_pair            the (reference chain, model chain) of a seed number
Layout. xyz_ref float32 [Nr, 3] or [1, Nr, 3] holds the reference's Cr chains back to back (ref_offsets [Cr + 1], ref_group [Cr]: the
entity of every chain); xyz float32 [F, Nm, 3] are F models of one chain layout (offsets [Cm + 1], group [Cm]). All chains of a group,
on both sides, share one residue index space: they have the same length L_g and slot r is the same residue of the entity in each; a
residue a chain lacks has NaN coordinates. A group may occur on one side only: its chains stay unmapped. One point per residue,
normally CA. scale multiplies distances (the default 10 turns nanometres into angstroms). The lead argument xyz decides where a call
runs (_lib.Side): NumPy in, NumPy out; ROCm tensors in, ROCm tensors out on torch's current stream. There is no CPU or PyTorch fallback.
Arguments are checked on the host before any launch (ValueError); the library checks offsets and groups again, on the host as well (it
brings device arrays over first), and launches nothing when it refuses them.

Definition. Everything is in double from the float32 inputs.
    L_norm        the reference's residues with finite coordinates, over all chains; norm_len= overrides it
    d0            tmscore.default_d0(L_norm); d0= overrides it
    s(a, b | T)   sum_r 1 / (1 + (d_r / d0)^2) over the slots r finite in both reference chain a and model chain b (one group),
                  d_r = |T x_{b,r} - y_{a,r}| * scale
    assignment    under T, in every group with n_r reference and n_m model chains, min(n_r, n_m) pairs, every chain at most once, so
                  that the sum of s is the exact maximum (a subset DP, not a greedy choice). total(T) = the sum over the groups,
                  score(T) = total(T) / L_norm. Ties between assignments of equal sums: the lowest set of chains used on the side with
                  more chains, read as a bit mask over that side's chains of the group in their order; then, from the last chain of the
                  side with fewer chains backwards, the lowest chain of the other side that attains the sum. (No test depends on it.)
    seeds         every pair (a, b) of one group with at least 3 common finite slots; its number is a * Cm + b (seed_pair). The seed's
                  first fit is that of chain b onto chain a on the common slots (the fit of pesto_fit.h; point sets equal bit for bit are
                  fitted by the identity itself, so a model that IS its reference scores exactly 1).
    one search    up to n_iter (5; 1 .. 64) fits. For a fit, the assignment and the score: the fit is *visited*. If the mapping equals
                  that of the seed's previous fit, stop. Else the next fit is the ONE fit of all mapped chains' common slots taken
                  together (a mapping with fewer than 3 such slots ends the seed).
    score[f]      float32, rounded once: the maximum of score(T) over all visited fits of all seeds
    seed[f], round[f]   int32: the lowest seed number that attains it, and the first visit of that seed that does (from 0)
    mapping[f]    int32 [Cr]: the model chain under every reference chain at that fit, -1 for none; n_mapped[f] counts them
    chain_score[f]   float32 [Cr]: s(a, mapping[a]) / (finite slots of a), 0 where the chain is unmapped
    rotation[f], translation[f]   float64 [3, 3] and [3]: that fit as x' = x @ R + t, the convention of tm_score
A frame with an infinite coordinate, or without any seed, gets score NaN, a NaN transform, mapping, seed and round -1. An infinite
coordinate in the reference raises ValueError. Every output is bit-identical from call to call, between host and device inputs, and
between a frame scored alone and in a batch.

Not built: groups of more than 12 chains (24-mers, capsids: they need a Hungarian or greedy assignment); sequence-free mapping of
chains whose entity is unknown (structalign.py aligns such chains); more than one point per residue. (The interface-based objective,
QS-score, and the mapping that maximises it: qsscore.py.)

Limits: at most MAX_GROUP = 12 chains of a group and MAX_CHAINS = 64 chains per side, 3 <= L_g <= MAX_LENGTH = 4096, F <= 2**23,
Nr, Nm < 2**30, 1 <= n_iter <= MAX_ITER = 64. Every excess raises ValueError before any launch.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from .docking import _frames
from .trajectory import _model_of

MAX_FRAMES = 2 ** 23            # PESTO_CHAINMAP_MAX_FRAMES
MAX_CHAINS = 64                 # PESTO_CHAINMAP_MAX_CHAINS
MAX_GROUP = 12                  # PESTO_CHAINMAP_MAX_GROUP
MAX_LENGTH = 4096               # PESTO_CHAINMAP_MAX_LENGTH
MAX_ITER = 64                   # PESTO_CHAINMAP_MAX_ITER

ChainMap = namedtuple("ChainMap", "score mapping chain_score n_mapped seed round rotation translation")


def seed_pair(seed, n_model_chains):
    """(reference chain, model chain) of a seed number: seed = a * Cm + b"""
    return divmod(int(seed), int(n_model_chains))


def _offsets(offsets, N, name):
    """offsets as int64 [C + 1], C >= 1: from 0 to N (None: wherever they end) in ascending order"""
    o = np.asarray(_lib.host(offsets)).reshape(-1).astype(np.int64)
    if o.size < 2 or o[0] != 0 or (N is not None and o[-1] != N) or np.any(np.diff(o) <= 0):
        raise ValueError(f"{name}offsets must start at 0{'' if N is None else f', end at {N}'} and ascend")
    return o


def _chains(offsets, group, N, name):
    """(offsets int32 [C + 1], group int64 [C]) of one side, checked"""
    o = np.asarray(_lib.host(offsets)).reshape(-1)
    g = np.asarray(_lib.host(group)).reshape(-1)
    if not (np.issubdtype(o.dtype, np.integer) and np.issubdtype(g.dtype, np.integer)):
        raise ValueError(f"{name}offsets and {name}group must be integers")
    C = g.size
    if not 1 <= C <= MAX_CHAINS or o.size != C + 1:
        raise ValueError(f"{name}group names 1 to {MAX_CHAINS} chains and {name}offsets has one entry more, got {C} and {o.size}")
    o = _offsets(o, N, name)
    L = np.diff(o)
    if L.min() < 3 or L.max() > MAX_LENGTH:
        raise ValueError(f"{name}offsets: every chain has 3 to {MAX_LENGTH} slots, got {int(L.min())} to {int(L.max())}")
    if np.bincount(np.unique(g, return_inverse=True)[1]).max() > MAX_GROUP:
        raise ValueError(f"{name}group: at most {MAX_GROUP} chains of a group on a side")
    return o.astype(np.int32), g.astype(np.int64)


def _positive(value, name, default):
    if value is None:
        return float(default)
    v = float(value)
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"{name} must be positive and finite, got {value!r}")
    return v


def _numeric(a):
    """the module whose functions take a: torch for a tensor, NumPy for an array"""
    if _lib.is_torch(a):
        import torch
        return torch
    return np


def _oligomer(xyz_ref, ref_offsets, ref_group, xyz, offsets, group):
    """The input every oligomer entry point takes (chain_map, qsscore.qs_score, qsscore.qs_map), checked: (y [1, Nr, 3], x [F, Nm, 3],
    F, Nr, Nm, ro, rg, mo, mg) with int32 offsets and the int32 group ids numbered densely over both sides."""
    y = _frames(xyz_ref, "xyz_ref")
    if int(y.shape[0]) != 1:
        raise ValueError(f"xyz_ref must be the one reference, [Nr, 3] or [1, Nr, 3], got {int(y.shape[0])} frames")
    x = _frames(xyz, "xyz")
    F, Nr, Nm = int(x.shape[0]), int(y.shape[1]), int(x.shape[1])
    if not 1 <= F <= MAX_FRAMES or Nr >= 2 ** 30 or Nm >= 2 ** 30:
        raise ValueError(f"1 to 2**23 frames and fewer than 2**30 residues on each side, got {F} frames, {Nr} and {Nm} residues")
    ro, rg = _chains(ref_offsets, ref_group, Nr, "ref_")
    mo, mg = _chains(offsets, group, Nm, "")
    # the groups' ids, numbered densely over both sides (the library takes ids below 128)
    ids = np.unique(np.concatenate([rg, mg]), return_inverse=True)[1].astype(np.int32)
    rg, mg = np.ascontiguousarray(ids[:rg.size]), np.ascontiguousarray(ids[rg.size:])
    length = {}
    for g, L in zip(np.concatenate([rg, mg]), np.concatenate([np.diff(ro), np.diff(mo)])):
        if length.setdefault(int(g), int(L)) != int(L):
            raise ValueError(f"all chains of a group share its slots: a chain of {int(L)} slots in a group of {length[int(g)]}")
    if bool(_numeric(y).isinf(y).any()):
        raise ValueError("xyz_ref: a coordinate of the reference is infinite (a missing residue is NaN)")
    return y, x, F, Nr, Nm, ro, rg, mo, mg


def chain_map(xyz_ref, ref_offsets, ref_group, xyz, offsets, group, *, norm_len=None, d0=None, n_iter=5, scale=10.0, model=None):
    """ChainMap(score float32 [F], mapping int32 [F, Cr], chain_score float32 [F, Cr], n_mapped int32 [F], seed int32 [F], round int32 [F],
    rotation float64 [F, 3, 3], translation float64 [F, 3]) of the F models xyz against the reference: see the module's definition."""
    from .tmscore import default_d0
    y, x, F, Nr, Nm, ro, rg, mo, mg = _oligomer(xyz_ref, ref_offsets, ref_group, xyz, offsets, group)
    if isinstance(n_iter, bool) or n_iter != int(n_iter) or not 1 <= n_iter <= MAX_ITER:
        raise ValueError(f"1 <= n_iter <= {MAX_ITER} (an integer) expected, got {n_iter!r}")
    sc = _positive(scale, "scale", 10.0)
    n_finite = int(_numeric(y).isfinite(y[0]).all(1).sum())
    if norm_len is None and n_finite < 1:
        raise ValueError("xyz_ref: the reference has no residue with finite coordinates")
    ln = _positive(norm_len, "norm_len", n_finite)
    dz = _positive(d0, "d0", default_d0(ln))
    model = _model_of(model, x)
    side = _lib.Side(x, model._gpu)
    xd, yd = side.put(x, np.float32), side.put(y, np.float32)
    rod, rgd, mod, mgd = (side.put(v, np.int32) for v in (ro, rg, mo, mg))
    Cr, Cm = int(rg.size), int(mg.size)
    score, cs = side.empty((F,), np.float32), side.empty((F, Cr), np.float32)
    mapping, n_mapped, seed, rnd = side.empty((F, Cr), np.int32), side.empty((F,), np.int32), side.empty((F,), np.int32), side.empty((F,), np.int32)
    rot, tr = side.empty((F, 3, 3), np.float64), side.empty((F, 3), np.float64)
    lib = _lib.load()
    _lib.check(lib.pesto_chainmap(model.handle, F, Nr, Nm, Cr, Cm, side.ptr(rod), side.ptr(rgd), side.ptr(mod), side.ptr(mgd), side.ptr(yd), side.ptr(xd),
                                  ln, dz, int(n_iter), sc, side.ptr(score), side.ptr(mapping), side.ptr(cs), side.ptr(n_mapped), side.ptr(seed),
                                  side.ptr(rnd), side.ptr(rot), side.ptr(tr), side.kind, side.stream), lib.pesto_chainmap_last_error)
    return ChainMap(*(side.result(v) for v in (score, mapping, cs, n_mapped, seed, rnd, rot, tr)))


def apply_mapping(xyz, offsets, mapping, ref_offsets):
    """float32 [F, Nr, 3]: the model's chains gathered into the reference's chain order under ``mapping`` (int32 [Cr], or [F, Cr] with a
    row per frame, as chain_map returns it); the residues of a reference chain without a model chain are NaN. The result has the
    reference's layout and feeds lddt, tm_score and dockq unchanged. NumPy in, NumPy out; a tensor in, a tensor on its device out. A
    mapped model chain must have its reference chain's length (ValueError)."""
    x = _frames(xyz, "xyz")
    F, Nm = int(x.shape[0]), int(x.shape[1])
    mo, ro = _offsets(offsets, Nm, ""), _offsets(ref_offsets, None, "ref_")
    m = np.asarray(_lib.host(mapping)).astype(np.int64)
    m = m[None] if m.ndim == 1 else m
    Cr, Cm = ro.size - 1, mo.size - 1
    if m.ndim != 2 or m.shape[1] != Cr or m.shape[0] not in (1, F) or m.min() < -1 or m.max() >= Cm:
        raise ValueError(f"mapping must be [{Cr}] or [{F}, {Cr}] with model chains in [-1, {Cm}), got {list(m.shape)}")
    Lr, Lm = np.diff(ro), np.diff(mo)
    if np.any((m >= 0) & (Lm[np.maximum(m, 0)] != Lr[None])):
        raise ValueError("a mapped model chain must have as many slots as its reference chain")
    chain = np.repeat(np.arange(Cr), Lr)
    slot = np.arange(int(ro[-1])) - ro[chain]
    mc = m[:, chain]                                    # [1 or F, Nr]: the model chain of every reference residue
    idx = np.where(mc >= 0, mo[np.maximum(mc, 0)] + slot[None], -1)
    idx = np.broadcast_to(idx, (F, idx.shape[1]))
    if _lib.is_torch(x):
        import torch
        it = torch.from_numpy(np.ascontiguousarray(idx)).to(x.device)
        out = torch.gather(x.to(torch.float32), 1, it.clamp(min=0)[:, :, None].expand(-1, -1, 3)).clone()
        out[it < 0] = float("nan")
        return out
    out = np.asarray(x, np.float32)[np.arange(F)[:, None], np.maximum(idx, 0)]
    out[idx < 0] = np.nan
    return out


def structure_chainmap(reference, predicted, min_identity=0.9, model=None, **kw):
    """(ChainMap, chains, match): the chains of the structure ``predicted`` mapped onto those of ``reference``. Each is a PDB path, a
    structure_io.Structure or a structure dict, in angstroms (scale 1). The protein chains of both (sequences.structure_sequences) are
    grouped into entities by ONE cluster_sequences call over their union (min_identity); the representative of a group is its longest
    reference chain (the lowest index on ties) and every chain of the group is put on the representative's residues, the slots, by ONE
    align_maps call (mode "overlap"); the same call aligns the other chains of a group with each other, and a residue that the
    representative lacks gets a further slot, behind the representative's, which it shares with the residues it is aligned to in those
    chains: no residue is lost to the slots. Groups without a reference chain, and groups whose representative has fewer than 3 residues, are
    left out. The points are the CA atoms (structalign.ca_traces). ChainMap is chain_map's result for the one model (F = 1) over the
    chains kept, ``chains`` the (reference chain, model chain) names of the mapped pairs in the reference's order, and ``match`` is
    sequences.match_atoms' five results with the residues paired by the slots under the found mapping: lddt.lddt, tmscore.tm_score and
    dockq take it directly."""
    from .lddt import _structure_dict
    from .structalign import ca_traces
    if "scale" in kw:
        raise ValueError("structure_chainmap works in angstroms: scale is not taken")
    a, b = _structure_dict(reference), _structure_dict(predicted)
    ta, tb = ca_traces(a), ca_traces(b)
    if not ta or not tb:
        raise ValueError("each structure needs a protein chain")
    kept_a, kept_b, side_arrays, result_of = _entity_slots(a, b, ta, tb, min_identity, model)
    ya, ro, rg = side_arrays(kept_a, ta, 0)
    xb, mo, mg = side_arrays(kept_b, tb, len(ta))
    out = chain_map(ya, ro, rg, xb[None], mo, mg, scale=1.0, model=model, **kw)
    chains, match = result_of(np.asarray(_lib.host(out.mapping))[0])
    return out, chains, match


def _entity_slots(a, b, ta, tb, min_identity, model):
    """The entities and slots of two structure dicts a (the reference) and b, as structure_chainmap states them, from their per-chain
    traces ta and tb (structalign.ca_traces, or any list of the same residues such as qsscore.interface_points). Returns (kept_a, kept_b,
    side_arrays, result_of): the chains of either side that belong to a kept entity (indices into ta and tb); side_arrays(chains,
    traces, base) -> (xyz float32 [N, 3] with NaN where a chain lacks a slot, offsets int32, group int64) of one side's kept chains
    (base 0 for the reference, len(ta) for the model) with the points of ``traces``; result_of(mapping) -> (chains, match) of a
    mapping over the kept chains: the names of the mapped pairs and sequences.match_atoms' five results."""
    from .sequences import _matched, align_maps, cluster_sequences
    na = len(ta)
    seqs = [t[2] for t in ta + tb]
    labels = np.asarray(_lib.host(cluster_sequences(seqs, min_identity=min_identity, model=model))).astype(np.int64)
    rep = {}
    for i in range(na):                                 # the longest reference chain of every group, the lowest index on ties
        g = int(labels[i])
        if g not in rep or len(seqs[i]) > len(seqs[rep[g]]):
            rep[g] = i
    rep = {g: i for g, i in rep.items() if len(seqs[i]) >= 3}
    kept = [i for i in range(len(seqs)) if int(labels[i]) in rep]
    kept_b = [i - na for i in kept if i >= na]
    if not kept_b:
        raise ValueError("no chain of the model belongs to an entity of the reference")
    kept_a = [i for i in kept if i < na]
    slots = {i: np.arange(len(seqs[i]), dtype=np.int32) for i in rep.values()}                  # the slot of every residue, or -1
    others = [i for i in kept if i not in slots]
    n_slots = {g: len(seqs[i]) for g, i in rep.items()}
    if others:
        # the one align_maps call: every other chain against its representative, then the other chains of a group among themselves
        among = [(i, j) for x, i in enumerate(others) for j in others[x + 1:] if labels[i] == labels[j]]
        mp = align_maps(seqs, np.array([(i, rep[int(labels[i])]) for i in others] + among, np.int32), mode="overlap", model=model)
        amap = np.asarray(_lib.host(mp.map))
        rows = [amap[mp.map_offsets[q]:mp.map_offsets[q + 1]] for q in range(len(others) + len(among))]
        slots.update({i: rows[q].copy() for q, i in enumerate(others)})
        # A residue that the representative lacks gets a slot behind the representative's, shared with the residues of the other chains
        # it is aligned to (classes of a union-find that never joins two residues of one chain), so no residue is lost to the slots.
        root, chains_of = {}, {}

        def find(k):
            while root[k] != k:
                root[k] = root[root[k]]
                k = root[k]
            return k
        for i in others:
            for r in np.nonzero(slots[i] < 0)[0]:
                root[(i, int(r))] = (i, int(r))
                chains_of[(i, int(r))] = {i}
        for (i, j), row in zip(among, rows[len(others):]):
            for r in np.nonzero((slots[i] < 0) & (row >= 0))[0]:
                if slots[j][row[r]] < 0:
                    p, q = find((i, int(r))), find((j, int(row[r])))
                    if p != q and not chains_of[p] & chains_of[q]:
                        root[q] = p
                        chains_of[p] |= chains_of.pop(q)
        slot_of = {}
        for k in sorted(root):                          # (chain, residue) ascending: the classes' slots in the order of their first members
            p = find(k)
            if p not in slot_of:
                g = int(labels[k[0]])
                slot_of[p] = n_slots[g]
                n_slots[g] += 1
            slots[k[0]][k[1]] = slot_of[p]

    def side_arrays(chains, traces, base):
        sizes = [n_slots[int(labels[base + c])] for c in chains]
        offs = _lib.offsets(sizes)
        xyz = np.full((int(offs[-1]), 3), np.nan, np.float32)
        for k, c in enumerate(chains):
            s = slots[base + c]
            xyz[offs[k] + s[s >= 0]] = traces[c][1][s >= 0]
        return xyz, offs, np.array([labels[base + c] for c in chains], np.int64)

    def result_of(mapping):
        mapped = [(kept_a[k], kept_b[int(j)]) for k, j in enumerate(mapping) if j >= 0]

        def partner_of(da, db, fa, fb):
            row_a = {int(f): r for r, f in enumerate(fa)}
            row_b = {int(f): r for r, f in enumerate(fb)}
            partner = np.full(fa.size, -1, np.int64)
            for i, j in mapped:
                sa, sb = slots[i], slots[na + j]
                of_slot = {int(s): q for q, s in enumerate(sb) if s >= 0}
                for r, s in enumerate(sa):
                    q = of_slot.get(int(s), -1) if s >= 0 else -1
                    if q >= 0:
                        partner[row_a[int(ta[i][3][r])]] = row_b[int(tb[j][3][q])]
            return partner
        match = _matched(a, b, model, partner_of)[:5]
        return [(ta[i][0], tb[j][0]) for i, j in mapped], match
    return kept_a, kept_b, side_arrays, result_of
