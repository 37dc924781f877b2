"""QS-score and the interface contact score of assemblies on the GPU, for a given chain mapping or for the mapping that maximises it,
over every frame of a run or every decoy of a set in one call.

lddt, tmscore and dockq score residues, folds and two-body docking; chainmap pairs the chains of an oligomer by a TM-like sum under
rigid superpositions, an objective that cannot see what matters most at interfaces: a model whose chains are all well placed but which
contacts the wrong copy, or whose interface has slid, keeps a high TM sum. QS-score (Bertoni et al. 2017) asks whether the right
residues of the right chains are in contact, needs no superposition, is what OpenStructure and CASP's assembly category report beside
lDDT, and is the objective OpenStructure's chain mapper maximises. This module has (pesto_qsscore.hip):
    qs_score             QSScore(qs_best, qs_global, ics, ics_precision, ics_recall, counts, interface_qs) of F frames under a mapping
    qs_map               QSMap(mapping, n_mapped, index, n_mappings, + the QSScore fields): the mapping of the largest qs_global,
                         exactly, by enumeration of all mappings over one table of chain-pair terms per frame
    n_mappings           how many mappings qs_map enumerates; mapping_of_index: the mapping of a number of the enumeration
    interface_points     CB, or CA where a residue has no CB, of every protein residue of a structure
    structure_qsscore    two structures or two PDB paths: entities and slots as chainmap.structure_chainmap builds them, then the above
Layout. That of chainmap: xyz_ref float32 [Nr, 3] or [1, Nr, 3] holds the reference's Cr chains back to back (ref_offsets [Cr + 1],
ref_group [Cr]); xyz float32 [F, Nm, 3] are F models of one chain layout (offsets [Cm + 1], group [Cm]). All chains of a group, on both
sides, share one residue index space of L_g slots; a residue a chain lacks has NaN coordinates. One point per residue: CB, with CA for
glycine or where CB is missing (interface_points). scale multiplies distances (the default 10 turns nanometres into angstroms). The
lead argument xyz decides where a call runs (_lib.Side): NumPy in, NumPy out; ROCm tensors in, ROCm tensors out on torch's current
stream. There is no CPU or PyTorch fallback. Arguments are checked on the host before any launch (ValueError); a mapping with a row per
frame is checked by a kernel whose verdict is read before anything is written.

Definition (ours, after Bertoni et al. 2017 in the form OpenStructure states it; no equality with OpenStructure is claimed).
Everything is in double from the float32 inputs.
    w(d)          1 for d <= 5; exp(-2 ((d - 5) / 4.28)^2) for 5 < d < 12; 0 for d >= 12 (angstroms after scale)
    mapping       m[a] = the model chain under reference chain a, or -1; one to one, chains of one group only. A reference interface
                  (a, a'), a < a', is mapped if both chains are: b = m[a], b' = m[a'].
    common        a slot pair (r, s) of a mapped interface with y[a,r], y[a',s], x[b,r] and x[b',s] all finite;
                  d1 = |y[a,r] - y[a',s]| scale, d2 = |x[b,r] - x[b',s]| scale
    terms         of a mapped interface, summed over its common slot pairs:
                  num     w(min(d1, d2)) (1 - |d1 - d2| / 12)    where d1 < 12 and d2 < 12
                  shared  w(min(d1, d2))                         the same pairs
                  extra   w of the one distance below 12         where exactly one of d1, d2 is below 12
                  mref    w(d1) where d1 < 12;  mmdl  w(d2) where d2 < 12
    Wref, Wmdl[f] the sum of w(d) over ALL chain pairs of the reference (of frame f) and all their slot pairs finite on that side
    qs_best       sum num / sum (shared + extra) over the mapped interfaces
    qs_global     sum num / (sum (shared + extra) + (Wref - sum mref) + (Wmdl - sum mmdl)): contacts of chains that are not mapped, or of
                  residues the other side lacks, count against the model
    interface_qs  [a, a'] = num / (shared + extra) of one mapped interface; symmetric, NaN on the diagonal and where not mapped
    ICS           a contact is d < contact_thr (8 A on these points). n_ref, n_model: the inter-chain contacts of the reference, of the
                  frame; n_shared: the common slot pairs of mapped interfaces in contact on both sides. ics_precision = n_shared /
                  n_model, ics_recall = n_shared / n_ref, ics = 2 n_shared / (n_ref + n_model). counts = (n_ref, n_model, n_shared), exact.
A denominator that is not positive gives NaN. A frame with an infinite coordinate gets NaN scores and counts of -1 (qs_map: mapping -1,
n_mapped 0, index -1); an infinite coordinate in the reference raises ValueError. Every sum has one order (the slot pairs of a lane, the
wave's butterfly, the waves, the blocks of 64 slots, the interfaces in ascending (a, a')) and no result is accumulated with atomics:
every output is bit-identical from call to call, between host and device inputs, and between a frame alone and in a batch.

qs_map maximises qs_global over ALL mappings that map min(n_r, n_m) chains in every group present on both sides; ties go to the larger
qs_best, then to the lowest index of the enumeration (mapping_of_index states the order; no test depends on it). A frame where no
mapping has a qs_global gets mapping -1 and NaN scores. Its scores are bit-equal to qs_score's for the mapping it returns.

Not built: more than MAX_MAPPINGS = 2**20 mappings (qs_map raises ValueError: nine copies of one entity, A6B6 and A4B4C4 fit; beyond,
chainmap.chain_map finds a mapping and qs_score scores it); heuristic QS mapping of large assemblies; more than one point per residue;
per-residue contact tables.

Limits: those of chainmap (MAX_CHAINS = 64 chains per side, MAX_GROUP = 12 of a group, 3 <= L_g <= 4096, F <= 2**23, Nr, Nm < 2**30).
"""
from collections import namedtuple

import numpy as np

from . import _lib
from .chainmap import _oligomer, _positive
from .trajectory import _model_of

MAX_MAPPINGS = 2 ** 20          # PESTO_QSSCORE_MAX_MAPPINGS

QSScore = namedtuple("QSScore", "qs_best qs_global ics ics_precision ics_recall counts interface_qs")
QSMap = namedtuple("QSMap", "mapping n_mapped index n_mappings qs_best qs_global ics ics_precision ics_recall counts interface_qs")


def _group_lists(ref_group, group):
    """[(reference chains, model chains)] of the groups present on both sides, in ascending group id"""
    rg, mg = np.asarray(_lib.host(ref_group)).reshape(-1), np.asarray(_lib.host(group)).reshape(-1)
    return [(np.nonzero(rg == g)[0], np.nonzero(mg == g)[0]) for g in np.intersect1d(rg, mg)]


def n_mappings(ref_group, group):
    """The number of mappings qs_map enumerates: the product over the groups present on both sides of max! / (max - min)!, for n_r
    reference and n_m model chains of the group (a Python int; 1 where no group is shared: the one mapping that maps nothing)."""
    n = 1
    for ra, mb in _group_lists(ref_group, group):
        few, many = sorted((len(ra), len(mb)))
        for k in range(few):
            n *= many - k
    return n


def mapping_of_index(index, ref_group, group):
    """int64 [Cr]: mapping number ``index`` of qs_map's enumeration. The index is a mixed-radix number over the groups present on both
    sides, the lowest group id the least significant digit. A group's digit is again mixed-radix, over the chains of its side with fewer
    chains (the reference's on a tie), the first of them the least significant: the digit q of the k-th of them, in [0, max - k), picks
    the q-th chain, in ascending order, of the other side that is still free."""
    index = int(index)
    if not 0 <= index < n_mappings(ref_group, group):
        raise ValueError(f"index must lie in [0, {n_mappings(ref_group, group)}), got {index}")
    m = -np.ones(np.asarray(_lib.host(ref_group)).size, np.int64)
    for ra, mb in _group_lists(ref_group, group):
        few, many = sorted((len(ra), len(mb)))
        radix = 1
        for k in range(few):
            radix *= many - k
        index, d = divmod(index, radix)
        free = list(range(many))
        for k in range(few):
            d, q = divmod(d, many - k)
            c = free.pop(q)
            if len(ra) <= len(mb):
                m[ra[k]] = mb[c]
            else:
                m[ra[c]] = mb[k]
    return m


def _layout(xyz_ref, ref_offsets, ref_group, xyz, offsets, group, contact_thr, scale):
    """the checked arguments both entry points share: (y, x, F, Nr, Nm, ro, rg, mo, mg, contact_thr, scale)"""
    lay = _oligomer(xyz_ref, ref_offsets, ref_group, xyz, offsets, group)
    sc = _positive(scale, "scale", 10.0)
    return (*lay, _positive(contact_thr, "contact_thr", 8.0), sc)


def _check_mapping(m, rg, mg):
    """one row of a mapping, on the host"""
    used = m[m >= 0]
    if m.min() < -1 or m.max() >= mg.size or np.unique(used).size != used.size:
        raise ValueError(f"mapping must hold model chains in [-1, {mg.size}), each at most once, got {m.tolist()}")
    if np.any(rg[m >= 0] != mg[used]):
        raise ValueError(f"mapping must join chains of one group only, got {m.tolist()}")


def _score_outputs(side, F, Cr):
    return (side.empty((F,), np.float32), side.empty((F,), np.float32), side.empty((F,), np.float32), side.empty((F,), np.float32),
            side.empty((F,), np.float32), side.empty((F, 3), np.int32), side.empty((F, Cr, Cr), np.float32))


def qs_score(xyz_ref, ref_offsets, ref_group, xyz, offsets, group, mapping, *, contact_thr=8.0, scale=10.0, model=None):
    """QSScore(qs_best, qs_global, ics, ics_precision, ics_recall float32 [F], counts int32 [F, 3] = (n_ref, n_model, n_shared), interface_qs
    float32 [F, Cr, Cr]) of the F models xyz against the reference under ``mapping``: int32 [Cr], or [F, Cr] with a row per frame, as
    chain_map and qs_map return it (-1: no model chain). See the module's definition. One row is checked on the host (ValueError); rows
    per frame are checked on the device, and a refused call raises PestoError having written nothing."""
    y, x, F, Nr, Nm, ro, rg, mo, mg, thr, sc = _layout(xyz_ref, ref_offsets, ref_group, xyz, offsets, group, contact_thr, scale)
    Cr, Cm = int(rg.size), int(mg.size)
    mapping = mapping if _lib.is_torch(mapping) else np.asarray(mapping)
    shape = tuple(int(v) for v in mapping.shape)
    if shape not in ((Cr,), (1, Cr), (F, Cr)):
        raise ValueError(f"mapping must be [{Cr}] or [{F}, {Cr}], got {list(shape)}")
    if not np.issubdtype(_lib.host(mapping[:0]).dtype, np.integer):
        raise ValueError("mapping must hold integers")
    rows = 1 if len(shape) == 1 or shape[0] == 1 else F
    if rows == 1:
        _check_mapping(_lib.host(mapping).reshape(-1).astype(np.int64), rg, mg)
    model = _model_of(model, x)
    side = _lib.Side(x, model._gpu)
    xd, yd = side.put(x, np.float32), side.put(y, np.float32)
    md = side.put(mapping, np.int32)
    lay = [side.put(v, np.int32) for v in (ro, rg, mo, mg)]
    outs = _score_outputs(side, F, Cr)
    lib = _lib.load()
    _lib.check(lib.pesto_qsscore(model.handle, F, Nr, Nm, Cr, Cm, *(side.ptr(v) for v in lay), side.ptr(yd), side.ptr(xd),
                                 side.ptr(md), rows, thr, sc, *(side.ptr(v) for v in outs), side.kind, side.stream), lib.pesto_qsscore_last_error)
    return QSScore(*(side.result(v) for v in outs))


def qs_map(xyz_ref, ref_offsets, ref_group, xyz, offsets, group, *, contact_thr=8.0, scale=10.0, model=None):
    """QSMap(mapping int32 [F, Cr], n_mapped int32 [F], index int64 [F], n_mappings int, and QSScore's seven fields for that mapping): the
    mapping of the largest qs_global of every frame, over all n_mappings(ref_group, group) mappings (at most MAX_MAPPINGS: ValueError
    beyond); index is its number in the enumeration (mapping_of_index). See the module's definition."""
    y, x, F, Nr, Nm, ro, rg, mo, mg, thr, sc = _layout(xyz_ref, ref_offsets, ref_group, xyz, offsets, group, contact_thr, scale)
    Cr, Cm = int(rg.size), int(mg.size)
    n = n_mappings(rg, mg)
    if n > MAX_MAPPINGS:
        raise ValueError(f"{n} chain mappings exceed MAX_MAPPINGS = 2**20: find a mapping with chainmap.chain_map and score it with qs_score")
    model = _model_of(model, x)
    side = _lib.Side(x, model._gpu)
    xd, yd = side.put(x, np.float32), side.put(y, np.float32)
    lay = [side.put(v, np.int32) for v in (ro, rg, mo, mg)]
    mapping, n_mapped, index = side.empty((F, Cr), np.int32), side.empty((F,), np.int32), side.empty((F,), np.int64)
    outs = _score_outputs(side, F, Cr)
    lib = _lib.load()
    _lib.check(lib.pesto_qsmap(model.handle, F, Nr, Nm, Cr, Cm, *(side.ptr(v) for v in lay), side.ptr(yd), side.ptr(xd),
                               thr, sc, side.ptr(mapping), side.ptr(n_mapped), side.ptr(index), *(side.ptr(v) for v in outs), side.kind, side.stream),
               lib.pesto_qsscore_last_error)
    return QSMap(side.result(mapping), side.result(n_mapped), side.result(index), n, *(side.result(v) for v in outs))


def interface_points(structure):
    """[(chain_name, xyz float32 [R_c, 3], codes uint8 [R_c], first-atom index of each residue int64 [R_c])] per protein chain of a
    structure, as structalign.ca_traces lists them, with the point QS-score takes of a residue: its (first) CB atom, or its CA where
    the residue has no CB (glycine, or a model without side chains)."""
    from .lddt import _structure_dict
    from .sequences import _residues, structure_sequences
    d = _structure_dict(structure)
    xyz = np.asarray(d["xyz"], np.float32).reshape(-1, 3)
    name = np.char.strip(np.asarray(d["name"]).astype(str))
    ca_at, cb_at = np.nonzero(name == "CA")[0], np.nonzero(name == "CB")[0]
    # where EVERY residue of the structure starts (those structure_sequences leaves out too: without a CA, of a ligand), so that a
    # residue's atoms end at the next residue's first atom, whatever that residue is
    starts = np.append(np.asarray(_residues(d)[0], np.int64), name.size)
    out = []
    for chain, codes, first in structure_sequences(d):
        first = np.asarray(first, np.int64)
        at = ca_at[np.searchsorted(ca_at, first, "left")]           # the first CA at or after a residue's first atom: its own
        if cb_at.size:
            end = starts[np.searchsorted(starts, first, "right")]   # the first atom of the next residue
            k = np.minimum(np.searchsorted(cb_at, first, "left"), cb_at.size - 1)
            at = np.where((cb_at[k] >= first) & (cb_at[k] < end), cb_at[k], at)
        out.append((chain, np.ascontiguousarray(xyz[at]), codes, first))
    return out


def structure_qsscore(reference, predicted, min_identity=0.9, mapping="qs", model=None, **kw):
    """(QSMap or QSScore, chains, match): the QS-score of the structure ``predicted`` against ``reference``. Each is a PDB path, a
    structure_io.Structure or a structure dict, in angstroms (scale 1). Entities and slots are those of chainmap.structure_chainmap
    (one cluster_sequences and one align_maps call); the points are interface_points. ``mapping`` says how the chains are paired:
    "qs" by qs_map (QSMap comes back), "tm" by chainmap.chain_map on the CA atoms and then qs_score, or a list of (reference chain name,
    model chain name) pairs that the caller gives (QSScore comes back for both). ``chains`` are the names of the mapped pairs in the
    reference's order and ``match`` is sequences.match_atoms' five results under that mapping, as structure_chainmap returns them:
    lddt.lddt, tmscore.tm_score and dockq take it directly. contact_thr is passed on."""
    from .chainmap import _entity_slots, chain_map
    from .lddt import _structure_dict
    from .structalign import ca_traces
    if "scale" in kw:
        raise ValueError("structure_qsscore works in angstroms: scale is not taken")
    a, b = _structure_dict(reference), _structure_dict(predicted)
    ta, tb = ca_traces(a), ca_traces(b)
    if not ta or not tb:
        raise ValueError("each structure needs a protein chain")
    kept_a, kept_b, side_arrays, result_of = _entity_slots(a, b, ta, tb, min_identity, model)
    ya, ro, rg = side_arrays(kept_a, interface_points(a), 0)
    xb, mo, mg = side_arrays(kept_b, interface_points(b), len(ta))
    if isinstance(mapping, str) and mapping == "qs":
        out = qs_map(ya, ro, rg, xb[None], mo, mg, scale=1.0, model=model, **kw)
        m = np.asarray(_lib.host(out.mapping))[0]
    else:
        if isinstance(mapping, str) and mapping == "tm":
            ca_a, _, _ = side_arrays(kept_a, ta, 0)
            ca_b, _, _ = side_arrays(kept_b, tb, len(ta))
            m = np.asarray(_lib.host(chain_map(ca_a, ro, rg, ca_b[None], mo, mg, scale=1.0, model=model).mapping))[0]
        elif isinstance(mapping, str):
            raise ValueError(f'mapping must be "qs", "tm" or pairs of chain names, got {mapping!r}')
        else:
            row_a = {ta[i][0]: k for k, i in enumerate(kept_a)}
            row_b = {tb[j][0]: k for k, j in enumerate(kept_b)}
            m = -np.ones(len(kept_a), np.int64)
            for ca, cb in mapping:
                if ca not in row_a or cb not in row_b:
                    raise ValueError(f"mapping: chain {ca!r} of the reference or {cb!r} of the model is none of the chains of a shared entity")
                m[row_a[ca]] = row_b[cb]
        out = qs_score(ya, ro, rg, xb[None], mo, mg, m.astype(np.int32), scale=1.0, model=model, **kw)
    chains, match = result_of(m)
    return out, chains, match
