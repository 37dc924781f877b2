"""GPU tests of pesto_amd.qsscore (pesto_qsscore.hip) against the NumPy definition of tests/test_qsscore_fixture.py, through host arrays
and through ROCm tensors: the seeded sweep at the kernel's edges, the hand-worked cases on dyadic lattices, the bit identities, the
planted mappings (one on which chain_map and qs_map must disagree), structure_qsscore in front of lddt, and the refused calls.

The sweep's cases (test_qsscore_fixture.SWEEP) come from the sizes built: k_qs_tile takes 64 slots of the row chain per workgroup, 16 per
wave, and 64 slots of the column chain per step; k_qs_enum 256 mappings per workgroup; 32768 frames per launch.
    chain lengths      3, 63, 64, 65 (one below, at, above the slot block), 129 (two blocks plus one)
    groups             (2) L3x2, (1, 1) L63-L64, (4) L65x4 (24 mappings), (3, 2) L129x3-L40x2 (12 mappings)
    3 against 5        3v5 (60 mappings), and the reverse 5v3
    a group on one side only     one-side
    a mapping with -1 entries    every case, qs_score under the planted mapping with one entry taken out
    NaN slots          random ones, and slots 63 and 64 of chains above 64 slots
    frames             F = 1, 2, 65 (one above a wave's lanes); 32769 (one above a launch) in the bit identities

Bounds. counts, mapping, n_mapped and index equal the definition's (every sweep system keeps DISTANCE_GAP and MAPPING_GAP, conditions
on the inputs checked on the CPU, so none of them is decided by rounding). Every float32 output lies within ONE float32 unit of the
definition's double rounded to float32: the double sums of at most 4096^2 terms err far below a float32 spacing, and the one unit
covers a double that rounds at a tie.

Worst observed share of every bound (pytest -s prints them; MI355X): see DESIGN.md, the qsscore section."""
import math

import numpy as np
import pytest

from test_qsscore_fixture import (SCALE, SWEEP, THR, FrameDef, lattice_system, make_qs_system, single_pair_system, sweep_system, threshold_system,
                                  with_holes, wrong_partner_system)

pytestmark = pytest.mark.gpu

SIDES = pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
FLOATS = ("qs_best", "qs_global", "ics", "ics_precision", "ics_recall")
WORST = {k + " / float32 unit": 0.0 for k in FLOATS + ("interface_qs",)}


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def same_result(a, b, rows=slice(None)):
    return all(same_bits(host(x)[rows], host(y)) for x, y in zip(a, b) if not isinstance(x, int))


def units32(got, want64):
    """|got - float32(want64)| in units of float32(want64)'s spacing; 0 where both are NaN, inf where one is"""
    if want64 != want64 or got != got:
        return 0.0 if (want64 != want64 and got != got) else np.inf
    want = np.float32(want64)
    return abs(float(got) - float(want)) / float(np.spacing(np.abs(want)) if want != 0 else np.float32(1e-45))


def share(name, value, bound=1.0):
    WORST[name] = max(WORST[name], float(value) / bound)
    return value <= bound


def put_of(on_device):
    return dev if on_device else np.ascontiguousarray


def score(s, mapping, on_device, **kw):
    from pesto_amd import qsscore as Q
    put = put_of(on_device)
    out = Q.qs_score(put(s["xyz_ref"]), s["ro"], s["rg"], put(s["xyz"]), s["mo"], s["mg"], put(np.asarray(mapping, np.int32)), scale=SCALE, **kw)
    assert all((v.is_cuda if on_device else isinstance(v, np.ndarray)) for v in out)
    return Q.QSScore(*(host(v) for v in out))


def search(s, on_device, **kw):
    from pesto_amd import qsscore as Q
    put = put_of(on_device)
    out = Q.qs_map(put(s["xyz_ref"]), s["ro"], s["rg"], put(s["xyz"]), s["mo"], s["mg"], scale=SCALE, **kw)
    assert all((v.is_cuda if on_device else isinstance(v, np.ndarray)) for v in out if not isinstance(v, int))
    return Q.QSMap(*(v if isinstance(v, int) else host(v) for v in out))


def check_scores(out, fds, mappings, tag):
    """the seven QSScore fields of every frame against the definition under mappings[f]"""
    F, Cr = len(fds), len(fds[0].ref)
    assert all(getattr(out, k).dtype == np.float32 and getattr(out, k).shape == (F,) for k in FLOATS)
    assert out.counts.dtype == np.int32 and out.counts.shape == (F, 3) and out.interface_qs.dtype == np.float32 and out.interface_qs.shape == (F, Cr, Cr)
    for f, fd in enumerate(fds):
        want = fd.score(mappings[f])
        assert tuple(out.counts[f].tolist()) == want["counts"], (tag, f, out.counts[f], want["counts"])
        for k in FLOATS:
            assert share(k + " / float32 unit", units32(getattr(out, k)[f], want[k])), (tag, f, k, getattr(out, k)[f], want[k])
        iq = out.interface_qs[f]
        assert np.array_equal(np.isnan(iq), np.isnan(want["interface_qs"])) and np.array_equal(iq, iq.T, equal_nan=True), (tag, f)
        for a, ap in zip(*np.nonzero(~np.isnan(iq))):
            assert share("interface_qs / float32 unit", units32(iq[a, ap], want["interface_qs"][a, ap])), (tag, f, a, ap)


@SIDES
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: c[0])
def test_seeded_sweep(case, on_device):
    s, fds, maps = sweep_system(case[0])
    F = len(fds)
    out = search(s, on_device)
    assert out.mapping.dtype == np.int32 and out.n_mapped.dtype == np.int32 and out.index.dtype == np.int64 and out.n_mappings == maps[0]["n"]
    for f, mp in enumerate(maps):
        assert np.array_equal(out.mapping[f], mp["mapping"]) and out.index[f] == mp["index"] and out.n_mapped[f] == (mp["mapping"] >= 0).sum(), (f, out.mapping[f], mp)
    check_scores(out, fds, [mp["mapping"] for mp in maps], case[0] + " qs_map")
    # qs_map's scores are qs_score's at the mapping it returns, bit for bit
    assert same_result(out[4:], score(s, out.mapping, on_device))
    check_scores(score(s, s["planted"], on_device), fds, s["planted"], case[0] + " planted")
    holes = np.stack([with_holes(m) for m in s["planted"]])
    check_scores(score(s, holes, on_device), fds, holes, case[0] + " holes")
    if F > 1:       # one mapping for all frames
        check_scores(score(s, s["planted"][0], on_device), fds, [s["planted"][0]] * F, case[0] + " one row")
    print("\nworst shares so far:", {k: "%.3g" % v for k, v in WORST.items()})


@SIDES
def test_hand_worked_cases_on_dyadic_lattices(on_device):
    # a model that IS its reference: exactly 1
    xyz, off, grp = lattice_system()
    s = {"xyz_ref": xyz, "ro": off, "rg": grp, "xyz": xyz[None], "mo": off, "mg": grp}
    out = score(s, [0, 1, 2], on_device)
    assert out.qs_best[0] == 1.0 and out.qs_global[0] == 1.0 and out.ics[0] == 1.0 and out.ics_precision[0] == 1.0 and out.ics_recall[0] == 1.0
    n = out.counts[0]
    assert n[0] > 0 and n[0] == n[1] == n[2] and FrameDef(xyz, off, xyz, off).score([0, 1, 2])["counts"] == tuple(n.tolist())
    iq = out.interface_qs[0]
    assert np.isnan(np.diag(iq)).all() and (iq[~np.eye(3, dtype=bool)] == 1.0).all()
    best = search(s, on_device)
    assert best.mapping.tolist() == [[0, 1, 2]] and best.qs_global[0] == 1.0 and best.n_mapped[0] == 3 and best.n_mappings == 2
    # its chains moved 64 A apart: nothing shared
    apart = xyz.copy()
    for c in range(3):
        apart[off[c]:off[c + 1], 0] += 64.0 * c
    out = score({**s, "xyz": apart[None]}, [0, 1, 2], on_device)
    assert out.qs_best[0] == 0.0 and out.qs_global[0] == 0.0 and out.ics[0] == 0.0 and out.ics_recall[0] == 0.0 and np.isnan(out.ics_precision[0])
    assert out.counts[0].tolist() == [n[0], 0, 0] and (out.interface_qs[0][~np.eye(3, dtype=bool)] == 0.0).all()
    # one slot pair, d1 = 4 and d2 = 7: w(4) (1 - 3 / 12)
    ref, ro, rg, x, mo, mg = single_pair_system()
    p = {"xyz_ref": ref, "ro": ro, "rg": rg, "xyz": x, "mo": mo, "mg": mg}
    out = score(p, [0, 1], on_device)
    assert out.qs_best[0] == 0.75 and out.qs_global[0] == 0.75 and out.interface_qs[0, 0, 1] == 0.75 and out.counts[0].tolist() == [1, 1, 1]
    assert score(p, [1, 0], on_device).qs_best[0] == 0.75
    # slot pairs AT the thresholds on both sides: 12 A weighs nothing (<), 8 A weighs w(8) and is no contact of ICS (<)
    ref, ro, rg, x, mo, mg = threshold_system()
    out = score({"xyz_ref": ref, "ro": ro, "rg": rg, "xyz": x, "mo": mo, "mg": mg}, [0, 1], on_device)
    w8 = math.exp(-2.0 * (3.0 / 4.28) ** 2)
    assert units32(out.qs_best[0], (0.75 + w8) / (1.0 + w8)) <= 1.0 and same_bits(out.qs_best, out.qs_global) and out.counts[0].tolist() == [1, 1, 1]
    # an unmapped third model chain in contact: qs_best stays, qs_global = 0.75 / (1 + w(4) + w(sqrt 65))
    ref, ro, rg, x, mo, mg = single_pair_system(extra_chain=True)
    q = {"xyz_ref": ref, "ro": ro, "rg": rg, "xyz": x, "mo": mo, "mg": mg}
    out = score(q, [0, 1], on_device)
    w65 = math.exp(-2.0 * ((math.sqrt(65.0) - 5.0) / 4.28) ** 2)
    assert out.qs_best[0] == 0.75 and units32(out.qs_global[0], 0.75 / (2.0 + w65)) <= 1.0 and out.qs_global[0] < 0.75
    assert out.counts[0].tolist() == [1, 2, 1] and out.ics_precision[0] == 0.5 and out.ics_recall[0] == 1.0
    # other thresholds and units follow the definition: nanometres with the default scale, contacts below 5 A
    nm = {**q, "xyz_ref": ref / 10.0, "xyz": x / 10.0}
    from pesto_amd import qsscore as Q
    put = put_of(on_device)
    out = Q.QSScore(*(host(v) for v in Q.qs_score(put(nm["xyz_ref"]), ro, rg, put(nm["xyz"]), mo, mg, [0, 1], contact_thr=5.0)))
    assert out.counts[0].tolist() == [1, 1, 0] and units32(out.qs_best[0], 0.75) <= 1.0
    # no contact anywhere: NaN
    lone = ref.copy()
    lone[3:, 1] += 50.0
    out = score({**p, "xyz_ref": lone, "xyz": lone[None]}, [0, 1], on_device)
    assert all(np.isnan(getattr(out, k)[0]) for k in FLOATS) and out.counts[0].tolist() == [0, 0, 0] and np.isnan(out.interface_qs).all()
    best = search({**p, "xyz_ref": lone, "xyz": lone[None]}, on_device)
    assert best.mapping.tolist() == [[-1, -1]] and best.index[0] == -1 and best.n_mapped[0] == 0 and np.isnan(best.qs_global[0])
    # an infinite coordinate in one frame: NaN and -1 there, the other frames' bits as they were
    s, fds, maps = sweep_system("3v5")
    x3 = np.repeat(s["xyz"][:1], 3, 0)
    x3[1, 7, 2] = np.inf
    one = {**s, "xyz": x3[:1]}
    for out, alone in ((score({**s, "xyz": x3}, s["planted"][0], on_device), score(one, s["planted"][0], on_device)),
                       (search({**s, "xyz": x3}, on_device), search(one, on_device))):
        assert all(np.isnan(getattr(out, k)[1]) for k in FLOATS) and out.counts[1].tolist() == [-1, -1, -1] and np.isnan(out.interface_qs[1]).all()
        assert same_result(out, alone, slice(0, 1)) and same_result(out, alone, slice(2, 3))
        assert not np.isnan(alone.qs_global[0])
    assert out.mapping[1].tolist() == [-1, -1, -1] and out.index[1] == -1 and out.n_mapped[1] == 0


def test_identical_bits_alone_in_a_batch_between_sides_and_calls():
    s, fds, maps = sweep_system("F65")
    a, b, c = search(s, False), search(s, True), search(s, True)
    assert same_result(a, b) and same_result(b, c)
    p, q, r = score(s, s["planted"], False), score(s, s["planted"], True), score(s, s["planted"], True)
    assert same_result(p, q) and same_result(q, r)
    for f in (0, 7, 64):
        assert same_result(a, search({**s, "xyz": s["xyz"][f:f + 1]}, f % 2 == 0), slice(f, f + 1)), f
        assert same_result(p, score({**s, "xyz": s["xyz"][f:f + 1]}, s["planted"][f], f % 2 == 1), slice(f, f + 1)), f
    # one frame above the frames of a launch: the two frames of a small system, tiled
    s, fds, maps = sweep_system("L63-L64")
    F = 32769
    tiled = {**s, "xyz": s["xyz"][np.arange(F) % 2]}
    two, many = search(s, True), search(tiled, True)
    for f in (0, 1, 32766, 32767, 32768):
        assert all(same_bits(host(x)[f], host(y)[f % 2]) for x, y in zip(many, two) if not isinstance(x, int)), f
    assert (many.mapping == two.mapping[np.arange(F) % 2]).all() and same_bits(many.qs_global, two.qs_global[np.arange(F) % 2])


@SIDES
def test_qs_map_recovers_a_planted_mapping_where_chain_map_pairs_the_wrong_copies(on_device):
    from pesto_amd import chainmap as C
    put = put_of(on_device)
    # the shuffled homotetramer: the planted mapping
    s, fds, maps = sweep_system("L65x4")
    out = search(s, on_device)
    assert np.array_equal(out.mapping, s["planted"]) and not np.array_equal(s["planted"][0], np.arange(4))
    # one copy docked on the wrong partner: each chain a near-rigid copy, so the TM-like sum keeps A1 on A1; the interface says otherwise
    w, tm_mapping, qs_mapping = wrong_partner_system()
    cm = C.chain_map(put(w["xyz_ref"]), w["ro"], w["rg"], put(w["xyz"]), w["mo"], w["mg"], scale=SCALE)
    qm = search(w, on_device)
    assert host(cm.mapping)[0].tolist() == tm_mapping.tolist() and qm.mapping[0].tolist() == qs_mapping.tolist()
    fd = FrameDef(w["xyz_ref"], w["ro"], w["xyz"][0], w["mo"])
    assert fd.score(qs_mapping)["qs_global"] > fd.score(tm_mapping)["qs_global"]
    under_tm = score(w, host(cm.mapping), on_device)
    assert qm.qs_global[0] > 0.9 and under_tm.qs_global[0] == 0.0
    check_scores(qm, [fd], [qs_mapping], "wrong partner")
    # a dimer: tested for its score only (its two mappings tie in a symmetric complex)
    s, fds, maps = sweep_system("L3x2")
    check_scores(search(s, on_device), fds, [mp["mapping"] for mp in maps], "dimer")


def test_structure_qsscore_on_the_6O1T_homodimer_with_its_chains_swapped(tmp_path):
    from pesto_amd import qsscore as Q
    from pesto_amd.lddt import _structure_dict
    from test_sequences_fixture import pdb_path
    reference = pdb_path(tmp_path, "6O1T.pdb1")
    d = _structure_dict(reference)
    order = np.concatenate([np.nonzero(d["chain_name"] == "B:1")[0], np.nonzero(d["chain_name"] == "A:0")[0]])
    swapped = {k: v[order] for k, v in d.items()}
    swapped["chain_name"] = np.where(swapped["chain_name"] == "A:0", "B:1", "A:0")
    out, chains, match = Q.structure_qsscore(reference, swapped)
    assert chains == [("A:0", "B:1"), ("B:1", "A:0")] and host(out.mapping).tolist() == [[1, 0]] and out.n_mappings == 2
    assert host(out.qs_best)[0] == 1.0 and host(out.qs_global)[0] == 1.0 and host(out.ics)[0] == 1.0 and host(out.counts)[0, 2] > 0
    # the pairing by name loses the interface's residues that only one copy resolves, not the interface: still high, below 1
    named, chains2, _ = Q.structure_qsscore(reference, swapped, mapping=[("A:0", "A:0"), ("B:1", "B:1")])
    assert chains2 == [("A:0", "A:0"), ("B:1", "B:1")] and isinstance(named, Q.QSScore) and host(named.qs_global)[0] < 1.0
    by_tm, chains3, _ = Q.structure_qsscore(reference, swapped, mapping="tm")
    assert chains3 == chains and all(same_bits(x, y) for x, y in zip(by_tm, out[4:]))
    # the points: CB, CA for glycine
    pts = Q.interface_points(d)
    name, resname = np.char.strip(d["name"].astype(str)), np.char.strip(d["resname"].astype(str))
    chain, xyz, codes, first = pts[0]
    gly = np.nonzero(resname[first] == "GLY")[0]
    assert gly.size and all(np.array_equal(xyz[r], d["xyz"][first[r] + list(name[first[r]:first[r] + 4]).index("CA")]) for r in gly[:5])
    ala = np.nonzero(resname[first] == "ALA")[0]
    assert ala.size and all(np.array_equal(xyz[r], d["xyz"][first[r] + list(name[first[r]:first[r] + 5]).index("CB")]) for r in ala[:5])


def write_pdb(path, chains, seq):
    """chains: [(name, atoms float [L, 4, 3]: N, CA, C, CB)]; glycine has no CB"""
    lines, serial = [], 1
    for cname, atoms in chains:
        for r, res in enumerate(seq):
            for k, an in enumerate(("N", "CA", "C", "CB")):
                if an == "CB" and res == "GLY":
                    continue
                x, y, z = atoms[r, k]
                lines.append(f"ATOM  {serial:5d}  {an:<3s} {res:3s} {cname}{r + 1:4d}    {x:8.3f}{y:8.3f}{z:8.3f}  1.00  0.00          {an[0]:>2s}")
                serial += 1
        lines.append("TER")
    lines.append("END")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return str(path)


def test_structure_qsscore_undoes_a_permutation_of_three_chains_in_front_of_lddt(tmp_path):
    from pesto_amd import lddt as ld, qsscore as Q, sequences as sq
    from pesto_amd.lddt import _structure_dict
    from test_chainmap_fixture import rotation, walk
    rng = np.random.default_rng(41)
    L = 30
    ca = walk(rng, L)
    ca -= ca.mean(0)
    res = np.stack([ca + (-1.2, 0.5, 0.0), ca, ca + (1.1, 0.6, 0.3), ca + (0.3, -0.9, 1.2)], 1)                    # [L, 4, 3]
    three = np.array("ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL".split())
    seq = three[rng.integers(20, size=L)]
    assert "GLY" in seq
    copies = [res @ rotation(rng) + rng.normal(scale=6.0, size=3) for _ in range(3)]
    noisy = [c + rng.normal(scale=0.2, size=c.shape) for c in copies]
    reference = write_pdb(tmp_path / "ref.pdb", list(zip("ABC", copies)), seq)
    model = write_pdb(tmp_path / "model.pdb", list(zip("ABC", noisy)), seq)
    permuted = write_pdb(tmp_path / "permuted.pdb", list(zip("ABC", [noisy[2], noisy[0], noisy[1]])), seq)          # model chain A holds copy C, ...
    names = list(dict.fromkeys(_structure_dict(reference)["chain_name"].tolist()))
    assert len(names) == 3
    out, chains, match = Q.structure_qsscore(reference, permuted)
    assert chains == [(names[0], names[1]), (names[1], names[2]), (names[2], names[0])] and host(out.mapping).tolist() == [[1, 2, 0]]
    assert host(out.n_mapped)[0] == 3 and out.n_mappings == 6 and host(out.qs_global)[0] > 0.8 and host(out.counts)[0].min() > 0
    straight, chains2, _ = Q.structure_qsscore(reference, model)
    # the same model in the reference's order: the same entries, bit for bit (Wmdl alone is summed in the model's chain order)
    assert [b for _, b in chains2] == names and all(same_bits(getattr(straight, k), getattr(out, k)) for k in ("qs_best", "ics", "counts", "interface_qs"))
    assert units32(host(out.qs_global)[0], float(host(straight.qs_global)[0])) <= 1.0
    mine = ld.lddt(*match[:4], scale=1.0)
    direct, _ = sq.structure_lddt(reference, model)
    for k in ("score", "residue", "preserved", "total"):
        assert same_bits(getattr(mine, k), getattr(direct, k)), k
    greedy, _ = sq.structure_lddt(reference, permuted)
    assert host(greedy.score)[0] < host(mine.score)[0]
    with pytest.raises(ValueError, match="none of the chains"):
        Q.structure_qsscore(reference, permuted, mapping=[(names[0], "Z")])
    with pytest.raises(ValueError, match='"qs", "tm" or pairs'):
        Q.structure_qsscore(reference, permuted, mapping="best")


@SIDES
def test_refused_calls_write_nothing_and_the_next_call_is_served(on_device):
    from pesto_amd import _lib, qsscore as Q
    from pesto_amd.patches import _default_model
    s = make_qs_system(1, [(8, 2, 2), (9, 1, 1)], F=2)
    put = put_of(on_device)
    good = score(s, s["planted"], on_device)
    with pytest.raises(ValueError, match="each at most once"):
        Q.qs_score(put(s["xyz_ref"]), s["ro"], s["rg"], put(s["xyz"]), s["mo"], s["mg"], [0, 0, 2])
    with pytest.raises(ValueError, match="share its slots"):
        Q.qs_map(put(s["xyz_ref"]), s["ro"], s["rg"], put(s["xyz"][:, :24]), np.array([0, 8, 15, 24]), s["mg"])
    # rows per frame are the device's to check: the verdict, with nothing written
    for rows, text in (([[0, 1, 2], [1, 1, 2]], "a mapping holds model chains in [-1, 3), each at most once"),
                       ([[0, 1, 2], [0, 3, 2]], "a mapping holds model chains in [-1, 3), each at most once"),
                       ([[0, 2, 1], [0, 1, 2]], "a mapping joins chains of one group only")):
        with pytest.raises(_lib.PestoError) as e:
            Q.qs_score(put(s["xyz_ref"]), s["ro"], s["rg"], put(s["xyz"]), s["mo"], s["mg"], put(np.array(rows, np.int32)), scale=SCALE)
        assert str(e.value) == "libpesto_hip error -1: qsscore: " + text
    assert same_result(score(s, s["planted"], on_device), good)
    # through the C ABI (the Python layer refuses some of these first)
    model, lib = _default_model(0), _lib.load()
    y, x = put(s["xyz_ref"]), put(s["xyz"])
    side = _lib.Side(x, model._gpu)
    shapes = ((2, np.float32),) * 5 + ((6, np.int32), (18, np.float32))
    outs = [put(np.full(n, 7, t)) for n, t in shapes]
    mouts = [put(np.full(n, 7, t)) for n, t in ((6, np.int32), (2, np.int32), (2, np.int64))]
    i32 = lambda v: np.ascontiguousarray(v, np.int32)

    def call(ro, rg, mo, mg, mapping):
        layout = [put(i32(v)) for v in (ro, rg, mo, mg)]           # where the side says, like the coordinates
        m = put(i32(mapping))
        return lib.pesto_qsscore(model.handle, 2, 25, 25, 3, 3, *(side.ptr(v) for v in layout), side.ptr(y), side.ptr(x), side.ptr(m), 2, THR, SCALE,
                                 *(side.ptr(v) for v in outs), side.kind, side.stream)

    def refused(rc, text, arrays=outs):
        assert rc == -1
        with pytest.raises(_lib.PestoError) as e:
            _lib.check(rc, lib.pesto_qsscore_last_error)
        assert str(e.value) == "libpesto_hip error -1: " + text
        assert all((host(v) == 7).all() for v in arrays)
    planted = s["planted"]
    refused(call(s["ro"], s["rg"], s["mo"], s["mg"], [[0, 1, 2], [1, 1, 2]]), "qsscore: a mapping holds model chains in [-1, 3), each at most once")
    refused(call(s["ro"], s["rg"], s["mo"], s["mg"], [[0, 2, 1], [0, 1, 2]]), "qsscore: a mapping joins chains of one group only")
    refused(call([0, 2, 16, 25], s["rg"], s["mo"], s["mg"], planted), "qsscore: a chain must have 3 to 4096 slots, as many as every chain of its group")
    refused(call(s["ro"], s["rg"], [0, 16, 8, 25], s["mg"], planted), "qsscore: offsets must start at 0, end at the number of residues and ascend")
    refused(call(s["ro"], [0, 0, 128], s["mo"], s["mg"], planted), "qsscore: group ids must lie in [0, 128)")
    # more than MAX_MAPPINGS: ten copies of one entity
    big = make_qs_system(2, [(3, 10, 10)], n_nan=0)
    lay = [put(i32(big[k])) for k in ("ro", "rg", "mo", "mg")]
    yb, xb = put(big["xyz_ref"]), put(big["xyz"])
    bouts = [put(np.full(n, 7, t)) for n, t in ((10, np.int32), (1, np.int32), (1, np.int64)) + ((1, np.float32),) * 5 + ((3, np.int32), (100, np.float32))]
    rc = lib.pesto_qsmap(model.handle, 1, 30, 30, 10, 10, *(side.ptr(v) for v in lay), side.ptr(yb), side.ptr(xb), THR, SCALE, *(side.ptr(v) for v in bouts),
                         side.kind, side.stream)
    refused(rc, "qsmap: more than 2^20 chain mappings: map the chains with pesto_chainmap and score that mapping with pesto_qsscore", bouts)
    # 13 chains of one group on the reference side
    huge = make_qs_system(2, [(3, 13, 1)], n_nan=0)
    lay = [put(i32(huge[k])) for k in ("ro", "rg", "mo", "mg")]
    yh, xh = put(huge["xyz_ref"]), put(huge["xyz"])
    houts = [put(np.full(n, 7, t)) for n, t in ((13, np.int32), (1, np.int32), (1, np.int64)) + ((1, np.float32),) * 5 + ((3, np.int32), (169, np.float32))]
    rc = lib.pesto_qsmap(model.handle, 1, 39, 3, 13, 1, *(side.ptr(v) for v in lay), side.ptr(yh), side.ptr(xh), THR, SCALE, *(side.ptr(v) for v in houts),
                         side.kind, side.stream)
    refused(rc, "qsmap: at most 12 chains of a group on a side", houts)
    # and the next calls are served, with the Python layer's bits
    assert call(s["ro"], s["rg"], s["mo"], s["mg"], planted) == 0
    assert all(same_bits(host(a).reshape(-1), host(b).reshape(-1)) for a, b in zip(outs, good))
    lay = [put(i32(s[k])) for k in ("ro", "rg", "mo", "mg")]
    assert lib.pesto_qsmap(model.handle, 2, 25, 25, 3, 3, *(side.ptr(v) for v in lay), side.ptr(y), side.ptr(x), THR, SCALE, *(side.ptr(v) for v in mouts),
                           *(side.ptr(v) for v in outs), side.kind, side.stream) == 0
    want = search(s, on_device)
    assert all(same_bits(host(a).reshape(-1), host(b).reshape(-1)) for a, b in zip(mouts + outs, [v for v in want if not isinstance(v, int)]))
