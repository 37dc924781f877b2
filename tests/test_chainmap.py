"""GPU tests of pesto_amd.chainmap (pesto_chainmap.hip) against the NumPy definition of tests/test_chainmap_fixture.py, through host arrays
and through ROCm tensors: the seeded sweep at the kernel's edges, the hand-worked and identity cases, the bit identities, apply_mapping
and structure_chainmap in front of the scorers, and the refused calls.

Bounds. mapping, n_mapped and round are decisions: equal to the definition's FOR THE RETURNED SEED (several seeds reach the same global
fit, so the lowest seed that attains the maximum may differ by double rounding: the definition's maximum at the returned seed must lie
within 1e-12 of its overall maximum, both as SCORES, total / L_norm, the unit of the output they explain and of the same check in
test_tmscore.py; the margin below is in units of the TM sum). Every sweep system keeps MARGIN_CAP = 1e-9 between the best and second-best assignment at every
visited fit, 1e4 times the double rounding of a sum of 4096 terms, so no decision is within rounding. score and chain_score: one float32
unit around the definition's value rounded to float32. rotation: orthonormal with determinant 1 within 1e-12.

Worst observed share of every bound (pytest -s prints them; MI355X): see DESIGN.md, the chainmap section."""
import numpy as np
import pytest

from test_chainmap_fixture import SCALE, SWEEP, cm_def, chains_of, dyadic_system, make_system, pair_sums, sweep_system

pytestmark = pytest.mark.gpu

SIDES = pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
WORST = {"seed maximum / 1e-12": 0.0, "score / float32 unit": 0.0, "recomputed score / float32 unit": 0.0, "chain_score / float32 unit": 0.0,
         "rotation / 1e-12": 0.0}


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def same_result(a, b, rows=slice(None)):
    return all(same_bits(host(x)[rows], host(y)) for x, y in zip(a, b))


def share(name, value, bound):
    WORST[name] = max(WORST[name], float(value) / bound)
    return value <= bound


def units32(got, want64):
    """|got - float32(want64)| in units of float32(want64)'s spacing"""
    want = np.float32(want64)
    return abs(float(got) - float(want)) / float(np.spacing(np.abs(want)) if want != 0 else np.float32(1e-45))


def run(s, on_device, **kw):
    from pesto_amd import chainmap as C
    put = dev if on_device else np.ascontiguousarray
    out = C.chain_map(put(s["xyz_ref"]), s["ro"], s["rg"], put(s["xyz"]), s["mo"], s["mg"], scale=SCALE, **kw)
    assert all((v.is_cuda if on_device else isinstance(v, np.ndarray)) for v in out)
    return C.ChainMap(*(host(v) for v in out))


def check(out, s, defs, tag=""):
    F, Cr = s["xyz"].shape[0], len(s["rg"])
    assert out.score.dtype == np.float32 and out.score.shape == (F,) and out.mapping.dtype == np.int32 and out.mapping.shape == (F, Cr)
    assert out.chain_score.dtype == np.float32 and out.chain_score.shape == (F, Cr) and out.rotation.shape == (F, 3, 3)
    assert out.rotation.dtype == np.float64 and out.translation.shape == (F, 3) and all(v.dtype == np.int32 for v in (out.n_mapped, out.seed, out.round))
    ref = chains_of(s["xyz_ref"], s["ro"])
    for f, d in enumerate(defs):
        seed = int(out.seed[f])
        assert seed in d["seeds"], (tag, f, seed)
        total, rnd, mapping, cs, _, _ = d["seeds"][seed]
        assert share("seed maximum / 1e-12", (d["total"] - total) / d["L_norm"], 1e-12), (tag, f, seed, d["best"])
        assert np.array_equal(out.mapping[f], mapping), (tag, f, out.mapping[f], mapping)
        assert out.n_mapped[f] == (mapping >= 0).sum() and out.round[f] == rnd, (tag, f, out.round[f], rnd)
        assert share("score / float32 unit", units32(out.score[f], total / d["L_norm"]), 1.0), (tag, f, out.score[f], total / d["L_norm"])
        R, t = out.rotation[f], out.translation[f]
        assert share("rotation / 1e-12", max(np.abs(R @ R.T - np.eye(3)).max(), abs(np.linalg.det(R) - 1.0)), 1e-12), (tag, f)
        mod = chains_of(s["xyz"][f], s["mo"])
        again = sum(pair_sums(ref[a][None], mod[b][None], R, t, d["d0"], SCALE)[0, 0] for a, b in enumerate(mapping) if b >= 0)
        assert share("recomputed score / float32 unit", units32(out.score[f], again / d["L_norm"]), 1.0), (tag, f)
        for a in range(Cr):
            want = cs[a] / d["finite"][a] if mapping[a] >= 0 and d["finite"][a] else 0.0
            assert share("chain_score / float32 unit", units32(out.chain_score[f, a], want), 1.0), (tag, f, a)
        assert np.array_equal(out.mapping[f], s["planted"][f]), (tag, f)


@SIDES
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: c[0])
def test_seeded_sweep(case, on_device):
    s, defs = sweep_system(case[0])
    check(run(s, on_device, n_iter=case[4]), s, defs, case[0])
    print("\nworst shares so far:", {k: "%.3g" % v for k, v in WORST.items()})


@SIDES
def test_hand_worked_and_identity_cases(on_device):
    from pesto_amd import chainmap as C, tmscore as T
    put = dev if on_device else np.ascontiguousarray
    # the model IS the reference up to chain order, a signed axis permutation and a dyadic shift
    for sizes in ((4,), (2, 3), (1, 1)):
        ref, mod, shuffle = dyadic_system(sizes)
        out = C.chain_map(put(ref["xyz"]), ref["offsets"], ref["group"], put(mod["xyz"]), mod["offsets"], mod["group"], scale=1.0)
        assert host(out.score)[0] == 1.0 and np.array_equal(host(out.mapping)[0], shuffle) and (host(out.chain_score) == 1.0).all(), sizes
        assert host(out.n_mapped)[0] == len(shuffle)
        moved = mod["xyz"][0].astype(np.float64) @ host(out.rotation)[0] + host(out.translation)[0]
        back = C.apply_mapping(moved.astype(np.float32), mod["offsets"], host(out.mapping)[0], ref["offsets"])[0]
        assert np.abs(back - ref["xyz"]).max() < 1e-4
    # a heterodimer that is bit-equal to its reference: the identity itself, as tm_score's `same` path gives it
    ref, _, _ = dyadic_system((1, 1))
    out = C.chain_map(put(ref["xyz"]), ref["offsets"], ref["group"], put(ref["xyz"][None]), ref["offsets"], ref["group"], scale=1.0)
    tm = T.tm_score(put(ref["xyz"]), put(ref["xyz"][None]), scale=1.0)
    assert same_bits(out.rotation, tm.rotation) and same_bits(out.translation, tm.translation) and host(out.score)[0] == 1.0
    assert np.array_equal(host(out.rotation)[0], np.eye(3)) and not host(out.translation).any() and host(out.mapping).tolist() == [[0, 1]]
    assert host(out.seed)[0] == 0 and host(out.round)[0] == 0
    # norm_len and d0 follow the definition
    s, _ = sweep_system("3v5")
    want = [cm_def(s["xyz_ref"], s["ro"], s["rg"], x, s["mo"], s["mg"], 5, SCALE, norm_len=77.0, d0=2.5) for x in s["xyz"]]
    check(run(s, on_device, norm_len=77.0, d0=2.5), s, want, "norm_len")
    # frames that are not finite: an infinite coordinate, and no seed at all
    x = np.repeat(s["xyz"][:1], 3, 0)
    x[0, 5, 1] = np.inf
    x[2] = np.nan
    out = run({**s, "xyz": x}, on_device)
    for f in (0, 2):
        assert np.isnan(out.score[f]) and (out.mapping[f] == -1).all() and out.seed[f] == -1 and out.round[f] == -1 and out.n_mapped[f] == 0
        assert np.isnan(out.rotation[f]).all() and np.isnan(out.translation[f]).all() and not out.chain_score[f].any()
    assert same_result(out, run({**s, "xyz": x[1:2]}, on_device), slice(1, 2))


def test_identical_bits_alone_in_a_batch_between_sides_and_calls():
    s, _ = sweep_system("F65")
    a, b, c = run(s, False), run(s, True), run(s, True)
    assert same_result(a, b) and same_result(b, c)
    for f in (0, 7, 64):
        assert same_result(a, run({**s, "xyz": s["xyz"][f:f + 1]}, f % 2 == 0), slice(f, f + 1)), f


@SIDES
def test_apply_mapping_gives_tm_score_the_unshuffled_model(on_device):
    from pesto_amd import chainmap as C, tmscore as T
    put = dev if on_device else np.ascontiguousarray
    s = make_system(21, [(40, 4, 4)], F=2, noise=1.0, n_nan=0)
    out = C.chain_map(put(s["xyz_ref"]), s["ro"], s["rg"], put(s["xyz"]), s["mo"], s["mg"], scale=1.0)
    assert np.array_equal(host(out.mapping), s["planted"]) and not np.array_equal(s["planted"][0], np.arange(4))
    gathered = C.apply_mapping(put(s["xyz"]), s["mo"], out.mapping, s["ro"])
    assert gathered.is_cuda if on_device else isinstance(gathered, np.ndarray)
    unshuffled = np.stack([np.concatenate([s["xyz"][f, s["mo"][b]:s["mo"][b + 1]] for b in s["planted"][f]]) for f in range(2)])
    assert same_bits(gathered, unshuffled)
    sel = np.nonzero(np.isfinite(s["xyz_ref"]).all(1))[0]
    mine, theirs = T.tm_score(put(s["xyz_ref"]), gathered, sel, scale=1.0), T.tm_score(s["xyz_ref"], unshuffled, sel, scale=1.0)
    assert same_result(mine, theirs)
    shuffled = T.tm_score(s["xyz_ref"], s["xyz"], sel, scale=1.0)
    assert (host(shuffled.tm) < host(mine.tm)).all()


def dimer_dicts():
    """(reference, model with its two chains in the reference's order, the same model with the chains' names and order swapped): a
    synthetic homodimer of 30 residues (N, CA, C) per chain whose two copies are placed by an arbitrary rigid motion (no C2 axis, so the
    two pairings differ), the model with 0.3 A noise"""
    from test_chainmap_fixture import rotation, walk
    rng = np.random.default_rng(33)
    L = 30
    ca = walk(rng, L)
    ca -= ca.mean(0)
    res = np.stack([ca + (-1.2, 0.5, 0.0), ca, ca + (1.1, 0.6, 0.3)], 1).reshape(-1, 3)
    second = res @ rotation(rng) + (9.0, 4.0, -3.0)
    three = np.array("ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL".split())
    seq = three[rng.integers(20, size=L)]

    def structure(first, then):
        return {"xyz": np.concatenate([first, then]).astype(np.float32), "name": np.tile(["N", "CA", "C"], 2 * L),
                "resname": np.tile(np.repeat(seq, 3), 2), "resid": np.tile(np.repeat(np.arange(1, L + 1), 3), 2),
                "chain_name": np.repeat(["A", "B"], 3 * L)}
    ma, mb = res + rng.normal(scale=0.3, size=res.shape), second + rng.normal(scale=0.3, size=res.shape)
    return structure(res, second), structure(ma, mb), structure(mb, ma)


def test_structure_chainmap_undoes_a_swap_in_front_of_lddt():
    from pesto_amd import chainmap as C, lddt as ld, sequences as sq
    reference, model, swapped = dimer_dicts()
    out, chains, match = C.structure_chainmap(reference, swapped)
    assert chains == [("A", "B"), ("B", "A")] and host(out.mapping).tolist() == [[1, 0]] and host(out.n_mapped)[0] == 2
    mine = ld.lddt(*match[:4], scale=1.0)
    straight, _ = sq.structure_lddt(reference, model)
    for k in ("score", "residue", "preserved", "total"):
        assert same_bits(getattr(mine, k), getattr(straight, k)), k
    assert match[4]["chain_model"][0] == "B" and match[4]["chain_model"][-1] == "A"
    # the gap that motivated the module: the greedy pairing by sequence puts chain A on chain A and loses the interface
    greedy, _ = sq.structure_lddt(reference, swapped)
    assert host(greedy.score)[0] < host(mine.score)[0]
    same, chains2, _ = C.structure_chainmap(reference, model)
    assert chains2 == [("A", "A"), ("B", "B")] and same_bits(same.score, out.score)


def test_structure_chainmap_on_the_6O1T_homodimer_with_its_chains_swapped(tmp_path):
    """tests/golden/pdb/6O1T.pdb1: two copies of one entity, chain A:0 with 195 residues (three of them calcium ions, code X) and chain
    B:1 with 186; A lacks B's residue 71 and B lacks A's 160-165, 238 and the ions, so the slots have gaps on both sides and residue 71
    needs a slot the representative (A:0, the longer) does not have. The reference is read from the file; the model is the structure
    with 0.2 A of noise, its chains renamed and reordered (B's atoms first, as chain A:0)."""
    from pesto_amd import chainmap as C, lddt as ld, sequences as sq
    from pesto_amd.lddt import _structure_dict
    from test_sequences_fixture import pdb_path
    reference = pdb_path(tmp_path, "6O1T.pdb1")
    d = _structure_dict(reference)
    assert sorted(set(d["chain_name"])) == ["A:0", "B:1"]
    model = dict(d, xyz=(d["xyz"] + np.random.default_rng(5).normal(scale=0.2, size=d["xyz"].shape)).astype(np.float32))
    order = np.concatenate([np.nonzero(d["chain_name"] == "B:1")[0], np.nonzero(d["chain_name"] == "A:0")[0]])
    swapped = {k: v[order] for k, v in model.items()}
    swapped["chain_name"] = np.where(swapped["chain_name"] == "A:0", "B:1", "A:0")
    out, chains, match = C.structure_chainmap(reference, swapped)
    assert chains == [("A:0", "B:1"), ("B:1", "A:0")] and host(out.mapping).tolist() == [[1, 0]] and host(out.n_mapped)[0] == 2
    mine = ld.lddt(*match[:4], scale=1.0)
    straight, table = sq.structure_lddt(reference, model)
    for k in ("score", "residue", "preserved", "total"):
        assert same_bits(getattr(mine, k), getattr(straight, k)), k
    # every residue keeps the partner that the direct alignment of the unswapped chains gives it, residue 71 of chain B among them
    assert np.array_equal(match[4]["resid_model"], table["resid_model"])
    at = np.nonzero((match[4]["chain_name"] == "B:1") & (match[4]["resid"] == 71))[0]
    assert at.size == 1 and match[4]["resid_model"][at[0]] == 71 and match[4]["chain_model"][at[0]] == "A:0"
    assert set(match[4]["chain_model"][match[4]["chain_name"] == "A:0"]) <= {"B:1", ""}
    # (The greedy pairing by sequence is not fooled by THIS swap: the copies differ in the residues they resolve, so chain A:0 has more
    # identical residues with its own copy than with the other, and structure_lddt of the swapped model gives the same score.) Cut to the
    # protein residues both copies have (no ion, no lipid), the two sequences are equal, every pairing ties, chain A goes on chain A and
    # the interface is lost:
    protein = d["het_flag"] != "H"
    both = np.intersect1d(d["resid"][protein & (d["chain_name"] == "A:0")], d["resid"][protein & (d["chain_name"] == "B:1")])
    cut = lambda s: {k: v[np.isin(s["resid"], both) & (s["het_flag"] != "H")] for k, v in s.items()}
    reference, model, swapped = cut(d), cut(model), cut(swapped)
    out, chains, match = C.structure_chainmap(reference, swapped)
    assert chains == [("A:0", "B:1"), ("B:1", "A:0")] and host(out.mapping).tolist() == [[1, 0]]
    mine = ld.lddt(*match[:4], scale=1.0)
    straight, table = sq.structure_lddt(reference, model)
    for k in ("score", "residue", "preserved", "total"):
        assert same_bits(getattr(mine, k), getattr(straight, k)), k
    greedy, _ = sq.structure_lddt(reference, swapped)
    assert host(greedy.score)[0] < host(mine.score)[0]


@SIDES
def test_refused_calls_write_nothing_and_the_next_call_is_served(on_device):
    from pesto_amd import _lib, chainmap as C
    from pesto_amd.patches import _default_model
    s = make_system(1, [(8, 2, 2)])
    put = dev if on_device else np.ascontiguousarray
    good = run(s, on_device)
    with pytest.raises(ValueError, match="share its slots"):
        C.chain_map(put(s["xyz_ref"]), s["ro"], s["rg"], put(s["xyz"][:, :15]), np.array([0, 8, 15]), s["mg"])
    big = make_system(2, [(3, 13, 1)], n_nan=0)
    with pytest.raises(ValueError, match="at most 12 chains"):
        C.chain_map(put(big["xyz_ref"]), big["ro"], big["rg"], put(big["xyz"]), big["mo"], big["mg"])
    with pytest.raises(ValueError, match="ascend"):
        C.chain_map(put(s["xyz_ref"]), s["ro"], s["rg"], put(s["xyz"]), np.array([0, 16, 8]), s["mg"])
    with pytest.raises(ValueError, match="n_iter"):
        C.chain_map(put(s["xyz_ref"]), s["ro"], s["rg"], put(s["xyz"]), s["mo"], s["mg"], n_iter=0)
    assert same_result(run(s, on_device), good)
    # the library's own refusals, through the C ABI (the Python layer refuses these first)
    model, lib = _default_model(0), _lib.load()
    y, x = put(s["xyz_ref"]), put(s["xyz"])
    side = _lib.Side(x, model._gpu)

    def sentinels(Cr):
        return [put(np.full(n, 7, t)) for n, t in ((1, np.float32), (Cr, np.int32), (Cr, np.float32), (1, np.int32), (1, np.int32), (1, np.int32),
                                                    (9, np.float64), (3, np.float64))]
    outs = sentinels(2)

    def call(ro, rg, mo, mg, y=y, x=x, outs=outs):
        arrays = [put(np.asarray(v, np.int32)) for v in (ro, rg, mo, mg)]
        return lib.pesto_chainmap(model.handle, 1, int(y.shape[0]), int(x.shape[1]), len(rg), len(mg), *(side.ptr(v) for v in arrays), side.ptr(y),
                                  side.ptr(x), 16.0, 0.5, 5, 1.0, *(side.ptr(v) for v in outs), side.kind, side.stream)

    def refused(rc, text, arrays=outs):
        assert rc == -1
        with pytest.raises(_lib.PestoError) as e:
            _lib.check(rc, lib.pesto_chainmap_last_error)
        assert str(e.value) == "libpesto_hip error -1: chainmap: " + text
        assert all((host(v) == 7).all() for v in arrays)
    refused(call(s["ro"], s["rg"], [0, 16, 8], s["mg"]), "offsets must start at 0, end at the number of residues and ascend")
    refused(call([0, 9, 16], s["rg"], s["mo"], s["mg"]), "a chain must have 3 to 4096 slots, as many as every chain of its group")
    refused(call(s["ro"], [0, 128], s["mo"], s["mg"]), "group ids must lie in [0, 128)")
    # 13 chains of one group on the reference side
    bouts = sentinels(13)
    refused(call(big["ro"], big["rg"], big["mo"], big["mg"], put(big["xyz_ref"]), put(big["xyz"]), bouts), "at most 12 chains of a group on a side", bouts)
    # a group that only the model has, with chains of 3 and 4 slots: all chains of a group, on both sides, share its slots
    refused(call(s["ro"], s["rg"], [0, 8, 11, 15], [0, 1, 1], x=put(s["xyz"][:, :15])), "a chain must have 3 to 4096 slots, as many as every chain of its group")
    assert call(s["ro"], s["rg"], s["mo"], s["mg"]) == 0
    want = C.chain_map(y, s["ro"], s["rg"], x, s["mo"], s["mg"], norm_len=16.0, d0=0.5, scale=1.0)
    assert all(same_bits(host(a).reshape(-1), host(b).reshape(-1)) for a, b in zip(outs, want))
