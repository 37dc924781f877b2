"""GPU tests of pesto_amd.sequences (pesto_align.hip) against the definition of test_sequences_fixture.py. Every output is an integer and
every comparison is by equality; there is no tolerance anywhere. Each case runs from host arrays and from ROCm tensors with identical
bits between the two, from call to call, and alone against in a batch.

The layout's edges (pesto_align.hip): a lane's strip is W = 8 columns, one pass of 64 strips is a column block of 512 columns, a wave has
64 lanes. So the sweep's lengths are 1, 2, 7, 8, 9 (one below, at, above the strip), 63, 64, 65, 127, 128, 129, and 511, 512, 513 (one
below, at, above the column block: the boundary column goes through memory, and lane 63 is the last active lane or not), on either
side of the pair, with 1 x 300 and 300 x 1, and mutated copies (substitutions; one long deletion; many short insertions) so that all
three states carry the path. Two alphabets: 20 letters under BLOSUM62 (11 / 1), and 2 letters under match_matrix(1, -1) with gap_open =
gap_extend = 1, where nearly every cell ties, so the order D, U, L and the end-cell rule are what is tested."""
import numpy as np
import pytest

from test_sequences_fixture import FIELDS, align_def, align_diag, components, from_map, pass_matrix, passes, pdb_path

pytestmark = pytest.mark.gpu

MODES = ("global", "overlap", "local")
SMALL = (1, 2, 7, 8, 9, 63, 64, 65)
LARGE = ((127, 129), (128, 128), (129, 127), (128, 8), (9, 128), (511, 513), (512, 512), (513, 511), (513, 8), (7, 513), (512, 65), (1, 300), (300, 1))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def packed(seqs):
    from pesto_amd import _lib
    return np.concatenate(seqs).astype(np.uint8), _lib.offsets([len(s) for s in seqs])


def alphabet(which):
    """(letters, matrix, go, ge, unknown) of the sweep's two scoring schemes"""
    from pesto_amd import sequences as sq
    return (20, sq.BLOSUM62, 11, 1, 20) if which == "blosum" else (2, sq.match_matrix(1, -1, 2), 1, 1, None)


def mutants(rng, base, letters):
    """copies of base: substitutions at a fifth of the places; one deletion of a quarter; an insertion of one or two at every eleventh"""
    sub = base.copy()
    at = rng.choice(base.size, max(1, base.size // 5), replace=False)
    sub[at] = (sub[at] + rng.randint(1, letters, at.size)) % letters
    k = base.size // 4
    s = int(rng.randint(1, base.size - k))
    dele = np.concatenate([base[:s], base[s + k:]])
    parts, last = [], 0
    for p in range(5, base.size, 11):
        parts += [base[last:p], rng.randint(0, letters, rng.randint(1, 3)).astype(base.dtype)]
        last = p
    ins = np.concatenate(parts + [base[last:]])
    return sub, dele, ins


def sweep_system(which):
    """(sequences, pairs) of the sweep: random sequences at the layout's edges and the mutated copies"""
    letters = alphabet(which)[0]
    rng = np.random.RandomState(11 if which == "blosum" else 12)
    seqs, pairs = [], []

    def add(s):
        seqs.append(np.asarray(s, np.uint8))
        return len(seqs) - 1
    for m in SMALL:
        for n in SMALL:
            pairs.append((add(rng.randint(0, letters, m)), add(rng.randint(0, letters, n))))
    for m, n in LARGE:
        pairs.append((add(rng.randint(0, letters, m)), add(rng.randint(0, letters, n))))
    for size in (64, 129, 513):
        base = rng.randint(0, letters, size).astype(np.uint8)
        b = add(base)
        sub, dele, ins = (add(v) for v in mutants(rng, base, letters))
        pairs += [(b, sub), (b, dele), (b, ins), (dele, b), (ins, b), (dele, ins)]
    pairs.append((0, 0))
    return seqs, np.array(pairs, np.int32)


_reference = {}


def reference(which, mode):
    """the definition's outputs for the sweep, computed once per (alphabet, mode) and shared"""
    if (which, mode) not in _reference:
        _, mat, go, ge, unk = alphabet(which)
        seqs, pairs = sweep_system(which)
        out = [align_diag(seqs[i], seqs[j], mat, go, ge, mode, unk) for i, j in pairs]
        _reference[which, mode] = {k: np.array([o[k] for o in out], np.int32) for k in FIELDS}
    return _reference[which, mode]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["blosum", "two"])
def test_sweep_scores_and_maps(which, mode):
    from pesto_amd import sequences as sq
    _, mat, go, ge, unk = alphabet(which)
    seqs, pairs = sweep_system(which)
    want = reference(which, mode)
    kw = dict(mode=mode, matrix=mat, gap_open=go, gap_extend=ge, unknown=unk)
    got = sq.align_scores(seqs, pairs, **kw)
    for k in FIELDS:
        v = getattr(got, k)
        assert isinstance(v, np.ndarray) and v.dtype == np.int32
        bad = np.nonzero((v != want[k]).reshape(len(pairs), -1).any(1))[0]
        assert bad.size == 0, (k, bad[:5], [(len(seqs[i]), len(seqs[j])) for i, j in pairs[bad[:5]]], v[bad[:5]], want[k][bad[:5]])
    # the device side, a second call, a pair alone
    codes, offs = packed(seqs)
    on_dev = sq.align_scores((dev(codes), offs), pairs, **kw)
    again = sq.align_scores((codes, offs), pairs, **kw)
    for k in FIELDS:
        assert getattr(on_dev, k).is_cuda and same_bits(getattr(on_dev, k), getattr(got, k)) and same_bits(getattr(again, k), getattr(got, k))
    for p in (0, 70, len(pairs) - 3):
        alone = sq.align_scores(seqs, pairs[p:p + 1], **kw)
        assert all(same_bits(getattr(alone, k), getattr(got, k)[p:p + 1]) for k in FIELDS)
    # the maps: the same five outputs to the bit, the map of the loop where that is quick, and the counts the map implies everywhere
    maps = sq.align_maps(seqs, pairs, **kw)
    for k in FIELDS:
        assert same_bits(getattr(maps, k), getattr(got, k)), k
    lengths = np.array([len(seqs[i]) for i, _ in pairs])
    assert maps.map.dtype == np.int32 and np.array_equal(maps.map_offsets, np.concatenate([[0], np.cumsum(lengths)]))
    for p, (i, j) in enumerate(pairs):
        row = maps.map[maps.map_offsets[p]:maps.map_offsets[p + 1]]
        assert row.min() >= -1 and row.max() < len(seqs[j])
        hit = row[row >= 0]
        assert np.all(np.diff(hit) > 0)
        i0, j0, i1, j1 = got.span[p]
        assert np.all(row[:i0] == -1) and np.all(row[i1:] == -1) and (hit.size == 0 or (hit[0] >= j0 and hit[-1] < j1))
        fm = from_map(seqs[i], seqs[j], row, unk)
        assert (fm[:2] if fm else (0, 0)) == (got.n_ident[p], got.n_aligned[p])
        if len(seqs[i]) * len(seqs[j]) <= 600:
            assert np.array_equal(row, align_def(seqs[i], seqs[j], mat, go, ge, mode, unk)["map"]), (p, len(seqs[i]), len(seqs[j]))
    on_dev = sq.align_maps((dev(codes), offs), pairs, **kw)
    assert on_dev.map.is_cuda and same_bits(on_dev.map, maps.map) and all(same_bits(getattr(on_dev, k), getattr(maps, k)) for k in FIELDS)


def test_maps_of_mutated_copies_equal_the_loop():
    """the three states on the path: a 64-residue base against its deletion and insertion copies, every map against the loop's"""
    from pesto_amd import sequences as sq
    for which in ("blosum", "two"):
        _, mat, go, ge, unk = alphabet(which)
        seqs, pairs = sweep_system(which)
        sel = np.array([p for p, (i, j) in enumerate(pairs) if 40 <= len(seqs[i]) <= 90 and 40 <= len(seqs[j]) <= 90 and p >= len(SMALL) ** 2])
        assert sel.size == 6
        for mode in MODES:
            maps = sq.align_maps(seqs, pairs[sel], mode=mode, matrix=mat, gap_open=go, gap_extend=ge, unknown=unk)
            for q, (i, j) in enumerate(pairs[sel]):
                want = align_def(seqs[i], seqs[j], mat, go, ge, mode, unk)
                assert np.array_equal(maps.map[maps.map_offsets[q]:maps.map_offsets[q + 1]], want["map"]), (which, mode, q)
                assert tuple(maps.span[q]) == want["span"] and maps.n_cols[q] == want["n_cols"]


@pytest.mark.parametrize("mode", MODES)
def test_longest_pairs(mode):
    """4096 x 4096 (eight column blocks, the longest carry) and 4096 x 37, scores and maps"""
    from pesto_amd import sequences as sq
    rng = np.random.RandomState(3)
    base = rng.randint(0, 20, 4096).astype(np.uint8)
    sub, dele, ins = mutants(rng, base, 20)
    other = np.concatenate([dele[:2000], ins[2100:]])[:4096]
    other = np.concatenate([other, rng.randint(0, 20, 4096 - other.size).astype(np.uint8)])
    short = sub[1000:1037].copy()
    seqs, pairs = [base, other, short], np.array([(0, 1), (0, 2), (2, 0)], np.int32)
    got = sq.align_scores(seqs, pairs, mode=mode)
    maps = sq.align_maps(seqs, pairs, mode=mode)
    for p, (i, j) in enumerate(pairs):
        want = align_diag(seqs[i], seqs[j], sq.BLOSUM62, 11, 1, mode, 20)
        assert all(np.array_equal(getattr(got, k)[p], want[k]) for k in FIELDS), (p, [getattr(got, k)[p] for k in FIELDS], want)
    for k in FIELDS:
        assert same_bits(getattr(maps, k), getattr(got, k)), k
    for p, (i, j) in enumerate(pairs):
        row = maps.map[maps.map_offsets[p]:maps.map_offsets[p + 1]]
        fm = from_map(seqs[i], seqs[j], row)
        assert fm[:2] == (got.n_ident[p], got.n_aligned[p]) and np.all(np.diff(row[row >= 0]) > 0)
        assert fm[3][0] >= got.span[p][0] and fm[3][2] <= got.span[p][2]
    codes, offs = packed(seqs)
    on_dev = sq.align_scores((dev(codes), offs), pairs, mode=mode)
    assert all(same_bits(getattr(on_dev, k), getattr(got, k)) for k in FIELDS)


def test_all_against_all_equals_the_list():
    from pesto_amd import sequences as sq
    rng = np.random.RandomState(8)
    S = 70
    seqs = [rng.randint(0, 20, rng.randint(1, 60)).astype(np.uint8) for _ in range(S - 2)] + [rng.randint(0, 20, n).astype(np.uint8) for n in (520, 600)]
    pairs = np.array([(i, j) for i in range(S) for j in range(i + 1, S)], np.int32)
    assert len(pairs) == 2415                           # more than one launch's first wave of workgroups can hold at four pairs each
    for mode in MODES:
        full = sq.align_scores(seqs, mode=mode)
        listed = sq.align_scores(seqs, pairs, mode=mode)
        assert all(same_bits(getattr(full, k), getattr(listed, k)) for k in FIELDS), mode
        for p in rng.choice(len(pairs), 25, replace=False).tolist() + [len(pairs) - 1]:
            i, j = pairs[p]
            want = align_diag(seqs[i], seqs[j], sq.BLOSUM62, 11, 1, mode, 20)
            assert all(np.array_equal(getattr(full, k)[p], want[k]) for k in FIELDS), (mode, p)
    codes, offs = packed(seqs)
    on_dev = sq.align_scores((dev(codes), offs))
    assert all(same_bits(getattr(on_dev, k), getattr(sq.align_scores(seqs), k)) for k in FIELDS)
    one = sq.align_scores(seqs[:1])
    assert one.score.shape == (0,) and one.span.shape == (0, 4)


def families():
    """seeded families: a parent of 40 and children at 6, 8, 9 and 11 substitutions (the threshold of 0.8 over 40 is 32 identical), a
    chain A - B - C whose ends differ twice as much, singletons, copies, and short fragments"""
    rng = np.random.RandomState(21)
    seqs = []
    for _ in range(2):
        parent = rng.randint(0, 20, 40).astype(np.uint8)
        seqs.append(parent)
        for k in (6, 8, 9, 11):
            c = parent.copy()
            at = rng.choice(40, k, replace=False)
            c[at] = (c[at] + rng.randint(1, 20, k)) % 20
            seqs.append(c)
    a = rng.randint(0, 20, 40).astype(np.uint8)
    b, c = a.copy(), None
    b[:7] = (b[:7] + 1) % 20
    c = b.copy()
    c[-7:] = (c[-7:] + 1) % 20
    chain = len(seqs)
    seqs += [a, b, c]
    seqs += [rng.randint(0, 20, 40).astype(np.uint8), seqs[0].copy(), seqs[3].copy(), seqs[0][:25].copy(), seqs[0][5:38].copy(), seqs[0].copy(),
             np.full(30, 20, np.uint8), np.full(30, 20, np.uint8)]
    order = rng.permutation(len(seqs))
    return [seqs[k] for k in order], tuple(int(np.nonzero(order == chain + k)[0][0]) for k in range(3))


@pytest.mark.parametrize("over,mode,cov", [("shorter", "global", 0.0), ("aligned", "local", 0.7), ("columns", "overlap", 0.0), ("shorter", "global", 0.9)])
def test_clusters_are_the_components_of_the_pass_matrix(over, mode, cov):
    from pesto_amd import sequences as sq
    seqs, (ia, ib, ic) = families()
    id_bp, cov_bp = 8000, int(round(cov * 10000))
    P = pass_matrix(seqs, sq.BLOSUM62, 11, 1, mode, 20, id_bp, cov_bp, over)
    want = components(P)
    got = sq.cluster_sequences(seqs, 0.8, cov, over, mode)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, want), (got, want)
    # numbered by smallest member
    firsts = [int(np.nonzero(got == c)[0][0]) for c in range(got.max() + 1)]
    assert firsts == sorted(firsts) and 1 < got.max() + 1 < len(seqs)
    # the two host-side reductions change nothing; nor do the side or a second call
    assert np.array_equal(sq.cluster_sequences(seqs, 0.8, cov, over, mode, _reduce=False), want)
    codes, offs = packed(seqs)
    on_dev = sq.cluster_sequences((dev(codes), offs), 0.8, cov, over, mode)
    assert on_dev.is_cuda and same_bits(on_dev, got) and same_bits(sq.cluster_sequences((dev(codes), offs), 0.8, cov, over, mode, _reduce=False), got)
    assert same_bits(sq.cluster_sequences(seqs, 0.8, cov, over, mode), got)
    if (over, mode, cov) == ("shorter", "global", 0.0):
        # the chain: A - B and B - C pass, A - C does not, and the three are one cluster; the all-X copies have no identical residue and stay apart
        assert P[ia, ib] and P[ib, ic] and not P[ia, ic] and got[ia] == got[ib] == got[ic]
        xs = [k for k, s in enumerate(seqs) if (s == 20).all()]
        assert len(xs) == 2 and got[xs[0]] != got[xs[1]]
        # the integer test at its edge: 32 of 40 passes at 8000 basis points, 31 does not
        assert passes(dict(n_ident=32, n_aligned=40, n_cols=40), 40, 40, 8000, 0, "shorter") and not passes(dict(n_ident=31, n_aligned=40, n_cols=40), 40, 40, 8000, 0, "shorter")
        assert np.array_equal(sq.cluster_sequences(seqs[:1]), [0])


PAIRS = (("6I9F.pdb", "6I9F_i0.pdb", 155), ("1ZNS.pdb1", "1ZNS_ion.pdb", 118), ("7KHT.pdb1", "7KHT_lipid.pdb", 235 + 12))


@pytest.mark.parametrize("ref,mod,n_ca", PAIRS)
def test_match_atoms_by_alignment_on_renumbered_files(tmp_path, ref, mod, n_ca):
    from pesto_amd import lddt as ld, sequences as sq
    a, b = pdb_path(tmp_path, ref), pdb_path(tmp_path, mod)
    y, x, res, chain, table = sq.match_atoms(a, b)
    names = np.char.strip(np.asarray(ld._structure_dict(a)["name"]).astype(str))
    ca = names == "CA"
    protein = np.isin(table["resname"][res], list(sq.THREE_TO_ONE)) & ca
    matched = np.isfinite(x[0]).all(1)
    assert y.dtype == np.float32 and x.shape == (1, y.shape[0], 3) and res.dtype == np.int32 and chain.dtype == np.int32
    assert int(protein.sum()) == n_ca and int((matched & ca).sum()) == n_ca           # every residue is matched
    assert np.all(table["resid_model"][res[matched]] >= 1) and "resid_model" in table
    # the model is a copy of the file, so a matched atom has the reference's coordinates
    assert np.array_equal(x[0][matched], y[matched])
    # matching by number, as every other module does, does not get there: this documents the gap
    x_num = ld.match_atoms(a, b)[1]
    assert int((np.isfinite(x_num[0]).all(1) & ca).sum()) < n_ca
    if ref == "6I9F.pdb":
        out, tab = sq.structure_tmscore(a, b)
        assert out.tm[0] == 1.0 and out.gdt_ts[0] == 1.0 and tab["n_ref"] == 155 and tab["resid"][0] == -11 and tab["resid_model"][0] == 1
        assert ld.lddt(y, x, res, chain, sel=matched, scale=1.0).score[0] == 1.0
        score, _ = sq.structure_lddt(a, b, ca_only=True)
        assert score.score[0] == 1.0


def test_structure_lddt_equals_the_numbered_one_where_numbers_agree(tmp_path):
    from pesto_amd import lddt as ld, sequences as sq
    a, b = pdb_path(tmp_path, "1thf_D.pdb"), pdb_path(tmp_path, "1thf_D_i0.pdb")
    mine, table = sq.structure_lddt(a, b)
    theirs, table2 = ld.structure_lddt(a, b)
    for k in ("score", "residue", "preserved", "total"):
        assert same_bits(getattr(mine, k), getattr(theirs, k)), k
    assert mine.n_pairs == theirs.n_pairs and np.array_equal(table["resid"], table2["resid"]) and np.array_equal(table["resid_model"], table2["resid"])


def test_a_refused_call_leaves_the_handle_serving():
    """a code outside the alphabet in a device tensor: the host cannot see it, the kernel's verdict refuses the call"""
    from pesto_amd import _lib, sequences as sq
    seqs, pairs = sweep_system("blosum")
    codes, offs = packed(seqs[:20])
    bad = codes.copy()
    bad[offs[7] + 1] = 21
    want = sq.align_scores((codes, offs), mode="local")
    for call in (lambda c: sq.align_scores((c, offs), mode="local"), lambda c: sq.align_maps((c, offs), [[0, 1], [6, 7]]),
                 lambda c: sq.cluster_sequences((c, offs), _reduce=False)):
        with pytest.raises(_lib.PestoError, match=r"\[0, 21\)"):
            call(dev(bad))
        got = sq.align_scores((dev(codes), offs), mode="local")
        assert all(same_bits(getattr(got, k), getattr(want, k)) for k in FIELDS)
    with pytest.raises(ValueError):
        sq.align_scores((bad, offs))                    # the same array on the host is refused before any launch
