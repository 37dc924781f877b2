"""The definition of pesto_amd.sequences in two forms, hand-worked cases, and the module's host side (no GPU).

align_def is the readable statement: the cell-by-cell loop over the three states with an explicit traceback. align_diag is the same
recursion over anti-diagonals in NumPy, every state carrying the counts of its own path through the same choice that picks its value (the
tie order D, U, L; the end rules); it is asserted equal to align_def on every small case here and used by the GPU tests where the loop is
too slow. pass_matrix / components restate the integer link test and single linkage for the clustering tests."""
import gzip
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

NEG = -(1 << 40)                    # minus infinity: no sum of at most 8193 int8 scores and gap costs comes near it
FIELDS = ("score", "n_ident", "n_aligned", "n_cols", "span")


def first_max(cands):
    k = 0
    for c in range(1, len(cands)):
        if cands[c] > cands[k]:
            k = c
    return k


def align_def(a, b, matrix, go=11, ge=1, mode="global", unknown=20):
    """dict(score, n_ident, n_aligned, n_cols, span, map) of a against b: the module docstring's definition, cell by cell"""
    a, b, matrix = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(matrix, np.int64)
    m, n = a.size, b.size
    D = np.full((m + 1, n + 1), NEG, np.int64)
    U, L = D.copy(), D.copy()
    pD, pU, pL = (np.zeros((m + 1, n + 1), np.int8) for _ in range(3))
    if mode == "global":
        D[0, 0] = 0
        for i in range(1, m + 1):
            U[i, 0], pU[i, 0] = -(go + (i - 1) * ge), (0 if i == 1 else 1)
        for j in range(1, n + 1):
            L[0, j], pL[0, j] = -(go + (j - 1) * ge), (0 if j == 1 else 2)
    elif mode == "overlap":
        D[:, 0] = 0
        D[0, :] = 0
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            c = [D[i - 1, j - 1], U[i - 1, j - 1], L[i - 1, j - 1]] + ([0] if mode == "local" else [])
            k = first_max(c)
            D[i, j], pD[i, j] = matrix[a[i - 1], b[j - 1]] + c[k], k
            c = [D[i - 1, j] - go, U[i - 1, j] - ge, L[i - 1, j] - go]
            k = first_max(c)
            U[i, j], pU[i, j] = c[k], k
            c = [D[i, j - 1] - go, U[i, j - 1] - go, L[i, j - 1] - ge]
            k = first_max(c)
            L[i, j], pL[i, j] = c[k], k
    amap = np.full(m, -1, np.int32)
    if mode == "global":
        i, j = m, n
        st = first_max([D[m, n], U[m, n], L[m, n]])
        score = [D, U, L][st][m, n]
    else:
        cells = [(i, j) for i in range(m + 1) for j in range(n + 1) if (i == m or j == n if mode == "overlap" else i >= 1 and j >= 1)]
        score, i, j = max(((D[i, j], i, j) for i, j in cells), key=lambda t: (t[0], -t[1], -t[2]))
        st = 0
        if mode == "local" and score <= 0:
            return dict(score=0, n_ident=0, n_aligned=0, n_cols=0, span=(0, 0, 0, 0), map=amap)
    i1, j1, n_ident, n_aligned, n_cols = i, j, 0, 0, 0
    while True:
        if (mode == "global" and i == 0 and j == 0) or (mode == "overlap" and st == 0 and (i == 0 or j == 0)):
            break
        n_cols += 1
        if st == 0:
            k = pD[i, j]
            amap[i - 1] = j - 1
            n_aligned += 1
            n_ident += int(a[i - 1] == b[j - 1] and a[i - 1] != unknown)
            i, j = i - 1, j - 1
            if k == 3:
                break
        elif st == 1:
            k = pU[i, j]
            i -= 1
        else:
            k = pL[i, j]
            j -= 1
        st = k
    return dict(score=int(score), n_ident=n_ident, n_aligned=n_aligned, n_cols=n_cols, span=(i, j, i1, j1), map=amap)


def _pick(cands):
    """(value, carry) of the first maximum among [(value, carry), ...], elementwise"""
    v, c = cands[0]
    for v2, c2 in cands[1:]:
        better = v2 > v
        v, c = np.where(better, v2, v), np.where(better, c2, c)
    return v, c


def align_diag(a, b, matrix, go=11, ge=1, mode="global", unknown=20):
    """align_def's five outputs (no map) over anti-diagonals: index i of a diagonal's arrays is the cell (i, d - i). A carry is
    n_ident | n_aligned << 16 | i0 << 32 | j0 << 48 and travels with the value it belongs to."""
    a, b, matrix = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(matrix, np.int64)
    m, n = a.size, b.size
    rows = np.arange(m + 1, dtype=np.int64)
    same = lambda x, y: ((x == y) & (x != unknown)).astype(np.int64)                               # noqa: E731

    def border(d, D, U, L):
        """the border cells (d, 0) and (0, d) of diagonal d, written into its arrays"""
        for i, j in ((d, 0), (0, d)):
            if i > m or j > n:
                continue
            for S in (D, U, L):
                S[0][i], S[1][i] = NEG, 0
            if mode == "global":
                if d == 0:
                    D[0][i] = 0
                elif j == 0:
                    U[0][i] = -(go + (i - 1) * ge)
                else:
                    L[0][i] = -(go + (j - 1) * ge)
            elif mode == "overlap":
                D[0][i], D[1][i] = 0, (i << 32) | (j << 48)

    def blank():
        return [np.full(m + 1, NEG, np.int64), np.zeros(m + 1, np.int64)]
    prev2 = prev1 = None
    best = None                                         # (value, i, j, carry)
    for d in range(m + n + 1):
        D, U, L = blank(), blank(), blank()
        if d >= 2:
            i = rows[1:]
            j = d - i
            s = matrix[a[i - 1], b[np.clip(j - 1, 0, n - 1)]]
            mv, mc = _pick([(S[0][:-1], S[1][:-1]) for S in prev2])
            dv, dc = s + mv, mc
            if mode == "local":
                fresh = mv < 0
                dv = np.where(fresh, s, dv)
                dc = np.where(fresh, ((i - 1) << 32) | (np.maximum(j - 1, 0) << 48), dc)
            D[0][1:], D[1][1:] = dv, dc + (1 << 16) + same(a[i - 1], b[np.clip(j - 1, 0, n - 1)])
            pD, pU, pL = prev1
            U[0][1:], U[1][1:] = _pick([(pD[0][:-1] - go, pD[1][:-1]), (pU[0][:-1] - ge, pU[1][:-1]), (pL[0][:-1] - go, pL[1][:-1])])
            L[0][1:], L[1][1:] = _pick([(pD[0][1:] - go, pD[1][1:]), (pU[0][1:] - go, pU[1][1:]), (pL[0][1:] - ge, pL[1][1:])])
        border(d, D, U, L)
        lo, hi = max(0, d - n), min(m, d)               # the cells of the diagonal that exist
        if mode == "global":
            if d == m + n:
                v, c = _pick([(S[0][m:m + 1], S[1][m:m + 1]) for S in (D, U, L)])
                best = (int(v[0]), m, n, int(c[0]))
        else:
            i = rows[lo:hi + 1]
            j = d - i
            ok = ((i == m) | (j == n)) if mode == "overlap" else ((i >= 1) & (j >= 1))
            if ok.any():
                v = np.where(ok, D[0][lo:hi + 1], NEG)
                k = int(np.argmax(v))                   # the first maximum: the smallest i of this diagonal
                cand = (int(v[k]), int(i[k]), int(j[k]), int(D[1][lo + k]))
                if best is None or (cand[0], -cand[1], -cand[2]) > (best[0], -best[1], -best[2]):
                    best = cand
        prev2, prev1 = prev1, (D, U, L)
    score, i1, j1, c = best
    if mode == "local" and score <= 0:
        return dict(score=0, n_ident=0, n_aligned=0, n_cols=0, span=(0, 0, 0, 0))
    n_ident, n_aligned, i0, j0 = c & 0xffff, c >> 16 & 0xffff, c >> 32 & 0xffff, c >> 48 & 0xffff
    return dict(score=score, n_ident=n_ident, n_aligned=n_aligned, n_cols=(i1 - i0) + (j1 - j0) - n_aligned, span=(i0, j0, i1, j1))


def from_map(a, b, amap, unknown=20):
    """(n_ident, n_aligned, n_cols, span) that a map implies, None for a map without any aligned residue. The counts are those of the
    path; n_cols and the span are the path's only when it begins and ends with an aligned column - a path may also begin or end with gap
    columns, and then its span contains this one"""
    amap = np.asarray(amap)
    hit = np.nonzero(amap >= 0)[0]
    if hit.size == 0:
        return None
    i0, i1, j0, j1 = int(hit[0]), int(hit[-1]) + 1, int(amap[hit[0]]), int(amap[hit[-1]]) + 1
    aa, bb = np.asarray(a)[hit], np.asarray(b)[amap[hit]]
    return int(((aa == bb) & (aa != unknown)).sum()), int(hit.size), (i1 - i0) + (j1 - j0) - int(hit.size), (i0, j0, i1, j1)


def passes(r, m, n, id_bp, cov_bp, over):
    denom = {"shorter": min(m, n), "aligned": r["n_aligned"], "columns": r["n_cols"]}[over]
    return denom > 0 and r["n_ident"] * 10000 >= id_bp * denom and r["n_aligned"] * 10000 >= cov_bp * max(m, n)


def pass_matrix(seqs, matrix, go, ge, mode, unknown, id_bp, cov_bp, over):
    S = len(seqs)
    P = np.zeros((S, S), bool)
    for i in range(S):
        for j in range(i + 1, S):
            P[i, j] = P[j, i] = passes(align_diag(seqs[i], seqs[j], matrix, go, ge, mode, unknown), len(seqs[i]), len(seqs[j]), id_bp, cov_bp, over)
    return P


def components(P):
    """labels of the graph's connected components, numbered by smallest member"""
    S = P.shape[0]
    lab = np.full(S, -1, np.int32)
    nxt = 0
    for s in range(S):
        if lab[s] >= 0:
            continue
        stack = [s]
        lab[s] = nxt
        while stack:
            x = stack.pop()
            for y in np.nonzero(P[x])[0]:
                if lab[y] < 0:
                    lab[y] = nxt
                    stack.append(int(y))
        nxt += 1
    return lab


def pdb_path(tmp, name):
    """a golden PDB file unpacked under tmp (structure readers take plain files)"""
    p = os.path.join(str(tmp), name)
    if not os.path.exists(p):
        with gzip.open(os.path.join(GOLDEN, "pdb", name + ".gz"), "rb") as fi, open(p, "wb") as fo:
            fo.write(fi.read())
    return p


TWO = np.array([[1, -1], [-1, 1]], np.int8)


def small_cases():
    rng = np.random.RandomState(5)
    out = []
    for _ in range(60):
        m, n = rng.randint(1, 9, 2)
        out.append((rng.randint(0, 2, m), rng.randint(0, 2, n), TWO, 1, 1, 5))
    from pesto_amd.sequences import BLOSUM62
    for _ in range(30):
        m, n = rng.randint(1, 14, 2)
        out.append((rng.randint(0, 21, m), rng.randint(0, 21, n), BLOSUM62, int(rng.randint(1, 12)), 1, 20))
    for _ in range(20):
        m, n = rng.randint(1, 9, 2)
        go = int(rng.randint(0, 4))
        out.append((rng.randint(0, 3, m), rng.randint(0, 3, n), rng.randint(-2, 3, (3, 3)).astype(np.int8), go, int(rng.randint(0, go + 1)), 2))
    return out


@pytest.mark.parametrize("mode", ["global", "overlap", "local"])
def test_diagonal_form_equals_the_loop(mode):
    ties = 0
    for a, b, mat, go, ge, unk in small_cases():
        want = align_def(a, b, mat, go, ge, mode, unk)
        got = align_diag(a, b, mat, go, ge, mode, unk)
        assert all(got[k] == want[k] for k in FIELDS), (mode, a, b, go, ge, got, want)
        # the map says the same as the counts
        fm = from_map(a, b, want["map"], unk)
        if fm is None:
            assert want["n_aligned"] == 0
        else:
            assert fm[:2] == (want["n_ident"], want["n_aligned"])
            (i0, j0, i1, j1), (s0, t0, s1, t1) = fm[3], want["span"]
            assert s0 <= i0 and t0 <= j0 and s1 >= i1 and t1 >= j1 and want["n_cols"] >= fm[2]
            if mode == "local":                         # a local path begins and ends with an aligned column
                assert fm[2:] == (want["n_cols"], want["span"])
        ties += 1
    assert ties == 110


def test_hand_worked_cases():
    # a gap that may open on either side: [0 1] against [1 0], +1 / -1, gaps 1 / 1. Both "- 0 1 / 1 0 -" and "0 1 - / - 1 0" score -1; the end
    # cell has D = -2, U = L = -1, U comes first: a[1] faces a gap, before it a[0] ~ b[1], before that b[0] faces a gap
    r = align_def([0, 1], [1, 0], TWO, 1, 1, "global", 5)
    assert (r["score"], r["n_ident"], r["n_aligned"], r["n_cols"], r["span"]) == (-1, 1, 1, 3, (0, 0, 2, 2)) and r["map"].tolist() == [1, -1]
    # D = U = L at the end cell: [0] against [1] with mismatch -2 and gaps 1 / 1: D = -2, U = L[0][1] - 1 = -2, L = U[1][0] - 1 = -2, so D
    r = align_def([0], [1], np.array([[1, -2], [-2, 1]], np.int8), 1, 1, "global", 5)
    assert (r["score"], r["n_ident"], r["n_aligned"], r["n_cols"], r["span"]) == (-2, 0, 1, 1, (0, 0, 1, 1)) and r["map"].tolist() == [0]
    # equal maxima at two end cells, local: [0] against [0 0] has D = 1 at (1, 1) and (1, 2): the smaller j
    r = align_def([0], [0, 0], TWO, 1, 1, "local", 5)
    assert (r["score"], r["span"], r["map"].tolist()) == (1, (0, 0, 1, 1), [0])
    # ... and [0 0] against [0] at (1, 1) and (2, 1): the smaller i
    r = align_def([0, 0], [0], TWO, 1, 1, "local", 5)
    assert (r["score"], r["span"], r["map"].tolist()) == (1, (0, 0, 1, 1), [0, -1])
    # the same pair in overlap: the candidates are row 2 and column 1; D = 1 at (1, 1) and (2, 1), 0 at (0, 1) and (2, 0)
    r = align_def([0, 0], [0], TWO, 1, 1, "overlap", 5)
    assert (r["score"], r["n_cols"], r["span"], r["map"].tolist()) == (1, 1, (0, 0, 1, 1), [0, -1])
    # an all-negative local pair is empty; in overlap the start cell (0, n) wins with 0
    r = align_def([0], [1], TWO, 1, 1, "local", 5)
    assert (r["score"], r["n_ident"], r["n_aligned"], r["n_cols"], r["span"], r["map"].tolist()) == (0, 0, 0, 0, (0, 0, 0, 0), [-1])
    r = align_def([0], [1, 1], TWO, 1, 1, "overlap", 5)
    assert (r["score"], r["n_aligned"], r["n_cols"], r["span"], r["map"].tolist()) == (0, 0, 0, (0, 2, 0, 2), [-1])
    # unknown on the diagonal scores by the matrix but is not identical
    from pesto_amd.sequences import match_matrix
    r = align_def([2, 0], [2, 0], match_matrix(1, -1, 3), 1, 1, "global", 2)
    assert (r["score"], r["n_ident"], r["n_aligned"]) == (2, 1, 2)
    assert align_def([2, 0], [2, 0], match_matrix(1, -1, 3), 1, 1, "global", None)["n_ident"] == 2
    # an overlap proper: the tail of a on the head of b
    r = align_def([1, 1, 0, 1, 0], [0, 1, 0, 0, 0], TWO, 1, 1, "overlap", 5)
    assert (r["score"], r["n_ident"], r["span"], r["map"].tolist()) == (3, 3, (2, 0, 5, 3), [-1, -1, 0, 1, 2])


def test_encode_and_tables():
    from pesto_amd import sequences as sq
    assert sq.AMINO == "ARNDCQEGHILKMFPSTWYV" and sq.encode(sq.AMINO).tolist() == list(range(20))
    assert sq.encode("XBZa-*").tolist() == [20] * 6 and sq.encode("").size == 0 and sq.encode(b"AV").tolist() == [0, 19]
    B = sq.BLOSUM62
    assert B.dtype == np.int8 and B.shape == (21, 21) and np.array_equal(B, B.T)
    assert B.diagonal().tolist() == [4, 5, 6, 6, 9, 5, 5, 6, 8, 4, 4, 5, 5, 6, 7, 4, 5, 11, 7, 4, -1]
    assert (B[20] == -1).all() and (B[:, 20] == -1).all() and not B.flags.writeable
    assert "typed in" in sq._blosum62.__doc__
    M = sq.match_matrix(2, -3, 4)
    assert M.dtype == np.int8 and M.shape == (4, 4) and M.diagonal().tolist() == [2] * 4 and M[0, 1] == -3
    for kw in (dict(A=0), dict(A=33), dict(match=128), dict(mismatch=-129), dict(match=1.5)):
        with pytest.raises(ValueError):
            sq.match_matrix(**kw)
    with pytest.raises(ValueError):
        sq.encode(5)


def test_structure_sequences_on_the_golden_files(tmp_path):
    from pesto_amd import sequences as sq
    want = {"6I9F.pdb": [155], "6I9F_i0.pdb": [155], "1ZNS.pdb1": [118], "1ZNS_ion.pdb": [118], "7KHT.pdb1": [238 - 3, 12], "7KHT_lipid.pdb": [235, 12]}
    seqs = {}
    for name, lengths in want.items():
        out = sq.structure_sequences(pdb_path(tmp_path, name))
        assert [o[1].size for o in out] == lengths, (name, [o[1].size for o in out])
        for chain, codes, first in out:
            assert isinstance(chain, str) and codes.dtype == np.uint8 and codes.max() <= 20 and first.size == codes.size and np.all(np.diff(first) > 0)
        seqs[name] = out
    for x, y in (("6I9F.pdb", "6I9F_i0.pdb"), ("1ZNS.pdb1", "1ZNS_ion.pdb"), ("7KHT.pdb1", "7KHT_lipid.pdb")):
        assert all(np.array_equal(p[1], q[1]) for p, q in zip(seqs[x], seqs[y]))
    # a dict without resname: every residue with a CA is X, and a chain of X alone is left out
    d = dict(xyz=np.zeros((4, 3), np.float32), name=np.array(["N", "CA", "CA", "O"]), resid=np.array([1, 1, 2, 3]))
    assert sq.structure_sequences(d) == []
    d["resname"] = np.array(["ALA", "ALA", "MSE", "GLY"])
    (chain, codes, first), = sq.structure_sequences(d)
    assert chain == "" and codes.tolist() == [0, 20] and first.tolist() == [0, 2]           # GLY 3 has no CA
    d["icode"] = np.array(["", "A", "A", ""])
    assert [o[1].tolist() for o in sq.structure_sequences(d)] == [[0, 20]] and sq.structure_sequences(d)[0][2].tolist() == [1, 2]


def notebook_split(clusters, excluded, train_ratio, seed):
    """the reference notebook's cells 4 and 5 on lists of member ids (clusters in file order)"""
    kept = [c for c in clusters if not any(s in excluded for s in c)]
    barred = [c for c in clusters if any(s in excluded for s in c)]
    np.random.seed(seed)
    ids = np.arange(len(kept))
    np.random.shuffle(ids)
    n = int(len(kept) * train_ratio)
    train = [s for i in ids[:n] for s in kept[i]]
    test = [s for i in ids[n:] for s in kept[i]]
    return train, test, [s for c in barred for s in c]


def test_split_clusters_restates_the_notebook():
    from pesto_amd import sequences as sq
    rng = np.random.RandomState(2)
    labels = rng.randint(0, 40, 300)
    labels = np.unique(labels, return_index=True)[1].argsort().argsort()[np.unique(labels, return_inverse=True)[1]]   # by smallest member
    clusters = [np.nonzero(labels == c)[0].tolist() for c in range(labels.max() + 1)]
    for excluded, ratio, seed in (([], 0.8, 1337), ([3, 17, 250], 0.8, 1337), ([0], 0.5, 7), (list(range(300)), 0.8, 1), ([], 0.0, 3), ([], 1.0, 3)):
        tr, te, va = sq.split_clusters(labels, ratio, seed, excluded or None)
        w = notebook_split(clusters, set(excluded), ratio, seed)
        assert (tr.tolist(), te.tolist(), va.tolist()) == w and tr.dtype == te.dtype == va.dtype == np.int64
        assert sorted(tr.tolist() + te.tolist() + va.tolist()) == list(range(300))
        assert not set(labels[tr]) & set(labels[te]) and not set(labels[va]) & (set(labels[tr]) | set(labels[te]))
    mask = np.zeros(300, bool)
    mask[[3, 17, 250]] = True
    assert all(np.array_equal(x, y) for x, y in zip(sq.split_clusters(labels, excluded=mask), sq.split_clusters(labels, excluded=[3, 17, 250])))
    for kw in (dict(labels=[]), dict(labels=[-1, 0]), dict(labels=[0.5]), dict(train_ratio=1.5), dict(seed=-1), dict(seed=1.5), dict(excluded=[300]),
               dict(excluded=np.zeros(5, bool)), dict(excluded=[0.5])):
        args = dict(labels=labels)
        args.update(kw)
        with pytest.raises(ValueError):
            sq.split_clusters(**args)


def test_identity_is_for_reading():
    from pesto_amd import sequences as sq
    r = sq.AlignScores(np.array([0, 0], np.int32), np.array([3, 0], np.int32), np.array([4, 0], np.int32), np.array([6, 0], np.int32), np.zeros((2, 4), np.int32))
    assert sq.identity(r, [5, 2], [8, 9]).tolist() == [0.6, 0.0] and sq.identity(r, None, None, "aligned").tolist() == [0.75, 0.0]
    assert sq.identity(r, None, None, "columns").tolist() == [0.5, 0.0]
    with pytest.raises(ValueError):
        sq.identity(r, [5, 2], [8, 9], "longer")
    with pytest.raises(ValueError):
        sq.identity(r, [5], [8])


def test_every_value_error():
    """everything the host refuses, before a handle or the library is touched"""
    from pesto_amd import sequences as sq
    ok = ["ACDE", "ACD"]
    bad_seqs = ([], "ACDE", ["A", ""], ["A" * 4097, "A"], [np.zeros((2, 2), np.uint8), "A"], [np.array([0.5]), "A"], [np.array([300]), "A"],
                [np.array([21], np.uint8), "A"], (np.zeros(3, np.uint8), [0, 2]), (np.zeros(3, np.uint8), [1, 3]), (np.zeros(3, np.uint8), [0, 0, 3]),
                (np.zeros(3, np.uint8), [0.0, 3.0]), (np.zeros(3, np.uint8), [0]))
    for s in bad_seqs:
        with pytest.raises(ValueError):
            sq.align_scores(s)
    bad = (dict(mode="semi"), dict(matrix=np.zeros((3, 4), np.int8)), dict(matrix=np.zeros((33, 33), np.int8)), dict(matrix=np.zeros((21, 21))),
           dict(matrix=np.full((21, 21), 200)), dict(matrix=np.zeros((3, 3), np.int8)), dict(gap_open=1, gap_extend=2), dict(gap_extend=-1),
           dict(gap_open=128), dict(gap_open=1.0), dict(gap_open=True), dict(unknown=-1), dict(unknown=32), dict(unknown=1.0),
           dict(pairs=[[0, 2]]), dict(pairs=[[-1, 0]]), dict(pairs=[0, 1]), dict(pairs=[[0.0, 1.0]]), dict(pairs=np.zeros((1, 3), np.int32)))
    for kw in bad:
        with pytest.raises(ValueError):
            sq.align_scores(ok, **kw)
    for kw in (dict(pairs=None), dict(pairs=np.zeros((0, 2), np.int32)), dict(pairs=[[0, 2]]), dict(pairs=[[0, 1]], mode="x")):
        args = dict(pairs=[[0, 1]])
        args.update(kw)
        with pytest.raises(ValueError):
            sq.align_maps(ok, **args)
    for kw in (dict(min_identity=1.5), dict(min_identity=-0.1), dict(min_coverage=2), dict(over="longer"), dict(mode="x"), dict(gap_open=-1)):
        with pytest.raises(ValueError):
            sq.cluster_sequences(ok, **kw)
    y = dict(xyz=np.zeros((6, 3), np.float32), name=np.array(["CA"] * 6), resid=np.arange(6))
    with pytest.raises(ValueError):
        sq.structure_tmscore(y, y, sel=[0])
    with pytest.raises(ValueError):
        sq.structure_sequences(dict(xyz=np.zeros((0, 3)), name=np.array([]), resid=np.array([], np.int64)))
    with pytest.raises(ValueError):
        sq.structure_sequences(5)


def test_new_symbols_are_declared_exported_and_bound():
    import pesto_amd
    from pesto_amd import _lib, sequences as sq
    from pesto_amd.csrc import build
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    lib = _lib.load()
    for name in ("pesto_align_last_error", "pesto_align_scores", "pesto_align_maps"):
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert lib.pesto_align_last_error.restype is not None
    for key, value in (("MAX_LENGTH", sq.MAX_LENGTH), ("MAX_ALPHABET", sq.MAX_ALPHABET), ("MAX_GAP", sq.MAX_GAP)):
        assert int(re.search(rf"PESTO_ALIGN_{key} = (\d+)", hdr).group(1)) == value
    assert (sq.MAX_LENGTH, sq.MAX_ALPHABET, sq.MAX_GAP) == (4096, 32, 127)
    assert int(re.search(r"PESTO_ALIGN_MAX_SEQUENCES = 1 << (\d+)", hdr).group(1)) == 20 and sq.MAX_SEQUENCES == 2 ** 20
    assert int(re.search(r"PESTO_ALIGN_MAPS_WORKSPACE = 1 << (\d+)", hdr).group(1)) == 28 and sq.MAPS_WORKSPACE == 2 ** 28
    for name in ("align_scores", "align_maps", "cluster_sequences", "split_clusters", "structure_sequences"):
        assert name in pesto_amd.__all__ and getattr(pesto_amd, name) is getattr(sq, name)
    assert pesto_amd.sequences is sq and "pesto_align.hip" in build.SOURCES
    assert sq.AlignScores._fields == FIELDS and sq.AlignMaps._fields == FIELDS + ("map", "map_offsets")
    src = open(os.path.join(ROOT, "pesto_amd", "csrc", "pesto_align.hip")).read()
    assert "asm" not in src and "__shfl_up" in src and "pesto_patches" not in src.split("#include")[1]
    assert "align" in open(os.path.join(ROOT, "pesto_amd", "csrc", "pesto_call.h")).read().split("#pragma once")[0]
