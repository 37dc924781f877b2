"""The NumPy definition of pesto_amd.structalign (structalign_def: float64, the fits by SVD, the TM searches through tm_def), the
hand-worked cases that pin it, the seeded sweep systems the GPU tests reuse, and the host side of the module. CPU only.

The dynamic programme is stated twice: dp_loop is the cell-by-cell loop over the three states with an explicit traceback, dp_diag the
same recursion over anti-diagonals in NumPy; the two are asserted equal on small pairs and dp_diag serves where the loop is too slow.

structalign_def also returns two DECISION MARGINS. ``margin`` is tm_def's own, over every search it ran: the smallest distance of any
d_i from a cut-off it was compared with. ``qmargin`` is the quantisation margin: the smallest distance of any v = Q / (1 + u) from a
half-integer, over every cell of every DP and every term of every threading sum. The sweep systems must keep qmargin >= 1e-8 score units
and margin >= MARGIN_CAP: conditions on the inputs, so that double-precision rounding (about 1e-10 in v) cannot change an integer - they
are not tolerances. A case that misses one gets another seed; the caps are never lowered."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_tmscore_fixture import MARGIN_CAP, _fits, _rotation, d0_def, domain16, sweep_system, tm_def

Q = 1024
QMARGIN_CAP = 1e-8
NEG = -(1 << 40)


# ------------------------------------------------------------------ the cell score and the dynamic programme
def transform_def(X, R, t):
    return X @ R + t


def scores_def(X, Y, R, t, k):
    """(s int64 [m, n], the quantisation margin) of the float64 points X under (R, t) against Y; k = scale^2 / d0s^2"""
    P = transform_def(X, R, t)
    E = P[:, None, :] - Y[None, :, :]
    u = ((E[..., 0] * E[..., 0] + E[..., 1] * E[..., 1]) + E[..., 2] * E[..., 2]) * k
    v = Q / (1.0 + u)
    f = np.floor(v + 0.5)
    return f.astype(np.int64), float(np.abs(v + 0.5 - np.round(v + 0.5)).min()) if v.size else np.inf


def pair_scores_def(X, Y, R, t, k):
    """scores_def of the pairs (X[i], Y[i]) alone"""
    E = transform_def(X, R, t) - Y
    v = Q / (1.0 + ((E[:, 0] * E[:, 0] + E[:, 1] * E[:, 1]) + E[:, 2] * E[:, 2]) * k)
    return np.floor(v + 0.5).astype(np.int64), float(np.abs(v + 0.5 - np.round(v + 0.5)).min())


def first_max(c):
    k = 0
    for q in range(1, len(c)):
        if c[q] > c[k]:
            k = q
    return k


def _end_and_walk(D, pD, pU, pL, m, n):
    """(map, score, n_aligned) from the filled states: the end is the largest D over the cells with i = m or j = n (the border cells
    (0, n) and (m, 0) of value 0 too), ties to the smallest i, then the smallest j; the path goes back through the predecessors"""
    cells = [(int(D[i, n]), i, n) for i in range(m + 1)] + [(int(D[m, j]), m, j) for j in range(n)]
    score, i, j = max(cells, key=lambda c: (c[0], -c[1], -c[2]))
    amap = np.full(m, -1, np.int32)
    st, na = 0, 0
    while not (st == 0 and (i == 0 or j == 0)):
        if st == 0:
            k = pD[i, j]
            amap[i - 1] = j - 1
            na += 1
            i, j = i - 1, j - 1
        elif st == 1:
            k = pU[i, j]
            i -= 1
        else:
            k = pL[i, j]
            j -= 1
        st = int(k)
    return amap, int(score), na


def dp_loop(s, go):
    """the recursion of sequences.py in "overlap" mode with s[i-1][j-1] in the place of the matrix lookup, gap_extend 0, cell by cell"""
    m, n = s.shape
    D = np.full((m + 1, n + 1), NEG, np.int64)
    U, L = D.copy(), D.copy()
    pD, pU, pL = (np.zeros((m + 1, n + 1), np.int8) for _ in range(3))
    D[:, 0] = 0
    D[0, :] = 0
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            c = [D[i - 1, j - 1], U[i - 1, j - 1], L[i - 1, j - 1]]
            k = first_max(c)
            D[i, j], pD[i, j] = s[i - 1, j - 1] + c[k], k
            c = [D[i - 1, j] - go, U[i - 1, j], L[i - 1, j] - go]
            k = first_max(c)
            U[i, j], pU[i, j] = c[k], k
            c = [D[i, j - 1] - go, U[i, j - 1] - go, L[i, j - 1]]
            k = first_max(c)
            L[i, j], pL[i, j] = c[k], k
    return _end_and_walk(D, pD, pU, pL, m, n)


def dp_diag(s, go):
    """dp_loop over anti-diagonals: the cells (i, d - i) of a diagonal at once; np.argmax takes the first maximum, the order D, U, L"""
    m, n = s.shape
    D = np.full((m + 1, n + 1), NEG, np.int64)
    U, L = D.copy(), D.copy()
    pD, pU, pL = (np.zeros((m + 1, n + 1), np.int8) for _ in range(3))
    D[:, 0] = 0
    D[0, :] = 0
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        c = np.stack([D[i - 1, j - 1], U[i - 1, j - 1], L[i - 1, j - 1]])
        k = np.argmax(c, 0)
        D[i, j], pD[i, j] = s[i - 1, j - 1] + np.take_along_axis(c, k[None], 0)[0], k
        c = np.stack([D[i - 1, j] - go, U[i - 1, j], L[i - 1, j] - go])
        k = np.argmax(c, 0)
        U[i, j], pU[i, j] = np.take_along_axis(c, k[None], 0)[0], k
        c = np.stack([D[i, j - 1] - go, U[i, j - 1] - go, L[i, j - 1]])
        k = np.argmax(c, 0)
        L[i, j], pL[i, j] = np.take_along_axis(c, k[None], 0)[0], k
    return _end_and_walk(D, pD, pU, pL, m, n)


# ------------------------------------------------------------------ the definition
def fit_def(X, Y):
    """(R, t) of the fit of the float64 points X onto Y as x' = x R + t, t = m_ref - m R; equal point sets: the identity itself"""
    R, mx, my, same = _fits(np.ones((1, X.shape[0]), bool), X, Y)
    if same[0]:
        return np.eye(3), np.zeros(3)
    return R[0], my[0] - mx[0] @ R[0]


def frag_starts_def(length, f, frag_starts):
    last = length - f
    stride = max(1, -(-last // (frag_starts - 1)))
    out = list(range(0, last + 1, stride))
    if out[-1] != last:
        out.append(last)
    return out


def search_def(X, Y, amap, norm_len, d0, step, scale):
    """tm_def on the aligned pairs of amap: a's residues onto b's"""
    hit = np.nonzero(amap >= 0)[0]
    return tm_def(Y[amap[hit]], X[hit][None], norm_len=norm_len, d0=d0, step=step, scale=scale)


def structalign_def(a, b, codes_a=None, codes_b=None, init=None, gap_open=0.6, rounds=20, frag_starts=16, scale=10.0, dp=dp_diag):
    """dict of every output of align_structures for the one pair (a onto b), plus per (unit, round): maps[u][r] (the alignment searched),
    tm64 [units, rounds] (NaN where a unit did not run), and the two margins; i1 = (k, sum), i2 = (start in a, start in b, score)"""
    a32, b32 = np.asarray(a, np.float32).reshape(-1, 3), np.asarray(b, np.float32).reshape(-1, 3)
    m, n = a32.shape[0], b32.shape[0]
    NU = 6 if init is not None else 4
    out = dict(map=np.full(m, -1, np.int32), n_aligned=0, n_ident=0, dp_score=0, unit=-1, round=-1, tm_a=np.float32(0), tm_b=np.float32(0),
               rotation=np.eye(3), translation=np.zeros(3), rmsd=np.float32(np.nan), history=np.full((NU, rounds, 3), np.nan),
               tm64=np.full((NU, rounds), np.nan), maps=[[None] * rounds for _ in range(NU)], margin=np.inf, qmargin=np.inf)
    if not (np.isfinite(a32).all() and np.isfinite(b32).all()):
        out.update(tm_a=np.float32(np.nan), tm_b=np.float32(np.nan), rotation=np.full((3, 3), np.nan), translation=np.full(3, np.nan))
        return out
    X, Y = a32.astype(np.float64), b32.astype(np.float64)
    lmin = min(m, n)
    d0s = d0_def(lmin)
    k = (scale * scale) / (d0s * d0s)
    go = int(round(gap_open * Q))

    def note(q):
        out["qmargin"] = min(out["qmargin"], q)

    # I1
    minov = max(3, (lmin + 1) // 2)
    best = None
    for off in range(-(m - minov), n - minov + 1):
        fa = max(0, -off)
        ov = min(m, n - off) - fa
        Xo, Yo = X[fa:fa + ov], Y[fa + off:fa + off + ov]
        R, t = fit_def(Xo, Yo)
        s, q = pair_scores_def(Xo, Yo, R, t, k)
        note(q)
        total = int(s.sum())
        if best is None or total > best[1]:
            best = (off, total)
    out["i1"] = best
    rows = np.arange(m)
    inits = [np.where((rows + best[0] >= 0) & (rows + best[0] < n), rows + best[0], -1).astype(np.int32)]
    # I2
    f = min(lmin, max(4, min(20, lmin // 3)))
    best = None
    for sa in frag_starts_def(m, f, frag_starts):
        for sb in frag_starts_def(n, f, frag_starts):
            R, t = fit_def(X[sa:sa + f], Y[sb:sb + f])
            s, q = scores_def(X, Y, R, t, k)
            note(q)
            amap, score, na = dp(s, 0)
            if best is None or score > best[2]:
                best = (sa, sb, score, amap)
    out["i2"] = best[:3]
    inits.append(best[3])
    if init is not None:
        inits.append(np.asarray(init, np.int32))
    best_tm, choice = -1.0, None
    for u in range(NU):
        cur = inits[u // 2].copy()
        gap = go if u % 2 == 0 else 0
        for r in range(rounds):
            na = int((cur >= 0).sum())
            if na < 3:
                break
            got = search_def(X, Y, cur, lmin, d0s, max(1, na >> 3), scale)
            out["margin"] = min(out["margin"], got["margin"])
            s, q = scores_def(X, Y, got["rotation"][0], got["translation"][0], k)
            note(q)
            new, score, new_na = dp(s, gap)
            out["maps"][u][r] = cur
            out["tm64"][u, r] = got["tm64"][0]
            out["history"][u, r] = (float(got["tm"][0]), score, na)
            tm32 = float(got["tm"][0])
            if tm32 > best_tm:
                best_tm, choice = tm32, (u, r)
            if np.array_equal(new, cur):
                break
            cur = new
    if choice is not None:
        out.update(chosen_def(a32, b32, out, *choice, codes_a=codes_a, codes_b=codes_b, scale=scale))
    return out


def chosen_def(a, b, d, unit, rnd, codes_a=None, codes_b=None, scale=10.0):
    """the outputs of the pair if (unit, round) is the one chosen: its searched alignment scored at step 1 by m and by n"""
    a32, b32 = np.asarray(a, np.float32).reshape(-1, 3), np.asarray(b, np.float32).reshape(-1, 3)
    X, Y = a32.astype(np.float64), b32.astype(np.float64)
    m, n = X.shape[0], Y.shape[0]
    amap = d["maps"][unit][rnd]
    hit = np.nonzero(amap >= 0)[0]
    ga = search_def(X, Y, amap, m, d0_def(m), 1, scale)
    gb = search_def(X, Y, amap, n, d0_def(n), 1, scale)
    g = ga if m <= n else gb
    ni = 0 if codes_a is None else int((np.asarray(codes_a)[hit] == np.asarray(codes_b)[amap[hit]]).sum())
    return dict(map=amap, n_aligned=int(hit.size), n_ident=ni, dp_score=int(d["history"][unit, rnd, 1]), unit=unit, round=rnd, tm_a=ga["tm"][0],
                tm_b=gb["tm"][0], tm_a64=ga["tm64"][0], tm_b64=gb["tm64"][0], rotation=g["rotation"][0], translation=g["translation"][0],
                final_margin=min(ga["margin"], gb["margin"]))


# ------------------------------------------------------------------ the sweep systems
@functools.lru_cache(maxsize=None)
def sweep_pair(m, n, seed):
    """(a float32 [m, 3], b float32 [n, 3]) in nanometres: b is a CA-like trace of sweep_system; a is the same trace with 1 A of noise, its
    second half moved as a rigid domain (sweep_system's frame), then residues deleted from it or inserted into it until it has m"""
    L = max(m, n)
    s = sweep_system(L, 1, seed)
    rng = np.random.default_rng(77 * m + n + 1000 * seed)

    def shortened(x, to):
        """x without L - to residues of its middle third (one deletion); more than a third to lose: its first `to` residues"""
        if L - to > L // 3:
            return x[:to]
        cut = int(rng.integers(L // 3, max(L // 3 + 1, 2 * L // 3 - (L - to))))
        return np.concatenate([x[:cut], x[cut + (L - to):]])
    a = shortened(s["xyz"][0], m) if m < L else s["xyz"][0]
    b = shortened(s["ref"], n) if n < L else s["ref"]           # (an insertion from b's point of view)
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


# (m, n, seed, frag_starts). A seed other than 0 replaced one whose case missed a margin (noted next to it).
SWEEP = [(3, 3, 0, 16), (4, 9, 0, 16), (8, 8, 0, 16), (9, 8, 0, 16), (63, 65, 0, 16), (64, 64, 0, 16), (65, 63, 0, 16), (129, 127, 0, 16)]
BLOCKS = (513, 511, 0, 3)       # the second column block and the boundary row handed between blocks
LONGEST = (4096, 64, 0, 2)      # rounds = 1


@functools.lru_cache(maxsize=None)
def sweep_def(m, n, seed, frag_starts, rounds=20):
    a, b = sweep_pair(m, n, seed)
    return structalign_def(a, b, frag_starts=frag_starts, rounds=rounds)


# ------------------------------------------------------------------ tests of the definition itself
def test_diagonal_form_equals_the_loop():
    rng = np.random.default_rng(3)
    for _ in range(60):
        m, n = rng.integers(1, 12, 2)
        s = rng.integers(0, 6, (m, n)).astype(np.int64) * int(rng.integers(1, 300))
        for go in (0, int(rng.integers(1, 700))):
            want, got = dp_loop(s, go), dp_diag(s, go)
            assert np.array_equal(want[0], got[0]) and want[1:] == got[1:], (s, go, want, got)
            amap = want[0]
            hit = amap[amap >= 0]
            assert hit.size == want[2] and (np.diff(hit) > 0).all()


def test_ties_take_d_then_u_then_l_by_hand():
    # two equal columns: aligning a_1 to b_1 or b_2 scores the same; the end rule takes the smaller i, then j, and D precedes L
    s = np.array([[5, 5]], np.int64)
    assert dp_loop(s, 0)[0].tolist() == [0] and dp_loop(s, 0)[1] == 5
    # a gap of cost 0 lets both diagonal cells count; with cost 7 one of them alone wins
    s = np.array([[4, 0, 0], [0, 0, 4]], np.int64)
    assert dp_loop(s, 0)[1] == dp_diag(s, 0)[1] == 8 and dp_loop(s, 0)[0].tolist() == dp_diag(s, 0)[0].tolist() == [0, 2]
    assert dp_loop(s, 7)[1] == 4


def test_fragment_starts_by_hand():
    assert frag_starts_def(10, 10, 16) == [0] and frag_starts_def(12, 4, 16) == list(range(9))
    assert frag_starts_def(100, 20, 16) == [0, 6, 12, 18, 24, 30, 36, 42, 48, 54, 60, 66, 72, 78, 80]
    assert frag_starts_def(100, 20, 2) == [0, 80] and frag_starts_def(513, 20, 3) == [0, 247, 493]


def test_a_chain_against_itself():
    a, _ = sweep_pair(64, 64, 0)
    got = structalign_def(a, a, codes_a=np.arange(64) % 20, codes_b=np.arange(64) % 20)
    assert got["map"].tolist() == list(range(64)) and got["tm_a"] == 1.0 and got["tm_b"] == 1.0
    assert (got["unit"], got["round"]) == (0, 0) and got["i1"] == (0, 64 * Q) and got["n_ident"] == 64 and got["n_aligned"] == 64
    assert np.array_equal(got["rotation"], np.eye(3)) and np.array_equal(got["translation"], np.zeros(3))


def test_displaced_domain_by_hand():
    ref, x, _ = domain16()
    got = structalign_def(x[0], ref, scale=1.0)
    assert got["map"].tolist() == list(range(16))
    assert got["tm_a64"] == (8 + 8 / 40001) / 16 and got["tm_a"] == got["tm_b"]


def planted_deletion():
    """(a: the copy of 20 residues, b: the chain of 24, the planted map): dyadic coordinates; the copy lacks residues 8..11 and is moved by a signed axis
    permutation and a dyadic shift, so every sum is exact"""
    i = np.arange(24)
    b = np.stack([4.0 * i, 4.0 * ((i * i) % 5), 4.0 * ((3 * i) % 7)], 1)
    keep = np.r_[0:8, 12:24]
    Pm = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0]])    # det +1
    a = b[keep] @ Pm + np.array([8.0, -16.0, 32.0])
    return a.astype(np.float32), b.astype(np.float32), keep.astype(np.int32)


def test_a_planted_deletion():
    a, b, planted = planted_deletion()
    got = structalign_def(a, b, scale=1.0)
    m = a.shape[0]
    far = np.array([r for r in range(m) if min(abs(r - 7), abs(r - 8)) >= 3])
    assert np.array_equal(got["map"][far], planted[far])
    assert got["n_aligned"] >= b.shape[0] - 4 - 6 and got["n_aligned"] == m == 20
    # a signed axis permutation and a dyadic shift of dyadic coordinates: every sum is exact, every aligned pair coincides, and the copy
    # is the shorter chain, so the residual 1 - tm normalised by it is 0 before rounding
    assert got["tm_a64"] == 1.0 and got["tm_a"] == 1.0 and np.array_equal(got["map"], planted)


def test_the_shortest_lengths_and_a_nan_chain():
    for m, n in ((3, 3), (4, 4), (3, 4)):
        a, b = sweep_pair(m, n, 0)
        got = structalign_def(a, b)
        assert got["n_aligned"] >= 3 and 0 < got["tm_a"] <= 1 and got["unit"] >= 0
    a, b = sweep_pair(8, 8, 0)
    bad = a.copy()
    bad[2, 1] = np.nan
    got = structalign_def(bad, b)
    assert np.isnan(got["tm_a"]) and np.isnan(got["tm_b"]) and got["unit"] == -1 and (got["map"] == -1).all()
    assert np.isnan(got["rotation"]).all() and np.isnan(got["history"]).all()


def disagreeing_pair():
    """a pair whose best gapless offset (0: the first half in place) is not where its best alignment comes from: the fragment seed at
    (14, 20) lies behind the deletion, on the displaced domain, and its unit wins in round 0"""
    return sweep_pair(30, 36, 1)


def test_a_pair_not_won_by_the_first_unit():
    a, b = disagreeing_pair()
    got = structalign_def(a, b)
    print("disagreeing pair: i1", got["i1"], "i2", got["i2"], "winner", got["unit"], got["round"], "tm", got["tm_a"], got["tm_b"])
    assert got["i1"][0] == 0 and got["i2"][:2] == (14, 20) and (got["unit"], got["round"]) == (2, 0)
    assert got["qmargin"] >= QMARGIN_CAP and min(got["margin"], got["final_margin"]) >= MARGIN_CAP


@pytest.mark.parametrize("case", SWEEP + [BLOCKS], ids=lambda c: "m%d-n%d" % c[:2])
def test_sweep_pairs_keep_their_margins(case):
    got = sweep_def(*case)
    fm = got.get("final_margin", np.inf)
    print(f"{case}: qmargin {got['qmargin']:.3g}, margin {min(got['margin'], fm):.3g} A, winner {got['unit']}, {got['round']}, "
          f"tm {got['tm_a']:.4f} / {got['tm_b']:.4f}, n_aligned {got['n_aligned']}")
    assert got["qmargin"] >= QMARGIN_CAP and min(got["margin"], fm) >= MARGIN_CAP
    assert got["unit"] >= 0 and 0 < got["tm_a"] <= 1


# ------------------------------------------------------------------ the host side of pesto_amd.structalign
def test_arguments_raise_before_any_launch():
    from pesto_amd import structalign as SA
    m = object()                # no handle: the checks must come first
    x = np.zeros((12, 3), np.float32)
    bad = (dict(sizes=[6, 5]), dict(sizes=[10, 2]), dict(sizes=None), dict(pairs=[[0, 2]]), dict(pairs=[[-1, 0]]), dict(pairs=np.zeros((0, 2), np.int32)),
           dict(gap_open=-0.1), dict(gap_open=1.5), dict(rounds=0), dict(rounds=65), dict(rounds=1.5), dict(frag_starts=1), dict(frag_starts=65),
           dict(scale=0.0), dict(scale=np.nan), dict(init=[np.zeros(5, np.int32)]), dict(init=[np.full(6, 6, np.int32)]), dict(init=[np.full(6, -2, np.int32)]), dict(init=[np.array([1, 0, 2, 3, 4, 5], np.int32)]),
           dict(coords=np.zeros((12, 2), np.float32)), dict(codes=np.zeros(11, np.uint8)))
    for kw in bad:
        args = dict(coords=x, sizes=[6, 6], model=m)
        args.update(kw)
        with pytest.raises(ValueError):
            SA.align_structures(**args)
    with pytest.raises(ValueError, match="4096"):
        SA.align_structures(np.zeros((4100, 3), np.float32), [4097, 3], model=m)
    with pytest.raises(ValueError):
        SA.tm_matrix(x, [12], model=m)
    with pytest.raises(ValueError):
        SA.tm_matrix(x, [6, 6], pairs=[[0, 1]], model=m)


def test_new_symbols_are_declared_and_bound():
    from pesto_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    for name in ("pesto_structalign_last_error", "pesto_structalign"):
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.ABI_SYMBOLS
    from pesto_amd import structalign as SA
    for name, value in (("Q", SA.Q), ("MIN_LENGTH", SA.MIN_LENGTH), ("MAX_LENGTH", SA.MAX_LENGTH), ("MAX_ROUNDS", SA.MAX_ROUNDS),
                        ("MIN_FRAG_STARTS", SA.MIN_FRAG_STARTS), ("MAX_FRAG_STARTS", SA.MAX_FRAG_STARTS)):
        assert int(re.search(rf"PESTO_STRUCTALIGN_{name} = (\d+)", hdr).group(1)) == value
    assert int(re.search(r"PESTO_STRUCTALIGN_MAX_PAIRS = 1 << (\d+)", hdr).group(1)) == 20 and SA.MAX_PAIRS == 2 ** 20
    import pesto_amd
    assert pesto_amd.align_structures is SA.align_structures and pesto_amd.tm_matrix is SA.tm_matrix and pesto_amd.structalign is SA
    assert pesto_amd.ca_traces is SA.ca_traces and pesto_amd.structure_align is SA.structure_align
    csrc = os.path.join(ROOT, "pesto_amd", "csrc")
    src = open(os.path.join(csrc, "pesto_structalign.hip")).read()
    assert not re.search(r"\basm\b|atomic[A-Z]|__hip_atomic", src)              # plain C++: no inline assembly, no atomics
    assert "tm_search_launch" in src and "k_tm_search" not in src.split("namespace pesto {")[1]     # the search is launched, not copied
    assert "align_wave<MODE_OVERLAP, TRACE>" in src and "kabsch_fit_wave" in src and "kabsch_fit<NT, true>" in src and "moved_deviation<NT>" in src
    align = open(os.path.join(csrc, "pesto_align.hip")).read()
    assert "pesto_alignwave.h" in align and "shift_up" not in align                     # the recursion lives in the shared header alone
    build = open(os.path.join(csrc, "build.py")).read()
    assert all(f in build for f in ("pesto_structalign.hip", "pesto_alignwave.h", "pesto_tmsearch.h"))
