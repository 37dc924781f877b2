"""Deterministic case generators of the assembly sweeps (a plain module, in the shape of tests/analysis_sweep.py: tests/test_assembly_sweep_fixture.py
checks the generators and definitions without a GPU, tests/test_assembly_sweep.py puts every case through its entry point on one).

A case is a tuple (family, seed, shape); the lists are fixed. ``build(entry, case)`` returns the inputs and the expected outputs of the
vectorised NumPy definitions below, which the fixture test pins to the restatements the CPU suite already trusts (dataset_fixture.np_contacts
/ np_typed_keys and the recorded dataset_*.npz, the recorded eval_scores.npz, test_patches_fixture.definition). Inputs come from
numpy.random.default_rng([seed, attempt]); no builder looks at the library.

contacts (pesto_contacts.hip behind the cell grid: the radix sort of pesto_radix.h, RADIX_TILE = 2048 keys per tile in 8 rounds of 256 and
a result that lies in the second buffer after an odd number of moving passes; the 1024-thread k_ct_scan, k_ct_gather's search over the
per-atom offsets, the typed keys whose 22-bit group field lies in key bits 42..63, the swapped keys' second sort, the capacities)
    family = lattice | rough, + typed | untyped | mix (about 30 % untyped) | planted (mix, and two planted residue pairs: typed contacts
    then an untyped LAST one - no key -, untyped contacts then a typed LAST one - a key), + nt128 | nt1 (n_types, else 79 = MOLECULE_IDS;
    nt128 has type 127 on both sides of a key), + r8191 (the first contact lies in residues 0, the last, typed, in residues 8191)
    shape = the assemblies of the call, each with sizes known from its construction:
    (comb, K, m, split, lone)  receptor atoms 100 A apart on a line (subunit A, a residue each), K partner atoms m beside each of the first
                               toothed receptors (2.5 A away), bare receptors (no contact: a repeated per-atom offset) in between. split
                               0: the partners are one subunit (G = 1); 1: each partner a single-atom subunit of its own (G = K). lone: one
                               more single-atom subunit 50 A off the line, without any contact. Exactly K contacts.
    (ball, n_sub, atoms)       subunits of ``atoms`` atoms (23: 2 and 3 in turn) in a ball of radius 2.4 A: every pair of atoms of two
                               subunits is a contact, G = n_sub (n_sub - 1) / 2
    (fan, n)                   atom 0 with n partners of the next subunit whose index DEscends along (z, y, x), the order of the cell
                               walk: the insertion sort of its range gets them the wrong way round; K = n, G = 1
    (cloud, n_sub, n)          n atoms in a box, subunits of random sizes, about three atoms per residue (no promise but K > 0)
scores (k_bc_scores: BC_THREADS = 256 rows per pass, BC_TILE = 2048 rows staged, the outer class P <= N)
    shape = (rows per structure, classes); scores are multiples of 2^-24 in [0, 1]: every float64 sum of them is exact in any order
    family: distinct | grid8 (eight values: heavy ties) | allpos | allneg | P1 | N1 | PeqN | PgtN | half (0.5 and 0.5 + 2^-24 only) | const
patches (pesto_patches.hip: SMALL_THREADS = TILE = 256, LARGE_THREADS = 1024, PESTO_PATCHES_SMALL_MAX = 4096 rows)
    shape = (((graph, nodes, layout), ...), classes); layout alone: node rows only (one non-node row when there is no node); mixed:
    2 n + 3 rows, the non-node rows in turn p at the threshold, afs at the threshold, no CA, NaN; a number: that many rows. Node rows pass
    in every class, so every selection has exactly ``nodes`` nodes (family +varied: random p, the node set differs per selection).
    graph: chain (8 A steps, a few 12 A gaps) | star (every leaf within reach of node 0) | clique | dust (12 A grid: no edge) |
    twocliques (nodes 0..255 and 256.., ONE edge, between nodes 255 and 256; residue order kept) | lattice (planted pairs 10 apart
    exactly - no edge -, with s = s* = 100 - 2^-17, whose root rounds to 10 - no edge, where `s <= s*` would make one -, and one unit
    further in - an edge) | rough. Residue order is shuffled against spatial order but for twocliques.
labels (k_contact_labels): 2 to 3 assemblies of 3 to 5 subunits, partner masks 0, 1 << 31 and multi-bit words, a receptor subset,
    residues shared by several atoms.
"""
import functools

import numpy as np

from analysis_sweep import case_id, chain_dist, drawn, lattice_points, parse, rough_points  # noqa: F401  (case_id: the tests' ids)

R_THR = 5.0
P_GRID = 2.0 ** -24


def ident(case):
    """analysis_sweep.case_id of the case with its nested shape entries flattened (and a long list of them counted)"""
    family, seed, shape = case
    flat = tuple(v if not isinstance(v, tuple) else f"{len(v)}items" if len(v) > 8 else
                 tuple("".join(str(e) for e in x) if isinstance(x, tuple) else x for x in v) for v in shape)
    return case_id((family, seed, flat))


# ================================================================== contacts
CONTACTS = (
    ("lattice+typed", 301, (("comb", 0, 1, 0, 0),)),
    ("rough+mix", 302, (("comb", 1, 1, 0, 1),)),
    ("lattice+untyped", 303, (("comb", 255, 4, 0, 0),)),
    ("rough+typed+nt128", 304, (("comb", 100, 2, 0, 0), ("comb", 0, 1, 0, 0), ("comb", 156, 3, 0, 1))),
    ("lattice+planted", 305, (("comb", 257, 2, 0, 0),)),
    ("rough+mix", 306, (("comb", 511, 4, 0, 0),)),
    ("lattice+typed+nt1", 307, (("comb", 512, 4, 0, 0),)),
    ("rough+planted+r8191", 308, (("comb", 513, 3, 0, 1),)),
    ("lattice+mix", 309, (("comb", 1023, 5, 0, 0),)),
    ("rough+typed", 310, (("comb", 1024, 5, 0, 0),)),
    ("lattice+mix+nt128", 311, (("comb", 1025, 5, 0, 0),)),
    ("lattice+typed", 312, (("comb", 63, 1, 1, 0),)),
    ("rough+mix", 313, (("comb", 64, 1, 1, 0),)),
    ("lattice+mix", 314, (("comb", 65, 1, 1, 1),)),
    ("rough+typed", 315, (("comb", 254, 1, 1, 0),)),
    ("lattice+mix", 316, (("comb", 255, 1, 1, 0),)),
    ("rough+mix+r8191", 317, (("comb", 256, 1, 1, 0),)),
    ("lattice+typed", 318, (("comb", 257, 1, 1, 0),)),
    ("rough+mix", 319, (("ball", 5, 23), ("comb", 0, 1, 0, 0), ("fan", 70), ("cloud", 4, 90), ("ball", 3, 3), ("comb", 7, 2, 1, 1))),
    ("lattice+mix+r8191", 320, (("cloud", 6, 200), ("fan", 66))),
    ("rough+mix", 321, (("ball", 40, 23),)),
    ("lattice+mix", 323, (("comb", 2047, 5, 0, 0),)),
    ("rough+typed", 324, (("comb", 2048, 5, 0, 1),)),
    ("lattice+planted", 325, (("comb", 2000, 4, 0, 0), ("comb", 49, 1, 1, 0))),
    ("rough+mix", 326, (("comb", 4000, 5, 0, 0), ("comb", 97, 1, 1, 1))),
    ("lattice+mix+nt1", 322, (("ball", 260, 2),)),              # K = 134,680, G = 33,670: three calls at the default capacities
)
BIG_BALL = CONTACTS[-1]


def _ball_sizes(n_sub, atoms):
    return [2 + (i % 2) if atoms == 23 else atoms for i in range(n_sub)]


def promised(spec):
    """(atoms, subunits, K, G) of an assembly from its construction alone; K and G None where the construction promises none"""
    kind = spec[0]
    if kind == "comb":
        _, K, m, split, lone = spec
        teeth = -(-K // m)
        n_part = max(K, 1)
        return teeth + teeth // 8 + 1 + n_part + lone, 1 + (n_part if split else 1) + lone, K, (K if split else min(K, 1))
    if kind == "ball":
        sizes = _ball_sizes(spec[1], spec[2])
        n = sum(sizes)
        return n, spec[1], (n * n - sum(v * v for v in sizes)) // 2, spec[1] * (spec[1] - 1) // 2
    if kind == "fan":
        return spec[1] + 3, 2, spec[1], 1
    return spec[2], spec[1], None, None


def _call_sizes(shape):
    p = [promised(s) for s in shape]
    known = all(v[2] is not None for v in p)
    return sum(v[0] for v in p), sum(v[1] for v in p), sum(v[2] for v in p) if known else None, sum(v[3] for v in p) if known else None


def _ball_points(rng, kind, n, radius):
    out = np.zeros((0, 3), np.float32)
    while out.shape[0] < n:
        c = lattice_points(rng, (4 * n, 3), radius) if kind == "lattice" else rough_points(rng, (4 * n, 3), radius)
        out = np.concatenate([out, c[(c.astype(np.float64) ** 2).sum(1) < radius * radius]])
    return out[:n]


def _assembly(rng, kind, spec):
    """(xyz float32 [n, 3], local subunit int32 [n] ascending, residue int32 [n]) of one assembly"""
    what = spec[0]
    if what == "comb":
        _, K, m, split, lone = spec
        teeth = -(-K // m)
        n_rec = teeth + teeth // 8 + 1
        toothed = np.sort(rng.choice(n_rec, teeth, replace=False))                  # the bare receptors lie in between
        rec = np.zeros((n_rec, 3), np.float32)
        rec[:, 0] = 100.0 * np.arange(n_rec)
        if kind == "rough":
            rec += rough_points(rng, (n_rec, 3), 0.4)
        near = np.array([[1.5, 2.0, 0.0], [-1.5, 2.0, 0.0], [0.0, -2.0, 1.5], [0.0, 2.0, -1.5], [2.0, 0.0, 1.5]], np.float32)   # 2.5 away
        part = np.stack([rec[toothed[k // m]] + near[k % m] for k in range(K)]) if K else rec[:1] + np.float32([0.0, 50.0, 0.0])
        if kind == "rough" and K:
            part = part + rough_points(rng, part.shape, 0.4)
        xyz = [rec, part.astype(np.float32)]
        sub = [np.zeros(n_rec, np.int32), 1 + (np.arange(part.shape[0]) if split else np.zeros(part.shape[0])).astype(np.int32)]
        res = [np.arange(n_rec, dtype=np.int32), (np.arange(part.shape[0]) // m // 2 if not split else np.zeros(part.shape[0])).astype(np.int32)]
        if lone:
            xyz.append(rec[-1:] + np.float32([0.0, -50.0, 0.0])); sub.append(sub[1][-1:] + 1); res.append(np.zeros(1, np.int32))
        return np.concatenate(xyz).astype(np.float32), np.concatenate(sub), np.concatenate(res)
    if what == "ball":
        sizes = _ball_sizes(spec[1], spec[2])
        sub = np.repeat(np.arange(spec[1]), sizes).astype(np.int32)
        return _ball_points(rng, kind, sub.size, 2.4), sub, rng.integers(0, 2, sub.size).astype(np.int32)
    if what == "fan":
        n = spec[1]
        b = _ball_points(rng, kind, n, 4.9)
        b = b[np.lexsort((b[:, 0], b[:, 1], b[:, 2]))[::-1]]                        # the index descends along (z, y, x)
        anchors = np.float32([[-20.0, -20.0, -20.0], [20.0, 20.0, 20.0]])             # (of atom 0's subunit: a grid of several cells)
        xyz = np.concatenate([np.zeros((1, 3), np.float32), anchors, b]).astype(np.float32)
        return xyz, np.concatenate([np.zeros(3, np.int32), np.ones(n, np.int32)]), np.concatenate([np.zeros(3), np.arange(n) // 4]).astype(np.int32)
    _, n_sub, n = spec
    side = max(6.0, (40.0 * n) ** (1.0 / 3.0))
    xyz = lattice_points(rng, (n, 3), side / 2) if kind == "lattice" else rough_points(rng, (n, 3), side / 2)
    sub = np.sort(np.concatenate([np.arange(n_sub), rng.integers(0, n_sub, n - n_sub)])).astype(np.int32)
    res = np.concatenate([np.sort(rng.integers(0, max(1, c // 3), c)) for c in np.bincount(sub)]).astype(np.int32)
    return xyz, sub, res


def contacts_def(X, sub, res, typ, offs, n_types, r_thr=R_THR):
    """The call's outputs restated. Per assembly the float32 distance chain over all atoms; the pairs with sub[a] < sub[b] and D < r_thr
    ordered by (sub[a], sub[b], a, b); the group table from the runs; per group the LAST contact of each (r0, r1) decides its slab
    (a key where both atoms are typed); the sorted typed rows are the keys, the swapped rows sorted the reverse keys; T from the keys."""
    thr = np.float32(r_thr)
    n = X.shape[0]
    A, B, Dd, ties = [], [], [], np.zeros(n, np.uint8)
    for s in range(len(offs) - 1):
        o0, o1 = int(offs[s]), int(offs[s + 1])
        x, su = X[o0:o1], sub[o0:o1].astype(np.int64)
        ia, ib, dd = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
        for c0 in range(0, o1 - o0, 512):
            D = chain_dist(x[c0:c0 + 512], x).astype(np.float32)
            rows = su[c0:c0 + 512, None]
            with np.errstate(invalid="ignore"):
                ties[o0 + c0:o0 + c0 + D.shape[0]] = ((D == thr) & (rows != su[None, :])).any(1)
                a, b = np.nonzero((D < thr) & (rows < su[None, :]))
            ia.append(a + c0); ib.append(b); dd.append(D[a, b])
        ia, ib, dd = np.concatenate(ia), np.concatenate(ib), np.concatenate(dd)
        order = np.lexsort((ib, ia, su[ib], su[ia]))
        A.append(ia[order] + o0); B.append(ib[order] + o0); Dd.append(dd[order])
    a, b, d = np.concatenate(A), np.concatenate(B), np.concatenate(Dd).astype(np.float32)
    K = a.size
    gkey = sub[a].astype(np.int64) * 65536 + sub[b]
    first = np.ones(K, bool)
    first[1:] = gkey[1:] != gkey[:-1]
    start = np.nonzero(first)[0]
    G = start.size
    gid = np.cumsum(first) - 1
    groups = np.zeros((G, 4), np.int32)
    groups[:, 0], groups[:, 1], groups[:, 2] = sub[a[start]], sub[b[start]], start
    r0, r1, t0, t1 = res[a].astype(np.int64), res[b].astype(np.int64), typ[a].astype(np.int64), typ[b].astype(np.int64)
    key = (gid << 26) | (r0 << 13) | r1
    order = np.argsort(key, kind="stable")
    ks = key[order]
    last = np.ones(K, bool)
    last[:-1] = ks[1:] != ks[:-1]
    pick = order[last]
    pick = pick[(t0[pick] >= 0) & (t1[pick] >= 0)]
    kg = gid[pick]
    groups[:, 3] = np.bincount(kg, minlength=G)[:G] if G else 0
    keys = np.stack([r0[pick], r1[pick], t0[pick], t1[pick]], 1).astype(np.uint16).reshape(-1, 4)
    rev = np.lexsort((r0[pick], r1[pick], kg))
    rkeys = np.ascontiguousarray(keys[rev][:, [1, 0, 3, 2]])
    T = np.zeros((G, n_types, n_types), np.uint8)
    T[kg, t0[pick], t1[pick]] = 1
    # what the three radix sorts order by, from their lowest sorted bit up: the subunit pair (32 bits), (group, r0, r1) of every contact
    # and (group, r1, r0) of every typed key (48 bits each)
    sort_keys = dict(regroup=gkey, typed=key, swapped=(kg << 26) | (r1[pick] << 13) | r0[pick])
    return dict(pairs=np.stack([a, b], 1).astype(np.int32).reshape(-1, 2), d=d, groups=groups, keys=keys, rkeys=rkeys, T=T, ties=ties, K=int(K), G=int(G),
                U=int(pick.size), run_key=key, gid=gid, sort_keys=sort_keys)


SORT_BYTES = dict(regroup=4, typed=6, swapped=6)


def moving_passes(keys, n_bytes):
    """radix passes of 8 bits that move keys: every pass but those in which all keys share the digit (none of no key)"""
    return sum(1 for i in range(n_bytes) if np.unique((keys >> (8 * i)) & 255).size > 1)


def n_types_of(flags):
    return 128 if "nt128" in flags else 1 if "nt1" in flags else 79


def build_contacts(case):
    family, seed, shape = case
    kind, flags = parse(family)
    nt = n_types_of(flags)

    def draw(rng):
        X, sub, res, offs, base = [], [], [], [0], 0
        for spec in shape:
            x, su, r = _assembly(rng, kind, spec)
            X.append(x); sub.append(su + base); res.append(r)
            base += int(su.max()) + 1
            offs.append(offs[-1] + x.shape[0])
        X, sub, res = np.concatenate(X), np.concatenate(sub), np.concatenate(res)
        n = X.shape[0]
        typ = rng.integers(0, nt, n).astype(np.int32)
        if "untyped" in flags:
            typ[:] = -1
        elif flags & {"mix", "planted"}:
            typ[rng.random(n) < 0.3] = -1
        offs = np.array(offs, np.int64)
        want = contacts_def(X, sub, res, typ, offs, nt)
        if want["K"] == 0 and _call_sizes(shape)[2] != 0:
            return None
        if "r8191" in flags:                                # the first contact's atoms in residue 0, the last one's, typed, in residue 8191
            (a0, b0), (a1, b1) = want["pairs"][0], want["pairs"][-1]
            res[a0] = res[b0] = 0
            res[a1] = res[b1] = 8191
            typ[a1] = typ[b1] = nt - 1
            want = contacts_def(X, sub, res, typ, offs, nt)
        planted = None
        if want["K"] and (flags & {"planted", "nt128"}):
            # runs of one (group, r0, r1) in contact order, longer than one contact, whose partner atoms (column b) have no other contact
            key, pairs = want["run_key"], want["pairs"]
            runs = [np.nonzero(key == k)[0] for k in np.unique(key)]
            runs = [r for r in runs if r.size >= 2 and np.all(np.bincount(pairs[:, 1], minlength=n)[pairs[r, 1]] == 1)
                    and np.unique(pairs[r, 0]).size == 1]
            if len(runs) < 3:
                return None
            if "planted" in flags:
                no, yes = runs[0], runs[1]
                typ[pairs[no, 0]] = typ[pairs[no, 1]] = 0
                typ[pairs[no[-1], 1]] = -1                                              # typed, ..., untyped LAST: no key
                typ[pairs[yes, 1]] = -1
                typ[pairs[yes[-1], 0]] = typ[pairs[yes[-1], 1]] = nt - 1                # untyped, ..., typed LAST: a key
                planted = (int(key[no[0]]), int(key[yes[0]]))
            if "nt128" in flags:
                typ[pairs[runs[2], 0]] = typ[pairs[runs[2], 1]] = 127
            want = contacts_def(X, sub, res, typ, offs, nt)
        sizes = np.diff(offs)
        rows = []
        for s in range(len(shape)):
            o0, o1 = int(offs[s]), int(offs[s + 1])
            rows.append([(f"a{s}s{v}", X[o0:o1][sub[o0:o1] == v], res[o0:o1][sub[o0:o1] == v], typ[o0:o1][sub[o0:o1] == v],
                          int(res[o0:o1][sub[o0:o1] == v].max()) + 1) for v in np.unique(sub[o0:o1])])
        return dict(X=X, sub=sub, res=res, typ=typ, offs=offs, sizes=sizes, rows=rows, n_types=nt, n_sub=int(sub.max()) + 1, planted=planted, want=want)
    return drawn(draw, seed)


# ================================================================== scores
SIZES60 = tuple((1, 2, 255, 256, 257, 31)[k % 6] for k in range(60))
SCORES = (
    ("distinct", 401, ((1,), 1)),
    ("grid8", 402, ((2, 255, 256), 5)),
    ("PeqN", 403, ((256, 2048, 2), 5)),
    ("PgtN", 404, ((257, 2047, 2049), 1)),
    ("distinct", 405, ((4097,), 1)),
    ("allpos", 406, ((255, 1, 2), 5)),
    ("allneg", 407, ((2048, 257, 1), 1)),
    ("P1", 408, ((2049, 2, 256), 5)),
    ("N1", 409, ((2047, 255, 2), 1)),
    ("half", 410, ((257, 2048, 4097), 5)),
    ("const", 411, ((256, 2, 2049), 1)),
    ("grid8", 412, (SIZES60, 5)),
    ("distinct", 413, ((2047, 2048, 2049), 5)),
)


def n_positive(family, R):
    """positives of a class of R rows (None: drawn, about 30 %: P < N)"""
    return dict(allpos=R, allneg=0, P1=1, N1=R - 1, PeqN=R // 2, PgtN=R - max(1, R // 4) if R >= 3 else R).get(family)


def scores_def(y, p):
    """float32 [8, C] of one structure: integer TP, FP, P, N; rows 0 to 5 in float32, operation for operation as k_bc_scores evaluates
    them (every product of mcc rounded, sqrt, then the division; inf becomes NaN); auc = float32(2U / (2.0 P N)) with the integer 2U =
    sum of 2 (p+ > p-) + (p+ == p-) found by sorting; std = float32 of the float64 unbiased std."""
    y = np.asarray(y) != 0
    p = np.asarray(p, np.float32)
    R, C = p.shape
    f = np.float32
    out = np.zeros((8, C), np.float32)
    nan = f(np.nan)
    with np.errstate(all="ignore"):
        for c in range(C):
            yc, pc = y[:, c], p[:, c]
            q = np.rint(pc) != 0
            tp, fp, P = int((yc & q).sum()), int((~yc & q).sum()), int(yc.sum())
            N = R - P
            TP, FP, FN, TN = f(tp), f(fp), f(P - tp), f(N - fp)
            fin = lambda v: nan if np.isinf(v) else f(v)          # noqa: E731
            out[0, c] = (TP + TN) / (((TP + TN) + FP) + FN)
            out[1, c] = TP / (TP + FP) if P > 0 else nan
            out[2, c] = TN / (TN + FN) if N > 0 else nan
            out[3, c] = fin(TP / (TP + FN))
            out[4, c] = fin(TN / (TN + FP))
            num = f(f(TP * TN) - f(FP * FN))
            den = np.sqrt(f(f(f((TP + FP) * (TP + FN)) * (TN + FP)) * (TN + FN)))
            out[5, c] = fin(num / den)
            if P > 0 and N > 0:
                neg = np.sort(pc[~yc])
                lt, le = np.searchsorted(neg, pc[yc], "left"), np.searchsorted(neg, pc[yc], "right")
                u2 = 2 * int(lt.sum()) + int((le - lt).sum())
                out[6, c] = f(np.float64(u2) / (2.0 * np.float64(P) * np.float64(N)))
            else:
                out[6, c] = nan
            out[7, c] = f(np.std(pc.astype(np.float64), ddof=1)) if R > 1 else nan
    return out


def build_scores(case):
    family, seed, (sizes, C) = case
    rng = np.random.default_rng([seed, 0])
    ys, ps = [], []
    for R in sizes:
        y, p = np.zeros((R, C), np.uint8), np.zeros((R, C), np.float32)
        for c in range(C):
            P = n_positive(family, R)
            if P is None:
                y[:, c] = rng.random(R) < 0.3
            else:
                y[rng.permutation(R)[:P], c] = 1
            if family == "grid8":
                k = rng.integers(0, 8, R) * (1 << 21) + (1 << 20)
            elif family == "half":
                k = (1 << 23) + rng.integers(0, 2, R)
            elif family == "const":
                k = np.full(R, int(rng.integers(0, (1 << 24) + 1)))
            else:
                k = rng.permutation(np.unique(np.concatenate([rng.integers(0, (1 << 24) + 1, 2 * R + 8), [0, 1 << 24]])))[:R]
                assert np.unique(k).size == R
            p[:, c] = (k.astype(np.float64) * P_GRID).astype(np.float32)
        ys.append(y); ps.append(p)
    return dict(ys=ys, ps=ps, want=np.stack([scores_def(y, p) for y, p in zip(ys, ps)]), attempt=0)


# ================================================================== patches
THR = (70.0, 0.5, 10.0)                     # afs_thr, p_thr, d_thr (pesto_amd.patches' defaults)
SMALL70 = tuple((("chain", "rough", "dust", "star", "clique")[k % 5], (0, 1, 2, 3, 5, 8, 13, 21, 34)[k % 9], ("alone", "mixed")[k % 2]) for k in range(70))
PATCHES = (
    ("chain", 501, ((("chain", 0, "alone"),), 1)),
    ("chain", 502, ((("chain", 1, "alone"), ("chain", 2, "mixed"), ("dust", 255, "alone")), 5)),
    ("star", 503, ((("star", 256, "mixed"),), 5)),
    ("rough", 504, ((("rough", 257, "alone"), ("chain", 511, "mixed"), ("star", 512, "alone")), 1)),
    ("clique", 505, ((("clique", 513, "alone"),), 5)),
    ("chain", 506, ((("chain", 1023, "mixed"), ("rough", 1024, "alone"), ("chain", 1025, "mixed")), 1)),
    ("twocliques", 507, ((("twocliques", 512, "alone"), ("twocliques", 512, "mixed"), ("twocliques", 257, "alone")), 5)),
    ("lattice", 508, ((("lattice", 257, "mixed"),), 5)),
    ("dust", 509, ((("dust", 513, "alone"), ("dust", 1025, "mixed")), 1)),
    ("rough", 510, ((("rough", 300, 4096), ("rough", 300, 4097), ("chain", 2, "mixed")), 5)),
    ("rough+varied", 511, ((("rough", 200, "alone"), ("rough", 90, "mixed"), ("rough", 255, "alone")), 5)),
    ("rough", 512, (SMALL70, 11)),
)


def _graph(rng, graph, n):
    """float32 [n, 3] node coordinates in node (= residue) order"""
    if n == 0:
        return np.zeros((0, 3), np.float32)
    if graph == "chain":
        step = np.where(rng.random(n) < 0.02, 12.0, 8.0)
        x = np.stack([np.cumsum(step), np.zeros(n), np.zeros(n)], 1)
    elif graph == "star":
        u = rng.normal(0, 1, (n, 3))
        x = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(6.0, 9.5, (n, 1))
        x[0] = 0.0
    elif graph == "clique":
        x = _ball_points(rng, "rough", n, 4.9)
    elif graph == "dust":
        side = int(np.ceil(n ** (1.0 / 3.0)))
        k = np.arange(n)
        x = 12.0 * np.stack([k % side, (k // side) % side, k // (side * side)], 1)
    elif graph == "twocliques":
        x = _ball_points(rng, "rough", n, 1.5).astype(np.float64)
        x[256:, 0] += 17.0
        x[255], x[256] = [5.0, 0.0, 0.0], [12.0, 0.0, 0.0]
        return x.astype(np.float32)
    elif graph == "lattice":
        x = lattice_points(rng, (n, 3), 30.0).astype(np.float64) + [1000.0, 0.0, 0.0]
        for k, e in enumerate((0, 1, 2, 0, 1, 2)):            # pairs along z, 40 apart: exactly 10 | s = s* | one unit further in
            x[2 * k] = [0.0, 0.0, 40.0 * k]
            x[2 * k + 1] = [6.0, 8.0 - e * 2.0 ** -21, 40.0 * k] if k < 3 else [10.0 - e * 2.0 ** -20, 0.0, 40.0 * k]
        return x.astype(np.float32)                            # (node order kept: the planted pairs are nodes 0 .. 11)
    else:
        side = (n * 1400.0) ** (1.0 / 3.0)
        x = rng.uniform(0, side, (n, 3))
    return x[rng.permutation(n)].astype(np.float32)


def _structure(rng, spec, C, varied):
    """(xyz, p, afs, has_ca, node rows) of one structure"""
    graph, n, layout = spec
    R = max(n, 1) if layout == "alone" else 2 * n + 3 if layout == "mixed" else int(layout)
    rows = np.sort(rng.choice(R, n, replace=False)) if layout != "alone" else np.arange(n)
    xyz = rough_points(rng, (R, 3), 40.0)
    xyz[rows] = _graph(rng, graph, n)
    grid = lambda lo, hi, shape: (rng.integers(lo, hi, shape).astype(np.float64) * P_GRID).astype(np.float32)     # noqa: E731
    p = grid(0, (1 << 24) + 1, (R, C)) if varied else grid((1 << 23) + 1, (1 << 24) + 1, (R, C))
    afs = rng.uniform(71.0, 100.0, R).astype(np.float32)
    has = np.ones(R, np.uint8)
    off = np.setdiff1d(np.arange(R), rows)
    for k, r in enumerate(off):
        if k % 4 == 0:
            p[r] = 0.5
        elif k % 4 == 1:
            afs[r] = 70.0
        elif k % 4 == 2:
            has[r] = 0
        else:
            p[r] = np.nan
    return xyz, p, afs, has, rows


def patches_def(xyz, p, afs, has, sels, reuse):
    """(patch_of int32 [K, R], n_patches int32 [K], patch_size int32 [K, R], patch_mean float32 [K, R, 2]) of one structure: the membership
    of test_patches_fixture.definition; sizes are counts; each mean float32(float64 sum / count) at the patch's smallest row.
    reuse: the node set is the same for every selection (asserted), so the membership is computed once."""
    from test_patches_fixture import definition
    R, K = p.shape[0], len(sels)
    po, ps, pm, npch = np.full((K, R), -1, np.int32), np.zeros((K, R), np.int32), np.zeros((K, R, 2), np.float32), np.zeros(K, np.int32)
    with np.errstate(invalid="ignore"):
        ok = (has != 0) & (afs > np.float32(THR[0]))
        masks = [(p[:, i] > np.float32(THR[1])) & (p[:, j] > np.float32(THR[1])) & ok for i, j in sels]
    comps = None
    for k, (i, j) in enumerate(sels):
        if reuse:
            assert np.array_equal(masks[k], masks[0])
        if comps is None or not reuse:
            with np.errstate(invalid="ignore"):
                comps = definition(xyz, p, afs, has, (i, j), THR)
        assert sorted(r for c in comps for r in c) == np.nonzero(masks[k])[0].tolist()
        npch[k] = len(comps)
        for q, m in enumerate(comps):
            m = np.asarray(m)
            po[k, m] = q
            ps[k, m[0]] = m.size
            pm[k, m[0]] = [np.float32(p[m, i].astype(np.float64).sum() / m.size), np.float32(p[m, j].astype(np.float64).sum() / m.size)]
    return po, npch, ps, pm


def build_patches(case):
    family, seed, (structs, C) = case
    _, flags = parse(family)
    rng = np.random.default_rng([seed, 0])
    sels = [(i, j) for i in range(C) for j in range(i, C)]
    parts = [_structure(rng, spec, C, "varied" in flags) for spec in structs]
    outs = [patches_def(x, p, a, h, sels, "varied" not in flags) for x, p, a, h, _ in parts]
    return dict(xyzs=[v[0] for v in parts], ps=[v[1] for v in parts], afss=[v[2] for v in parts], has=[v[3] for v in parts],
                nodes=[v[4] for v in parts], sels=sels, patch_of=np.concatenate([o[0] for o in outs], 1), n_patches=np.stack([o[1] for o in outs]),
                patch_size=np.concatenate([o[2] for o in outs], 1), patch_mean=np.concatenate([o[3] for o in outs], 1), attempt=0)


# ================================================================== labels
# shape: ((subunits, atoms per subunit), ...)
LABELS = (
    ("lattice", 601, ((3, 20), (5, 12))),
    ("rough", 602, ((4, 33), (3, 7), (5, 40))),
    ("lattice", 603, ((5, 64), (3, 3), (4, 17))),
    ("rough", 604, ((3, 90), (4, 50))),
)


def labels_def(X, sub, res, receptor, mask, offs, n_res, r_thr=R_THR):
    """labels[res[a]] |= mask[b] for every receptor atom a and atom b of another subunit of its assembly with D < r_thr (the float32
    chain); ties[a]: a receptor atom with such a b, of a non-zero mask, at exactly r_thr"""
    thr = np.float32(r_thr)
    labels, ties = np.zeros(n_res, np.uint32), np.zeros(X.shape[0], np.uint8)
    for s in range(len(offs) - 1):
        o0, o1 = int(offs[s]), int(offs[s + 1])
        D = chain_dist(X[o0:o1], X[o0:o1]).astype(np.float32)
        use = (sub[o0:o1, None] != sub[None, o0:o1]) & (receptor[o0:o1, None] != 0) & (mask[None, o0:o1] != 0)
        a, b = np.nonzero(use & (D < thr))
        np.bitwise_or.at(labels, res[o0:o1][a], mask[o0:o1][b])
        ties[o0:o1] = (use & (D == thr)).any(1)
    return labels, ties


def build_labels(case):
    family, seed, shape = case
    kind, _ = parse(family)

    def draw(rng):
        X, sub, res, offs, s0, r0 = [], [], [], [0], 0, 0
        for n_sub, per in shape:
            n = n_sub * per
            side = max(6.0, (40.0 * n) ** (1.0 / 3.0))
            x = lattice_points(rng, (n, 3), side / 2) if kind == "lattice" else rough_points(rng, (n, 3), side / 2)
            if kind == "lattice":
                x[per] = x[0] + np.float32([3.0, 4.0, 0.0]) * (-1 if x[0, 0] > 0 else 1)          # d = r_thr exactly: a tie, no contact
            X.append(x); sub.append(s0 + np.repeat(np.arange(n_sub), per))
            r = np.unique(rng.integers(0, max(1, n // 3), n), return_inverse=True)[1].reshape(-1)      # shared by several atoms, across subunits too
            res.append(r0 + r)
            s0 += n_sub; r0 += int(r.max()) + 1
            offs.append(offs[-1] + n)
        X, sub, res = np.concatenate(X), np.concatenate(sub).astype(np.int32), np.concatenate(res).astype(np.int32)
        n = X.shape[0]
        receptor = (rng.random(n) < 0.6).astype(np.uint8)
        words = np.array([0, 1 << 31, 1, (1 << 31) | 5, 0x00f0f000, 0x7fffffff, 0xffffffff], np.uint32)
        mask = np.where(rng.random(n) < 0.5, words[rng.integers(0, words.size, n)], rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
        if kind == "lattice":
            receptor[0], mask[shape[0][1]] = 1, np.uint32(1 << 31)
        offs = np.array(offs, np.int64)
        labels, ties = labels_def(X, sub, res, receptor, mask, offs, r0)
        if not labels.any() or (labels != 0).all() or (kind == "lattice" and not ties.any()):
            return None
        return dict(X=X, sub=sub, res=res, receptor=receptor, mask=mask.astype(np.uint32), sizes=np.diff(offs), offs=offs, n_res=r0, labels=labels, ties=ties)
    return drawn(draw, seed)


# ================================================================== the registry
CASES = dict(contacts=CONTACTS, scores=SCORES, patches=PATCHES, labels=LABELS)
BUILDERS = dict(contacts=build_contacts, scores=build_scores, patches=build_patches, labels=build_labels)
ENTRY_POINTS = dict(contacts=("dataset._contacts_call", "pesto_contacts"), scores=("evaluate.bc_scores_batch",),
                    patches=("patches.patch_labels", "patches.interface_patches_batch"), labels=("evaluate.contact_labels",))


@functools.lru_cache(maxsize=None)
def build(entry, case):
    return BUILDERS[entry](case)


def all_cases():
    return [(entry, case) for entry, cases in CASES.items() for case in cases]


def every_third(entry, case):
    """the cases that also run from host arrays"""
    return CASES[entry].index(case) % 3 == 0


def coverage():
    """{(case list, constant): the set of values the list's shapes hit}"""
    t = {}

    def hit(entry, name, values):
        t.setdefault((entry, name), set()).update(values)
    for case in CONTACTS:
        family, _, shape = case
        kind, flags = parse(family)
        _, n_sub, K, G = _call_sizes(shape)
        hit("contacts", "RADIX_TILE,rounds,scan:K", [K]); hit("contacts", "G", [G]); hit("contacts", "G>16384", [G is not None and G > 16384])
        hit("contacts", "n_sub", [n_sub]); hit("contacts", "assemblies", [len(shape)]); hit("contacts", "coordinates", [kind])
        hit("contacts", "types", flags & {"typed", "untyped", "mix", "planted"}); hit("contacts", "n_types", [n_types_of(flags)])
        hit("contacts", "residues 0 and 8191", ["r8191" in flags])
        specs = [s for s in shape]
        hit("contacts", "features", ["K = 0 between"] if any(promised(specs[k])[2] == 0 and promised(specs[k - 1])[2] and promised(specs[k + 1])[2]
                                                              for k in range(1, len(specs) - 1)) else [])
        hit("contacts", "features", ["lone subunit"] if any(s[0] == "comb" and s[4] for s in specs) else [])
        hit("contacts", "features", ["single-atom subunits"] if any(s[0] == "comb" and s[3] for s in specs) else [])
        hit("contacts", "features", ["descending partners >= 64"] if any(s[0] == "fan" and s[1] >= 64 for s in specs) else [])
        # per sort the number of passes that move keys, from the case's own definition keys, and its class: an odd number leaves the
        # sorted keys in the second buffer
        for name, keys in build("contacts", case)["want"]["sort_keys"].items():
            moves = moving_passes(keys, SORT_BYTES[name])
            hit("contacts", f"{name} sort: moving passes", [moves, "0" if moves == 0 else "odd" if moves % 2 else "even > 0"])
    for family, _, (sizes, C) in SCORES:
        hit("scores", "BC_THREADS,BC_TILE:R", sizes); hit("scores", "C", [C]); hit("scores", "S", [len(sizes)]); hit("scores", "family", [family])
    for family, _, (structs, C) in PATCHES:
        hit("patches", "nodes", [n for _, n, _ in structs]); hit("patches", "layout", [lay if isinstance(lay, str) else "rows" for _, _, lay in structs])
        hit("patches", "SMALL_MAX:R", [lay for _, _, lay in structs if not isinstance(lay, str)]); hit("patches", "S", [len(structs)])
        hit("patches", "n_class", [C]); hit("patches", "graph", [g for g, _, _ in structs])
        rows = [max(n, 1) if lay == "alone" else 2 * n + 3 if lay == "mixed" else lay for _, n, lay in structs]
        hit("patches", "small and large in one call", [min(rows) <= 4096 < max(rows)])
    for _, _, shape in LABELS:
        hit("labels", "assemblies", [len(shape)]); hit("labels", "subunits", [s for s, _ in shape])
    return t


REQUIRED = {
    ("contacts", "RADIX_TILE,rounds,scan:K"): {0, 1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4097},
    ("contacts", "regroup sort: moving passes"): {"0", "odd", "even > 0"}, ("contacts", "typed sort: moving passes"): {"0", "odd", "even > 0"},
    ("contacts", "swapped sort: moving passes"): {"0", "odd", "even > 0"}, ("contacts", "G"): {0, 1, 63, 64, 65, 255, 256, 257},
    ("contacts", "G>16384"): {True}, ("contacts", "n_sub"): {2, 3, 255, 256, 257}, ("contacts", "assemblies"): {1, 2, 3, 6},
    ("contacts", "features"): {"K = 0 between", "lone subunit", "single-atom subunits", "descending partners >= 64"},
    ("contacts", "residues 0 and 8191"): {True}, ("contacts", "types"): {"typed", "untyped", "mix", "planted"}, ("contacts", "n_types"): {79, 128, 1},
    ("contacts", "coordinates"): {"lattice", "rough"},
    ("scores", "BC_THREADS,BC_TILE:R"): {1, 2, 255, 256, 257, 2047, 2048, 2049, 4097}, ("scores", "C"): {1, 5}, ("scores", "S"): {1, 3, 60},
    ("scores", "family"): {"distinct", "grid8", "allpos", "allneg", "P1", "N1", "PeqN", "PgtN", "half", "const"},
    ("patches", "nodes"): {0, 1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025}, ("patches", "layout"): {"alone", "mixed"},
    ("patches", "SMALL_MAX:R"): {4096, 4097}, ("patches", "small and large in one call"): {True}, ("patches", "S"): {1, 3, 70},
    ("patches", "n_class"): {1, 5, 11}, ("patches", "graph"): {"chain", "star", "clique", "dust", "twocliques", "lattice", "rough"},
    ("labels", "assemblies"): {2, 3}, ("labels", "subunits"): {3, 4, 5},
}
